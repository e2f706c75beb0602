"""Float64 restatement of the latent diagnostics of mosesvae.VAE (test helper): the importance-sampling draw, the IW log-likelihood and
ELBO, the pairwise Gaussian log-sum-exp, and He et al.'s (2019) MI and active units, over the whole evaluated set.
log p(x | z) comes from beam_ref.teacher_forced (the decoder in float64)."""
import numpy as np

import beam_ref as BR

LOG2PI = np.log(2.0 * np.pi)


def logsumexp(v, axis=-1):
    v = np.asarray(v, np.float64)
    m = np.max(v, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        return np.squeeze(m, axis) + np.log(np.sum(np.exp(v - m), axis=axis))


def iw_draw(mu, logvar, eps):
    """mu, logvar [B, dz], eps [B, K, dz] -> z [B, K, dz], log N(z; 0, I) - log N(z; mu, sigma^2) [B, K]."""
    mu, logvar, eps = (np.asarray(a, np.float64) for a in (mu, logvar, eps))
    z = mu[:, None] + np.exp(0.5 * logvar)[:, None] * eps
    return z, 0.5 * np.sum(eps ** 2 + logvar[:, None] - z ** 2, -1)


def log_weights(p64, seqs, mu, logvar, eps):
    """log w [B, K] = log p(x | z_k) (teacher forced, float64) + the Gaussian part; also the log p(x | z_k) alone."""
    z, lg = iw_draw(mu, logvar, eps)
    lp = np.array([[BR.teacher_forced(p64, z[b, k], np.asarray(seqs[b]))[0].sum() for k in range(z.shape[1])] for b in range(len(seqs))])
    return lp + lg, lp


def iw_estimates(logw):
    """log w [B, K] -> (log p_K(x) = logsumexp_k log w - log K, elbo_K = mean_k log w)."""
    logw = np.asarray(logw, np.float64)
    return logsumexp(logw, -1) - np.log(logw.shape[-1]), logw.mean(-1)


def gauss_logpdf_pairs(z, mu, logvar):
    """[Nz, Nx] log N(z_i; mu_j, exp(logvar_j)) as the direct difference."""
    z, mu, logvar = (np.asarray(a, np.float64) for a in (z, mu, logvar))
    out = np.empty((z.shape[0], mu.shape[0]))
    s = np.exp(-0.5 * logvar)
    c = -0.5 * logvar.sum(1) - 0.5 * z.shape[1] * LOG2PI
    for i in range(z.shape[0]):
        out[i] = c - 0.5 * np.sum(((z[i] - mu) * s) ** 2, 1)
    return out


def pairwise_lse(z, mu, logvar):
    """out[i] = logsumexp_j log N(z_i; mu_j, sigma_j^2), and the dominant exponent max_j of each row."""
    lp = gauss_logpdf_pairs(z, mu, logvar)
    return logsumexp(lp, 1), lp.max(1)


def mutual_info(mu, logvar, z):
    """He et al.'s calc_mi over the whole set: one draw z_i per molecule."""
    mu, logvar = np.asarray(mu, np.float64), np.asarray(logvar, np.float64)
    N, dz = mu.shape
    neg_entropy = np.mean(-0.5 * dz * LOG2PI - 0.5 * np.sum(1.0 + logvar, 1))
    log_qz = pairwise_lse(z, mu, logvar)[0] - np.log(N)
    return neg_entropy - log_qz.mean()


def active_units(mu, delta=0.01):
    mu = np.asarray(mu, np.float64)
    return int(np.sum(np.var(mu, axis=0, ddof=1) > delta))


def kl(mu, logvar):
    mu, logvar = np.asarray(mu, np.float64), np.asarray(logvar, np.float64)
    return float(np.mean(0.5 * np.sum(np.exp(logvar) + mu ** 2 - 1.0 - logvar, 1)))
