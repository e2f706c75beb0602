"""CPU tests of the latent diagnostics surface (mvae_gauss_iw_draw, mvae_group_logmeanexp, mvae_gauss_pairwise_lse, VAE.iw_log_likelihood,
train.moses_latent_diagnostics): the entry points are declared, bound and exported at ABI 12, bad arguments are refused before anything is
launched, and the float64 restatement of tests/latent_ref.py checks itself."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import molecular_vae_amd as mv
from molecular_vae_amd import _lib as L, mosesvae as MV, ops, vocab as VC
import latent_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mvae_gauss_iw_draw", "mvae_group_logmeanexp", "mvae_gauss_pairwise_lse", "mvae_gauss_pairwise_lse_workspace")


def test_latent_entry_points_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvae.h")).read(), flags=re.S)
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", header).group(1)) == 12 == L.ABI_VERSION
    lib = L.load()
    assert lib.mvae_abi_version() == 12
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert "moses_latent_diagnostics" in mv.__all__ and mv.moses_latent_diagnostics is mv.train.moses_latent_diagnostics
    assert callable(MV.VAE.iw_log_likelihood)
    assert all(callable(getattr(ops, n)) for n in ("gauss_iw_draw", "group_logmeanexp", "gauss_pairwise_lse"))
    build = open(os.path.join(ROOT, "molecular-vae_amd", "csrc", "build.sh")).read()
    assert build.count("conv latent capi; do") == 2 and "build/latent.o" in build and "build/tune/latent.o" in build


def test_latent_entry_points_refuse_bad_arguments_before_launching():
    """Everything below returns before any HIP call (no device needed)."""
    lib = L.load()
    fake = ctypes.c_void_p(256)                                  # never dereferenced: every call below is refused first

    def draw(B=4, K=3, dz=8, ld=8, mu=fake, lv=fake, z=fake, w=fake):
        return lib.mvae_gauss_iw_draw(B, K, dz, mu, lv, ld, None, 1, 0, z, w, None)
    assert draw(B=0) == -1 and draw(K=0) == -1 and draw(dz=0) == -1 and draw(ld=7) == -1
    assert draw(mu=None) == -1 and draw(lv=None) == -1 and draw(z=None) == -1 and draw(w=None) == -1

    def lme(G=4, K=3, a=fake, o1=fake, o2=fake):
        return lib.mvae_group_logmeanexp(G, K, a, None, o1, o2, None)
    assert lme(G=0) == -1 and lme(K=0) == -1 and lme(a=None) == -1 and lme(o1=None) == -1 and lme(o2=None) == -1

    def pw(Nz=300, Nx=4099, dz=160, ldz=160, ldp=160, z=fake, mu=fake, lv=fake, out=fake, ws=None, nb=0):
        return lib.mvae_gauss_pairwise_lse(Nz, Nx, dz, z, ldz, mu, lv, ldp, out, ws, nb, None)
    assert pw(Nz=0) == -1 and pw(Nx=0) == -1 and pw(dz=0) == -1 and pw(ldz=159) == -1 and pw(ldp=159) == -1
    assert pw(z=None) == -1 and pw(mu=None) == -1 and pw(lv=None) == -1 and pw(out=None) == -1
    assert pw(dz=193, ldz=200, ldp=200) == -3                      # the z row lives in registers: d_z <= 192
    need = lib.mvae_gauss_pairwise_lse_workspace(300, 4099, 160)
    assert need > 0 and pw() == -2 and pw(ws=fake, nb=need - 1) == -2 and pw(ws=ctypes.c_void_p(260), nb=need) == -1
    assert lib.mvae_gauss_pairwise_lse_workspace(0, 10, 4) == 0 and lib.mvae_gauss_pairwise_lse_workspace(1, 1, 1) == 0


def test_iw_log_likelihood_refuses_bad_arguments():
    torch.manual_seed(0)
    model = MV.VAE(VC.OneHotVocab(list("abc")), dtype=torch.float32)
    with pytest.raises(ValueError, match="n_samples"):
        model.iw_log_likelihood(["ab", "c"], n_samples=0)
    with pytest.raises(ValueError, match="eps must be"):
        model.iw_log_likelihood(["ab", "c"], n_samples=3, eps=torch.zeros(2, 2, model.d_z))
    with pytest.raises(L.MvaeError, match="MI355X only"):                     # a CPU model: no fallback
        model.iw_log_likelihood(["ab", "c"], n_samples=3)


def test_reference_single_draw_is_the_log_weight():
    """K = 1: log p_1(x) = elbo_1 = log w, and log w is log p(x|z) + log N(z; 0, I) - log N(z; mu, sigma^2) written out."""
    rs = np.random.RandomState(3)
    mu, lv, eps = rs.standard_normal((5, 7)), rs.uniform(-3, 1, (5, 7)), rs.standard_normal((5, 1, 7))
    lpx = rs.standard_normal((5, 1)) * 10
    z, lg = LR.iw_draw(mu, lv, eps)
    direct = (-0.5 * np.sum(z[:, 0] ** 2, 1) - 3.5 * LR.LOG2PI) - (-0.5 * np.sum(eps[:, 0] ** 2 + lv, 1) - 3.5 * LR.LOG2PI)
    assert np.allclose(lg[:, 0], direct, rtol=1e-12, atol=1e-12)
    log_px, elbo = LR.iw_estimates(lpx + lg)
    assert np.allclose(log_px, (lpx + lg)[:, 0], rtol=0, atol=1e-12) and np.allclose(elbo, log_px, rtol=0, atol=1e-12)


def test_reference_iw_bound_is_above_the_elbo_and_tightens():
    rs = np.random.RandomState(4)
    logw = rs.standard_normal((6, 400)) * 3 - 20
    log_px, elbo = LR.iw_estimates(logw)
    assert (log_px >= elbo).all()
    assert np.allclose(LR.iw_estimates(np.repeat(logw[:, :1], 9, 1))[0], logw[:, 0])      # equal weights: no gap
    assert np.allclose(LR.logsumexp(np.full((2, 3), -np.inf)), -np.inf)


def test_reference_active_units_and_mi_on_constructed_codes():
    """mu varies in 3 of 6 dimensions (by 1, 0.2 and 0.11 in standard deviation: variance 1, 0.04, 0.0121) -> AU = 3; posteriors that
    ignore x (one shared mu / logvar): log q(z) is that one Gaussian's log-density, so MI is neg_entropy minus its mean over the draws."""
    rs = np.random.RandomState(5)
    N = 2000
    mu = np.zeros((N, 6))
    for d, sd in ((0, 1.0), (2, 0.2), (5, 0.11)):
        x = rs.standard_normal(N)
        mu[:, d] = sd * (x - x.mean()) / x.std(ddof=1)
    mu[:, 1] = 0.09 * rs.standard_normal(N) * 0.5
    assert LR.active_units(mu) == 3
    shared_mu, shared_lv = np.tile(rs.standard_normal(4), (50, 1)), np.tile(rs.uniform(-2, 0, 4), (50, 1))
    z, _ = LR.iw_draw(shared_mu, shared_lv, rs.standard_normal((50, 1, 4)))
    lv = shared_lv[0]
    logq = -0.5 * np.sum((z[:, 0] - shared_mu[0]) ** 2 / np.exp(lv), 1) - 0.5 * lv.sum() - 2 * LR.LOG2PI
    neg_entropy = -2 * LR.LOG2PI - 0.5 * np.sum(1 + lv)
    assert abs(LR.mutual_info(shared_mu, shared_lv, z[:, 0]) - (neg_entropy - logq.mean())) < 1e-12
    lse, top = LR.pairwise_lse(z[:, 0], shared_mu, shared_lv)
    assert np.allclose(lse, logq + np.log(50)) and np.allclose(top, logq)


def test_active_units_uses_the_sample_variance_and_the_0_01_threshold():
    """N = 21 rows; sample variances (N - 1) of 0.01029 (population 0.0098), 0.0099, 0.0101 (population 0.00962) and 0: the sample
    variance makes dimensions 0 and 2 active, a population variance would make none, and the threshold sits between 0.0099 and 0.0101."""
    rs = np.random.RandomState(9)
    N = 21
    mu = np.zeros((N, 4))
    for d, var in ((0, 0.0098 * N / (N - 1)), (1, 0.0099), (2, 0.0101)):
        x = rs.standard_normal(N)
        mu[:, d] = np.sqrt(var) * (x - x.mean()) / x.std(ddof=1)
    assert LR.active_units(mu) == 2 and int(mv.train.active_units(torch.from_numpy(mu).float())) == 2
    assert int(mv.train.active_units(torch.from_numpy(mu[:1]))) == 0
