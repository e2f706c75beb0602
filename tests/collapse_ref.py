"""float64 reference of the posterior-collapse remedies of mosesvae.VAE: the token-dropout rule, the free-bits
value with its analytic gradient, and the full model's forward and gradients with separate decoder input tokens, injected inter-layer
dropout masks and free bits.  The full model is built from oracle.np_oracle's GRU layer (gru_layer_fwd / gru_layer_bwd); with the remedies
off it must reproduce np_oracle.moses_forward (tests/test_collapse_host.py pins that to 1e-10)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import np_oracle as O          # noqa: E402


# ------------------------------------------------------------------------------------------------ token dropout
def keep_hash(seed, B, T, p):
    """keep[b, t] = mvae_dropout_keep(seed, b * T + t, p): the counter hash at the flat position of the padded batch (bool [B, T])."""
    M = np.uint64(0xFFFFFFFF)
    idx = np.arange(B * T, dtype=np.uint64) & M
    h = ((idx * np.uint64(0x9E3779B1)) & M) ^ np.uint64(int(seed) & 0xFFFFFFFF)
    h ^= h >> np.uint64(16); h = (h * np.uint64(0x85EBCA6B)) & M
    h ^= h >> np.uint64(13); h = (h * np.uint64(0xC2B2AE35)) & M
    h ^= h >> np.uint64(16)
    return (h >= np.uint64(int(float(np.float32(p)) * 4294967296.0))).reshape(B, T)


def eligible(lengths, T):
    """bool [B, T]: 1 <= t <= lengths[b] - 2 -- never <bos>, the last input token (<eos>) or padding."""
    t = np.arange(T)[None, :]
    return (t >= 1) & (t <= np.asarray(lengths)[:, None] - 2)


def token_dropout(x, lengths, unk, keep):
    """x int64 [B, T], keep bool-like [B, T] -> (x_out, number of replaced positions)."""
    x = np.asarray(x)
    rep = eligible(lengths, x.shape[1]) & ~(np.asarray(keep) != 0)
    return np.where(rep, unk, x).astype(np.int64), int(rep.sum())


# ------------------------------------------------------------------------------------------------ free bits
def free_bits(mu, logvar, lam):
    """-> dict(kl_dim [dz] = m_j, obj = sum_j max(m_j, lam), kl = sum_j m_j, gate [dz] = m_j >= lam) in float64."""
    mu, lv = np.asarray(mu, np.float64), np.asarray(logvar, np.float64)
    m = (0.5 * (np.expm1(lv) - lv + mu * mu)).mean(0)          # exp(lv) + mu^2 - 1 - lv without the cancellation
    return dict(kl_dim=m, obj=float(np.maximum(m, lam).sum()), kl=float(m.sum()), gate=m >= lam)


def free_bits_grads(mu, logvar, eps, lam, dz=None, dkl=1.0, dlv_ext=None):
    """Analytic gradient of  <dz, mu + exp(lv / 2) eps> + dkl * obj + <dlv_ext, lv>  w.r.t. (mu, lv), plus the sums of the magnitudes of the
    terms of each element (the scale a fp32 evaluation's rounding error is measured against)."""
    mu, lv, eps = (np.asarray(a, np.float64) for a in (mu, logvar, eps))
    B = mu.shape[0]
    g = free_bits(mu, lv, lam)["gate"][None, :] * float(dkl)
    dz = np.zeros_like(mu) if dz is None else np.asarray(dz, np.float64)
    ext = np.zeros_like(mu) if dlv_ext is None else np.asarray(dlv_ext, np.float64)
    t_mu = (dz, g * mu / B)
    t_lv = (dz * eps * 0.5 * np.exp(lv / 2), g * 0.5 * np.exp(lv) / B, -g * 0.5 / B * np.ones_like(lv), ext)
    return dict(dmu=sum(t_mu), dlogvar=sum(t_lv), mag_mu=sum(np.abs(t) for t in t_mu), mag_lv=sum(np.abs(t) for t in t_lv))


# ------------------------------------------------------------------------------------------------ the full model
def moses_forward(p, seqs, eps, pad, x_in=None, lam=0.0, n_dec_layers=3, z_override=None, drop_masks=None, drop_p=0.0):
    """np_oracle.moses_forward with the two remedies: x_in [B, T] (None: the clean batch) are the tokens the DECODER reads -- the encoder
    and the cross-entropy targets keep the clean ones -- and lam > 0 makes `kl` the free-bits objective (`kl_true` is the KL, `kl_dim` its
    per-dimension batch means) with the gate in the gradient.  Returns dict(kl, kl_true, kl_dim, recon, mu, logvar, z, y, x_pad, grads_for)."""
    E = p["x_emb.weight"]
    dt = E.dtype
    B = len(seqs)
    lengths = np.array([len(s) for s in seqs])
    T = int(lengths.max())
    x_pad = np.full((B, T), pad, np.int64)
    for b, s in enumerate(seqs):
        x_pad[b, :len(s)] = s
    x_dec = x_pad if x_in is None else np.asarray(x_in, np.int64)
    assert x_dec.shape == x_pad.shape
    xe = np.ascontiguousarray(E[x_pad].transpose(1, 0, 2))              # [T, B, V]: what the encoder reads
    xd = np.ascontiguousarray(E[x_dec].transpose(1, 0, 2))              # what the decoder reads
    Hq = p["encoder_rnn.weight_hh_l0"].shape[1]
    _, hq, qc = O.gru_layer_fwd(xe, lengths, p["encoder_rnn.weight_ih_l0"], p["encoder_rnn.weight_hh_l0"],
                                p["encoder_rnn.bias_ih_l0"], p["encoder_rnn.bias_hh_l0"], np.zeros((B, Hq), dt))
    m1 = O.linear(hq, p["q_mu.0.weight"], p["q_mu.0.bias"]); m1r = np.maximum(m1, 0)
    mu = O.linear(m1r, p["q_mu.2.weight"], p["q_mu.2.bias"])
    l1 = O.linear(hq, p["q_logvar.0.weight"], p["q_logvar.0.bias"]); l1r = np.maximum(l1, 0)
    logvar = O.linear(l1r, p["q_logvar.2.weight"], p["q_logvar.2.bias"])
    z = mu + np.exp(logvar / 2.0) * eps
    if z_override is not None:
        z = np.asarray(z_override, dt)
    kl_dim = (0.5 * (np.exp(logvar) + mu ** 2 - 1.0 - logvar)).mean(0)
    kl_true = 0.5 * (np.exp(logvar) + mu ** 2 - 1.0 - logvar).sum(1).mean()
    gate = kl_dim >= lam if lam > 0 else np.ones_like(kl_dim, bool)
    kl = np.maximum(kl_dim, lam).sum() if lam > 0 else kl_true
    dz_ = z.shape[1]
    xin = np.concatenate([xd, np.broadcast_to(z[None], (T, B, dz_))], 2)
    h0 = O.linear(z, p["decoder_lat.weight"], p["decoder_lat.bias"])
    layer_in = xin
    dcaches = []
    keep = [None] * n_dec_layers
    for l in range(n_dec_layers):
        layer_in, _, c = O.gru_layer_fwd(layer_in, lengths, p[f"decoder_rnn.weight_ih_l{l}"], p[f"decoder_rnn.weight_hh_l{l}"],
                                         p[f"decoder_rnn.bias_ih_l{l}"], p[f"decoder_rnn.bias_hh_l{l}"], h0)
        dcaches.append(c)
        if drop_masks is not None and l + 1 < n_dec_layers:
            keep[l] = np.asarray(drop_masks[l], dt) / (1.0 - drop_p)
            layer_in = layer_in * keep[l]
    out = layer_in
    y_tb = O.linear(out.reshape(T * B, -1), p["decoder_fc.weight"], p["decoder_fc.bias"]).reshape(T, B, -1)
    y = np.ascontiguousarray(y_tb.transpose(1, 0, 2))
    logits = y[:, :-1]
    tgt = x_pad[:, 1:]                                                   # the CLEAN tokens are predicted
    msk = tgt != pad
    mx = logits.max(-1, keepdims=True)
    lse = mx[..., 0] + np.log(np.exp(logits - mx).sum(-1))
    nll = lse - np.take_along_axis(logits, tgt[..., None], -1)[..., 0]
    ntok = msk.sum()
    recon = (nll * msk).sum() / ntok
    res = dict(kl=kl, kl_true=kl_true, kl_dim=kl_dim, recon=recon, mu=mu, logvar=logvar, z=z, y=y, x_pad=x_pad, x_in=x_dec)

    def grads_for(kl_w):
        g = {}
        sm = np.exp(logits - lse[..., None])
        dl = sm.copy()
        np.put_along_axis(dl, tgt[..., None], np.take_along_axis(dl, tgt[..., None], -1) - 1.0, -1)
        dl = dl * msk[..., None] / ntok
        dy_b = np.zeros_like(y); dy_b[:, :-1] = dl
        dy_tb = np.ascontiguousarray(dy_b.transpose(1, 0, 2)).reshape(T * B, -1)
        g["decoder_fc.weight"] = dy_tb.T @ out.reshape(T * B, -1)
        g["decoder_fc.bias"] = dy_tb.sum(0)
        dout = (dy_tb @ p["decoder_fc.weight"]).reshape(T, B, -1)
        dh0 = np.zeros_like(h0)
        for l in range(n_dec_layers - 1, -1, -1):
            if keep[l] is not None:
                dout = dout * keep[l]
            dout, dh0_l, dwi, dwh, dbi, dbh = O.gru_layer_bwd(dout, np.zeros_like(h0), dcaches[l])
            g[f"decoder_rnn.weight_ih_l{l}"], g[f"decoder_rnn.weight_hh_l{l}"] = dwi, dwh
            g[f"decoder_rnn.bias_ih_l{l}"], g[f"decoder_rnn.bias_hh_l{l}"] = dbi, dbh
            dh0 += dh0_l
        V = E.shape[1]
        dxe = dout[:, :, :V].copy()
        dz = dout[:, :, V:].sum(0)
        g["decoder_lat.weight"] = dh0.T @ z
        g["decoder_lat.bias"] = dh0.sum(0)
        dz = dz + dh0 @ p["decoder_lat.weight"]
        g["_dz"] = dz.copy()
        gk = kl_w * gate[None, :]                                        # d max(m_j, lam) / d m_j = [m_j >= lam]
        dmu = dz + gk * mu / B
        dlogvar = dz * eps * 0.5 * np.exp(logvar / 2.0) + gk * 0.5 * (np.exp(logvar) - 1.0) / B
        g["q_mu.2.weight"] = dmu.T @ m1r; g["q_mu.2.bias"] = dmu.sum(0)
        dm1 = (dmu @ p["q_mu.2.weight"]) * (m1 > 0)
        g["q_mu.0.weight"] = dm1.T @ hq; g["q_mu.0.bias"] = dm1.sum(0)
        g["q_logvar.2.weight"] = dlogvar.T @ l1r; g["q_logvar.2.bias"] = dlogvar.sum(0)
        dl1 = (dlogvar @ p["q_logvar.2.weight"]) * (l1 > 0)
        g["q_logvar.0.weight"] = dl1.T @ hq; g["q_logvar.0.bias"] = dl1.sum(0)
        dhq = dm1 @ p["q_mu.0.weight"] + dl1 @ p["q_logvar.0.weight"]
        dxe2, _, dwi, dwh, dbi, dbh = O.gru_layer_bwd(np.zeros((T, B, Hq), dt), dhq, qc)
        g["encoder_rnn.weight_ih_l0"], g["encoder_rnn.weight_hh_l0"] = dwi, dwh
        g["encoder_rnn.bias_ih_l0"], g["encoder_rnn.bias_hh_l0"] = dbi, dbh
        d_dec, d_enc = np.zeros_like(E), np.zeros_like(E)
        np.add.at(d_dec, x_dec.T.reshape(-1), dxe.reshape(T * B, -1))   # the decoder's share lands on the rows it READ (<unk> included)
        np.add.at(d_enc, x_pad.T.reshape(-1), dxe2.reshape(T * B, -1))
        d_dec[pad] = 0.0; d_enc[pad] = 0.0
        g["x_emb.weight"] = d_dec + d_enc
        g["_x_emb_dec"], g["_x_emb_enc"] = d_dec, d_enc
        return g

    res["grads_for"] = grads_for
    return res


# ------------------------------------------------------------------------------------------------ inputs of the free-bits kernel tests
def fb_inputs(seed, B, dz):
    """(mu, logvar) fp32 [B, dz]: every third dimension nearly collapsed (scale 0.05 .. 0.25), the others in use (0.9 .. 1.4)."""
    rs = np.random.RandomState(seed)
    u = rs.uniform(0, 1, dz)
    scale = np.where(np.arange(dz) % 3 == 0, 0.05 + 0.2 * u, 0.9 + 0.5 * u)
    mu = (scale * rs.standard_normal((B, dz))).astype(np.float32)
    lv = (scale * rs.uniform(-1, 1, (B, dz))).astype(np.float32)
    return mu, lv


def fb_case(B, dz, lam=0.1, margin=0.02):
    """The first seed >= 1000 * B + dz whose float64 per-dimension means all keep a relative distance >= margin from lam, so that the
    gate of a fp32 evaluation cannot differ from the reference's.  -> (seed, mu, logvar)."""
    s = 1000 * B + dz
    while True:
        mu, lv = fb_inputs(s, B, dz)
        if (np.abs(free_bits(mu, lv, lam)["kl_dim"] - lam) / lam).min() >= margin:
            return s, mu, lv
        s += 1
