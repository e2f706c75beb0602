"""CPU tests of the posterior-collapse remedies of mosesvae.VAE (word dropout, free-bits KL, cyclical KL weight): the entry points are
declared, bound and exported at ABI 12, argument checks refuse before anything is launched, bad attributes raise on a CPU model, and the
float64 reference of tests/collapse_ref.py is itself pinned -- to np_oracle.moses_forward with the remedies off, to torch.clamp autograd
for free bits, to mvae_dropout_keep for the draw."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import molecular_vae_amd as mv
from molecular_vae_amd import _lib as L, mosesvae as MV, vocab as VC, ops
from oracle import np_oracle as O, initparams as ip
import collapse_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mvae_token_dropout", "mvae_moses_latent_fb_workspace", "mvae_moses_latent_fb_fwd", "mvae_moses_latent_fb_bwd")


def test_entry_points_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvae.h")).read(), flags=re.S)
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", header).group(1)) == 12 == L.ABI_VERSION
    lib = L.load()
    assert lib.mvae_abi_version() == 12
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert len(L.SIGNATURES["mvae_moses_latent_fb_fwd"][1]) == len(L.SIGNATURES["mvae_moses_latent_fwd"][1]) + 2      # free_bits, kl_dim
    assert len(L.SIGNATURES["mvae_moses_latent_fb_bwd"][1]) == len(L.SIGNATURES["mvae_moses_latent_bwd"][1]) + 2
    assert len(L.SIGNATURES["mvae_token_dropout"][1]) == 11
    for f in ("token_dropout", "moses_latent_fb_fwd", "moses_latent_fb_bwd"):
        assert callable(getattr(ops, f)), f
    assert "CyclicalKLAnnealer" in mv.__all__ and mv.CyclicalKLAnnealer is mv.train.CyclicalKLAnnealer


def test_entry_points_refuse_bad_arguments_before_launching():
    """Everything below returns before any HIP call (no device needed)."""
    lib = L.load()
    fake = ctypes.c_void_p(256)                                  # never dereferenced: every call below is refused first

    def drop(x=fake, lengths=fake, B=4, T=9, p=0.3, x_out=fake):
        return lib.mvae_token_dropout(x, lengths, B, T, 3, p, 1, None, x_out, None, None)
    for bad in (dict(p=1.0), dict(p=-0.1), dict(p=1.5), dict(p=float("nan")), dict(B=0), dict(T=0), dict(x=None), dict(lengths=None),
                dict(x_out=None)):
        assert drop(**bad) == -1, bad

    need = lib.mvae_moses_latent_fb_workspace(64, 160)
    assert need >= 2 * 160 * 4 and lib.mvae_moses_latent_fb_workspace(1, 1) >= 4

    def fwd(B=64, dz=160, mu=fake, lv=fake, eps=fake, eps_out=None, fb=0.1, z=fake, kl2=fake, kl_dim=fake, ws=fake, nb=need):
        return lib.mvae_moses_latent_fb_fwd(B, dz, mu, lv, eps, 0, 0, eps_out, fb, z, kl2, kl_dim, ws, nb, None)
    for bad in (dict(fb=-0.1), dict(fb=float("nan")), dict(B=0), dict(dz=0), dict(mu=None), dict(lv=None), dict(eps=None), dict(z=None),
                dict(kl2=None), dict(kl_dim=None), dict(fb=-1.0, nb=0)):
        assert fwd(**bad) == -1, bad
    assert fwd(nb=need - 1) == -2 and fwd(ws=None) == -2 and fwd(nb=0) == -2

    def bwd(B=64, dz=160, mu=fake, kl_dim=fake, fb=0.1, dmu=fake):
        return lib.mvae_moses_latent_fb_bwd(B, dz, mu, fake, fake, fake, fake, None, kl_dim, fb, dmu, fake, None)
    for bad in (dict(fb=-0.1), dict(fb=float("nan")), dict(B=0), dict(dz=0), dict(mu=None), dict(kl_dim=None), dict(dmu=None)):
        assert bwd(**bad) == -1, bad


def _cpu_model():
    torch.manual_seed(0)
    return MV.VAE(VC.OneHotVocab(list("abc")), dtype=torch.float32)              # V = 7 (3 symbols + 4 specials)


def test_bad_attributes_raise_on_a_cpu_model_and_the_defaults_are_off():
    model = _cpu_model()
    assert model.word_dropout == 0.0 and model.free_bits == 0.0
    assert model.last_word_seed is None and model.last_kl is None and model.last_kl_per_dim is None
    assert not any("word_dropout" in k or "free_bits" in k or "last_kl" in k for k in model.state_dict())
    x = [model.string2tensor("abca", device="cpu"), model.string2tensor("ab", device="cpu")]
    z = torch.zeros(2, model.d_z)
    for mode in (model.train, model.eval):                       # validated whenever used, whatever the mode
        mode()
        for bad in (1.0, -0.1, 2.0, float("nan"), float("inf")):
            model.word_dropout = bad
            for call in (lambda: model(x), lambda: model.forward_decoder(x, z), lambda: model.forward_encoder(x)):
                with pytest.raises(ValueError, match="word_dropout"):
                    call()
        model.word_dropout = 0.0
        for bad in (-0.5, float("nan"), float("inf")):
            model.free_bits = bad
            for call in (lambda: model(x), lambda: model.forward_encoder(x), lambda: model.forward_decoder(x, z)):
                with pytest.raises(ValueError, match="free_bits"):
                    call()
        model.free_bits = 0.0
    model.train()
    model.word_dropout, model.free_bits = 0.3, 0.1
    with pytest.raises(L.MvaeError, match="MI355X only"):        # valid attributes: a CPU model still has no fallback
        model(x)
    with pytest.raises(L.MvaeError, match="MI355X only"):
        model.forward_decoder(x, z)


# ---------------------------------------------------------------------------------------------- the reference is pinned
def _g3(golden_dir):
    g = np.load(os.path.join(golden_dir, "g3_moses.npz"))
    V = int(g["V"])
    p64 = {k: v.astype(np.float64) for k, v in ip.init_params(ip.moses_shapes(V), 303, 1.5, np.float32).items()}
    return g, p64, [g[f"seq{b}"] for b in range(6)]


def test_reference_with_the_remedies_off_is_the_oracle_on_the_g3_fixture(golden_dir):
    g, p64, seqs = _g3(golden_dir)
    pad, kl_w = int(g["pad"]), float(g["kl_w"])
    want = O.moses_forward(p64, seqs, g["eps"].astype(np.float64), pad)
    got = CR.moses_forward(p64, seqs, g["eps"].astype(np.float64), pad, x_in=None, lam=0.0)
    close = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-10 * max(1.0, np.abs(np.asarray(b)).max())
    assert close(got["kl"], want["kl"]) and close(got["kl_true"], want["kl"]) and close(got["recon"], want["recon"])
    assert close(kl_w * got["kl"] + got["recon"], kl_w * want["kl"] + want["recon"])
    assert close(got["kl_dim"].sum(), want["kl"])
    for k in ("y", "z", "mu", "logvar"):
        assert close(got[k], want[k]), k
    assert (got["x_pad"] == want["x_pad"]).all() and (got["x_in"] == want["x_pad"]).all()
    gg, wg = got["grads_for"](kl_w), want["grads_for"](kl_w)
    assert set(wg) <= set(gg)
    for k in wg:
        assert close(gg[k], wg[k]), k
    # the same with an x_in that equals the clean batch, and with dropout masks handed through
    T, B = want["x_pad"].shape[1], 6
    masks = (np.random.RandomState(1).uniform(size=(2, T, B, 512)) >= 0.2).astype(np.uint8)
    want = O.moses_forward(p64, seqs, g["eps"].astype(np.float64), pad, drop_masks=[masks[0], masks[1]], drop_p=0.2)
    got = CR.moses_forward(p64, seqs, g["eps"].astype(np.float64), pad, x_in=want["x_pad"], drop_masks=[masks[0], masks[1]], drop_p=0.2)
    assert close(got["recon"], want["recon"]) and close(got["y"], want["y"])
    gg, wg = got["grads_for"](kl_w), want["grads_for"](kl_w)
    for k in wg:
        assert close(gg[k], wg[k]), k


def test_reference_full_model_follows_the_remedies(golden_dir):
    """Word dropout moves the decoder's share of the embedding gradient to the <unk> row and leaves the encoder half alone; free bits
    changes kl and only the gated dimensions' KL gradient."""
    g, p64, seqs = _g3(golden_dir)
    pad, unk = int(g["pad"]), VC.OneHotVocab([chr(ord("a") + i) for i in range(26)]).unk
    assert unk != pad and unk < int(g["V"])
    eps = g["eps"].astype(np.float64)
    base = CR.moses_forward(p64, seqs, eps, pad)
    x_pad = base["x_pad"]
    lens = [len(s) for s in seqs]
    keep = np.random.RandomState(4).uniform(size=x_pad.shape) >= 0.3
    x_in, n = CR.token_dropout(x_pad, lens, unk, keep)
    assert n > 0 and unk not in x_pad
    wd = CR.moses_forward(p64, seqs, eps, pad, x_in=x_in)
    assert wd["kl"] == base["kl"] and (wd["z"] == base["z"]).all() and wd["recon"] != base["recon"]
    gw, gb = wd["grads_for"](0.0), base["grads_for"](0.0)
    assert np.abs(gw["_x_emb_dec"][unk]).max() > 0 and np.abs(gb["_x_emb_dec"][unk]).max() == 0
    assert np.abs(gw["x_emb.weight"][pad]).max() == 0
    m = np.sort(base["kl_dim"])
    lam = float(0.5 * (m[79] + m[80]))
    fb = CR.moses_forward(p64, seqs, eps, pad, lam=lam)
    assert fb["kl_true"] == base["kl"] and fb["kl"] > base["kl"] and fb["recon"] == base["recon"]
    assert abs(fb["kl"] - (m[80:].sum() + 80 * lam)) < 1e-12 * fb["kl"]
    d1 = {k: fb["grads_for"](1.0)[k] - fb["grads_for"](0.0)[k] for k in ("q_mu.2.bias", "q_logvar.2.bias")}
    gate = base["kl_dim"] >= lam
    assert gate.sum() == 80 and (d1["q_mu.2.bias"][~gate] == 0).all() and (d1["q_logvar.2.bias"][~gate] == 0).all()
    assert (d1["q_mu.2.bias"][gate] != 0).all()


@pytest.mark.parametrize("B,dz,lam", [(1, 3, 0.1), (5, 7, 0.1), (64, 160, 0.1), (6, 160, 0.0)])
def test_free_bits_reference_equals_clamp_autograd(B, dz, lam):
    _, mu, lv = CR.fb_case(B, dz, lam) if lam > 0 else (0,) + CR.fb_inputs(7, B, dz)
    rs = np.random.RandomState(B)
    eps, dz_in, ext, dkl = rs.standard_normal((B, dz)), rs.standard_normal((B, dz)), rs.standard_normal((B, dz)) * 0.1, 0.7
    tm = torch.tensor(mu, dtype=torch.float64, requires_grad=True)
    tl = torch.tensor(lv, dtype=torch.float64, requires_grad=True)
    m = (0.5 * (tl.exp() + tm ** 2 - 1 - tl)).mean(0)
    obj = torch.clamp(m, min=lam).sum()
    z = tm + (tl / 2).exp() * torch.tensor(eps)
    ((z * torch.tensor(dz_in)).sum() + dkl * obj + (tl * torch.tensor(ext)).sum()).backward()
    ref = CR.free_bits(mu, lv, lam)
    assert np.allclose(ref["kl_dim"], m.detach().numpy(), rtol=1e-12, atol=0)
    assert abs(ref["obj"] - float(obj.detach())) <= 1e-12 * float(obj.detach()) and abs(ref["kl"] - float(m.detach().sum())) <= 1e-12 * float(m.detach().sum())
    assert (ref["gate"] == (m.detach().numpy() >= lam)).all()
    if lam == 0.0:
        assert ref["gate"].all() and ref["obj"] == ref["kl"]                      # `>=`: nothing is gated at 0
    gr = CR.free_bits_grads(mu, lv, eps, lam, dz=dz_in, dkl=dkl, dlv_ext=ext)
    assert np.abs(gr["dmu"] - tm.grad.numpy()).max() <= 1e-12 * gr["mag_mu"].max()
    assert np.abs(gr["dlogvar"] - tl.grad.numpy()).max() <= 1e-12 * gr["mag_lv"].max()
    assert (gr["mag_mu"] >= np.abs(gr["dmu"]) - 1e-15).all() and (gr["mag_lv"] >= np.abs(gr["dlogvar"]) - 1e-15).all()


def test_free_bits_gate_is_greater_or_equal():
    mu = np.zeros((2, 2)); lv = np.zeros((2, 2))
    mu[:, 0] = 0.5                                              # m_0 = 0.5 * 0.25 = 0.125 exactly, m_1 = 0
    ref = CR.free_bits(mu, lv, 0.125)
    assert ref["kl_dim"][0] == 0.125 and ref["gate"].tolist() == [True, False] and ref["obj"] == 0.25 and ref["kl"] == 0.125
    g = CR.free_bits_grads(mu, lv, np.zeros((2, 2)), 0.125)
    assert (g["dmu"][:, 0] == 0.25).all() and (g["dmu"][:, 1] == 0).all()       # the dimension AT the threshold keeps its gradient


def test_token_dropout_reference_rule_and_hash():
    lib = L.load()
    B, T, p, seed = 5, 9, 0.3, 77
    keep = CR.keep_hash(seed, B, T, p)
    for b in range(B):
        for t in range(T):
            assert bool(keep[b, t]) == bool(lib.mvae_dropout_keep(seed, b * T + t, p)), (b, t)
    assert (keep == ops.dropout_keep_mask(seed, (B, T), p).astype(bool)).all()
    big = CR.keep_hash(12345, 64, 66, 0.5)
    for i in (0, 1, 65, 66, 4000, 64 * 66 - 1):
        assert bool(big.flat[i]) == bool(lib.mvae_dropout_keep(12345, i, 0.5))
    lens = [9, 7, 3, 2, 2]
    x = np.arange(B * T).reshape(B, T) + 100
    out, n = CR.token_dropout(x, lens, 3, np.zeros((B, T), bool))          # nothing kept: every eligible position goes
    assert n == 7 + 5 + 1 and (out[0, 1:8] == 3).all() and out[0, 0] == 100 and out[0, 8] == 108
    assert (out[1, 1:6] == 3).all() and (out[1, 6:] == x[1, 6:]).all() and out[2, 1] == 3 and (out[3:] == x[3:]).all()
    out, n = CR.token_dropout(x, lens, 3, np.ones((B, T), bool))
    assert n == 0 and (out == x).all()
    out, n = CR.token_dropout(x, lens, 3, keep)
    assert n == int((CR.eligible(lens, T) & ~keep).sum()) and ((out == 3) == (CR.eligible(lens, T) & ~keep)).all()
    assert not CR.eligible([2], 2).any() and CR.eligible([3], 3).tolist() == [[False, True, False]]


@pytest.mark.parametrize("seed", [1, 2, 3, 12345])
@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_replaced_share_follows_p(seed, p):
    B, T = 64, 66
    x = np.full((B, T), 9, np.int64)
    out, n = CR.token_dropout(x, [T] * B, 3, CR.keep_hash(seed, B, T, p))
    assert CR.eligible([T] * B, T).sum() == 4096 and n == int((out == 3).sum())
    assert abs(n / 4096 - p) <= 5 * math.sqrt(p * (1 - p) / 4096), (n / 4096, p)


def test_cyclical_kl_annealer():
    a = mv.CyclicalKLAnnealer(100, ratio=0.5, w_max=1.0)
    assert a(0) == 0.0 and a(25) == 0.5 and a(50) == 1.0 and a(75) == 1.0 and a(99) == 1.0
    assert a(100) == 0.0 and a(125) == 0.5 and a(150) == 1.0 and a(1000) == 0.0 and a(1049) == 0.98
    b = mv.CyclicalKLAnnealer(10, ratio=0.2, w_max=0.5)
    assert [b(i) for i in range(12)] == [0.0, 0.25, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.0, 0.25]
    c = mv.CyclicalKLAnnealer(4, ratio=1.0)
    assert [c(i) for i in range(5)] == [0.0, 0.25, 0.5, 0.75, 0.0]
    assert mv.CyclicalKLAnnealer(8)(2) == 0.5                          # ratio defaults to 0.5, w_max to 1
    for bad in (dict(n_steps_per_cycle=0), dict(n_steps_per_cycle=10, ratio=0.0), dict(n_steps_per_cycle=10, ratio=1.5)):
        with pytest.raises(ValueError):
            mv.CyclicalKLAnnealer(**bad)
