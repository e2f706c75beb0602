"""GPU tests (-m gpu) of the posterior-collapse remedies of mosesvae.VAE: the token-dropout and free-bits kernels
against the float64 rules of tests/collapse_ref.py at their edge shapes, the model in train mode against the float64 full-model reference
(g3 fixture, f32 and bf16; the B = 40 ragged bf16 model with inter-layer and word dropout together), the device draw against its host
restatement, and the default / eval paths, which must launch nothing new and change nothing."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

import collapse_ref as CR          # noqa: E402

if torch.cuda.is_available():
    from gpu_helpers import ip, mv, rel
    from molecular_vae_amd import ops, mosesvae as MV, vocab as VC
    from test_gpu_parity import _moses_base, _moses_setup
    dev = torch.device("cuda", 0)

LAM = 0.1


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype)


# ---------------------------------------------------------------------------------------------- mvae_token_dropout
def _ragged(B, T, seed):
    """lengths sorted descending in [2, T], the first = T, the last two = 2 when there is room."""
    rs = np.random.RandomState(seed)
    lens = sorted(rs.randint(2, T + 1, size=B).tolist(), reverse=True)
    lens[0] = T
    if B >= 3:
        lens[-1] = lens[-2] = 2
    return lens


@pytest.mark.parametrize("B,T", [(1, 3), (1, 2), (5, 9), (64, 66), (257, 61)])
def test_token_dropout_kernel_equals_the_rule(B, T):
    rs = np.random.RandomState(100 * B + T)
    lens = _ragged(B, T, B + T)
    unk, pad = 29, 28
    x = rs.randint(0, 26, size=(B, T)).astype(np.int64)
    for b, n in enumerate(lens):
        x[b, n:] = pad
    tx, tl = _t(x), _t(np.array(lens, np.int32))
    n_dev = torch.full((1,), -7, dtype=torch.int32, device=dev)
    for p, seed in ((0.3, 11), (0.5, 12345), (0.9, 3)):                      # the device draw
        out = torch.full_like(tx, -1)
        ops.token_dropout(tx, tl, out, B, T, unk, p, seed=seed, n_dropped=n_dev)
        want, n = CR.token_dropout(x, lens, unk, CR.keep_hash(seed, B, T, p))
        assert (out.cpu().numpy() == want).all() and int(n_dev) == n, (p, seed)
        assert (CR.keep_hash(seed, B, T, p) == ops.dropout_keep_mask(seed, (B, T), p).astype(bool)).all()
    if T == 2:
        assert n == 0 and (want == x).all()                                   # nothing is eligible
    for q in (0.3, 1.0, 0.0):                                                 # an injected mask (1 = keep); p plays no part
        keep = (rs.uniform(size=(B, T)) >= q).astype(np.uint8)
        out = torch.full_like(tx, -1)
        ops.token_dropout(tx, tl, out, B, T, unk, 0.3, seed=5, keep_mask=_t(keep), n_dropped=n_dev)
        want, n = CR.token_dropout(x, lens, unk, keep)
        assert (out.cpu().numpy() == want).all() and int(n_dev) == n, q
    out = torch.full_like(tx, -1)
    ops.token_dropout(tx, tl, out, B, T, unk, 0.0, seed=9, n_dropped=n_dev)   # p = 0: x unchanged
    assert torch.equal(out, tx) and int(n_dev) == 0
    out2 = torch.full_like(tx, -1)
    ops.token_dropout(tx, tl, out2, B, T, unk, 0.0, seed=9)                   # n_dropped is optional
    assert torch.equal(out2, tx)


# ---------------------------------------------------------------------------------------------- mvae_moses_latent_fb_*
def _fb_run(mu, lv, eps, lam, seed=0, offset=0):
    B, dz = mu.shape
    z, kl2, kl_dim = torch.empty(B, dz, device=dev), torch.empty(2, device=dev), torch.empty(dz, device=dev)
    eps_out = torch.empty(B, dz, device=dev) if eps is None else None
    ops.moses_latent_fb_fwd(mu, lv, eps, z, kl2, kl_dim, B, dz, lam, seed=seed, offset=offset, eps_out=eps_out)
    return z, kl2, kl_dim, eps_out


@pytest.mark.parametrize("dz", [1, 2, 160, 161])
@pytest.mark.parametrize("B", [1, 5, 64, 257, 1024])
def test_free_bits_kernels_equal_the_float64_rule(B, dz):
    """Tolerances: kl_dim, kl2[0], kl2[1] within 2e-5 relative of float64 (non-negative terms: any fp32 order over n <= 1024 of them errs
    below n * 2^-24 ~ 6e-5 in the worst case, ~2e-6 typically; a dropped row is 1e-3 at B = 1024); dmu / dlogvar within 1e-5 of the sum
    of the magnitudes of their terms; z bitwise mvae_moses_latent_fwd's; the gate exact (the inputs keep every m_j 2 % away from lambda)."""
    s, mu, lv = CR.fb_case(B, dz, LAM)
    ref = CR.free_bits(mu, lv, LAM)
    assert (np.abs(ref["kl_dim"] - LAM) / LAM).min() >= 0.02
    if dz >= 160:
        assert 0.1 <= ref["gate"].mean() <= 0.9
    rs = np.random.RandomState(s)
    eps, dz_in, ext = (rs.standard_normal((B, dz)).astype(np.float32) for _ in range(3))
    ext *= 0.1
    tmu, tlv, teps = _t(mu), _t(lv), _t(eps)
    for e, seed, off in ((teps, 0, 0), (None, 1234, 77 + (1 << 33))):          # injected and device-drawn noise
        z0, kl0 = torch.empty(B, dz, device=dev), torch.empty(1, device=dev)
        e0 = torch.empty(B, dz, device=dev) if e is None else None
        ops.moses_latent_fwd(tmu, tlv, e, z0, kl0, B, dz, seed=seed, offset=off, eps_out=e0)
        z, kl2, kl_dim, e1 = _fb_run(tmu, tlv, e, LAM, seed, off)
        assert torch.equal(z, z0)
        if e is None:
            assert torch.equal(e1, e0)
        got = kl_dim.cpu().numpy().astype(np.float64)
        err = np.abs(got - ref["kl_dim"]) / ref["kl_dim"]
        print(f"B={B} dz={dz}: kl_dim rel err max {err.max():.2e}, obj {abs(float(kl2[0]) - ref['obj']) / ref['obj']:.2e}, "
              f"kl {abs(float(kl2[1]) - ref['kl']) / ref['kl']:.2e}")
        assert err.max() < 2e-5
        assert abs(float(kl2[0]) - ref["obj"]) < 2e-5 * ref["obj"] and abs(float(kl2[1]) - ref["kl"]) < 2e-5 * ref["kl"]
        assert ((got >= LAM) == ref["gate"]).all()
        z_b, kl2_b, kl_dim_b, _ = _fb_run(tmu, tlv, e, LAM, seed, off)         # two calls, the same bits
        assert torch.equal(z_b, z) and torch.equal(kl2_b, kl2) and torch.equal(kl_dim_b, kl_dim)
    # backward (with the kl_dim of the last forward and the injected eps)
    dkl = torch.tensor([0.7], device=dev)
    dmu, dlv = torch.empty(B, dz, device=dev), torch.empty(B, dz, device=dev)
    ops.moses_latent_fb_bwd(tmu, tlv, teps, _t(dz_in), dkl, _t(ext), kl_dim, LAM, dmu, dlv, B, dz)
    gr = CR.free_bits_grads(mu, lv, eps, LAM, dz=dz_in, dkl=float(np.float32(0.7)), dlv_ext=ext)
    e_mu = np.abs(dmu.cpu().numpy() - gr["dmu"]) / gr["mag_mu"]
    e_lv = np.abs(dlv.cpu().numpy() - gr["dlogvar"]) / gr["mag_lv"]
    print(f"B={B} dz={dz}: dmu err / magnitude max {e_mu.max():.2e}, dlogvar {e_lv.max():.2e}")
    assert e_mu.max() < 1e-5 and e_lv.max() < 1e-5
    off_cols = torch.from_numpy(~ref["gate"]).to(dev)
    assert torch.equal(dmu[:, off_cols], _t(dz_in)[:, off_cols])               # a gated dimension: no KL term at all
    if ref["gate"].any():
        on = torch.from_numpy(ref["gate"]).to(dev)
        assert not torch.equal(dmu[:, on], _t(dz_in)[:, on])
    dmu_b, dlv_b = torch.empty_like(dmu), torch.empty_like(dlv)
    ops.moses_latent_fb_bwd(tmu, tlv, teps, _t(dz_in), dkl, _t(ext), kl_dim, LAM, dmu_b, dlv_b, B, dz)
    assert torch.equal(dmu_b, dmu) and torch.equal(dlv_b, dlv)
    # lambda = 0 gates nothing: the objective is the KL, the gradients are mvae_moses_latent_bwd's
    z, kl2, kl_dim, _ = _fb_run(tmu, tlv, teps, 0.0)
    assert float(kl2[0]) == float(kl2[1])
    ops.moses_latent_fb_bwd(tmu, tlv, teps, _t(dz_in), dkl, _t(ext), kl_dim, 0.0, dmu, dlv, B, dz)
    dmu0, dlv0 = torch.empty_like(dmu), torch.empty_like(dlv)
    ops.moses_latent_bwd(tmu, tlv, teps, _t(dz_in), dkl, _t(ext), dmu0, dlv0, B, dz)
    assert rel(dmu.cpu().numpy(), dmu0.cpu().numpy()) < 1e-6 and rel(dlv.cpu().numpy(), dlv0.cpu().numpy()) < 1e-6


# ---------------------------------------------------------------------------------------------- the model on the g3 fixture
P_WORD = 0.3


@functools.lru_cache(maxsize=None)
def _g3_ref(golden_dir, case):
    """The float64 reference of one case, computed once: (reference dict, its gradients at the fixture's kl_w, word mask | None, lambda)."""
    g = np.load(os.path.join(golden_dir, "g3_moses.npz"))
    p64 = {k: v.astype(np.float64) for k, v in ip.init_params(ip.moses_shapes(int(g["V"])), 303, 1.5, np.float32).items()}
    seqs = [g[f"seq{b}"] for b in range(6)]
    pad, unk, eps = int(g["pad"]), int(g["unk"]), g["eps"].astype(np.float64)
    mask, x_in, lam = None, None, 0.0
    base = CR.moses_forward(p64, seqs, eps, pad)
    if case in ("word", "both"):
        mask = (np.random.RandomState(31).uniform(size=base["x_pad"].shape) >= P_WORD).astype(np.uint8)
        x_in, n = CR.token_dropout(base["x_pad"], [len(s) for s in seqs], unk, mask)
        assert n >= 5
    if case in ("fb", "both"):
        m = np.sort(base["kl_dim"])                              # lambda: the centre of the widest gap among ranks 40 .. 120
        i = 40 + int(np.argmax(np.diff(m[40:121])))
        lam = float(0.5 * (m[i] + m[i + 1]))
        assert (m[i + 1] - m[i]) / 2 / lam >= 0.01
    ref = base if case == "off" else CR.moses_forward(p64, seqs, eps, pad, x_in=x_in, lam=lam)
    return ref, ref["grads_for"](float(g["kl_w"])), mask, lam


def _g3_model(golden_dir, dtype):
    g, model, _ = _moses_setup(golden_dir, dtype)
    model.train()
    model.d_dropout = 0.0
    return g, model, [torch.from_numpy(g[f"seq{b}"]) for b in range(6)], torch.from_numpy(g["eps"].astype(np.float32)).to(dev)


def _grads(model):
    return {k: p_.grad.detach().cpu().numpy() for k, p_ in model.named_parameters()}


@pytest.mark.parametrize("case", ["word", "fb", "both"])
@pytest.mark.parametrize("dtype,tl,tg", [(torch.float32, 2e-5, 5e-4), (torch.bfloat16, 5e-3, 6e-2)])
def test_model_in_train_mode_equals_the_float64_reference(golden_dir, dtype, tl, tg, case):
    """Train mode, d_dropout = 0: (a) an injected word mask at p = 0.3, (b) free bits with lambda in the widest gap of the reference's
    per-dimension KLs, (c) both.  Loss terms, logits, last_kl and every parameter gradient of kl_w * kl + recon at the tolerances of
    test_gpu_round4.py::test_forward_decoder_on_the_fixture_latent."""
    ref, rg, mask, lam = _g3_ref(golden_dir, case)
    g, model, seqs, eps = _g3_model(golden_dir, dtype)
    kl_w = float(g["kl_w"])
    if mask is not None:
        model.word_dropout = P_WORD
    model.free_bits = lam
    kl, recon, z, logvar, x, y = model(seqs, eps, word_mask=None if mask is None else torch.from_numpy(mask))
    assert (x.cpu().numpy() == g["x"]).all()                                   # the returned batch stays clean
    assert abs(float(kl) - ref["kl"]) < tl * abs(ref["kl"]) and abs(float(recon) - ref["recon"]) < tl * abs(ref["recon"])
    assert rel(z.detach().cpu().numpy(), ref["z"]) < tl and rel(logvar.detach().cpu().numpy(), ref["logvar"]) < tl
    assert rel(y.detach().cpu().numpy(), ref["y"]) < max(tl, 1e-5)
    if lam > 0:
        assert model.last_kl.device.type == "cuda" and not model.last_kl.requires_grad and model.last_kl.dim() == 0
        assert abs(float(model.last_kl) - ref["kl_true"]) < tl * ref["kl_true"]
        assert float(kl) > float(model.last_kl)
        kd = model.last_kl_per_dim
        assert tuple(kd.shape) == (model.d_z,) and kd.device.type == "cuda" and not kd.requires_grad
        # a single dimension's mean lacks the averaging over d_z = 160 roundings that the summed KL's tolerance tl counts on: sqrt(160) ~ 13
        assert rel(kd.cpu().numpy(), ref["kl_dim"]) < 13 * tl
        assert ((kd.cpu().numpy() >= lam) == (ref["kl_dim"] >= lam)).all()
    else:
        assert model.last_kl is None and model.last_kl_per_dim is None
        assert abs(float(kl) - ref["kl_true"]) < tl * ref["kl_true"]
    model.zero_grad(set_to_none=True)
    (kl_w * kl + recon).backward()
    torch.cuda.synchronize()
    got = _grads(model)
    bad = {k: rel(got[k], rg[k]) for k in got if rel(got[k], rg[k]) > tg}
    assert not bad, bad
    ge = got["x_emb.weight"]
    assert np.abs(ge[model.pad]).max() == 0
    if mask is not None:
        assert np.abs(ge[model.unk]).max() > 0                                 # <unk> was read by the decoder: its row has a gradient
    else:
        assert np.abs(ge[model.unk]).max() == 0


def test_halves_take_the_remedies_like_the_fused_forward(golden_dir):
    """forward_encoder (free bits) + forward_decoder (word mask) equal forward with both, losses and logits bitwise, gradients to 2e-5."""
    ref, rg, mask, lam = _g3_ref(golden_dir, "both")
    g, model, seqs, eps = _g3_model(golden_dir, torch.float32)
    kl_w = float(g["kl_w"])
    model.word_dropout, model.free_bits = P_WORD, lam
    tm = torch.from_numpy(mask)
    kl, recon, z, logvar, x, y = model(seqs, eps, word_mask=tm)
    true_kl, per_dim = model.last_kl.clone(), model.last_kl_per_dim.clone()
    model.zero_grad(set_to_none=True)
    (kl_w * kl + recon).backward()
    fused = _grads(model)
    z2, kl2, lv2 = model.forward_encoder(seqs, eps)
    assert torch.equal(model.last_kl, true_kl) and torch.equal(model.last_kl_per_dim, per_dim)
    recon2, x2, y2 = model.forward_decoder(seqs, z2, word_mask=tm)
    assert torch.equal(z2, z) and torch.equal(kl2, kl) and torch.equal(lv2, logvar) and torch.equal(x2, x)
    assert torch.equal(y2, y) and torch.equal(recon2, recon)
    model.zero_grad(set_to_none=True)
    (kl_w * kl2 + recon2).backward()
    torch.cuda.synchronize()
    got = _grads(model)
    bad = {k: rel(got[k], fused[k]) for k in got if rel(got[k], fused[k]) > 2e-5}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- B = 40, bf16, ragged, both dropouts
@functools.lru_cache(maxsize=None)
def _b40():
    v = VC.OneHotVocab([chr(ord("a") + i) for i in range(26)])
    params = ip.init_params(ip.moses_shapes(len(v)), 21, 1.0, np.float32)
    rs = np.random.RandomState(9)
    B = 40
    lens = sorted(rs.randint(10, 58, size=B).tolist(), reverse=True)
    seqs = [np.concatenate([[v.bos], rs.randint(0, 26, size=n), [v.eos]]).astype(np.int64) for n in lens]
    T = max(len(s) for s in seqs)
    eps = rs.standard_normal((B, 160)).astype(np.float32)
    dmask = (rs.uniform(size=(2, T, B, 512)) >= 0.2).astype(np.uint8)
    wmask = (rs.uniform(size=(B, T)) >= 0.3).astype(np.uint8)
    x_pad = np.full((B, T), v.pad, np.int64)
    for b, s in enumerate(seqs):
        x_pad[b, :len(s)] = s
    x_in, n = CR.token_dropout(x_pad, [len(s) for s in seqs], v.unk, wmask)
    assert n > 100
    ref = CR.moses_forward({k: a.astype(np.float64) for k, a in params.items()}, seqs, eps.astype(np.float64), v.pad, x_in=x_in,
                           drop_masks=[dmask[0], dmask[1]], drop_p=0.2)
    return v, params, seqs, eps, dmask, wmask, ref, ref["grads_for"](0.5)


@pytest.mark.parametrize("split", [False, True], ids=["forward", "encoder+decoder"])
def test_word_and_inter_layer_dropout_together_at_b40_bf16(split):
    """The B = 40 bf16 ragged model of test_forward_decoder_on_an_arbitrary_latent_vs_oracle with an injected inter-layer mask AND a word
    mask, at that test's tolerances (loss 5e-3, logits 2e-2, gradients 8e-2), through forward and through forward_encoder + forward_decoder."""
    v, params, seqs, eps, dmask, wmask, ref, rg = _b40()
    model = MV.VAE(v, dtype=torch.bfloat16)
    model.load_state_dict({k: torch.from_numpy(params[_moses_base(k)]) for k in model.state_dict()})
    model = model.to(dev).train()
    model.word_dropout = 0.3
    ts, teps = [torch.from_numpy(s) for s in seqs], torch.from_numpy(eps).to(dev)
    if split:
        z, kl, lv = model.forward_encoder(ts, teps)
        recon, x, y = model.forward_decoder(ts, z, drop_mask=torch.from_numpy(dmask), word_mask=torch.from_numpy(wmask))
    else:
        kl, recon, z, lv, x, y = model(ts, teps, drop_mask=torch.from_numpy(dmask), word_mask=torch.from_numpy(wmask))
    assert (x.cpu().numpy() == ref["x_pad"]).all()
    assert abs(float(recon) - ref["recon"]) < 5e-3 * abs(ref["recon"]) and abs(float(kl) - ref["kl"]) < 5e-3 * abs(ref["kl"])
    assert rel(y.detach().cpu().numpy(), ref["y"]) < 2e-2
    (0.5 * kl + recon).backward()
    torch.cuda.synchronize()
    got = _grads(model)
    bad = {k: rel(got[k], rg[k]) for k in got if rel(got[k], rg[k]) > 8e-2}
    assert not bad, bad
    assert np.abs(got["x_emb.weight"][v.unk]).max() > 0 and np.abs(got["x_emb.weight"][v.pad]).max() == 0


# ---------------------------------------------------------------------------------------------- the device draw
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_word_seed_equals_the_host_restatement_of_its_draw(golden_dir, dtype):
    g, model, seqs, eps = _g3_model(golden_dir, dtype)
    model.word_dropout = 0.5
    B, T = g["x"].shape
    seed = 2024
    outs = []
    for kw in (dict(word_seed=seed), dict(word_mask=torch.from_numpy(ops.dropout_keep_mask(seed, (B, T), 0.5)))):
        kl, recon, z, logvar, x, y = model(seqs, eps, **kw)
        assert model.last_word_seed == (seed if "word_seed" in kw else None)
        model.zero_grad(set_to_none=True)
        (0.5 * kl + recon).backward()
        torch.cuda.synchronize()
        outs.append(([t.detach().clone() for t in (kl, recon, z, logvar, x, y)], {k: p_.grad.clone() for k, p_ in model.named_parameters()}))
    for a, b in zip(outs[0][0], outs[1][0]):
        assert torch.equal(a, b)
    for k in outs[0][1]:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k
    want, n = CR.token_dropout(g["x"], [len(g[f"seq{b}"]) for b in range(6)], model.unk, CR.keep_hash(seed, B, T, 0.5))
    assert n > 0                                                              # (the draw did replace tokens)
    torch.manual_seed(77)
    _, recon_a, *_ = model(seqs, eps)                                         # neither given: a seed is drawn as drop_seed is, and recorded
    s = model.last_word_seed
    assert isinstance(s, int) and 0 <= s < 2 ** 31 - 1
    _, recon_b, *_ = model(seqs, eps, word_seed=s)
    assert torch.equal(recon_a, recon_b)
    torch.manual_seed(77)
    model(seqs, eps)
    assert model.last_word_seed == s


# ---------------------------------------------------------------------------------------------- defaults and eval mode
def _step(model, seqs, eps, **kw):
    kl, recon, z, logvar, x, y = model(seqs, eps, **kw)
    model.zero_grad(set_to_none=True)
    (0.5 * kl + recon).backward()
    torch.cuda.synchronize()
    return [t.detach().clone() for t in (kl, recon, z, logvar, x, y)], {k: p_.grad.clone() for k, p_ in model.named_parameters()}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_defaults_and_eval_mode_launch_nothing_new_and_change_nothing(golden_dir, dtype, monkeypatch):
    g, plain, _ = _moses_setup(golden_dir, dtype)                              # never has the attributes touched
    _, model, _ = _moses_setup(golden_dir, dtype)
    seqs = [torch.from_numpy(g[f"seq{b}"]) for b in range(6)]
    eps = torch.from_numpy(g["eps"].astype(np.float32)).to(dev)

    def boom(*a, **k):
        raise AssertionError("a collapse-remedy launch on the default / eval path")
    for name in ("token_dropout", "moses_latent_fb_fwd", "moses_latent_fb_bwd"):
        monkeypatch.setattr(ops, name, boom)
    plain.eval(); model.eval()
    model.word_dropout, model.free_bits = 0.5, 0.2                             # eval mode: both set, neither applied
    want, got = _step(plain, seqs, eps), _step(model, seqs, eps)
    assert model.last_kl is None and model.last_kl_per_dim is None
    for a, b in zip(want[0], got[0]):
        assert torch.equal(a, b)
    for k in want[1]:
        assert torch.equal(want[1][k], got[1][k]), k
    z_a, kl_a, _ = plain.forward_encoder(seqs, eps)
    z_b, kl_b, _ = model.forward_encoder(seqs, eps)
    r_a, _, y_a = plain.forward_decoder(seqs, z_a)
    r_b, _, y_b = model.forward_decoder(seqs, z_b)
    assert torch.equal(kl_a, kl_b) and torch.equal(r_a, r_b) and torch.equal(y_a, y_b)
    plain.train(); model.train()
    model.word_dropout, model.free_bits = 0.0, 0.0                             # train mode at the defaults (inter-layer dropout on)
    want, got = _step(plain, seqs, eps, drop_seed=5), _step(model, seqs, eps, drop_seed=5)
    assert model.last_word_seed is None and model.last_kl is None
    for a, b in zip(want[0], got[0]):
        assert torch.equal(a, b)
    for k in want[1]:
        assert torch.equal(want[1][k], got[1][k]), k


def test_scoring_and_decoding_never_corrupt_their_inputs(golden_dir, monkeypatch):
    g, model, seqs, eps = _g3_model(golden_dir, torch.float32)                # train mode
    z = torch.from_numpy(g["z"].astype(np.float32)).to(dev)

    def run():
        ids, scores = model.decode(z, beam_width=2, max_len=12, return_tokens=True)
        return model.score(seqs, z), scores, [t for m in ids for t in m], model.iw_log_likelihood(seqs, n_samples=3, seed=8)
    want = run()
    model.word_dropout, model.free_bits = 0.5, 0.2

    def boom(*a, **k):
        raise AssertionError("score / decode / iw_log_likelihood applied a training-time remedy")
    for name in ("token_dropout", "moses_latent_fb_fwd", "moses_latent_fb_bwd"):
        monkeypatch.setattr(ops, name, boom)
    got = run()
    assert model.training
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
    assert all(torch.equal(a, b) for a, b in zip(want[2], got[2]))
    assert torch.equal(want[3][0], got[3][0]) and torch.equal(want[3][1], got[3][1])


# ---------------------------------------------------------------------------------------------- the train step
def test_train_step_with_both_remedies(golden_dir):
    g, model, seqs, _ = _g3_model(golden_dir, torch.bfloat16)
    model.d_dropout = 0.2
    model.word_dropout, model.free_bits = 0.3, 0.05
    opt = mv.FusedAdam(model.parameters(), lr=3e-4, max_grad_norm=50.0)
    kl_w = 0.3
    for _ in range(2):
        loss, kl, recon = mv.moses_train_step(model, opt, kl_w, seqs)
        vals = torch.stack([loss, kl, recon, model.last_kl]).tolist()
        assert all(np.isfinite(vals)), vals
        want = np.float32(kl_w) * np.float32(vals[1]) + np.float32(vals[2])
        assert abs(vals[0] - float(want)) <= 4 * 2.0 ** -24 * abs(float(want))      # loss == kl_weight * kl + recon to fp32 rounding
        assert vals[1] >= vals[3] > 0                                          # the objective is never below the KL
        assert isinstance(model.last_word_seed, int)
    post = mv.moses_train_epoch(model, 0, [seqs, seqs], kl_w, opt)
    assert np.isfinite(post["kl_true"]) and post["kl_loss"] >= post["kl_true"]
