"""GPU tests (pytest -m gpu) of the index-target ELBO: mvae_bce_kl_logits_fwd / _bwd against a float64 restatement of softmax -> BCE (log
clamp -100) -> KL and their gradients; the g1 / g2 fixtures through functional.decoder_elbo; MolecularVAE.elbo / elbo_train_step against
model(x) + bce_kl_loss / train_step (B = 1024, b = 128 on the persistent decoder backward, f32); determinism; peak memory; evaluate_elbo
against evaluate; the saved-state ring and no_grad; two data-parallel ranks."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_helpers as gh                        # noqa: E402
from gpu_helpers import mv, O, ip, rel          # noqa: E402
from molecular_vae_amd import ops, _lib as L    # noqa: E402
from molecular_vae_amd import data as D         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dev = torch.device("cuda")


# ------------------------------------------------------------------------------------------------ 1. the kernels vs float64
def _ref_elbo(logits_tm, idx, mu, lv, max_len, g):
    """float64 restatement: time-major logits [L*B, C] -> softmax -> BCELoss(mean, logs clamped at -100) on the one-hot of idx [B, L] ->
    times max_len, plus the swapped KL of train.py:36-37; and the gradients of g * total w.r.t. the logits (time-major), mu and logvar."""
    B, Lq = idx.shape
    C = logits_tm.shape[1]
    x = logits_tm.astype(np.float64).reshape(Lq, B, C).transpose(1, 0, 2)
    e = np.exp(x - x.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    t = np.eye(C)[idx]
    with np.errstate(divide="ignore"):
        lp, l1p = np.maximum(np.log(p), -100.0), np.maximum(np.log1p(-p), -100.0)
    n = p.size
    xent = max_len * -(t * lp + (1 - t) * l1p).sum() / n
    mu, lv = mu.astype(np.float64), lv.astype(np.float64)
    kl = -0.5 * np.mean(1 + mu - lv ** 2 - np.exp(mu))
    drecon = g * max_len / n * (p - t) / np.maximum(p * (1 - p), 1e-12)
    dl = p * (drecon - (drecon * p).sum(-1, keepdims=True))
    m = mu.size
    return dict(loss=xent + kl, xent=xent, kl=kl, dl=dl.transpose(1, 0, 2).reshape(Lq * B, C), p=p,
                dmu=g * (-0.5 / m) * (1 - np.exp(mu)), dlv=g * (-0.5 / m) * (-2 * lv))


def _case(B, Lq, C, dt, ldd, max_len, g, seed, saturate=True, bad=None):
    rs = np.random.RandomState(seed)
    logits = (1.5 * rs.standard_normal((Lq * B, C))).astype(np.float32)
    idx = rs.randint(0, C, size=(B, Lq)).astype(np.int64)
    if saturate:
        # rows whose target logit sits 150 below the rest (p_y == 0 in fp32: -log p_y hits the -100 clamp) and rows whose target sits 150
        # above it (every other p_c == 0: log(1 - p_c) == 0, p_y == 1)
        for k, r in enumerate(rs.choice(Lq * B, size=min(8, Lq * B), replace=False)):
            t_, b_ = divmod(int(r), B)
            logits[r, idx[b_, t_]] += -150.0 if k % 2 == 0 else 150.0
    if bad is not None:
        idx[bad] = C
    mu = (0.3 * rs.standard_normal((B, 16))).astype(np.float32)
    lv = (0.3 * rs.standard_normal((B, 16))).astype(np.float32)
    T = lambda a: torch.from_numpy(a).to(dev)
    tl, ti, tmu, tlv = T(logits), T(idx), T(mu), T(lv)
    out = torch.empty(3, device=dev)
    pred = torch.full((B, Lq), -1, dtype=torch.int64, device=dev)
    ops.bce_kl_logits_fwd(tl, C, ti, tmu, tlv, max_len, out, B, Lq, C, pred_out=pred)
    dl = torch.zeros(Lq * B, ldd, dtype=dt, device=dev)
    dlT = torch.zeros(C, Lq * B + 8, dtype=dt, device=dev) if dt == torch.float32 else None
    dmu, dlv = torch.empty_like(tmu), torch.empty_like(tlv)
    gt = None if g == 1.0 else torch.tensor([g], dtype=torch.float32, device=dev)
    ops.bce_kl_logits_bwd(tl, C, ti, tmu, tlv, max_len, gt, dl, dlT, dmu, dlv, B, Lq, C)
    torch.cuda.synchronize()
    return dict(logits=logits, idx=idx, mu=mu, lv=lv, out=out.cpu().numpy().astype(np.float64), pred=pred.cpu().numpy(),
                dl=dl.float().cpu().numpy(), dlT=None if dlT is None else dlT.cpu().numpy(), dmu=dmu.cpu().numpy(), dlv=dlv.cpu().numpy())


CASES = [  # (B, L, C, ldd, max_len, grad_out)
    (3, 24, 12, 16, 24.0, 1.0),
    (4, 120, 35, 128, 100.0, 0.37),
    (128, 120, 35, 40, 120.0, 2.5),
    (1024, 120, 35, 128, 120.0, 1.0),
    (2048, 256, 64, 128, 256.0, 1.0),
]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,Lq,C,ldd,max_len,g", CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in CASES])
def test_kernels_match_float64(B, Lq, C, ldd, max_len, g, dt):
    r = _case(B, Lq, C, dt, ldd, max_len, g, seed=B + Lq + C)
    ref = _ref_elbo(r["logits"], r["idx"], r["mu"], r["lv"], max_len, g)
    tol_loss = 2e-6
    assert abs(r["out"][0] - ref["loss"]) <= tol_loss * abs(ref["loss"]), (r["out"], ref["loss"])
    assert abs(r["out"][1] - ref["xent"]) <= tol_loss * abs(ref["xent"])
    assert abs(r["out"][2] - ref["kl"]) <= 1e-5 * abs(ref["kl"]) + 1e-7
    assert rel(r["dmu"], ref["dmu"]) < 1e-5 and rel(r["dlv"], ref["dlv"]) < 1e-5
    dl = r["dl"]
    assert not dl[:, C:].any(), "pad columns C..ldd-1 must stay zero"
    scale = np.abs(ref["dl"]).max()
    if dt == torch.float32:
        assert np.abs(dl[:, :C] - ref["dl"]).max() <= 1e-5 * scale
        assert np.array_equal(r["dlT"][:, :Lq * B], dl[:, :C].T) and not r["dlT"][:, Lq * B:].any()
    else:                                           # bf16 rounding of each element (8 significant bits) on top of the fp32 value
        assert (np.abs(dl[:, :C] - ref["dl"]) <= 2.0 ** -8 * np.abs(ref["dl"]) + 1e-6 * scale).all()
    # arg-max of the probabilities (first index on ties): equal wherever the top two are not tied to fp32 precision
    p = ref["p"]
    top2 = np.sort(p, -1)[..., -2:]
    clear = top2[..., 1] - top2[..., 0] > 1e-6 * top2[..., 1]
    assert (r["pred"][clear] == p.argmax(-1)[clear]).all() and ((r["pred"] >= 0) & (r["pred"] < C)).all()


def test_index_out_of_range_gives_nan_loss_without_fault():
    r = _case(8, 24, 12, torch.float32, 16, 24.0, 1.0, seed=3, saturate=False, bad=(5, 7))
    assert np.isnan(r["out"][0]) and np.isnan(r["out"][1]) and np.isfinite(r["out"][2])
    assert np.isfinite(r["dl"]).all() and np.isfinite(r["dmu"]).all()


# ------------------------------------------------------------------------------------------------ 3. the fixtures through decoder_elbo
def _fixture_elbo(dims, params, idx, eps, dtype):
    enc, dec = gh.build_modules(dims, params, dtype)
    tidx = torch.from_numpy(idx).to(dev)
    teps = torch.from_numpy(np.asarray(eps, np.float32)).to(dev)
    z, mu, logvar = enc(tidx, teps)
    dec.__dict__["_z_from_peer"] = True             # paired as MolecularVAE pairs them: the weight-gradient fork runs
    loss = mv.decoder_elbo(dec, z, tidx, mu, logvar, dims["i"])
    dec.__dict__["_z_from_peer"] = False
    loss.backward()
    torch.cuda.synchronize()
    grads = {"encoder." + k: p.grad.detach().cpu().numpy() for k, p in enc.named_parameters()}
    grads.update({"decoder." + k: p.grad.detach().cpu().numpy() for k, p in dec.named_parameters()})
    parts = dec.elbo_parts.cpu().numpy()
    assert parts[0] == float(loss.detach())
    return float(loss), parts, grads


def _oracle(dims, params, idx, eps):
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    return O.molvae_loss_and_grads(p64, idx, np.asarray(eps, np.float64), max_len=dims["i"], num_lstm=dims["n_enc"], num_gru=dims["n_dec"])


def test_g1_fixture_through_decoder_elbo(golden_dir):
    g = np.load(os.path.join(golden_dir, "g1_small.npz"))
    params = gh.g1_dims_params(np.float32)
    ref = _oracle(gh.G1, params, g["idx"], g["eps"])
    for dtype, tol_loss, tol_grad in ((torch.float32, 1e-5, 2e-4), (torch.bfloat16, 1e-4, 5e-2)):
        loss, parts, grads = _fixture_elbo(gh.G1, params, g["idx"], g["eps"], dtype)
        assert abs(loss - ref["loss"]) < tol_loss * abs(ref["loss"]) and abs(loss - float(g["loss"])) < tol_loss * abs(float(g["loss"]))
        assert abs(parts[1] - ref["xent"]) < tol_loss * abs(ref["xent"]) and abs(parts[2] - ref["kl"]) < 1e-4 * abs(ref["kl"]) + 1e-7
        bad = {k: v for k, v in gh.grad_report(grads, ref["grads"]).items() if v > tol_grad}
        assert not bad, (dtype, bad)
        if dtype == torch.float32:
            for k in [f for f in g.files if f.startswith("grad.")]:
                assert rel(grads[k[5:]], g[k]) < 2e-4, k


def test_g2_fixture_through_decoder_elbo(golden_dir):
    g = np.load(os.path.join(golden_dir, "g2_full.npz"))
    params = ip.init_params(ip.molvae_shapes(), 202, 1.5, np.float32)
    ref = _oracle(gh.FULL, params, g["idx"], g["eps"])
    for dtype, tol_loss, tol_grad in ((torch.float32, 1e-5, 5e-4), (torch.bfloat16, 1e-4, 5e-2)):
        loss, _, grads = _fixture_elbo(gh.FULL, params, g["idx"], g["eps"], dtype)
        assert abs(loss - ref["loss"]) < tol_loss * abs(ref["loss"]) and abs(loss - float(g["loss"])) < tol_loss * abs(float(g["loss"]))
        if dtype == torch.float32:
            for k, gr in grads.items():
                want = float(g["gnorm." + k])
                assert abs(np.sqrt((gr.astype(np.float64) ** 2).sum()) - want) < 5e-4 * want + 1e-12, k
        bad = {k: v for k, v in gh.grad_report(grads, ref["grads"]).items() if v > tol_grad}
        assert not bad, (dtype, bad)


# ------------------------------------------------------------------------------------------------ 4. fused vs existing path
def _grads_of(model, fn):
    model.zero_grad(set_to_none=True)
    loss = fn()
    loss.backward()
    torch.cuda.synchronize()
    return float(loss), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def _twin(model):
    """A second model with the same weights, paired with its OWN encoder (a deepcopy would keep the original's decoder-to-encoder weakref,
    and its decoder would park its weight-gradient work in the original's fork state)."""
    m = mv.MolecularVAE(i=model.decoder.repeat_vector.rep, o=model.decoder.latent_input[0].in_features,
                        c=model.decoder.decoded_mean.module[0].out_features, dtype=model.decoder.compute_dtype).to(dev)
    m.load_state_dict(model.state_dict())
    return m


def _both_paths(model, ref_model, x, eps, C, max_len):
    """(loss, grads) of ref_model through model(x) + bce_kl_loss on the one-hot, and of model through model.elbo."""
    ohe = torch.nn.functional.one_hot(x, C).float()
    loss_fn = mv.make_loss_function(max_len)

    def existing():
        recon, mu, logvar = ref_model(x, eps=eps)
        return loss_fn(recon, ohe, mu, logvar)
    la, ga = _grads_of(ref_model, existing)
    lb, gb = _grads_of(model, lambda: model.elbo(x, eps=eps, max_len=max_len)[0])
    return la, ga, lb, gb


def _compare(la, ga, lb, gb, tol_grad, norm_wise):
    assert abs(la - lb) <= 1e-6 * abs(la), (la, lb)
    for k in ga:
        a, b = ga[k].double(), gb[k].double()
        if norm_wise:
            err = float((a - b).norm() / (a.norm() + 1e-30))
        else:
            err = float((a - b).abs().max() / (a.abs().max() + 1e-30))
        assert err <= tol_grad, (k, err)


@pytest.mark.parametrize("B", [1024, 128])
def test_elbo_matches_the_existing_path_bf16(B, monkeypatch):
    torch.manual_seed(11)
    model = mv.MolecularVAE(dtype=torch.bfloat16).to(dev)
    ref_model = _twin(model)
    gen = torch.Generator().manual_seed(B)
    x = torch.randint(0, 35, (B, 120), generator=gen).to(dev)
    eps = (1e-2 * torch.randn(B, 292, generator=gen)).to(dev)
    _both_paths(model, ref_model, x, eps, 35, 120)         # first pass: workspaces, packs
    torch.cuda.synchronize()
    chose = []
    orig = ops.rnn_bwd_persist_wanted

    def spy(*a, **k):
        chose.append(orig(*a, **k))
        return chose[-1]
    monkeypatch.setattr(ops, "rnn_bwd_persist_wanted", spy)
    ops.persist_check(sync=True)
    n0 = ops.PERSIST_STATS["bwd_launches"]
    la, ga, lb, gb = _both_paths(model, ref_model, x, eps, 35, 120)
    ops.persist_check(sync=True)
    if B == 128:                                           # the per-rank shape of the 8-GPU configuration: the weights-resident decoder backward
        assert chose == [True, True] and ops.PERSIST_STATS["bwd_launches"] >= n0 + 2, (chose, "no persistent decoder backward at b = 128")
    assert ops.PERSIST_STATS["reruns"] == 0
    _compare(la, ga, lb, gb, 1e-3, norm_wise=True)


def test_elbo_matches_the_existing_path_f32_and_ten_adam_steps():
    torch.manual_seed(12)
    model_a = mv.MolecularVAE(i=24, o=16, c=12, dtype=torch.float32).to(dev)
    model_b = _twin(model_a)
    gen = torch.Generator().manual_seed(5)
    x = torch.randint(0, 12, (16, 24), generator=gen).to(dev)
    eps = [(1e-2 * torch.randn(16, 16, generator=gen)).to(dev) for _ in range(10)]
    la, ga, lb, gb = _both_paths(model_b, model_a, x, eps[0], 12, 24)
    _compare(la, ga, lb, gb, 1e-5, norm_wise=False)
    opt_a = mv.FusedAdam(model_a.parameters(), lr=1e-3, max_grad_norm=3.0)
    opt_b = mv.FusedAdam(model_b.parameters(), lr=1e-3, max_grad_norm=3.0)
    ohe = torch.nn.functional.one_hot(x, 12).float()
    loss_fn = mv.make_loss_function(24)
    for s in range(10):
        l_a = mv.train_step(model_a, opt_a, loss_fn, x, ohe, eps=eps[s])
        l_b = mv.elbo_train_step(model_b, opt_b, x, eps=eps[s])
        assert abs(float(l_a) - float(l_b)) <= 1e-5 * abs(float(l_a)), s
    for (k, pa), pb in zip(model_a.named_parameters(), model_b.parameters()):
        assert float((pa - pb).abs().max()) <= 1e-5 + 1e-4 * float(pa.abs().max()), k


def test_elbo_train_step_with_torch_adam_and_fused_sgd():
    torch.manual_seed(13)
    gen = torch.Generator().manual_seed(6)
    x = torch.randint(0, 12, (16, 24), generator=gen).to(dev)
    for make in (lambda ps: torch.optim.Adam(ps, lr=1e-3), lambda ps: mv.FusedSGD(ps, lr=1e-2, momentum=0.85, max_grad_norm=5.0)):
        model = mv.MolecularVAE(i=24, o=16, c=12, dtype=torch.float32).to(dev)
        opt = make(model.parameters())
        before = [p.detach().clone() for p in model.parameters()]
        losses = [float(mv.elbo_train_step(model, opt, x)) for _ in range(5)]
        assert all(np.isfinite(losses)), losses
        assert all(not torch.equal(a, p) for a, p in zip(before, model.parameters()))


# ------------------------------------------------------------------------------------------------ 5. determinism
def test_two_identical_fused_steps_are_bit_identical():
    torch.manual_seed(14)
    model = mv.MolecularVAE(dtype=torch.bfloat16).to(dev)
    gen = torch.Generator().manual_seed(7)
    x = torch.randint(0, 35, (256, 120), generator=gen).to(dev)
    eps = (1e-2 * torch.randn(256, 292, generator=gen)).to(dev)
    runs = [_grads_of(model, lambda: model.elbo(x, eps=eps)[0]) for _ in range(2)]
    assert runs[0][0] == runs[1][0]
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


# ------------------------------------------------------------------------------------------------ 6. memory
def test_fused_step_peak_memory_and_no_blc_tensor():
    B, Lq, C = 1024, 120, 35
    torch.manual_seed(15)
    model = mv.MolecularVAE(dtype=torch.bfloat16).to(dev)
    ref_model = _twin(model)
    gen = torch.Generator().manual_seed(8)
    x = torch.randint(0, C, (B, Lq), generator=gen).to(dev)
    loss_fn = mv.make_loss_function(Lq)

    def existing():
        # the existing step includes its float one-hot target, which DeviceDataset.batches writes for every step
        ohe = torch.zeros(B, Lq, C, device=dev).scatter_(2, x.unsqueeze(2), 1.0)
        r, mu, lv = ref_model(x)
        loss_fn(r, ohe, mu, lv).backward()

    def fused():
        model.elbo(x)[0].backward()

    peaks = {}
    for name, fn, m in (("existing", existing, ref_model), ("fused", fused, model)):
        for _ in range(2):                                # the first pass allocates the workspaces
            m.zero_grad(set_to_none=True)
            fn()
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
    blc = B * Lq * C * 4
    assert peaks["existing"] - peaks["fused"] >= 2 * blc, peaks        # recon + drecon + the one-hot: three such tensors fewer
    # no allocation of a [B, L, C] fp32 tensor anywhere in a fused step
    from torch.cuda import memory as cm
    model.zero_grad(set_to_none=True)
    cm._record_memory_history(max_entries=100000)
    try:
        fused()
        torch.cuda.synchronize()
        snap = cm._snapshot()
    finally:
        cm._record_memory_history(enabled=None)
    sizes = [e["size"] for trace in snap["device_traces"] for e in trace if e["action"] == "alloc"]
    assert sizes and blc not in sizes, sorted(set(sizes))[-8:]


# ------------------------------------------------------------------------------------------------ 7. evaluation
def test_evaluate_elbo_equals_evaluate_on_a_trained_model():
    smiles = D.synthetic_smiles(8, seed=1, lo=8, hi=20)
    vocab = D.build_vocab(smiles, 24)
    C = len(vocab)
    ds = D.DeviceDataset(D.encode_smiles(smiles * 32, vocab, 24), C)
    torch.manual_seed(16)
    model = mv.MolecularVAE(i=24, o=64, c=C, dtype=torch.bfloat16).to(dev)
    opt = mv.FusedAdam(model.parameters(), lr=2e-3, max_grad_norm=3.0)
    for ep in range(150):                                 # 600 steps of 64 over 8 distinct strings
        for idx in ds.batches(64, epoch=ep, want_onehot=False):
            mv.elbo_train_step(model, opt, idx[0] if isinstance(idx, tuple) else idx)

    def both(dset):
        model.encoder.lmbd.seed_noise(99)
        want = mv.evaluate(model, mv.make_loss_function(24), dset.batches(64, shuffle=False, drop_last=False))
        model.encoder.lmbd.seed_noise(99)
        got = mv.evaluate_elbo(model, dset.batches(64, shuffle=False, drop_last=False, want_onehot=False))
        # 1e-5, not 1e-6: a trained model's loss can be ~0.01, made of terms 1 - p_y and p_c at the fp32 rounding of p_y ~ 1 on both paths
        assert abs(got[0] - want[0]) <= 1e-5 * abs(want[0]) and got[1] == want[1], (got, want)
        return want[1]
    both(ds)
    # whether 600 steps reach exact matches varies from run to run: for a nonzero accuracy by construction, raise the head's bias of the pad
    # class and score all-pad rows (each of them then decodes to itself)
    with torch.no_grad():
        model.decoder.decoded_mean.module[0].bias[vocab[" "]] += 40.0
    assert both(D.DeviceDataset(D.encode_smiles([""] * 128, vocab, 24), C)) == 1.0
    # pred_out against recon.argmax(2) of the same forward noise, except where the top two probabilities tie
    x = next(iter(ds.batches(64, shuffle=False, want_onehot=False)))
    x = x[0] if isinstance(x, tuple) else x
    with torch.no_grad():
        model.encoder.lmbd.seed_noise(5)
        recon, _, _ = model(x)
        model.encoder.lmbd.seed_noise(5)
        pred = torch.empty_like(x)
        model.elbo(x, pred_out=pred)
    top2 = recon.topk(2, dim=2).values
    clear = top2[..., 0] > top2[..., 1]
    assert torch.equal(pred[clear], recon.argmax(2)[clear]) and bool(clear.float().mean() > 0.99)


# ------------------------------------------------------------------------------------------------ 8. saved state and no_grad
def test_saved_state_ring_and_no_grad():
    torch.manual_seed(17)
    model = mv.MolecularVAE(i=24, o=16, c=12, dtype=torch.float32).to(dev)
    gen = torch.Generator().manual_seed(9)
    xs = [torch.randint(0, 12, (8, 24), generator=gen).to(dev) for _ in range(2)]
    l0 = model.elbo(xs[0])[0]
    model.elbo(xs[1])                                       # a second forward of the same module without backward
    with pytest.raises(L.MvaeError, match="saved_state_depth"):
        l0.backward()
    model.zero_grad(set_to_none=True)
    l0 = model.elbo(xs[0])[0]
    with torch.no_grad():
        ln = model.elbo(xs[1])[0]
    assert not ln.requires_grad and ln.grad_fn is None and np.isfinite(float(ln))
    with pytest.raises(L.MvaeError, match="saved_state_depth"):   # the no_grad forward overwrote the workspace slot: refused, not wrong
        l0.backward()
    model.zero_grad(set_to_none=True)
    for m in (model.encoder, model.decoder):
        m.saved_state_depth = 2
    ls = [model.elbo(x)[0] for x in xs]
    for l_ in reversed(ls):
        l_.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


# ------------------------------------------------------------------------------------------------ 9. two ranks
def _port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def test_two_rank_fused_step_equals_existing_step(tmp_path):
    out = os.path.join(str(tmp_path), "elbo2.json")
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_port()), os.path.join(ROOT, "tests", "dp_elbo_equiv.py"), "--out", out, "--steps", "3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, f"--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-3000:]}"
    res = json.load(open(out))
    assert res["world"] == 2 and res["early_ranges"][0] == res["early_ranges"][1] > 0
    for s in range(3):
        assert abs(res["loss_a"][s] - res["loss_b"][s]) <= 1e-6 * abs(res["loss_a"][s]), res
        assert abs(res["gnorm_a"][s] - res["gnorm_b"][s]) <= 1e-5 * abs(res["gnorm_a"][s]), res
        assert abs(res["psum_a"][s] - res["psum_b"][s]) <= 1e-6 * abs(res["psum_a"][s]), res
