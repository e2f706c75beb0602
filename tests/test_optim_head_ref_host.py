"""tests/optim_head_ref.py checked without a GPU: every reference against torch in float64, the bound machinery against planted mutants of a
correct result (each must be rejected by the float bound, and by the bitwise integer comparison where it applies), the K constants against
their derivation (8 x the worst ratio of the float32 restatement over all cases of test_gpu_optim_head_kernels.py), and the argument
checks of the C entries, which refuse before anything is enqueued and so need no device."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import optim_head_ref as R
from molecular_vae_amd import _lib as L


# ------------------------------------------------------------------------------------------------ references against torch in float64
def _torch_adam(p, gs, hp, n):
    f = lambda k: float(np.float32(hp[k]))
    tp = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
    opt = torch.optim.Adam([tp], lr=f("lr"), betas=(f("b1"), f("b2")), eps=f("eps"))
    out = []
    for g in gs:
        tp.grad = torch.from_numpy(g.astype(np.float64)) * f("grad_scale")
        norm = torch.nn.utils.clip_grad_norm_([tp], f("max_norm"))
        opt.step()
        st = opt.state[tp]
        out.append((tp.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy(), float(norm)))
    return out


@pytest.mark.parametrize("case", ["defaults", "grad_scale", "betas_eps"])
def test_clip_adam_steps_is_clip_grad_norm_and_torch_adam(case):
    n = 257
    p, gs, _, _ = R.adam_inputs(n, case)
    hp = R.adam_hp(case)
    z = np.zeros(n, np.float32)
    ref = R.clip_adam_steps(p, gs, z, z, **hp)
    assert [float(s["coef"]) < 1.0 for s in ref] == [True, False, True, False]          # the clip binds on steps 1 and 3 only
    for s, (tp, tm, tv, tn) in zip(ref, _torch_adam(p, gs, hp, n)):
        assert abs(s["norm"] - tn) <= 1e-12 * tn
        for a, b in ((s["p"], tp), (s["m"], tm), (s["v"], tv)):
            assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    assert ref[-1]["nskipped"] == 0


def test_clip_adam_steps_skips_and_counts_a_non_finite_norm():
    n = 300
    p, gs, m, v = R.adam_inputs(n, "defaults")
    gs = [np.append(g, np.float32(0.0)) for g in gs]
    gs[1][n] = np.nan                                   # the poison slot behind the gradients
    gs[2][:n] = 1e20                                    # finite, but the squares overflow float32
    for dt in (np.float64, np.float32):
        ref = R.clip_adam_steps(p, gs, m, v, dt=dt, **R.ADAM_DEFAULT)
        assert [s["nskipped"] for s in ref] == [0, 1, 2, 2] and np.isnan(ref[1]["norm"]) and np.isinf(ref[2]["norm"])
        for k in "pmv":
            assert np.array_equal(ref[1][k], ref[0][k]) and np.array_equal(ref[2][k], ref[0][k]) and not np.array_equal(ref[3][k], ref[0][k])


def test_sumsq_partials_chunks():
    rs = np.random.RandomState(0)
    g = R.ints(rs, 2 * R.CHUNK + 5, -3, 3)
    got = R.sumsq_partials(g)
    assert got.shape == (3,) and got[2] == float((g[2 * R.CHUNK:].astype(np.float64) ** 2).sum())
    assert got[0] == float((g[:R.CHUNK].astype(np.float64) ** 2).sum()) and got.max() <= 9 * R.CHUNK < 2 ** 24


@pytest.mark.parametrize("soft", [False, True])
def test_bce_kl_matches_torch_binary_cross_entropy_and_autograd(soft):
    n, m = 210, 64
    recon, target, mu, logvar = (np.array(x) for x in R.bce_inputs(n, m, soft))
    recon[:5], target[:5] = R.BCE_CLAMP_P, R.BCE_CLAMP_T
    tr = torch.from_numpy(recon.astype(np.float64)).requires_grad_(True)
    tmu = torch.from_numpy(mu.astype(np.float64)).requires_grad_(True)
    tlv = torch.from_numpy(logvar.astype(np.float64)).requires_grad_(True)
    xent = R.MAX_LEN * F.binary_cross_entropy(tr, torch.from_numpy(target.astype(np.float64)))
    kl = -0.5 * torch.mean(1.0 + tmu - tlv ** 2 - tmu.exp())
    out, scale = R.bce_kl_fwd(recon, target, mu, logvar, R.MAX_LEN)
    want = np.array([float(x.detach()) for x in (xent + kl, xent, kl)])
    assert np.abs(out - want).max() <= 1e-12 * np.abs(want).max() and (scale >= np.abs(out) * (1 - 1e-12)).all()
    ((xent + kl) * 0.37).backward()
    (dr, dmu, dlv), _ = R.bce_kl_bwd(recon, target, mu, logvar, R.MAX_LEN, grad_out=0.37)
    g = float(np.float32(0.37)) / 0.37
    inner = (recon > 0) & (recon < 1)                    # at p = 0 / 1 torch's clamped log has gradient 0; the project's form is the header's
    assert np.abs(dr[inner] - g * tr.grad.numpy()[inner]).max() <= 1e-9 * np.abs(dr[inner]).max()
    assert np.abs(dmu - g * tmu.grad.numpy()).max() <= 1e-12 * np.abs(dmu).max()
    assert np.abs(dlv - g * tlv.grad.numpy()).max() <= 1e-12 * np.abs(dlv).max()
    sr = float(np.float32(0.37)) * R.MAX_LEN / n
    assert np.allclose(dr[:5], sr * np.array([-1e12, 1e12, 0.0, 0.0, -0.5 / 0.25]), rtol=1e-6)


def test_softmax_refs_match_torch_autograd():
    B, L, C = 5, 7, 3
    rs = np.random.RandomState(3)
    logits = (2.0 * rs.standard_normal((L * B, C + 2))).astype(np.float32)
    y = torch.from_numpy(logits[:, :C].astype(np.float64)).requires_grad_(True)
    p = torch.softmax(y, 1)
    dp = rs.standard_normal((B, L, C)).astype(np.float32)
    p_bm = R.softmax_fwd(logits, B, L, C)
    assert np.abs(p_bm - p.detach().numpy().reshape(L, B, C).transpose(1, 0, 2)).max() <= 1e-15
    p32 = p_bm.astype(np.float32)
    # autograd of softmax gives p (dp - sum dp p) for the exact p of y; hand the reference that p's float32 rounding and bound by it
    (p * torch.from_numpy(dp.astype(np.float64).transpose(1, 0, 2).reshape(L * B, C))).sum().backward()
    dl, dlT, scale = R.softmax_bwd(p32, dp)
    assert dl.shape == (L * B, C) and np.array_equal(dlT, dl.T)
    assert (np.abs(dl - y.grad.numpy()) <= 4 * 2.0 ** -24 * scale + 1e-15).all()


def test_table_refs_match_index_add_and_fancy_indexing():
    rs = np.random.RandomState(4)
    B, L, V, W, ldd = 5, 14, 7, 9, 16
    idx, never = R.token_ids(rs, B, L, V)
    assert (idx == -4).any() and (idx == V + 9).any() and not (idx == never).any()
    cl = torch.from_numpy(np.clip(idx, 0, V - 1))
    d = R.floats(rs, (L * B, ldd))
    d[:, W:] = np.nan
    td = torch.from_numpy(d[:, :W].astype(np.float64)).reshape(L, B, W)
    want = torch.zeros(V, W, dtype=torch.float64).index_add_(0, cl.t().reshape(-1), td.reshape(L * B, W))
    got, sa = R.scatter_rows_tb(idx, B, L, V, d, W)
    assert np.abs(got - want.numpy()).max() <= 1e-13 and not got[never].any() and (sa >= np.abs(got) - 1e-13).all()
    table, base = R.floats(rs, (V, W)), R.floats(rs, (B, W))
    g = R.gather_rows_tb(idx, B, L, V, table, base).reshape(L, B, W)
    g0 = R.gather_rows_tb(idx, B, L, V, table).reshape(L, B, W)
    for b in range(B):
        for t in range(L):
            assert np.array_equal(g[t, b], table[cl[b, t]] + base[b]) and np.array_equal(g0[t, b], table[cl[b, t]])
    oh = R.onehot_tb(idx, B, L, V, 8)
    assert np.array_equal(oh[:, :V], F.one_hot(cl.t().reshape(-1), V).numpy().astype(np.float32)) and not oh[:, V:].any()


# ------------------------------------------------------------------------------------------------ planted mutants
def _rejected(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except AssertionError:
        return True
    return False


def _adam_mutant(kind, p, g, m, v, hp, step):
    """The reference step with one planted mistake."""
    f = lambda k: float(np.float32(hp[k]))
    g64, p, m, v = (np.asarray(a, np.float64) for a in (g, p, m, v))
    norm = np.sqrt((g64 * g64).sum()) * (1.0 if kind == "clip_without_grad_scale" else f("grad_scale"))
    coef = min(1.0, f("max_norm") / (norm + float(np.float32(1e-6)))) if np.isfinite(norm) else norm      # a non-finite norm is applied
    gi = g64[:p.size] * coef * f("grad_scale")
    mi = f("b1") * m + (1 - f("b1")) * gi
    vi = f("b2") * v + (1 - f("b2")) * gi * gi
    bc1, bc2 = 1 - f("b1") ** step, 1 - f("b2") ** step
    if kind == "eps_inside_sqrt":
        denom = np.sqrt(vi / bc2 + f("eps"))
    elif kind == "no_bias_correction_on_v":
        denom = np.sqrt(vi) + f("eps")
    else:
        denom = np.sqrt(vi) / np.sqrt(bc2) + f("eps")
    return p - f("lr") / bc1 * mi / denom, mi, vi


@pytest.mark.parametrize("case", ["defaults", "grad_scale", "betas_eps", "zero_grads"])
def test_adam_bound_rejects_planted_mutants(case):
    n, hp = 257, R.adam_hp(case)
    p, gs, m, v = R.adam_inputs(n, case)
    ref = R.adam_step(p, gs[0], m, v, step=hp["step0"], **{k: hp[k] for k in hp if k != "step0"})
    chk = lambda q: [R.assert_within(q[i], ref[k], ref["s" + k], R.K_ADAM, k) for i, k in enumerate("pmv")]
    good = _adam_mutant("none", p, gs[0], m, v, hp, hp["step0"])
    chk(good)                                            # the unmutated restatement passes: the mutants below fail for their mistake alone
    for kind in ("eps_inside_sqrt", "no_bias_correction_on_v"):
        assert _rejected(chk, _adam_mutant(kind, p, gs[0], m, v, hp, hp["step0"])), kind
    if hp["grad_scale"] != 1.0:
        assert _rejected(chk, _adam_mutant("clip_without_grad_scale", p, gs[0], m, v, hp, hp["step0"]))
    gbad = np.append(gs[0], np.float32(np.nan))          # a poisoned step: the reference keeps the state, the mutant applies it
    ref2 = R.adam_step(p, gbad, m, v, step=hp["step0"], **{k: hp[k] for k in hp if k != "step0"})
    assert ref2["skipped"] and np.array_equal(ref2["p"], p)
    chk2 = lambda q: [R.assert_within(q[i], ref2[k], ref2["s" + k], R.K_ADAM, k) for i, k in enumerate("pmv")]
    chk2((p, m, v))
    assert _rejected(chk2, _adam_mutant("apply_non_finite", p, gbad, m, v, hp, hp["step0"]))


def _scatter_mutant(kind, idx, B, L, V, d, W):
    d = np.asarray(d, np.float64)[:, :W]
    out = np.zeros((V, W))
    rows = B * L
    parts = min((rows + 63) // 64, 1024)
    rpb = (rows + parts - 1) // parts
    for row in range(rows):
        t, b = divmod(row, B)
        i = int(idx[b, t])
        if kind == "ids_not_clamped":
            if not 0 <= i < V:
                continue
        else:
            i = min(max(i, 0), V - 1)
        if kind == "last_row_of_a_part_dropped" and (row % rpb == rpb - 1 or row == rows - 1):
            continue
        out[i] += d[b * L + t] if kind == "batch_major_rows" else d[row]
    return out


@pytest.mark.parametrize("integers", [True, False], ids=["ints", "floats"])
def test_scatter_bounds_reject_planted_mutants(integers):
    rs = np.random.RandomState(6)
    B, L, V, W = 16, 12, 7, 9                            # 192 rows: three 64-row parts
    idx, _ = R.token_ids(rs, B, L, V)
    d = R.ints(rs, (L * B, W)) if integers else R.floats(rs, (L * B, W))
    d[d == 0] = 1.0
    ref, sa = R.scatter_rows_tb(idx, B, L, V, d, W)
    chk = (lambda q: R.assert_exact(q, ref)) if integers else (lambda q: R.assert_sum_within(q, ref, sa))
    chk(_scatter_mutant("none", idx, B, L, V, d, W))
    for kind in ("batch_major_rows", "last_row_of_a_part_dropped", "ids_not_clamped"):
        assert _rejected(chk, _scatter_mutant(kind, idx, B, L, V, d, W)), kind


@pytest.mark.parametrize("integers", [True, False], ids=["ints", "floats"])
def test_sumsq_bounds_reject_a_dropped_chunk_tail(integers):
    rs = np.random.RandomState(7)
    for n in (3, 5, 1023, 70001, 2 * R.CHUNK + 5):
        g = R.ints(rs, n, -3, 3) if integers else R.floats(rs, n)
        g[g == 0] = 1.0
        ref = R.sumsq_partials(g)
        chk = (lambda q: R.assert_exact(q, ref)) if integers else (lambda q: R.assert_sum_within(q, ref, ref))
        chk(R.sumsq_partials(g, np.float32))
        assert _rejected(chk, R.sumsq_partials(g[:n - n % 4])), n       # the last n % 4 elements of the short chunk left out


def test_bce_bound_rejects_planted_mutants():
    n, m = 21, 64
    recon, target, mu, logvar = (np.array(x) for x in R.bce_inputs(n, m, False))
    recon[:5], target[:5] = R.BCE_CLAMP_P, R.BCE_CLAMP_T
    ref, scale = R.bce_kl_fwd(recon, target, mu, logvar, R.MAX_LEN)
    chk = lambda q: R.assert_within(q, ref, scale, R.K_BCE_FWD)
    chk(R.bce_kl_fwd(recon, target, mu, logvar, R.MAX_LEN, np.float32)[0])
    p, t, a, b = (x.astype(np.float64) for x in (recon, target, mu, logvar))
    with np.errstate(divide="ignore", invalid="ignore"):
        raw = np.where(t == 1, np.log(p), np.log1p(-p))                                 # no -100 clamp
    xent_raw = R.MAX_LEN * -raw.sum() / n
    assert _rejected(chk, np.array([xent_raw + ref[2], xent_raw, ref[2]]))
    kl_textbook = -0.5 * np.mean(1.0 + b - a * a - np.exp(b))
    assert _rejected(chk, np.array([ref[1] + kl_textbook, ref[1], kl_textbook]))
    (dr, dmu, dlv), (sr, smu, slv) = R.bce_kl_bwd(recon, target, mu, logvar, R.MAX_LEN)
    k = -0.5 / m
    assert _rejected(R.assert_within, k * (1.0 - np.exp(b)), dmu, smu, R.K_BCE_BWD)      # the textbook order's gradients
    assert _rejected(R.assert_within, k * (-2.0 * a), dlv, slv, R.K_BCE_BWD)
    with np.errstate(divide="ignore", invalid="ignore"):
        unclamped = (R.MAX_LEN / n) * (p - t) / (p * (1 - p))                            # no 1e-12 floor: 0 / 0 and 1 / 0 at the clamp rows
    assert _rejected(R.assert_within, unclamped, dr, sr, R.K_BCE_BWD)


# ------------------------------------------------------------------------------------------------ the K constants and their derivation
def _pow2_at_least(x):
    return 2.0 ** np.ceil(np.log2(x))


def _adam_cpu_ratio():
    """Step by step as the GPU test does: the float32 restatement runs on (its own float32 state), the float64 reference restates each step
    from the same float32 state."""
    worst = 0.0
    for n in R.ADAM_NS:
        for case in R.ADAM_CASES:
            hp = R.adam_hp(case)
            kw = {k: hp[k] for k in hp if k != "step0"}
            p, gs, m, v = R.adam_inputs(n, case)
            for i, g in enumerate(gs):
                r32 = R.adam_step(p, g, m, v, step=hp["step0"] + i, dt=np.float32, **kw)
                r64 = R.adam_step(p, g, m, v, step=hp["step0"] + i, **kw)
                worst = max([worst, R.ratio(r32["norm"], r64["norm"], r64["norm"])] +
                            [R.ratio(r32[k], r64[k], r64["s" + k]) for k in "pmv"])
                p, m, v = r32["p"], r32["m"], r32["v"]
    return worst


def _bce_fwd_cpu_ratio():
    worst = 0.0
    for n, m in R.BCE_SHAPES:
        for soft in (False, True):
            a = R.bce_inputs(n, m, soft)
            ref, scale = R.bce_kl_fwd(*a, R.MAX_LEN)
            worst = max(worst, R.ratio(R.bce_kl_fwd(*a, R.MAX_LEN, np.float32)[0], ref, scale))
    a = (R.BCE_CLAMP_P, R.BCE_CLAMP_T) + R.bce_inputs(5, 7, False)[2:]
    ref, scale = R.bce_kl_fwd(*a, R.MAX_LEN)
    return max(worst, R.ratio(R.bce_kl_fwd(*a, R.MAX_LEN, np.float32)[0], ref, scale))


def _bce_bwd_cpu_ratio():
    worst = 0.0
    cases = [R.bce_inputs(n, m, soft) + (g,) for n, m in R.BCE_SHAPES[:5] for soft in (False, True) for g in (None, 0.37)]
    mu, lv = R.bce_inputs(12, 7, False)[2:]
    cases += [(np.repeat(R.BCE_EDGE_P, 2), np.tile(np.array([0.0, 1.0], np.float32), 6), mu, lv, g) for g in (None, 0.37)]
    for recon, target, mu, lv, g in cases:
        ref, scale = R.bce_kl_bwd(recon, target, mu, lv, R.MAX_LEN, g)
        got, _ = R.bce_kl_bwd(recon, target, mu, lv, R.MAX_LEN, g, np.float32)
        worst = max([worst] + [R.ratio(x, y, s) for x, y, s in zip(got, ref, scale)])
    return worst


def _softmax_bwd_cpu_ratio():
    worst = 0.0
    for B, L_, C, _ in R.SOFTMAX_BWD_SHAPES:
        p, dp = R.softmax_inputs(B, L_, C)
        dl, _, scale = R.softmax_bwd(p, dp)
        worst = max(worst, R.ratio(R.softmax_bwd(p, dp, np.float32)[0], dl, scale))
    return worst


@pytest.mark.parametrize("name,fn", [("K_ADAM", _adam_cpu_ratio), ("K_BCE_FWD", _bce_fwd_cpu_ratio), ("K_BCE_BWD", _bce_bwd_cpu_ratio),
                                     ("K_SOFTMAX_BWD", _softmax_bwd_cpu_ratio)])
def test_k_constants_are_eight_times_the_float32_restatement_ratio(name, fn):
    r = fn()
    K = getattr(R, name)
    print(f"{name} = {K}: CPU ratio {r:.4g}, 8 x ratio = {8 * r:.4g}")
    assert r > 0 and K >= 8 * r, (name, K, r)
    # ... and is that product rounded up to a power of two; one more doubling is allowed for, since numpy's float32 log2 / exp differ by a
    # last bit between CPU instruction sets and 8 x ratio may sit next to a power of two
    assert K == 2.0 ** round(np.log2(K)) and K <= 2 * _pow2_at_least(8 * r), f"{name} = {K} is more than 8 x {r:.4g} rounded up"


def test_adam_cases_bind_the_clip_on_steps_one_and_three_only():
    for n in R.ADAM_NS[:3]:
        for case in R.ADAM_CASES:
            hp = R.adam_hp(case)
            p, gs, m, v = R.adam_inputs(n, case)
            ref = R.clip_adam_steps(p, gs, m, v, **hp)
            binds = [float(s["coef"]) < 1.0 for s in ref]
            assert binds == ([False] * 4 if hp["max_norm"] <= 0 else [True, False, True, False]), (n, case)
            for g in gs:
                nz = np.abs(g[g != 0])
                assert nz.size and nz.min() > 1e-6


# ------------------------------------------------------------------------------------------------ argument checks of the C entries
def _host(nfloats=64):
    buf = (ctypes.c_float * nfloats)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_clip_adam_and_sumsq_refuse_bad_arguments_without_a_device():
    lib = L.load()
    _keep, a = _host()

    def adam(n=8, npartial=1, step=1, null=None):
        q = {k: (None if k == null else a) for k in ("p", "g", "m", "v", "partial")}
        return lib.mvae_clip_adam(n, q["p"], q["g"], q["m"], q["v"], q["partial"], npartial, 1.0, 5.0, 1e-3, 0.9, 0.999, 1e-8, step, a, 2, None, None)
    bad = dict(n_zero=dict(n=0), n_negative=dict(n=-3), no_partials=dict(npartial=0), step_zero=dict(step=0))
    bad.update({"null_" + k: dict(null=k) for k in ("p", "g", "m", "v", "partial")})
    for what, kw in bad.items():
        assert adam(**kw) == -1, what
    base = (a.value + 15) & ~15
    assert lib.mvae_sumsq(8, ctypes.c_void_p(base + 4), a, None) == -1          # g not 16-byte aligned
    assert lib.mvae_sumsq(0, ctypes.c_void_p(base), a, None) == -1


def test_table_and_head_entries_refuse_before_anything_is_enqueued():
    lib = L.load()
    _keep, a = _host(4096)
    B, Lq, V, W = 2, 3, 4, 5
    need = lib.mvae_scatter_rows_tb_workspace(B, Lq, V, W)
    assert need == 1 * V * W * 4

    def scatter(dtype=L.MVAE_F32, nrows=V, ws_bytes=need):
        return lib.mvae_scatter_rows_tb(dtype, a, B, Lq, nrows, a, W, W, a, a, ws_bytes, None)
    assert scatter(nrows=12289) == -3                    # no column slice of the LDS table fits 48 KiB
    assert scatter(ws_bytes=need - 1) == -2
    assert scatter(dtype=7) == -1
    assert lib.mvae_softmax_tb_fwd(2, 3, 129, a, 129, a, None) == -3
    wneed = lib.mvae_bce_kl_loss_workspace(8, 4)
    big = (ctypes.c_char * (wneed + 16))()
    ws = ctypes.cast(big, ctypes.c_void_p)
    assert lib.mvae_bce_kl_loss_fwd(8, a, a, 4, a, a, 120.0, a, ws, wneed - 1, None) == -2
    assert lib.mvae_bce_kl_loss_fwd(8, a, a, 4, a, a, 120.0, a, None, wneed, None) == -2
    assert lib.mvae_bce_kl_loss_fwd(0, a, a, 4, a, a, 120.0, a, ws, wneed, None) == -1
