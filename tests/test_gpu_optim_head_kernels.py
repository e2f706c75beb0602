"""GPU tests (pytest -m gpu) of the kernels that run every training step of MolecularVAE but had no direct float64 test: mvae_sumsq +
mvae_clip_adam, mvae_gather_rows_tb, mvae_scatter_rows_tb, mvae_onehot_tb, mvae_bce_kl_loss_fwd / _bwd and the plain (one wave per row)
kernels of mvae_softmax_tb_fwd / _bwd.  Each entry is called through molecular_vae_amd.ops at the smallest shapes that reach every branch
of its launcher and kernel, and held to tests/optim_head_ref.py (float64; checked on the CPU by test_optim_head_ref_host.py).

Destinations start as NaN or a sentinel and NaN sits behind every source, so a stray write or a stray read shows.  Nothing here is outside
an entry's documented contract: out-of-range ids go only where include/mvae.h says they are clamped, NaN / inf only into the gradient of
mvae_clip_adam, where the header defines the skipped step; refusals are checked on the CPU.

Bounds (optim_head_ref.py): data movement and integer data bit for bit; reductions of floats within 2e-6 * sum|terms| and bitwise
repeatable; math kernels per element within K * 2^-24 * scale.

  kernel                  K                    CPU ratio (f32 restatement)   worst ratio on an MI355X
  mvae_clip_adam          K_ADAM = 64          6.97                          6.35
  mvae_bce_kl_loss_fwd    K_BCE_FWD = 32       3.05                          2.20
  mvae_bce_kl_loss_bwd    K_BCE_BWD = 64       4.36                          4.36
  mvae_softmax_tb_bwd     K_SOFTMAX_BWD = 32   3.09                          2.46
Every test prints its own worst ratio ("GPU ratio <kernel> <value>", pytest -s).
"""
import functools
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import optim_head_ref as R                      # noqa: E402
from molecular_vae_amd import ops               # noqa: E402

dev = torch.device("cuda")
NAN = float("nan")
SENT = -12345.0


def host(x):
    torch.cuda.synchronize()
    return x.detach().cpu()


def src(a, off=0, tail=3):
    """a on the device with NaN in front of it (off elements) and behind it: (whole buffer, the view the kernel gets)."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    h = np.full(off + a.size + tail, np.nan, np.float32)
    h[off:off + a.size] = a
    buf = torch.from_numpy(h).to(dev)
    return buf, buf[off:off + a.size]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def report(kernel, r):
    print(f"GPU ratio {kernel} {r:.4g}")


# ------------------------------------------------------------------------------------------------ mvae_sumsq
def _sumsq(g, padded=False):
    """partials of g[:n]; the buffer holds NaN behind g[n - 1], or (padded) zeros up to whole chunks, which the call then covers"""
    n = g.size
    nch = (n + R.CHUNK - 1) // R.CHUNK
    if padded:
        h = np.zeros(nch * R.CHUNK, np.float32)
        h[:n] = g
        view = torch.from_numpy(h).to(dev)
    else:
        _, view = src(g)
    partial = torch.full((nch + 1,), SENT, device=dev)
    ops.sumsq(view, partial[:nch])
    out = host(partial).numpy()
    assert out[nch] == SENT
    return out[:nch]


SUMSQ_NS = (1, 3, 4, 5, 1023, 65535, 65536, 65537, 70001, 131072 + 5)


@pytest.mark.parametrize("n", SUMSQ_NS)
def test_sumsq_exact_integers_floats_and_zero_padding(n):
    rs = np.random.RandomState(n)
    gi = R.ints(rs, n, -3, 3)                                # a chunk sums to at most 9 * 65536 = 589824 < 2^24
    R.assert_exact(_sumsq(gi), R.sumsq_partials(gi), "integers")
    gf = R.floats(rs, n)
    ref = R.sumsq_partials(gf)
    a, b = _sumsq(gf), _sumsq(gf)
    R.assert_sum_within(a, ref, ref, "floats")
    assert same_bits(a, b), "two runs differ"
    # the kernel's contract: a short last chunk sums exactly as the same chunk zero-padded to 65536 elements
    assert same_bits(a, _sumsq(gf, padded=True)), "g[:n] and its zero-padded form give different partial sums"


# ------------------------------------------------------------------------------------------------ mvae_clip_adam
def _adam_state(p, m, v, off):
    """p, m, v in buffers with a sentinel in front (off elements) and behind"""
    out = []
    for a in (p, m, v):
        h = np.full(off + a.size + 2, SENT, np.float32)
        h[off:off + a.size] = a
        buf = torch.from_numpy(h).to(dev)
        out.append((buf, buf[off:off + a.size]))
    return out


def _edges_intact(bufs, off, n):
    for buf, _ in bufs:
        h = host(buf).numpy()
        assert (h[:off] == SENT).all() and (h[off + n:] == SENT).all(), "a write outside [0, n)"


@pytest.mark.parametrize("case", list(R.ADAM_CASES))
@pytest.mark.parametrize("n", R.ADAM_NS)
def test_clip_adam_four_steps_element_by_element(n, case):
    hp, off = R.adam_hp(case), R.ADAM_CASES[case][2]
    kw = {k: hp[k] for k in hp if k != "step0"}
    p, gs, m, v = R.adam_inputs(n, case)
    binds = [float(s["coef"]) < 1.0 for s in R.clip_adam_steps(p, gs, m, v, **hp)]
    assert binds == ([False] * 4 if hp["max_norm"] <= 0 else [True, False, True, False])
    bufs = _adam_state(p, m, v, off)
    (_, tp), (_, tm), (_, tv) = bufs
    nch = (n + R.CHUNK - 1) // R.CHUNK
    worst = 0.0
    for i, g in enumerate(gs):
        _, g_al = src(g)                                     # mvae_sumsq wants 16-byte alignment; mvae_clip_adam reads g at the offset
        _, g_view = src(g, off) if off else (None, g_al)
        partial = torch.full((nch,), NAN, device=dev)
        norm_out = torch.tensor([NAN, 0.0], device=dev)
        ops.sumsq(g_al, partial)
        ops.clip_adam(tp, g_view, tm, tv, partial, hp["grad_scale"], hp["max_norm"], hp["lr"], hp["b1"], hp["b2"], hp["eps"],
                      hp["step0"] + i, norm_out)
        ref = R.adam_step(p, g, m, v, step=hp["step0"] + i, **kw)          # from the state the kernel started this step with
        p, m, v = host(tp).numpy(), host(tm).numpy(), host(tv).numpy()
        no = host(norm_out).numpy()
        assert no[1] == 0.0 and not ref["skipped"]
        rs_ = [R.assert_within(no[0], ref["norm"], ref["norm"], R.K_ADAM, f"norm, step {i + 1}")]
        rs_ += [R.assert_within(got, ref[k], ref["s" + k], R.K_ADAM, f"{k}, step {i + 1}") for k, got in zip("pmv", (p, m, v))]
        worst = max([worst] + rs_)
    _edges_intact(bufs, off, n)
    report("clip_adam", worst)


def test_clip_adam_skips_a_step_with_a_non_finite_norm():
    """The poison slot g[n] (covered by mvae_sumsq, as the optimiser lays it out) holds NaN on step 2; on step 3 it is finite but the
    gradients are 1e20, whose squares overflow: both steps leave p, m, v bit for bit, are counted in norm_out[1], and reset the slot."""
    n, hp = 70001, R.ADAM_DEFAULT
    kw = {k: hp[k] for k in hp if k != "step0"}
    p, gs, m, v = R.adam_inputs(n, "defaults")
    gs = [np.append(g, np.float32(0.0)) for g in gs]
    gs[1][n] = np.nan
    gs[2][:n] = 1e20
    bufs = _adam_state(p, m, v, 0)
    (_, tp), (_, tm), (_, tv) = bufs
    nch = (n + 1 + R.CHUNK - 1) // R.CHUNK
    norm_out = torch.tensor([NAN, 0.0], device=dev)
    want_skips, worst = [0, 1, 2, 2], 0.0
    for i, g in enumerate(gs):
        gbuf, g_all = src(g)                                 # n + 1 elements: the gradients and the slot; NaN behind the slot
        partial = torch.full((nch,), NAN, device=dev)
        ops.sumsq(g_all, partial)
        ops.clip_adam(tp, g_all[:n], tm, tv, partial, hp["grad_scale"], hp["max_norm"], hp["lr"], hp["b1"], hp["b2"], hp["eps"], i + 1,
                      norm_out, poison_reset=g_all[n:])
        ref = R.adam_step(p, g, m, v, step=i + 1, **kw)
        p1, m1, v1 = host(tp).numpy(), host(tm).numpy(), host(tv).numpy()
        no, slot = host(norm_out).numpy(), host(gbuf).numpy()[n]
        assert no[1] == want_skips[i] and slot == 0.0, (i, no, slot)
        if i in (1, 2):
            assert ref["skipped"] and not np.isfinite(no[0])
            assert same_bits(p1, p) and same_bits(m1, m) and same_bits(v1, v), f"step {i + 1} was applied"
        else:
            worst = max([worst, R.assert_within(no[0], ref["norm"], ref["norm"], R.K_ADAM, "norm")] +
                        [R.assert_within(got, ref[k], ref["s" + k], R.K_ADAM, f"{k}, step {i + 1}") for k, got in zip("pmv", (p1, m1, v1))])
        p, m, v = p1, m1, v1
    _edges_intact(bufs, 0, n)
    report("clip_adam", worst)


# ------------------------------------------------------------------------------------------------ mvae_gather_rows_tb
GATHER_SHAPES = ((1, 1, 1, 1), (1, 9, 5, 3), (7, 1, 5, 6), (70, 9, 30, 512), (33, 17, 30, 1000))   # the last: beyond 2048 * 256 elements


@pytest.mark.parametrize("with_base", [True, False], ids=["base", "nobase"])
@pytest.mark.parametrize("B,L,V,W", GATHER_SHAPES, ids=[f"B{s[0]}L{s[1]}V{s[2]}W{s[3]}" for s in GATHER_SHAPES])
def test_gather_rows_tb_bit_exact(B, L, V, W, with_base):
    rs = np.random.RandomState(B * 100 + L)
    idx, _ = R.token_ids(rs, B, L, V)
    table, base = R.floats(rs, (V, W)), (R.floats(rs, (B, W)) if with_base else None)
    _, ttable = src(table)
    tbase = src(base)[1] if with_base else None
    n = B * L * W
    out = torch.full((n + 7,), SENT, device=dev)
    ops.gather_rows_tb(torch.from_numpy(idx).to(dev), ttable, out, B, L, V, W, base=tbase)
    got = host(out).numpy()
    assert same_bits(got[:n].reshape(B * L, W), R.gather_rows_tb(idx, B, L, V, table, base)) and (got[n:] == SENT).all()


# ------------------------------------------------------------------------------------------------ mvae_scatter_rows_tb, mvae_onehot_tb
SCATTER_SHAPES = (
    (1, 1, 1, 1, 1),
    (5, 14, 7, 9, 16),             # 70 rows: 2 parts of 35 rows, not a multiple of the 8-row round
    (96, 21, 30, 768, 832),        # the model's shape: two column slices
    (1031, 64, 5, 8, 8),           # 65984 rows: the 1024-part cap, 65 rows per part
    (7, 10, 12288, 3, 3),          # one-column slices, 48 KiB of LDS
)


@pytest.mark.parametrize("integers", [True, False], ids=["ints", "floats"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,L,V,W,ldd", SCATTER_SHAPES, ids=[f"B{s[0]}L{s[1]}V{s[2]}W{s[3]}" for s in SCATTER_SHAPES])
def test_scatter_rows_tb_matches_float64(B, L, V, W, ldd, dt, integers):
    rs = np.random.RandomState(B + L + V)
    idx, never = R.token_ids(rs, B, L, V)
    rows = B * L
    d = np.full((rows + 1, ldd), np.nan, np.float32)         # NaN in the columns [W, ldd) and in a row behind the matrix
    d[:rows, :W] = R.ints(rs, (rows, W)) if integers else R.floats(rs, (rows, W), bf16=dt == torch.bfloat16)
    td = torch.from_numpy(d).to(dev).to(dt)
    tidx = torch.from_numpy(idx).to(dev)
    ref, sa = R.scatter_rows_tb(idx, B, L, V, d, W)
    runs = []
    for _ in range(2):
        dtable = torch.full((V * W + 5,), NAN, device=dev)
        ops.scatter_rows_tb(tidx, td, dtable, B, L, V, W, ldd=ldd)
        h = host(dtable).numpy()
        assert np.isnan(h[V * W:]).all()
        runs.append(h[:V * W].reshape(V, W))
    assert same_bits(runs[0], runs[1]), "two runs differ"
    if integers:
        R.assert_exact(runs[0], ref)
    else:
        R.assert_sum_within(runs[0], ref, sa)
    if never >= 0:
        assert not runs[0][never].any(), "the row of an id that never occurs must be exactly 0"


@pytest.mark.parametrize("round_to", [8, 32])
@pytest.mark.parametrize("B,L,V", [s[:3] for s in SCATTER_SHAPES[:3]], ids=[f"B{s[0]}L{s[1]}V{s[2]}" for s in SCATTER_SHAPES[:3]])
def test_onehot_tb_bit_exact(B, L, V, round_to):
    rs = np.random.RandomState(B + L + V)
    idx, _ = R.token_ids(rs, B, L, V)
    ld, rows = (V + round_to - 1) // round_to * round_to, B * L
    out = torch.full((rows + 2, ld), SENT, device=dev).to(torch.bfloat16)
    before = host(out).view(torch.int16).numpy().copy()
    ops.onehot_tb(torch.from_numpy(idx).to(dev), out, B, L, V)
    got = host(out).view(torch.int16).numpy()
    want = np.where(R.onehot_tb(idx, B, L, V, ld) == 1.0, 0x3F80, 0).astype(np.int16)
    assert np.array_equal(got[:rows], want) and np.array_equal(got[rows:], before[rows:])


# ------------------------------------------------------------------------------------------------ mvae_bce_kl_loss_fwd
@functools.lru_cache(maxsize=2)
def _bce_fwd_ref(n, m, soft):
    return R.bce_kl_fwd(*R.bce_inputs(n, m, soft), R.MAX_LEN)


def _bce_fwd_run(recon, target, mu, logvar, off):
    (_, tr), (_, tt), (_, tm), (_, tl) = src(recon, off), src(target, off), src(mu), src(logvar)
    outs = []
    for _ in range(3):                                       # one workspace (ops keeps it), the ticket reset by the kernel itself
        out = torch.full((4,), NAN, device=dev)
        ops.bce_kl_loss_fwd(tr, tt, tm, tl, R.MAX_LEN, out[:3])
        outs.append(host(out).numpy())
        assert np.isnan(outs[-1][3])
    assert same_bits(outs[0], outs[1]) and same_bits(outs[0], outs[2]), "three calls on one workspace differ"
    return outs[0][:3]


@pytest.mark.parametrize("n,m,soft,off", [s + (soft, off) for s, soft, off in itertools.product(R.BCE_SHAPES, (False, True), (0, 1))],
                         ids=lambda x: str(int(x)))
def test_bce_kl_loss_fwd_aligned_and_unaligned(n, m, soft, off):
    """off = 1: the operands start 4 bytes off a 16-byte boundary, so the kernel takes its scalar path (n4 = 0); the two paths sum in
    different orders and each is compared with float64, not with the other."""
    ref, scale = _bce_fwd_ref(n, m, soft)
    got = _bce_fwd_run(*R.bce_inputs(n, m, soft), off)
    report("bce_kl_loss_fwd", R.assert_within(got, ref, scale, R.K_BCE_FWD, "out[0..2]"))


@pytest.mark.parametrize("off", [0, 1])
def test_bce_kl_loss_fwd_clamps_both_logs_at_minus_100(off):
    mu, logvar = R.bce_inputs(5, 7, False)[2:]
    ref, scale = R.bce_kl_fwd(R.BCE_CLAMP_P, R.BCE_CLAMP_T, mu, logvar, R.MAX_LEN)
    assert abs(ref[1] - R.MAX_LEN * (200.0 + np.log(2.0)) / 5) < 1e-9
    got = _bce_fwd_run(R.BCE_CLAMP_P, R.BCE_CLAMP_T, mu, logvar, off)
    report("bce_kl_loss_fwd", R.assert_within(got, ref, scale, R.K_BCE_FWD, "out[0..2]"))


# ------------------------------------------------------------------------------------------------ mvae_bce_kl_loss_bwd
def _bce_bwd_check(recon, target, mu, logvar, gout, null):
    n, m = recon.size, mu.size
    (_, tr), (_, tt), (_, tm), (_, tl) = src(recon), src(target), src(mu), src(logvar)
    tg = None if gout is None else torch.tensor([gout], dtype=torch.float32, device=dev)
    drecon = torch.full((n + 2,), NAN, device=dev)
    drecon[n:] = SENT
    lat = torch.full((2 * m + 2,), SENT, device=dev)         # dmu | dlogvar | two sentinels
    ops.bce_kl_loss_bwd(tr, tt, tm, tl, R.MAX_LEN, tg, drecon[:n], None if null == "dmu" else lat[:m],
                        None if null == "dlogvar" else lat[m:2 * m])
    (dr, dmu, dlv), (sr, smu, slv) = R.bce_kl_bwd(recon, target, mu, logvar, R.MAX_LEN, gout)
    hd, hl = host(drecon).numpy(), host(lat).numpy()
    assert (hd[n:] == SENT).all() and (hl[2 * m:] == SENT).all()
    worst = R.assert_within(hd[:n], dr, sr, R.K_BCE_BWD, "drecon")
    if null == "dmu":
        assert (hl[:m] == SENT).all(), "dmu = NULL, yet its neighbour's place was written"
    else:
        worst = max(worst, R.assert_within(hl[:m], dmu, smu, R.K_BCE_BWD, "dmu"))
    if null == "dlogvar":
        assert (hl[m:2 * m] == SENT).all(), "dlogvar = NULL, yet its neighbour's place was written"
    else:
        worst = max(worst, R.assert_within(hl[m:2 * m], dlv, slv, R.K_BCE_BWD, "dlogvar"))
    return worst


@pytest.mark.parametrize("gout", [None, 0.37], ids=["g1", "g0.37"])
@pytest.mark.parametrize("n,m", R.BCE_SHAPES[:5], ids=[f"n{s[0]}m{s[1]}" for s in R.BCE_SHAPES[:5]])
def test_bce_kl_loss_bwd_element_by_element(n, m, gout):
    worst = 0.0
    for soft in (False, True):
        a = R.bce_inputs(n, m, soft)
        for null in (None, "dmu", "dlogvar"):
            worst = max(worst, _bce_bwd_check(*a, gout, null))
    report("bce_kl_loss_bwd", worst)


@pytest.mark.parametrize("gout", [None, 0.37], ids=["g1", "g0.37"])
def test_bce_kl_loss_bwd_at_the_ends_of_the_unit_interval(gout):
    """p in {0, 1e-30, 1e-7, 0.5, 1 - 2^-24, 1} against t in {0, 1}: the max(p (1 - p), 1e-12) denominator."""
    mu, logvar = R.bce_inputs(12, 7, False)[2:]
    recon, target = np.repeat(R.BCE_EDGE_P, 2), np.tile(np.array([0.0, 1.0], np.float32), 6)
    report("bce_kl_loss_bwd", _bce_bwd_check(recon, target, mu, logvar, gout, None))


# ------------------------------------------------------------------------------------------------ mvae_softmax_tb_bwd / _fwd, plain kernels
@pytest.mark.parametrize("mode", ["f32_dlT", "bf16_dlT", "f32"])
@pytest.mark.parametrize("B,L,C,ldd", R.SOFTMAX_BWD_SHAPES, ids=[f"B{s[0]}L{s[1]}C{s[2]}" for s in R.SOFTMAX_BWD_SHAPES])
def test_softmax_tb_bwd_plain_kernel(B, L, C, ldd, mode):
    """The default dispatch takes the plain kernel for f32 and whenever dlT is given (what _DecoderFn.backward runs in f32 training)."""
    dt = torch.bfloat16 if mode.startswith("bf16") else torch.float32
    p, dp = R.softmax_inputs(B, L, C)
    rows, ldT = B * L, B * L + 3
    (_, tp), (_, tdp) = src(p), src(dp)
    dl = torch.full((rows + 2, ldd), SENT, device=dev).to(dt)
    dlT = torch.full((C + 1, ldT), SENT, device=dev).to(dt) if mode.endswith("dlT") else None
    sent = float(host(dl)[rows, 0])
    ops.softmax_tb_bwd(tp, tdp, dl, dlT, B, L, C)
    ref, _, scale = R.softmax_bwd(p, dp)
    got = host(dl).float().numpy()
    if dt == torch.float32:
        report("softmax_tb_bwd", R.assert_within(got[:rows, :C], ref, scale, R.K_SOFTMAX_BWD, "dl"))
    else:
        R.assert_within_bf16(got[:rows, :C], ref, scale, R.K_SOFTMAX_BWD, "dl")
    assert not got[:rows, C:].any(), "dl[:, C:ldd] must be zero"
    assert (got[rows:] == sent).all(), "rows of dl behind B*L were written"
    if dlT is not None:
        gT = host(dlT).float().numpy()
        assert same_bits(gT[:C, :rows], got[:rows, :C].T), "dlT is not the transpose of dl bit for bit"
        assert (gT[:, rows:] == sent).all() and (gT[C:] == sent).all(), "dlT written at or behind column B*L, or behind row C"


@pytest.mark.parametrize("B,L,C", R.SOFTMAX_FWD_SHAPES, ids=[f"B{s[0]}L{s[1]}C{s[2]}" for s in R.SOFTMAX_FWD_SHAPES])
def test_softmax_tb_fwd_padded_logits(B, L, C):
    """ldl = C + 5 (the plain kernel), NaN in the padding columns."""
    rs = np.random.RandomState(B + C)
    ldl, rows = C + 5, B * L
    logits = np.full((rows, ldl), np.nan, np.float32)
    logits[:, :C] = 2.0 * rs.standard_normal((rows, C))
    _, tl = src(logits)
    recon = torch.full((rows * C + 3,), SENT, device=dev)
    ops.softmax_tb_fwd(tl, ldl, recon, B, L, C)
    got = host(recon).numpy()
    assert (got[rows * C:] == SENT).all()
    err = np.abs(got[:rows * C].reshape(B, L, C).astype(np.float64) - R.softmax_fwd(logits, B, L, C))
    assert (err <= 2e-6).all(), err.max()
