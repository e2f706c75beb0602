"""The split-once 3 x bf16 GEMM kernels of csrc/gemm.hip (gemm_tn_x3_kernel, gemm_nt_x3_kernel) against the same contraction in numpy float64.

How they are reached through the C ABI:
  * TN: mvae_gemm_tn_f32_multi with ONE problem whose x3 is set is the single launcher's launch (launch_gemm_tn_f32 with x3 = true: the
    split-once kernel where M and N are multiples of 4, gemm_tn_f32_body<true, *> otherwise) -- row groups, the ones column and accumulate are
    all fields of the problem;
  * NT: mvae_gemm_nt with MVAE_F32X3 (plain rows, with and without accumulate) and the input gradient of mvae_conv1d_act_bwd with
    MVAE_CONV_BWD_X3 (A rows = overlapping windows of the zero-padded dz);
  * the whole layer: mvae_conv1d_act_bwd with MVAE_CONV_BWD_X3 | ACT_NONE (dz = dy exactly, so dx, dw and db are pure contractions).

Tolerance (derived, not tuned): each operand is hi + lo + e with |e| <= 2^-17 |x|, the form drops lo . lo <= 2^-16 |a| |b|, so one product is
off by at most 2^-15 |a| |b|; fp32 accumulation over K terms adds at most K 2^-24 sum |a| |b|; the factor 2 is the margin for the split-K
reduction's extra roundings:  |C - C64| <= 2 (2^-15 + K 2^-24) sum_r |a_r| |b_r|, element by element.  Before a case relies on it on the GPU,
`_cpu_x3_ok` checks with a numpy restatement of split_x3 (tile_pipe.hpp) that the three-product form of the case's own operands, summed in
float64, stays inside the 2^-15 part of it alone.  Seeded normal inputs; one case scaled by 1e3, one by 1e-3.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_ref as G                                 # noqa: E402
from molecular_vae_amd import ops, _lib as L         # noqa: E402

dev = torch.device("cuda")
NAN = float("nan")
SENT = 7.0
GUARD = 3


def _up(n, m):
    return (n + m - 1) // m * m


def _split_x3(x):
    """numpy restatement of split_x3: hi = x truncated to bf16, lo = bf16(x - hi) rounded to nearest even; float64 results."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    lo = G.bf16_round(x - hi)
    return hi.astype(np.float64), lo.astype(np.float64)


def _bound(Am, Bm, K):
    """Am [K, M], Bm [K, N] -> (C64, bound) of C = Am^T . Bm."""
    A, B = np.asarray(Am, np.float64), np.asarray(Bm, np.float64)
    return A.T @ B, 2.0 * (2.0 ** -15 + K * 2.0 ** -24) * (np.abs(A).T @ np.abs(B))


def _cpu_x3_ok(Am, Bm, what):
    A, B = np.asarray(Am, np.float64), np.asarray(Bm, np.float64)
    ah, al = _split_x3(Am)
    bh, bl = _split_x3(Bm)
    c3 = al.T @ bh + ah.T @ bl + ah.T @ bh
    s = np.abs(A).T @ np.abs(B)
    worst = float((np.abs(c3 - A.T @ B) / np.maximum(2.0 ** -15 * s, 1e-300)).max()) if s.size else 0.0
    print(f"{what}: CPU three-product form, worst error / (2^-15 s) = {worst:.3g}")
    assert worst <= 1.0, (what, worst)


def _check(got, Am, Bm, K, what, c0=None):
    ref, bound = _bound(Am, Bm, K)
    if c0 is not None:
        ref = ref + np.asarray(c0, np.float64)
        bound = bound + 2.0 ** -23 * np.abs(ref)            # the one fp32 addition onto c0
    ok, worst, where = G.within(got, ref, bound)
    print(f"{what}: worst |got - ref| / bound = {worst:.3g} at {where}")
    assert ok, (what, worst, where)


def _np(x):
    return x.float().cpu().numpy().astype(np.float64)


def _out(M, N, ldc, c0=None):
    buf = torch.full((M + GUARD, ldc), SENT, device=dev)
    buf[:M, :N] = NAN if c0 is None else torch.from_numpy(np.asarray(c0, np.float32)).to(dev)
    return buf


def _guard_ok(buf, M, N):
    return bool((buf[:M, N:] == SENT).all()) and bool((buf[M:] == SENT).all())


def _flat(vals_rows, R, L_, ld, group, gstride):
    """Flat operand buffer: row r of vals_rows at gemm_ref.row_starts, NaN wherever no row reads (rows must not overlap here)."""
    starts = G.row_starts(R, ld, group, gstride)
    n = (int(starts.max()) + L_ if R else L_) + 4
    flat = np.full(_up(n, 4), np.nan, np.float32)
    for r, s in enumerate(starts):
        flat[s:s + L_] = vals_rows[r]
    return flat


def _tn_x3(fa, fb, M, N, R, lda, ldb, cs=False, c0=None, cs0=None, a_group=0, a_gs=0, b_group=0, b_gs=0, want_slabs=None, want_rc=0):
    """One x3 problem through mvae_gemm_tn_f32_multi, twice into fresh buffers (bit-equal); returns (C [M, N], column sums or None)."""
    lib = L.load()
    runs = []
    for _ in range(2):
        a, b = torch.from_numpy(fa).to(dev), torch.from_numpy(fb).to(dev)
        c = _out(M, N, N + 5, c0)
        csv = None
        if cs:
            csv = torch.full((M + GUARD,), SENT, device=dev)
            csv[:M] = NAN if cs0 is None else torch.from_numpy(np.asarray(cs0, np.float32)).to(dev)
        q = L.GemmTnF32Problem()
        q.M, q.N, q.K = M, N, R
        q.A, q.lda, q.a_group, q.a_gstride = a.data_ptr(), lda, a_group, a_gs
        q.B, q.ldb, q.b_group, q.b_gstride = b.data_ptr(), ldb, b_group, b_gs
        q.C, q.ldc, q.accumulate = c.data_ptr(), N + 5, 1 if c0 is not None else 0
        q.colsum_out = csv.data_ptr() if cs else None
        q.colsum_accumulate, q.x3 = (1 if cs0 is not None else 0), 1
        arr = (L.GemmTnF32Problem * 1)(q)
        need = lib.mvae_gemm_tn_f32_multi_workspace(1, arr)
        if want_slabs is not None:
            assert need == (_up(want_slabs * M * (N + (1 if cs else 0)) * 4, 256) if want_slabs > 1 else 0), (need, want_slabs)
        ws = ops.Scratch.get(need, dev, tag="tn_x3_test") if need else None
        rc = lib.mvae_gemm_tn_f32_multi(1, arr, L.ptr(ws), need, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == want_rc, rc
        if rc:
            assert bool((c[:M, :N] != c[:M, :N]).all()) and _guard_ok(c, M, N)       # refused: nothing written
            return None, None
        assert _guard_ok(c, M, N) and (csv is None or bool((csv[M:] == SENT).all()))
        runs.append((c, csv))
    (c1, s1), (c2, s2) = runs
    assert torch.equal(c1.view(torch.int32), c2.view(torch.int32)) and (s1 is None or torch.equal(s1.view(torch.int32), s2.view(torch.int32)))
    return _np(c1[:M, :N]), (_np(s1[:M]) if cs else None)


def _plain(rs, M, N, R, scale=1.0, pad_a=4, pad_b=8):
    Am, Bm = (G.floats(rs, (R, M)) * np.float32(scale)), (G.floats(rs, (R, N)) * np.float32(scale))
    lda, ldb = _up(M, 4) + pad_a, _up(N, 4) + pad_b
    fa = np.full((R + 2, lda), np.nan, np.float32); fa[:R, :M] = Am
    fb = np.full((R + 2, ldb), np.nan, np.float32); fb[:R, :N] = Bm
    return Am, Bm, fa.reshape(-1), fb.reshape(-1), lda, ldb


def _tn_case(M, N, R, what, seed, cs=False, acc=False, scale=1.0, want_slabs=None):
    rs = np.random.RandomState(seed)
    Am, Bm, fa, fb, lda, ldb = _plain(rs, M, N, R, scale)
    _cpu_x3_ok(Am, Bm, what)
    c0 = G.floats(rs, (M, N)) * np.float32(scale * scale) if acc else None
    cs0 = G.floats(rs, M) * np.float32(scale) if (acc and cs) else None
    c, csv = _tn_x3(fa, fb, M, N, R, lda, ldb, cs=cs, c0=c0, cs0=cs0, want_slabs=want_slabs)
    _check(c, Am, Bm, R, what, c0)
    if cs:
        _check(csv[:, None], Am, np.ones((R, 1), np.float32), R, what + ": column sums", None if cs0 is None else cs0[:, None])


# TN stage = 64 reduction rows = two 32-row steps; the split over K is the exact-f32 plan's (from 16 steps on, at least 8 steps per slab)
def test_tn_ragged_tile_and_last_stage_unsplit():
    """M = 120 (one whole 64-row tile + 56 rows), N = 2160 (16 whole 128-wide tiles + 112 columns; with the ones column 2161: it opens the
    17th tile's 113th column), K = 3 stages + 5 rows: one slab."""
    _tn_case(120, 2160, 3 * 64 + 5, "120 x 2160, K = 197, ones column", 1, cs=True, want_slabs=1)
    _tn_case(120, 2160, 3 * 64 + 5, "120 x 2160, K = 197, plain", 2, want_slabs=1)


def test_tn_split_k_slabs_and_reduce():
    """K = 517 rows = 17 steps of 32: two slabs of 9 and 8 steps (288 rows: the first ends half way through its fifth stage; 229 rows: the
    last step ragged), summed by gemm_splitk_reduce_kernel; inputs x 1e3."""
    _tn_case(120, 2160, 8 * 64 + 5, "120 x 2160, K = 517: 2 slabs, ones column, x 1e3", 3, cs=True, scale=1e3, want_slabs=2)


@pytest.mark.parametrize("cs", [False, True])
def test_tn_64_row_tile_with_and_without_the_ones_column(cs):
    """M = 64, N = 1152 (the conv_2 / conv_3 shape class): the 64 x 128 tile, 9 whole tiles; the ones column opens a 10th.  Inputs x 1e-3."""
    _tn_case(64, 1152, 3 * 64 + 5, f"64 x 1152, K = 197, ones column {cs}, x 1e-3", 4 + cs, cs=cs, scale=1e-3, want_slabs=1)


def test_tn_row_groups_make_it_a_convolution():
    """A grouped by Wout with a padded group stride, B as overlapping windows (b_group = Wout, ldb = ldx, b_gstride = x_bs): 3 molecules,
    W = 24, k = 18, Cin = 8 -> Wout = 7, N = k ldx = 144, K = 21; groups of 7 rows against passes of 8 (A, B) rows per thread."""
    Bn, W, k, Cin, Cout = 3, 24, 18, 8, 12
    Wout, ldx, lda = W - k + 1, 8, 16
    x_bs, a_gs = W * ldx + 8, Wout * lda + 8
    R, N = Bn * Wout, k * ldx
    rs = np.random.RandomState(6)
    Am = G.floats(rs, (R, Cout))
    fa = _flat(Am, R, Cout, lda, Wout, a_gs)
    fb = np.full(Bn * x_bs + 4, np.nan, np.float32)
    for b in range(Bn):
        fb[b * x_bs:b * x_bs + W * ldx] = G.floats(rs, W * ldx)
    Bm = G.rows(fb, R, N, ldx, Wout, x_bs)
    assert np.isfinite(Bm).all()
    _cpu_x3_ok(Am, Bm, "row groups")
    c, csv = _tn_x3(fa, fb, Cout, N, R, lda, ldx, cs=True, a_group=Wout, a_gs=a_gs, b_group=Wout, b_gs=x_bs, want_slabs=1)
    _check(c, Am, Bm, R, "row groups (3 molecules, W 24, k 18, Cin 8)")
    _check(csv[:, None], Am, np.ones((R, 1), np.float32), R, "row groups: column sums")


def test_tn_accumulates_onto_c_and_the_sums():
    _tn_case(120, 260, 2 * 64 + 9, "120 x 260, K = 137, C and column sums accumulated", 7, cs=True, acc=True)
    _tn_case(64, 132, 70, "64 x 132, K = 70, C accumulated", 8, acc=True)


def test_tn_shapes_the_new_loop_refuses():
    """M = 118 and N = 2158 are no multiples of 4: the launcher keeps them on gemm_tn_f32_body<true, *> and the answer is right all the same.
    A leading dimension that is no multiple of 4 is refused by every f32 TN launch (their float4 row loads), before and after this kernel:
    MVAE_ERR_INVALID with nothing written."""
    _tn_case(118, 2160, 3 * 64 + 5, "M = 118: fallback", 9, cs=True)
    _tn_case(120, 2158, 3 * 64 + 5, "N = 2158: fallback", 10)
    rs = np.random.RandomState(11)
    Am, Bm, fa, fb, lda, ldb = _plain(rs, 120, 64, 70, pad_a=5)
    assert lda % 4 == 1
    _tn_x3(fa, fb, 120, 64, 70, lda, ldb, want_rc=-1)


# ---- NT
def _nt_plain(M, N, K, what, seed, acc):
    rs = np.random.RandomState(seed)
    A, B = G.floats(rs, (M, K)), G.floats(rs, (N, K))
    _cpu_x3_ok(A.T, B.T, what)
    c0 = G.floats(rs, (M, N)) if acc else None
    runs = []
    for _ in range(2):
        a = torch.full((M + 1, K + 4), NAN, device=dev); a[:M, :K] = torch.from_numpy(A).to(dev)
        b = torch.full((N + 1, K + 8), NAN, device=dev); b[:N, :K] = torch.from_numpy(B).to(dev)
        c = _out(M, N, N + 5, c0)
        ops.gemm_nt(a, b, c, M, N, K, lda=K + 4, ldb=K + 8, ldc=N + 5, accumulate=acc, x3=True)
        torch.cuda.synchronize()
        assert _guard_ok(c, M, N)
        runs.append(c)
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
    _check(_np(runs[0][:M, :N]), A.T, B.T, K, what, c0)


@pytest.mark.parametrize("acc", [False, True])
def test_nt_plain_rows_with_and_without_accumulate(acc):
    """(424, 120, 2160): three whole 128-row tiles + 40 rows, the 128-wide tile ragged at 120, 33 whole stages + 48 k.  (136, 64, 1152): the
    128 x 64 tile, one whole tile + 8 rows, 18 whole stages."""
    _nt_plain(3 * 128 + 40, 120, 2160, f"NT 424 x 120 x 2160, accumulate {acc}", 20 + acc, acc)
    _nt_plain(2 * 64 + 8, 64, 1152, f"NT 136 x 64 x 1152, accumulate {acc}", 22 + acc, acc)


def test_nt_64_row_tile_beyond_512_tiles_of_128():
    """More than 512 tiles of 128 x 128 (M = 512 x 128 + 72 rows, N = 120): make_plan takes the 64 x 128 tile, 1026 tiles, the last of 8 rows;
    K = 132: two whole stages + one chunk."""
    _nt_plain(512 * 128 + 72, 120, 132, "NT 65608 x 120 x 132: 64 x 128 tiles", 24, False)


def _conv_bwd(Bn, W, Cin, Cout, k, what, seed, dw=True):
    """mvae_conv1d_act_bwd(ACT_NONE | X3) with ldx = Cin, ldo = Cout: dx (NT on windows of the padded dz), dw and db (TN, both grouped)."""
    rs = np.random.RandomState(seed)
    ldx, ldo = Cin, Cout
    Wout, x_bs = W - k + 1, W * ldx + 8
    Wp, M = Wout + 2 * (k - 1), Bn * (W - k + 1)
    xflat = np.full(Bn * x_bs, np.nan, np.float32)
    for b in range(Bn):
        xflat[b * x_bs:b * x_bs + W * ldx] = G.floats(rs, W * ldx)
    w = G.floats(rs, (Cout, Cin, k)); dy = G.floats(rs, (M, Cout))
    wq = np.ascontiguousarray(w[:, :, ::-1].transpose(1, 2, 0)).reshape(Cin, k * ldo)
    Xm = G.rows(xflat, M, k * ldx, ldx, Wout, x_bs)
    zref = np.zeros((Bn, Wp, ldo), np.float32); zref[:, k - 1:k - 1 + Wout, :] = dy.reshape(Bn, Wout, Cout)
    Zm = G.rows(zref.reshape(-1), Bn * W, k * ldo, ldo, W, Wp * ldo)
    _cpu_x3_ok(Zm.T, wq.T, what + ": dx")
    if dw:
        _cpu_x3_ok(dy, Xm, what + ": dw")
    runs = []
    for _ in range(2):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)        # noqa: E731
        dzp = torch.full((Bn * Wp + GUARD, ldo), NAN, device=dev); dzp[Bn * Wp:] = SENT
        dwt = torch.full((Cout * Cin * k + GUARD,), NAN, device=dev); dwt[Cout * Cin * k:] = SENT
        db = torch.full((Cout + GUARD,), SENT, device=dev); db[:Cout] = NAN
        dx = _out(Bn * W, Cin, ldx + 4)
        ops.conv1d_selu_bwd(Bn, W, Cin, ldx, x_bs, Cout, ldo, k, t(dy), torch.zeros(M, ldo, device=dev), t(xflat), t(wq), dzp,
                            dwt if dw else None, db if dw else None, dx, ldx + 4, act=L.ACT_NONE, x3=True)
        torch.cuda.synchronize()
        assert _guard_ok(dx, Bn * W, Cin) and bool((dzp[Bn * Wp:] == SENT).all()) and bool((dwt[Cout * Cin * k:] == SENT).all()) and bool((db[Cout:] == SENT).all())
        runs.append((dzp, dwt, db, dx))
    for u, v in zip(*runs):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), "second run differs"
    dzp, dwt, db, dx = runs[0]
    assert np.array_equal(_np(dzp[:Bn * Wp]), zref.reshape(Bn * Wp, ldo).astype(np.float64))
    _check(_np(dx[:Bn * W, :Cin]), Zm.T, wq.T, k * ldo, what + ": dx")
    if dw:
        got = _np(dwt[:Cout * Cin * k]).reshape(Cout, Cin, k).transpose(0, 2, 1).reshape(Cout, k * ldx)
        _check(got, dy, Xm, M, what + ": dw")
        _check(_np(db[:Cout])[:, None], dy, np.ones((M, 1), np.float32), M, what + ": db")


def test_nt_windows_of_the_padded_dz():
    """The two NT shapes with A rows as conv.hip passes them (a_group = W, a_gstride = Wp ldo): B W = 8 x 53 = 424 rows, N = Cin = 120,
    K = k ldo = 18 x 120 = 2160; and 4 x 34 = 136 rows, N = 64, K = 18 x 64 = 1152."""
    _conv_bwd(8, 53, 120, 120, 18, "dX 424 x 120 x 2160 on windows", 30, dw=False)
    _conv_bwd(4, 34, 64, 64, 18, "dX 136 x 64 x 1152 on windows", 31, dw=False)


@pytest.mark.parametrize("layer", [(120, 120, 120, 18), (103, 120, 64, 18), (86, 64, 64, 18)], ids=["conv_1", "conv_2", "conv_3"])
def test_whole_layer_backward_at_the_real_channel_counts(layer):
    """B = 4 at the three layers' (W, Cin, Cout, k): dx, dw and db against float64 under the bound with K = k ldo (dx) and K = B Wout (dw, db)."""
    W, Cin, Cout, k = layer
    _conv_bwd(4, W, Cin, Cout, k, f"layer W = {W}, Cin = {Cin}, Cout = {Cout}", 40 + Cin + Cout)
