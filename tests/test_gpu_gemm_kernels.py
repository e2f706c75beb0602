"""The GEMM entries called directly (ops.gemm_nt / gemm_tn / gemm_tn_f32_colsum / gemm_tn_colsum / gemm_tn_grouped / TnF32Batch and the
conv entries with ACT_NONE, which are pure grouped GEMMs) against tests/gemm_ref.py, element by element, in every branch of the three
launch plans of csrc/gemm.hip (make_plan, make_plan_tn, make_plan_tn_f32) and every epilogue.  Each case's comment names the branch it
reaches; where the branch shows outside the library -- the split count, through the *_workspace entry and the slab size M * N * 4 -- the
case asserts it.  K-step ke = KB / sizeof(T): 32 elements for f32, 64 for bf16.

How every case is run (`_nt`, `_tn`, `_conv`):
  * operands carry NaN in every pad column and pad row the kernel must not read.  Where the contract is that a pad holds zero the case says so:
    the NT entry reads whole 16-byte chunks, so the elements K .. roundup(K, 16 bytes) - 1 of each row of A and B are zero (include/mvae.h);
    the conv entries take pad channels [Cin, ldx) and [Cout, ldo) as zero.  The bf16 TN kernel reads its pad columns (they only reach
    accumulators of rows / columns outside the matrix, which are not stored) and gets zeros for rows >= K from the buffer descriptor.
  * C and the column-sum vector carry a sentinel in the columns N .. ldc - 1 and in guard rows behind, compared exactly afterwards;
  * the call is made twice into fresh buffers and the two results must agree bit for bit.

Two kinds of input (gemm_ref.py): small integers, where the kernel must return the float64 integer result exactly, whatever the tile, split
or order (ACT_NONE / ACT_RELU; a bf16 C: that integer rounded once) -- compared with numpy.array_equal, no tolerance -- and random floats
rounded to the storage type, bounded per element by gemm_ref.nt_bound: 4 rho s_ij + 2^-23 s_ij with the floor rho from the two CPU
references alone, + X3_C . 2^-16 s_ij for the three-bf16-product form (X3_C = 8.04, derived in gemm_ref's docstring from split_x3: the
dropped lo . lo term is <= 4.032 . 2^-16 |a b|, the rounding of lo costs <= 4 . 2^-16 |a b|), + one bf16 ulp for a bf16 C, the SELU bound
of the helper suite.  Activations: the bound passes through act's global Lipschitz constant, which holds across the kink at 0.

rho observed (CPU figures: they come from the two CPU references alone and are printed by every float case with `-s`), over the 257 float
comparisons of this file: 0 in 22 of them (K = 4 or 8 on a handful of elements, where the short float32 sums happen to be exact; R = 0
and R = 1), otherwise 9.3e-9 .. 2.1e-7, i.e. 0.08 .. 1.7 times 2^-23: what a K-step-wise float32 sum leaves.  Where rho is 0 the bound is the
2^-23 s_ij term alone.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_ref as G                                 # noqa: E402
from molecular_vae_amd import ops, _lib as L         # noqa: E402

dev = torch.device("cuda")
F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
SENT = 7.0
GUARD = 3
NONE, SELU, RELU = L.ACT_NONE, L.ACT_SELU, L.ACT_RELU
ACTS = {NONE: "none", RELU: "relu", SELU: "selu"}
KEY = {F32: "f32", BF16: "bf16"}


def _ke(dt):
    return G.KE[KEY[dt]]


def _epc(dt):
    return 4 if dt == F32 else 8                      # elements per 16-byte chunk


def _up(n, m):
    return (n + m - 1) // m * m


def _t(a, dt=F32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev).to(dt)


def _bits(x):
    return x.contiguous().view(torch.int32 if x.dtype == F32 else torch.int16)


def _op(a, ld, dt, extra_rows=0, zero_to=0):
    """[R + extra_rows, ld]: the values in [:R, :L], zeros in columns L .. zero_to - 1 (a pad the contract wants zero), NaN everywhere else."""
    R, L_ = a.shape
    buf = torch.full((R + extra_rows, ld), NAN, device=dev, dtype=dt)
    if zero_to > L_:
        buf[:R, L_:zero_to] = 0
    if L_:
        buf[:R, :L_] = _t(a, dt)
    return buf


def _out(M, N, ldc, dt, c0=None):
    """[M + GUARD, ldc]: NaN (or c0) where the kernel writes, the sentinel in columns N.. and in the guard rows."""
    buf = torch.full((M + GUARD, ldc), SENT, device=dev, dtype=dt)
    buf[:M, :N] = NAN if c0 is None else _t(c0, dt)
    return buf


def _guard_ok(buf, M, N):
    return bool((buf[:M, N:] == SENT).all()) and bool((buf[M:] == SENT).all())


def _vec(M, c0=None):
    v = torch.full((M + GUARD,), SENT, device=dev)
    v[:M] = NAN if c0 is None else _t(c0)
    return v


def _np(x):
    return x.float().cpu().numpy().astype(np.float64)


def _exact(got, ref, what, c_bf16=False):
    want = G.exact_out(ref, c_bf16)
    same = np.array_equal(got.astype(np.float32), want)
    assert same, (what, np.argwhere(got.astype(np.float32) != want)[:4].tolist())


def _close(got, ref, bound, rho, what):
    ok, worst, where = G.within(got, ref, bound)
    print(f"{what}: rho = {rho:.3g}, worst |got - ref| / bound = {worst:.3g} at {where}")
    assert ok, (what, worst, where)


def _splits_rule(tiles, ksteps, tile_cap, target=256):
    """The split rule the three plans share, restated: split only when tiles < tile_cap and ksteps >= 16; then ceil(target / tiles) slabs, at
    least 8 K-steps each, at most 64, re-balanced to equal step counts."""
    ksteps = max(ksteps, 1)
    s = 1
    if tiles < tile_cap and ksteps >= 16:
        s = max(1, min(-(-target // tiles), ksteps // 8, 64))
    per = -(-ksteps // s)
    return -(-ksteps // per), per


def _nt_splits(M, N, K, dt, x3=False):
    b = L.load().mvae_gemm_nt_workspace(M, N, K, L.MVAE_F32X3 if x3 else L.dt_code(dt))
    assert b % (M * N * 4) == 0
    return max(b // (M * N * 4), 1)


def _tn_splits(M, N, K):
    b = L.load().mvae_gemm_tn_workspace(M, N, K, L.MVAE_BF16)
    assert b % (M * N * 4) == 0
    return max(b // (M * N * 4), 1)


# =====================================================================================================================
# NT: mvae_gemm_nt
# =====================================================================================================================
def _nt(A, B, dt, bias=None, act=NONE, c_dt=F32, c0=None, lda=None, ldb=None, x3=False, pad_c=5):
    """Two runs of ops.gemm_nt on fresh buffers; returns C[:M, :N] as float64.  Contract pads: columns K .. roundup(K, chunk) - 1 zero."""
    (M, K), N = A.shape, B.shape[0]
    epc = _epc(dt)
    Kc = _up(K, epc)
    lda = Kc + epc if lda is None else lda
    ldb = Kc + 2 * epc if ldb is None else ldb
    ldc = N + pad_c
    bias_t = None if bias is None else _t(bias)
    res = []
    for _ in range(2):
        a, b = _op(A, lda, dt, extra_rows=2, zero_to=min(Kc, lda)), _op(B, ldb, dt, extra_rows=2, zero_to=min(Kc, ldb))     # + 2 rows of NaN behind
        c = _out(M, N, ldc, c_dt, c0)
        ops.gemm_nt(a, b, c, M, N, K, lda=lda, ldb=ldb, ldc=ldc, bias=bias_t, act=act, accumulate=c0 is not None, x3=x3)
        torch.cuda.synchronize()
        assert _guard_ok(c, M, N), "sentinel behind C overwritten"
        res.append(c)
    assert torch.equal(_bits(res[0]), _bits(res[1])), "second run differs"
    return _np(res[0][:M, :N])


def _nt_both(shape, dt, seed, what, bias=False, act=NONE, c_dt=F32, acc=False, x3=False, kinds=("int", "float"), bound_x3=None, **kw):
    """One NT case on the integer recipe (exact) and on random floats (per-element bound)."""
    M, N, K = shape
    rs = np.random.RandomState(seed)
    for kind in kinds:
        if kind == "int" and act == SELU:
            continue
        gen = G.ints if kind == "int" else (lambda r, s: G.floats(r, s, bf16=dt == BF16))
        A, B = gen(rs, (M, K)), gen(rs, (N, K))
        bv = (G.ints(rs, N) if kind == "int" else G.floats(rs, N)) if bias else None
        c0 = (G.ints(rs, (M, N)) if kind == "int" else G.floats(rs, (M, N))) if acc else None
        got = _nt(A, B, dt, bias=bv, act=act, c_dt=c_dt, c0=c0, x3=x3, **kw)
        if kind == "int":
            _exact(got, G.nt(A, B, bv, act, c0), f"{what} [int]", c_dt == BF16)
        else:
            ref, bound, rho = G.nt_bound(A, B, _ke(dt), bias=bv, act=act, c0=c0, c_bf16=c_dt == BF16, x3=x3 if bound_x3 is None else bound_x3)
            _close(got, ref, bound, rho, f"{what} [float]")


NT_PLAN_CASES = [
    # shape, splits, branch
    ((17, 9, 40), 1, "64 x 64, one tile, unsplit (tiles 1, ksteps 2 / 1); register-staged loop (K < 4 ke)"),
    ((1, 5, 8), 1, "64 x 64, M = 1; register-staged, K < ke"),
    ((4, 2, 4), 1, "64 x 64, N = 2, K = 4 (the 2-d model's head): one 16-byte chunk (f32) / half a chunk (bf16: zero chunk tail)"),
    ((70, 33, 16), 1, "64 x 64, 2 x 1 tiles, ragged in both; K < ke"),
    ((65, 130, 100), 1, "64 x 64, 2 x 3 tiles, one row / two columns in the last tiles; K not a multiple of the chunk for bf16"),
]


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", NT_PLAN_CASES, ids=[f"{c[0][0]}x{c[0][1]}x{c[0][2]}" for c in NT_PLAN_CASES])
def test_nt_64_tile_unsplit(case, dt):
    shape, splits, what = case
    assert _nt_splits(*shape, dt) == splits
    _nt_both(shape, dt, 11, what, bias=True, act=RELU)
    _nt_both(shape, dt, 12, what)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_nt_split_k_threshold_and_last_slab(dt):
    """make_plan splits when tiles < 128 and ksteps >= 16: ksteps 15 -> 1 slab, 16 -> 2 slabs of 8 steps (LDS-direct loop, kper % ke == 0),
    16 steps with K one element short -> 2 slabs in the register-staged loop, 73 steps -> 9 slabs of 9, 9, ..., 1 steps (the last slab is ONE
    K-step: the 4-deep LDS ring is never filled)."""
    ke = _ke(dt)
    M, N = 70, 33                                          # 2 x 1 tiles of 64 x 64
    for K, want in ((15 * ke, 1), (16 * ke, 2), (16 * ke - 1, 2), (73 * ke, 9)):
        assert _nt_splits(M, N, K, dt) == want == _splits_rule(2, -(-K // ke), 128)[0], (K, want)
        _nt_both((M, N, K), dt, K, f"64 x 64, ksteps {-(-K // ke)} -> {want} slab(s), K = {K}", kinds=("int",))
    _nt_both((M, N, 16 * ke), dt, 5, "64 x 64, 2 slabs, reduce kernel", bias=True, act=SELU, kinds=("float",))
    # the other condition, tiles < 128, on both sides at 16 steps: 127 x 1 tiles of 64 x 64 (N = 40 > 32 keeps the f32 128 x 32 tile away) against 128 x 1
    assert _nt_splits(127 * 64, 40, 16 * ke, dt) == 2 and _nt_splits(127 * 64 + 1, 40, 16 * ke, dt) == 1
    _nt_both((127 * 64, 40, 16 * ke), dt, 7, "127 tiles, 16 steps: 2 slabs", bias=True, kinds=("int",))
    _nt_both((127 * 64 + 1, 40, 16 * ke), dt, 8, "128 tiles, 16 steps: unsplit", bias=True, kinds=("int",))
    _nt_both((M, N, 73 * ke), dt, 6, "64 x 64, 9 slabs, last one K-step", kinds=("float",))


def test_nt_f32_128x32_tile_and_its_neighbours():
    """f32 only: N <= 32 and M >= 128 take the 128 x 32 tile (the conv stack's 9 / 10 channels); N = 33 or M = 127 fall back to 64 x 64.
    K = 96 < 4 ke: register-staged loop; K = 128: the LDS-direct loop on the 128 x 32 tile; 130 rows: a second, ragged tile row.
    None of these splits (ksteps < 16), so the plan is not observable from outside: the three shapes differ only in the kernel taken."""
    for shape, what in (((128, 32, 96), "128 x 32 tile, register-staged"), ((128, 33, 96), "64 x 64 (N = 33)"), ((127, 32, 96), "64 x 64 (M = 127)"),
                        ((130, 10, 128), "128 x 32 tile, LDS-direct, ragged rows and columns"),
                        ((130, 32, 16 * 32), "128 x 32 tile, 2 tiles, split-K: 2 slabs")):
        assert _nt_splits(*shape, F32) == (2 if shape[2] == 512 else 1)
        _nt_both(shape, F32, shape[0], what, bias=True, act=RELU)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_nt_128_tile_smallest_shape(dt):
    """128 x 128 needs t128 >= 192 and eff(t128) >= 0.8 eff(t64).  t128 = 192 gives eff 0.75, so t64 must leave its last round of 256 emptier
    than 0.9375: one tile row and 192 tile columns, N = 191 * 128 + 1 = 24449 -> t64 = 383, eff(t64) = 383 / 512 = 0.748: taken.  M = 3 rows
    of a 128-row tile; K = 4 ke (LDS-direct) and 4 ke + 1 (register-staged).  192 tiles >= 128: no split."""
    ke = _ke(dt)
    for K in (4 * ke, 4 * ke + 1):
        assert _nt_splits(3, 24449, K, dt) == 1
        _nt_both((3, 24449, K), dt, K, f"128 x 128, 192 tiles, K = {K}", bias=True, kinds=("int",))
    _nt_both((3, 24449, 4 * ke), dt, 3, "128 x 128, LDS-direct", bias=True, act=SELU, kinds=("float",))


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_nt_main_loop_selection(dt):
    """The LDS-direct ("pipe") loop needs K % ke == 0, K >= 4 ke, lda / ldb multiples of 16 bytes; everything else is register-staged."""
    ke, epc = _ke(dt), _epc(dt)
    M, N = 70, 33
    _nt_both((M, N, 4 * ke), dt, 1, "pipe: K = 4 ke, the smallest it takes", bias=True)
    _nt_both((M, N, 4 * ke - 1), dt, 2, "register-staged: K = 4 ke - 1 (zero chunk tail)", bias=True)
    _nt_both((M, N, 4 * ke + 1), dt, 3, "register-staged: K = 4 ke + 1 (one element in a fifth step)", bias=True)
    _nt_both((M, N, 5), dt, 4, "register-staged: K < ke", bias=True)
    _nt_both((M, N, 8 * ke), dt, 5, "pipe: two turns of the 4-deep ring")
    K = 4 * ke
    _nt_both((M, N, K), dt, 6, "register-staged: lda one element off the 16-byte rule", lda=K + 1, ldb=K + epc)
    _nt_both((M, N, K), dt, 7, "register-staged: ldb one element off the 16-byte rule", lda=K + epc, ldb=K + 1)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_nt_k_zero(dt):
    """K == 0: one empty pass (ksteps is clamped to 1, no split); the epilogue writes act(bias) -- zeros without a bias -- and under
    accumulate leaves C as it was (+ bias).  A and B are all NaN: nothing of them may be read."""
    M, N = 17, 9
    assert _nt_splits(M, N, 0, dt) == 1
    rs = np.random.RandomState(0)
    A, B = np.zeros((M, 0), np.float32), np.zeros((N, 0), np.float32)
    bias, c0 = G.floats(rs, N), G.floats(rs, (M, N))
    for act in (NONE, RELU, SELU):
        got = _nt(A, B, dt, bias=bias, act=act)
        want = G.act_fn(np.broadcast_to(bias.astype(np.float64), (M, N)), act)
        if act == SELU:
            assert G.within(got, want, G.bound_out(0.0, want, SELU))[0]           # nothing summed: the SELU term of gemm_ref alone
        else:
            assert np.array_equal(got, want), act
    assert np.array_equal(_nt(A, B, dt), np.zeros((M, N)))
    assert np.array_equal(_nt(A, B, dt, c0=c0), c0.astype(np.float64))
    assert np.array_equal(_nt(A, B, dt, c0=c0, bias=bias), (c0 + bias[None, :]).astype(np.float64))      # one fp32 add: numpy's is the same
    assert np.array_equal(_nt(A, B, dt, c_dt=BF16, bias=bias), np.broadcast_to(G.bf16_round(bias).astype(np.float64), (M, N)))


@pytest.mark.parametrize("split", [False, True], ids=["unsplit", "reduce-kernel"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_nt_epilogues(dt, split):
    """{no bias, bias} x {NONE, RELU, SELU} x {f32 C, bf16 C}, accumulate (f32 C), ldc = N + 5 (every case) -- once in the GEMM kernel's own
    epilogue (70 x 33 x 4 ke, 1 slab) and once in gemm_splitk_reduce_kernel, which restates all of it (70 x 33 x 16 ke, 2 slabs)."""
    ke = _ke(dt)
    shape = (70, 33, (16 if split else 4) * ke)
    assert _nt_splits(*shape, dt) == (2 if split else 1)
    seed = 0
    for bias in (False, True):
        for act in (NONE, RELU, SELU):
            for c_dt in (F32, BF16):
                seed += 1
                _nt_both(shape, dt, seed, f"bias={bias} act={ACTS[act]} C={KEY[c_dt]}", bias=bias, act=act, c_dt=c_dt)
            _nt_both(shape, dt, 100 + seed, f"accumulate, bias={bias} act={ACTS[act]}", bias=bias, act=act, acc=True)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_nt_bf16_c_with_accumulate_is_refused_before_any_write(dt):
    M, N, K = 17, 9, 40
    rs = np.random.RandomState(1)
    a, b = _op(G.ints(rs, (M, K)), K, dt), _op(G.ints(rs, (N, K)), K, dt)
    c = _out(M, N, N + 5, BF16, G.ints(rs, (M, N)))
    before = c.clone()
    with pytest.raises(L.MvaeError, match=r"-1 \(invalid argument\)"):
        ops.gemm_nt(a, b, c, M, N, K, ldc=N + 5, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(c), _bits(before))


def test_nt_x3_on_the_pipe_and_its_fallback_to_exact_f32():
    """x3 exists in the LDS-direct loop only.  (70, 33, 128) and the split (70, 33, 512) take it: bound = fp32 bound + X3_C . 2^-16 s_ij, and the
    ordering exact f32 < x3 < plain bf16 of the older test holds on the worst element's error in units of s_ij.  (70, 33, 127), K < 4 ke and
    a misaligned lda refuse the loop: the launcher runs exact f32, held to the exact-f32 bound.  So does the f32 128 x 32 tile (N <= 32,
    M >= 128), which has no x3 instantiation even where it takes the LDS-direct loop: (130, 10, 128).  Integers: exact either way."""
    for shape in ((70, 33, 128), (70, 33, 512)):
        assert _nt_splits(*shape, F32, x3=True) == _nt_splits(*shape, F32) == (2 if shape[2] == 512 else 1)
        _nt_both(shape, F32, 21, f"x3, pipe, K = {shape[2]}", bias=True, act=RELU, x3=True)
        rs = np.random.RandomState(22)
        A, B = G.floats(rs, shape[::2]), G.floats(rs, shape[1:])
        s, ref = G.nt_scale(A, B), G.nt(A, B)
        e = {}
        e["f32"] = (np.abs(_nt(A, B, F32) - ref) / s).max()
        e["x3"] = (np.abs(_nt(A, B, F32, x3=True) - ref) / s).max()
        e["bf16"] = (np.abs(_nt(G.bf16_round(A), G.bf16_round(B), BF16) - ref) / s).max()
        print("worst error / s_ij:", e)
        assert e["f32"] < e["x3"] < e["bf16"], e
    _nt_both((70, 33, 127), F32, 23, "x3 asked, K % ke != 0: exact f32", bias=True, x3=True, bound_x3=False)
    _nt_both((70, 33, 96), F32, 24, "x3 asked, K < 4 ke: exact f32", x3=True, bound_x3=False)
    _nt_both((70, 33, 128), F32, 25, "x3 asked, lda misaligned: exact f32", x3=True, bound_x3=False, lda=129, ldb=132)
    _nt_both((130, 10, 128), F32, 26, "x3 asked, 128 x 32 tile (LDS-direct): exact f32", bias=True, x3=True, bound_x3=False)


# =====================================================================================================================
# Row groups through the conv entries with ACT_NONE (mvae_conv1d_act_fwd / _bwd): pure grouped GEMMs
# =====================================================================================================================
def _conv(B, W, Cin, ldx, gap, Cout, ldo, k, what, kind="int", bwd=True, seed=0):
    """Forward (NT, A rows = overlapping windows: group = Wout, gstride = x_bs, ld = ldx), then dX (NT on the zero-padded dzp: group = W,
    gstride = Wp * ldo) and dW / db (f32 TN, both operands grouped, db as the ones column), all against gemm_ref.rows + nt / tn.  Contract
    pads held at zero: channels [Cin, ldx) of x, [Cout, ldo) of wq's rows, pad rows of wp; NaN: the gap behind each batch of x, dy's pad
    channels, y's pad columns (sentinel), everything the kernels write."""
    rs = np.random.RandomState(seed)
    gen = G.ints if kind == "int" else G.floats
    Wout, x_bs = W - k + 1, W * ldx + gap
    Wp = Wout + 2 * (k - 1)
    x = np.zeros((B, W, ldx), np.float32); x[:, :, :Cin] = gen(rs, (B, W, Cin))
    w = gen(rs, (Cout, Cin, k)); bias = gen(rs, Cout); dy = gen(rs, (B * Wout, Cout))
    wp = np.zeros((Cout, k, ldx), np.float32); wp[:, :, :Cin] = w.transpose(0, 2, 1); wp = wp.reshape(Cout, k * ldx)
    wq = np.zeros((Cin, k, ldo), np.float32); wq[:, :, :Cout] = w[:, :, ::-1].transpose(1, 2, 0); wq = wq.reshape(Cin, k * ldo)
    xflat = np.full(B * x_bs, np.nan, np.float32)
    for b in range(B):
        xflat[b * x_bs:b * x_bs + W * ldx] = x[b].reshape(-1)
    ke = 32
    Am = G.rows(xflat, B * Wout, k * ldx, ldx, Wout, x_bs)
    assert np.isfinite(Am).all()
    M = B * Wout
    runs = []
    for _ in range(2):
        xd = torch.from_numpy(xflat).to(dev)
        y = _out(M, Cout, ldo, F32)
        ops.conv1d_selu_fwd(xd, B, W, ldx, x_bs, Cout, k, _t(wp), _t(bias), y, ldo, act=NONE)
        torch.cuda.synchronize()
        assert _guard_ok(y, M, Cout)
        r = [y]
        if bwd:
            dyd = _op(dy, ldo, F32)
            yz = y.clone(); yz[:M, Cout:] = 0
            dzp = torch.full((B * Wp + GUARD, ldo), NAN, device=dev); dzp[B * Wp:] = SENT
            dw = torch.full((Cout * Cin * k + GUARD,), NAN, device=dev); dw[Cout * Cin * k:] = SENT
            db = _vec(Cout)
            dx = _out(B * W, Cin, ldx, F32)
            ops.conv1d_selu_bwd(B, W, Cin, ldx, x_bs, Cout, ldo, k, dyd, yz, xd, _t(wq), dzp, dw, db, dx, ldx, act=NONE)
            torch.cuda.synchronize()
            assert _guard_ok(dx, B * W, Cin) and bool((dzp[B * Wp:] == SENT).all()) and bool((dw[Cout * Cin * k:] == SENT).all())
            assert bool((db[Cout:] == SENT).all())
            r += [dzp, dw, db, dx]
        runs.append(r)
    for u, v in zip(*runs):
        assert torch.equal(_bits(u), _bits(v)), "second run differs"
    y = runs[0][0]
    checks = [("y", _np(y[:M, :Cout]), (Am, wp, bias))]
    if bwd:
        _, dzp, dw, db, dx = runs[0]
        zref = np.zeros((B, Wp, ldo), np.float32); zref[:, k - 1:k - 1 + Wout, :Cout] = dy.reshape(B, Wout, Cout)
        assert np.array_equal(_np(dzp[:B * Wp]), zref.reshape(B * Wp, ldo).astype(np.float64)), "dzp: dy in the interior, +0 elsewhere"
        Zm = G.rows(zref.reshape(-1), B * W, k * ldo, ldo, W, Wp * ldo)
        checks.append(("dx", _np(dx[:B * W, :Cin]), (Zm, wq, None)))
        Dz = G.rows(zref.reshape(-1)[(k - 1) * ldo:], M, Cout, ldo, Wout, Wp * ldo)
        assert np.array_equal(Dz, dy)
        dwp_got = np.zeros((Cout, k, ldx)); dwp_got[:, :, :Cin] = _np(dw[:Cout * Cin * k]).reshape(Cout, Cin, k).transpose(0, 2, 1)
        keep = np.zeros((Cout, k, ldx), bool); keep[:, :, :Cin] = True
        checks.append(("dw", dwp_got.reshape(Cout, k * ldx), (Dz.T, Am.T, None), keep.reshape(Cout, k * ldx)))
        checks.append(("db", _np(db[:Cout])[:, None], (Dz.T, np.ones((1, M), np.float32), None)))
    for name, got, (a, b, bv), *mask in checks:
        if kind == "int":
            ref = G.nt(a, b, bv)
            if mask:
                ref = np.where(mask[0], ref, 0.0)
            _exact(got, ref, f"{what}: {name} [int]")
        else:
            ref, bound, rho = G.nt_bound(a, b, ke, bias=bv)
            if mask:
                ref, bound = np.where(mask[0], ref, 0.0), np.where(mask[0], bound, 0.0)
            _close(got, ref, bound, rho, f"{what}: {name} [float]")


CONV_CASES = [
    # B, W, Cin, ldx, gap, Cout, ldo, k, bwd, branch
    (3, 30, 5, 8, 0, 6, 8, 1, True, "k = 1: window = one position, K = ldx = 8; dzp has no pad rows; register-staged (K < 4 ke)"),
    (70, 4, 3, 4, 8, 7, 8, 4, True, "W == k: Wout = 1, every group is one row (group = 1: 32 turns of row_step's loop per stage, 3 stages in dW); NaN gap behind each batch"),
    (3, 29, 6, 8, 24, 9, 12, 5, True, "Wout = 25: the first 64-row tile holds rows of three batches, 75 rows = 2 tiles; K = 40, NaN gap"),
    (3, 40, 7, 8, 16, 10, 12, 16, True, "Wout = 25 again with K = k ldx = 128 = 4 ke: the LDS-direct loop on row groups (fwd), 128 x 32 tile off (M < 128)"),
    (6, 40, 7, 8, 16, 10, 12, 16, True, "M = 150 >= 128, Cout <= 32: the f32 128 x 32 tile on row groups, LDS-direct; dX: K = k ldo = 192"),
    (3, 12, 3, 4, 2, 5, 8, 3, False, "x_bs % 4 != 0 (forward only; the backward entry refuses it): gstride off the 16-byte rule -> register-staged, misaligned rows"),
    (2, 300, 4, 4, 0, 3, 4, 140, True, "K = k ldx = 560 -> ksteps 18 >= 16 on 3 tiles of 128 x 32: forward and dX split-K (2 slabs) over row groups; dW: R = 322"),
]


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("case", CONV_CASES, ids=[f"B{c[0]}W{c[1]}k{c[7]}" for c in CONV_CASES])
def test_row_groups_through_the_conv_entries(case, kind):
    B, W, Cin, ldx, gap, Cout, ldo, k, bwd, what = case
    if k == 140:
        need = L.load().mvae_conv1d_selu_fwd_workspace(B, W, ldx, Cout, k)
        assert need == 2 * (B * (W - k + 1)) * Cout * 4
    _conv(B, W, Cin, ldx, gap, Cout, ldo, k, what, kind=kind, bwd=bwd, seed=W)


def test_conv_backward_refuses_a_batch_stride_off_the_16_byte_rule():
    B, W, Cin, ldx, Cout, ldo, k = 2, 6, 3, 4, 5, 8, 3
    x_bs, Wout = W * ldx + 2, W - k + 1
    z = lambda *s: torch.zeros(*s, device=dev)
    dzp, dw, db, dx = (torch.full(s, SENT, device=dev) for s in ((B * (Wout + 2 * k - 2), ldo), (Cout, Cin, k), (Cout,), (B * W, ldx)))
    with pytest.raises(L.MvaeError, match=r"-1 \(invalid argument\)"):
        ops.conv1d_selu_bwd(B, W, Cin, ldx, x_bs, Cout, ldo, k, z(B * Wout, ldo), z(B * Wout, ldo), z(B * x_bs), z(Cin, k * ldo), dzp, dw, db, dx, ldx, act=NONE)
    torch.cuda.synchronize()
    assert all(bool((v == SENT).all()) for v in (dzp, dw, db, dx))


# =====================================================================================================================
# TN: mvae_gemm_tn (bf16 and f32), mvae_gemm_tn_f32_colsum, mvae_gemm_tn_colsum
# =====================================================================================================================
def _tn(A, B, dt, bias=None, act=NONE, c_dt=F32, c0=None, colsum=None, cs0=None, pad_c=5, extra_rows=8):
    """Two runs of ops.gemm_tn (colsum: 'f32' -> ops.gemm_tn_f32_colsum) on fresh buffers.  A [K, M], B [K, N]; the buffers have 8 more rows
    of NaN behind K and NaN pad columns.  Returns (C, column sums or None)."""
    (K, M), N = A.shape, B.shape[1]
    al = 8 if dt == BF16 else 4
    lda, ldb, ldc = _up(M, al) + al, _up(N, al) + 2 * al, N + pad_c
    bias_t = None if bias is None else _t(bias)
    res = []
    for _ in range(2):
        a, b = _op(A, lda, dt, extra_rows=extra_rows), _op(B, ldb, dt, extra_rows=extra_rows)
        c = _out(M, N, ldc, c_dt, c0)
        cs = _vec(M, cs0)
        if colsum == "f32":
            ops.gemm_tn_f32_colsum(a, b, c, cs, M, N, K, lda=lda, ldb=ldb, ldc=ldc, accumulate=c0 is not None, colsum_accumulate=cs0 is not None)
        else:
            ops.gemm_tn(a, b, c, M, N, K, lda=lda, ldb=ldb, ldc=ldc, bias=bias_t, act=act, accumulate=c0 is not None)
        torch.cuda.synchronize()
        assert _guard_ok(c, M, N), "sentinel behind C overwritten"
        assert bool((cs[M:] == SENT).all()) and (colsum or bool(torch.isnan(cs[:M]).all())), "column-sum vector"
        res.append((c, cs))
    assert torch.equal(_bits(res[0][0]), _bits(res[1][0])) and torch.equal(_bits(res[0][1]), _bits(res[1][1])), "second run differs"
    return _np(res[0][0][:M, :N]), (_np(res[0][1][:M]) if colsum else None)


def _tn_both(shape, dt, seed, what, bias=False, act=NONE, c_dt=F32, acc=False, colsum=None, cs_acc=False, kinds=("int", "float")):
    M, N, K = shape
    rs = np.random.RandomState(seed)
    for kind in kinds:
        if kind == "int" and act == SELU:
            continue
        gen = G.ints if kind == "int" else (lambda r, s: G.floats(r, s, bf16=dt == BF16))
        genf = G.ints if kind == "int" else G.floats
        A, B = gen(rs, (K, M)), gen(rs, (K, N))
        bv = genf(rs, N) if bias else None
        c0 = genf(rs, (M, N)) if acc else None
        cs0 = genf(rs, M) if cs_acc else None
        got, gcs = _tn(A, B, dt, bias=bv, act=act, c_dt=c_dt, c0=c0, colsum=colsum, cs0=cs0)
        if kind == "int":
            _exact(got, G.nt(A.T, B.T, bv, act, c0), f"{what} [int]", c_dt == BF16)
            if colsum:
                _exact(gcs, G.colsum(A, cs0), f"{what}: column sums [int]")
        else:
            ref, bound, rho = G.tn_bound(A, B, _ke(dt), c0=c0, bias=bv, act=act, c_bf16=c_dt == BF16)
            _close(got, ref, bound, rho, f"{what} [float]")
            if colsum:
                ref, bound, rho = G.colsum_bound(A, _ke(dt), c0=cs0)
                _close(gcs, ref, bound, rho, f"{what}: column sums [float]")


TN_TILES = {"128": (128, 128), "256": (256, 128), "512": (256, 256)}       # MVAE_TN_BM tag -> tile rows, columns


@pytest.mark.parametrize("bm", ["128", "256", "512"])
def test_tn_bf16_forced_tiles_k_cases(bm, monkeypatch):
    """Each of the three kernels (gemm_tn_bf16_kernel<4, 4>, <3, 8>, gemm_tn_bf16_256_kernel) forced through MVAE_TN_BM on a shape one over the
    tile edge in M and one under in N (2 x 1 tiles).  K = 0 (nk = 0: the main loop returns at once, C = 0), 7 and 65 (rows >= K come back as
    zero from the buffer descriptor; the 8 rows behind K are NaN), 64; ksteps 15 -> 1 slab, 16 -> 2 slabs; 73 steps -> 9 slabs, the last of
    ONE step."""
    monkeypatch.setenv("MVAE_TN_BM", bm)
    tm, tn_ = TN_TILES[bm]
    M, N = tm + 1, tn_ - 1
    for K, want in ((0, 1), (7, 1), (64, 1), (65, 1), (960, 1), (1024, 2), (73 * 64, 9)):
        assert _tn_splits(M, N, K) == want == _splits_rule(2, -(-K // 64), 192)[0], (K, want)
        _tn_both((M, N, K), BF16, K, f"tile {tm} x {tn_}, K = {K}, {want} slab(s)", kinds=("int",))
    _tn_both((M, N, 65), BF16, 1, f"tile {tm} x {tn_}, K = 65", kinds=("float",))
    _tn_both((M, N, 73 * 64), BF16, 2, f"tile {tm} x {tn_}, 9 slabs", kinds=("float",))


@pytest.mark.parametrize("bm", ["128", "256", "512"])
def test_tn_bf16_forced_tiles_edges_and_epilogues(bm, monkeypatch):
    """M and N one under, at and one over the tile edge (K = 65 unsplit, K = 1024 two slabs), then bias / activation / bf16 C / accumulate in
    the kernel's own epilogue and in gemm_splitk_reduce_kernel."""
    monkeypatch.setenv("MVAE_TN_BM", bm)
    tm, tn_ = TN_TILES[bm]
    for dm, dn in ((-1, 1), (0, 0), (1, -1)):
        for K in (65, 1024):
            tiles = -(-(tm + dm) // tm) * -(-(tn_ + dn) // tn_)                  # 1 x 2, 1 x 1, 2 x 1 tiles: all < 192, so 16 steps split in 2
            assert tiles == (2 if dm > 0 else 1) * (2 if dn > 0 else 1)
            assert _tn_splits(tm + dm, tn_ + dn, K) == (2 if K == 1024 else 1) == _splits_rule(tiles, -(-K // 64), 192)[0]
            _tn_both((tm + dm, tn_ + dn, K), BF16, K + dm, f"tile {tm} x {tn_}, M = tile {dm:+d}, N = tile {dn:+d}, K = {K}", kinds=("int",))
    M, N = tm + 1, tn_ - 1
    for K in (65, 1024):
        where = "own epilogue" if K == 65 else "reduce kernel"
        assert _tn_splits(M, N, K) == (1 if K == 65 else 2)
        _tn_both((M, N, K), BF16, 3, f"{where}: bias + RELU", bias=True, act=RELU)
        _tn_both((M, N, K), BF16, 4, f"{where}: bias + SELU, bf16 C", bias=True, act=SELU, c_dt=BF16, kinds=("float",))
        _tn_both((M, N, K), BF16, 5, f"{where}: bf16 C", c_dt=BF16)
        _tn_both((M, N, K), BF16, 6, f"{where}: accumulate", acc=True)
        _tn_both((M, N, K), BF16, 7, f"{where}: accumulate + bias + RELU", acc=True, bias=True, act=RELU)


def test_tn_bf16_natural_tile_thresholds():
    """make_plan_tn unforced, on both sides of each tile's threshold, observed through the split count at K = 1024 (ksteps 16):
      256 x 128 when ceil(M / 256) ceil(N / 128) >= 128: (513, 5504) -> 3 x 43 = 129 tiles < 192 -> 2 slabs;
                 one tile column less, (513, 5376): 126 -> the 128 x 128 tile, 5 x 42 = 210 tiles >= 192 -> no split.
      256 x 256 when ceil(M / 256) ceil(N / 256) >= 32, N % 256 == 0, K >= 4096: (7937, 256, 4096) -> 32 tiles, 64 steps -> 8 slabs;
                 (7936, 256, 4096): 31 < 32 -> the 128 x 128 tile, 62 x 2 = 124 tiles -> 3 slabs; K = 4095 -> 128 x 128 too, 126 tiles, 3 slabs."""
    lib = L.load()
    assert lib.mvae_knob_int(b"MVAE_TN_BM", 0) == 0
    assert _tn_splits(513, 5504, 1024) == 2 and _tn_splits(513, 5376, 1024) == 1
    _tn_both((513, 5504, 1024), BF16, 1, "256 x 128 at its threshold, 2 slabs", kinds=("int",))
    _tn_both((513, 5376, 1024), BF16, 2, "128 x 128 one tile column under it, unsplit", kinds=("int",))
    assert _tn_splits(7937, 256, 4096) == 8 and _tn_splits(7936, 256, 4096) == 3 and _tn_splits(7937, 256, 4095) == 3
    _tn_both((7937, 256, 4096), BF16, 3, "256 x 256 at its threshold, 8 slabs", kinds=("int",))
    _tn_both((7936, 256, 4096), BF16, 4, "128 x 128 one tile row under it, 3 slabs", kinds=("int",))
    _tn_both((7937, 256, 4095), BF16, 5, "128 x 128: K one short of 64 * 64, 3 slabs", kinds=("int",))


def _colsum_call(M, N, K, A, B, c, cs, lda, ldb, cs_acc=False):
    """mvae_gemm_tn_colsum itself (ops.gemm_tn_colsum asks _supported first and would not call): returns the status."""
    lib = L.load()
    need = lib.mvae_gemm_tn_colsum_workspace(M, N, K)
    ws = ops.Scratch.get(need, A.device) if need else None
    return lib.mvae_gemm_tn_colsum(M, N, K, L.ptr(A), lda, L.ptr(B), ldb, L.ptr(c), c.stride(0), 0, L.ptr(cs), 1 if cs_acc else 0,
                                   L.ptr(ws), need, L.stream_ptr())


COLSUM_SIDES = [
    # M, N, K, supported, which condition
    (1793, 1024, 4096, True, "8 x 4 = 32 tiles of 256 x 256, 64 steps -> 8 slabs: served"),
    (1792, 1024, 4096, False, "7 x 4 = 28 tiles < 32: not the 256 x 256 tile"),
    (1793, 1024, 4095, False, "K < 64 * 64: not the 256 x 256 tile"),
    (2817, 768, 4096, False, "12 x 3 tiles: 256 x 256, split, but 3 tile columns"),
    (1793, 1280, 4096, False, "5 tile columns"),
    (12032, 1024, 4096, True, "47 x 4 = 188 tiles < 192: still split (2 slabs) -> served"),
    (12288, 1024, 4096, False, "48 x 4 = 192 tiles: no split, no reduction launch to sum the K-halves"),
]


@pytest.mark.parametrize("case", COLSUM_SIDES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in COLSUM_SIDES])
def test_tn_bf16_fused_colsum_and_supported_agree(case):
    """mvae_gemm_tn_colsum_supported == (pl.bm == 512 && pl.tiles_n == 4 && pl.splits > 1), on both sides of each condition, against the call's
    status: MVAE_ERR_UNSUPPORTED with nothing written, or the product and the column sums -- fresh and accumulated, rows K.. of A at NaN --
    exact on integers.  The two 12k-row shapes check C on their first 256 and last 300 rows (a float64 reference of all of it is 50 GFLOP);
    the column sums on every row."""
    M, N, K, sup, what = case
    lib = L.load()
    assert bool(lib.mvae_gemm_tn_colsum_supported(M, N, K)) == sup, what
    lda, ldb = _up(M, 8) + 8, N + 16
    rs = np.random.RandomState(M)
    if not sup:
        a = torch.zeros(K + 8, lda, device=dev, dtype=BF16); b = torch.zeros(K + 8, ldb, device=dev, dtype=BF16)
        c, cs = _out(M, N, N, F32), _vec(M)
        assert _colsum_call(M, N, K, a, b, c, cs, lda, ldb) == -3, what
        torch.cuda.synchronize()
        assert bool(torch.isnan(c[:M]).all()) and bool(torch.isnan(cs[:M]).all()) and _guard_ok(c, M, N)
        return
    A, B = G.ints(rs, (K, M)), G.ints(rs, (K, N))
    cs0 = G.ints(rs, M)
    rows_ = np.arange(M) if M < 4000 else np.r_[0:256, M - 300:M]
    ref = G.tn(A[:, rows_], B)
    a, b = _op(A, lda, BF16, extra_rows=8), _op(B, ldb, BF16, extra_rows=8)
    for acc in (False, True):
        res = []
        for _ in range(2):
            c, cs = _out(M, N, N + 8, F32), _vec(M, cs0 if acc else None)
            assert _colsum_call(M, N, K, a, b, c, cs, lda, ldb, cs_acc=acc) == 0
            torch.cuda.synchronize()
            assert _guard_ok(c, M, N) and bool((cs[M:] == SENT).all())
            res.append((c, cs))
        assert torch.equal(_bits(res[0][0]), _bits(res[1][0])) and torch.equal(_bits(res[0][1]), _bits(res[1][1]))
        assert not bool(torch.isnan(res[0][0][:M, :N]).any())
        _exact(_np(res[0][0][:M, :N])[rows_], ref, f"{what}: C")
        _exact(_np(res[0][1][:M]), G.colsum(A, cs0 if acc else None), f"{what}: column sums, accumulate={acc}")


def test_tn_bf16_grouped_launch_and_its_workgroup_cap():
    """mvae_gemm_tn_grouped_capped (and, once, mvae_gemm_tn_grouped): three problems in one launch -- K = 64 (one step), K = 200 (not a multiple of 64: the descriptor zero-fills
    the tail; N = 1024 with column sums, fresh), K = 130 with accumulate -- 2 + 8 + 2 = 12 tiles; and one problem alone.  max_workgroups 0
    and 12 launch one workgroup per tile (xcd_remap order), 11 and 1 loop over tiles in plain order: the same bits every time."""
    rs = np.random.RandomState(4)
    dims = [(257, 256, 64), (300, 1024, 200), (256, 512, 130)]
    As = [G.ints(rs, (K, M)) for M, N, K in dims]; Bs = [G.ints(rs, (K, N)) for M, N, K in dims]
    c2 = G.ints(rs, (256, 512))

    def launch(sel, cap):
        probs, outs = [], []
        for i in sel:
            M, N, K = dims[i]
            lda, ldb = _up(M, 8) + 8 + 8 * i, N + 16
            a, b = _op(As[i], lda, BF16, extra_rows=8), _op(Bs[i], ldb, BF16, extra_rows=8)
            c = _out(M, N, N + 8, F32, c2 if i == 2 else None)
            cs = _vec(M) if i == 1 else None
            assert ops.gemm_tn_grouped_supported(a, M, N, K, lda, ldb)
            probs.append(dict(A=a, B=b, out=c, M=M, N=N, K=K, lda=lda, ldb=ldb, accumulate=(i == 2), colsum_out=cs))
            outs.append((c, cs))
        if cap is None:
            lib = L.load()
            arr = (L.GemmTnProblem * len(probs))()
            for t_, q in zip(arr, probs):
                t_.M, t_.N, t_.K, t_.A, t_.lda, t_.B, t_.ldb = q["M"], q["N"], q["K"], q["A"].data_ptr(), q["lda"], q["B"].data_ptr(), q["ldb"]
                t_.C, t_.ldc, t_.accumulate = q["out"].data_ptr(), q["out"].stride(0), 1 if q["accumulate"] else 0
                t_.colsum_out = q["colsum_out"].data_ptr() if q["colsum_out"] is not None else None
                t_.colsum_accumulate = 0
            need = lib.mvae_gemm_tn_grouped_workspace(len(probs), arr)
            ws = ops.Scratch.get(need, dev, tag="tn_grouped") if need else None
            assert lib.mvae_gemm_tn_grouped(len(probs), arr, L.ptr(ws), need, L.stream_ptr()) == 0
        else:
            ops.gemm_tn_grouped(probs, max_workgroups=cap)
        torch.cuda.synchronize()
        for (c, cs), i in zip(outs, sel):
            assert _guard_ok(c, dims[i][0], dims[i][1]) and (cs is None or bool((cs[dims[i][0]:] == SENT).all()))
        return outs

    base = launch([0, 1, 2], 0)
    for i, (c, cs) in enumerate(base):
        M, N, K = dims[i]
        _exact(_np(c[:M, :N]), G.tn(As[i], Bs[i], c2 if i == 2 else None), f"grouped problem {i}")
        if cs is not None:
            _exact(_np(cs[:M]), G.colsum(As[i]), "grouped column sums")
    for cap in (12, 11, 1):
        for (c, cs), (c_, cs_) in zip(base, launch([0, 1, 2], cap)):
            assert torch.equal(_bits(c), _bits(c_)) and (cs is None or torch.equal(_bits(cs), _bits(cs_))), cap
    for (c, cs), (c_, cs_) in zip(base, launch([0, 1, 2], None)):     # mvae_gemm_tn_grouped itself (the entry without a cap)
        assert torch.equal(_bits(c), _bits(c_)) and (cs is None or torch.equal(_bits(cs), _bits(cs_)))
    for i in (0, 1):                                        # one problem alone: ntiles = 2 / 8
        alone = launch([i], 0)[0]
        assert torch.equal(_bits(alone[0]), _bits(base[i][0])) and (i == 0 or torch.equal(_bits(alone[1]), _bits(base[i][1])))
    z = torch.zeros(8, device=dev, dtype=BF16)
    assert ops.gemm_tn_grouped_supported(z, 256, 256, 64, 264, 272)
    assert not any(ops.gemm_tn_grouped_supported(z, *a) for a in ((255, 256, 64, 264, 272), (256, 255, 64, 264, 272), (256, 256, 63, 264, 272),
                                                                  (256, 256, 64, 260, 272), (256, 256, 64, 264, 268)))


def test_tn_bf16_operands_beyond_2_gib_in_equal_k_chunks():
    """launch_gemm_tn_bf16_colsum, operands of 2 GiB and more: M = N = 128, lda = ldb = 136, K = 7895201 > 2^31 / (2 * 136) rows -- the
    launcher cuts K into nch = 2 equal chunks of kc = 3947648 rows (a multiple of 64), each a launch of its own (128 x 128 tile, 64 slabs)
    that accumulates onto C.  Operands are zero except integers in the first 70 rows, 70 rows around every chunk boundary k0 and the last
    70 rows; the reference is float64 over those rows, the check exact.  With and without accumulate; the fused column sums are not served
    at this shape: status UNSUPPORTED, nothing written.  Allocating and clearing the two 2 GiB operands is most of this test's time
    (a fraction of a second on the MI355X)."""
    M = N = 128; ld = 136
    K = 7895201
    assert K * ld * 2 >= 1 << 31
    kmax = (((1 << 31) - 1) // (2 * ld)) // 4096 * 4096                   # the launcher's arithmetic, restated
    nch = -(-K // kmax)
    kc = _up(-(-K // nch), 64)
    k0s = list(range(0, K, kc))
    assert nch == 2 and kc == 3947648 and k0s == [0, 3947648]
    assert _tn_splits(M, N, K) == 64
    win = sorted(set(r for k0 in k0s for r in range(max(k0 - 35, 0), min(k0 + 35, K))) | set(range(70)) | set(range(K - 70, K)))
    rs = np.random.RandomState(9)
    Aw, Bw = G.ints(rs, (len(win), M)), G.ints(rs, (len(win), N))
    c0 = G.ints(rs, (M, N))
    a = torch.zeros(K, ld, device=dev, dtype=BF16); b = torch.zeros(K, ld, device=dev, dtype=BF16)
    idx = torch.tensor(win, device=dev)
    a[idx, :M] = _t(Aw, BF16); b[idx, :N] = _t(Bw, BF16)
    a[:, M:] = NAN; b[:, N:] = NAN
    for acc in (False, True):
        res = []
        for _ in range(2):
            c = _out(M, N, N + 5, F32, c0 if acc else None)
            ops.gemm_tn(a, b, c, M, N, K, lda=ld, ldb=ld, ldc=N + 5, accumulate=acc)
            torch.cuda.synchronize()
            assert _guard_ok(c, M, N)
            res.append(c)
        assert torch.equal(_bits(res[0]), _bits(res[1]))
        _exact(_np(res[0][:M, :N]), G.tn(Aw, Bw, c0 if acc else None), f"2 GiB path, accumulate={acc}")
    assert not ops.gemm_tn_colsum_supported(a, M, N, K)
    c, cs = _out(M, N, N, F32), _vec(M)
    assert _colsum_call(M, N, K, a, b, c, cs, ld, ld) == -3
    torch.cuda.synchronize()
    assert bool(torch.isnan(c[:M]).all()) and bool(torch.isnan(cs[:M]).all())
    with pytest.raises(L.MvaeError, match=r"-3 \(unsupported"):        # bias / activation / bf16 C are not served on this path either
        ops.gemm_tn(a, b, c, M, N, K, lda=ld, ldb=ld, act=RELU)


# ---- TN f32: gemm_tn_f32_kernel<X3, CS>, 64 x 64 tile, 32 rows per stage
@pytest.mark.parametrize("R", [0, 1, 31, 32, 33])
def test_tn_f32_tile_edges_with_and_without_the_ones_column(R):
    """N at 63, 64, 65 with the virtual ones column at index N (N = 64: a whole extra tile column that holds nothing else; N = 63: the last
    slot of the tile), M at 61 .. 65 (61 .. 63: the a_vec tail, the chunk's 4th lane stays zero), R (the contraction length) at 0 -- no
    stage: C = 0 and column sums 0, or C and the sums left as they were under accumulate -- 1, 31, 32 (one stage) and 33."""
    seed = 0
    for N in (63, 64, 65):
        for M in (61, 62, 63, 64, 65):
            seed += 1
            _tn_both((M, N, R), F32, seed, f"M = {M}, N = {N}, R = {R}, plain", kinds=("int",))
            _tn_both((M, N, R), F32, seed, f"M = {M}, N = {N}, R = {R}, ones column", colsum="f32", kinds=("int",))
    _tn_both((63, 64, R), F32, 77, f"R = {R}, ones column, both accumulated", colsum="f32", acc=True, cs_acc=True)
    _tn_both((65, 63, R), F32, 78, f"R = {R}, plain, accumulate", acc=True)


def _tnf_ws(M, N, R):
    return L.load().mvae_gemm_tn_workspace(M, N, R, L.MVAE_F32)


def test_tn_f32_split_threshold_on_both_sides():
    """make_plan_tn_f32 (target 768) splits when tiles < 512 and steps >= 16.  (448, 4671): 7 x 73 = 511 tiles (with and without the ones
    column) and 16 steps -> 2 slabs; the workspace entry answers for the column-sum form, 2 * M * (N + 1) * 4 bytes.  15 steps, or one more
    tile row (449 -> 8 x 73 = 584 tiles), or exactly 512 tiles -- (512, 4095): 8 x 64 with and without the ones column --: no split, no
    workspace.  73 steps on 2 tiles: 9 slabs, the last of one stage."""
    M, N = 448, 4671
    assert _tnf_ws(M, N, 512) == 2 * M * (N + 1) * 4 and _tnf_ws(M, N, 480) == 0 and _tnf_ws(M + 1, N, 512) == 0
    _tn_both((M, N, 512), F32, 1, "511 tiles, 16 steps: 2 slabs, ones column", colsum="f32", kinds=("int",))
    _tn_both((M, N, 480), F32, 2, "511 tiles, 15 steps: unsplit", kinds=("int",))
    _tn_both((M + 1, N, 512), F32, 3, "584 tiles: unsplit", colsum="f32", kinds=("int",))
    assert _tnf_ws(512, 4095, 512) == 0 and _tnf_ws(512, 4095 - 64, 512) == 2 * 512 * (4095 - 64 + 1) * 4       # 512 tiles against 8 x 63 = 504
    _tn_both((512, 4095, 512), F32, 5, "exactly 512 tiles, 16 steps: unsplit", colsum="f32", kinds=("int",))
    assert _tnf_ws(65, 63, 73 * 32) == 9 * 65 * 64 * 4
    _tn_both((65, 63, 73 * 32), F32, 4, "2 tiles, 73 steps: 9 slabs, ones column, accumulated", colsum="f32", acc=True, cs_acc=True)


def _tnf_problem(A, B, M, N, R, lda, ldb, ldc, c, cs=None, x3=False, acc=False, cs_acc=False, a_group=0, a_gs=0, b_group=0, b_gs=0):
    q = L.GemmTnF32Problem()
    q.M, q.N, q.K = M, N, R
    q.A, q.lda, q.a_group, q.a_gstride = A.data_ptr(), lda, a_group, a_gs
    q.B, q.ldb, q.b_group, q.b_gstride = B.data_ptr(), ldb, b_group, b_gs
    q.C, q.ldc, q.accumulate = c.data_ptr(), ldc, 1 if acc else 0
    q.colsum_out = cs.data_ptr() if cs is not None else None
    q.colsum_accumulate, q.x3 = (1 if cs_acc else 0), (1 if x3 else 0)
    return q


def _multi(problems, want_ws=None):
    """mvae_gemm_tn_f32_multi on a list of problems; returns the status.  want_ws: what mvae_gemm_tn_f32_multi_workspace must answer -- the
    sum over the problems of splits * M * (N + ones column) * 4 bytes, each rounded up to 256, 0 for a problem that does not split."""
    lib = L.load()
    n = len(problems)
    arr = (L.GemmTnF32Problem * n)(*problems)
    need = lib.mvae_gemm_tn_f32_multi_workspace(n, arr)
    assert want_ws is None or need == want_ws, (need, want_ws)
    ws = ops.Scratch.get(need, dev, tag="tn_f32_multi") if need else None
    rc = lib.mvae_gemm_tn_f32_multi(n, arr, L.ptr(ws), need, L.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _grouped_flat(rs, R, L_, ld, group, gstride, kind):
    """A flat buffer whose R rows of L_ elements sit at gemm_ref.row_starts: values where a row reads, NaN elsewhere."""
    starts = G.row_starts(R, ld, group, gstride)
    n = int(starts.max()) + L_ if R else L_
    flat = np.full(n + 4, np.nan, np.float32)
    vals = (G.ints if kind == "int" else G.floats)(rs, n)
    for s in starts:
        flat[s:s + L_] = vals[s:s + L_]
    return flat


MULTI_SPECS = [
    # M, N, R, a_group, b_group, x3, colsum, accumulate, branch
    (61, 63, 33, 0, 0, False, True, False, "plain rows, a_vec tail, ones column in the tile's last slot, 2 stages"),
    (64, 64, 100, 0, 0, True, True, False, "x3 with the ones column in an extra tile column: body<true, true>"),
    (70, 12, 96, 7, 7, False, False, False, "group 7 < 32: row_step's loop takes several turns per stage; B rows overlap (ldb 4 < N 12)"),
    (20, 12, 128, 32, 32, True, False, True, "group == 32: exactly one turn per stage; x3 without column sums: body<true, false>; accumulate"),
    (9, 24, 150, 50, 50, False, True, True, "group 50 > 32: 0 or 1 turns; ones column; C and sums accumulated"),
    (65, 130, 73 * 32, 0, 0, False, True, False, "73 steps: split-K inside a multi launch (slabs summed by gemm_splitk_reduce_multi_kernel)"),
    (10, 20, 0, 0, 0, False, True, False, "R = 0: no stage, C = 0 and column sums 0"),
    (66, 5, 0, 0, 0, True, True, True, "R = 0 under accumulate: C and the column sums stay as they were"),
]


def _multi_ws(spec):
    """The slab bytes of one problem of MULTI_SPECS, alone (target 768) and mixed (target 1536 / 8 = 192) alike: only the 73-step problem splits
    -- 2 x 3 tiles (N + 1 = 131 columns), min(ceil(target / 6), 73 / 8, 64) = 9 slabs of 9, ..., 9, 1 stages."""
    M, N, R, *_, cs, acc, what = spec
    return _up(9 * M * (N + 1) * 4, 256) if R == 73 * 32 else 0


def _multi_build(spec, kind, seed):
    M, N, R, ag, bg, x3, cs, acc, what = spec
    rs = np.random.RandomState(seed)
    gen = G.ints if kind == "int" else G.floats
    if ag:
        lda, ldb = _up(M, 4) + 4, 4                        # A: disjoint rows; B: overlapping windows of N floats every 4
        a_gs, b_gs = ag * lda + 8, _up((bg - 1) * 4 + N, 4) + 8
        fa, fb = _grouped_flat(rs, R, M, lda, ag, a_gs, kind), _grouped_flat(rs, R, N, ldb, bg, b_gs, kind)
        Am, Bm = G.rows(fa, R, M, lda, ag, a_gs), G.rows(fb, R, N, ldb, bg, b_gs)
    else:
        lda, ldb, a_gs, b_gs = _up(M, 4) + 4, _up(N, 4) + 8, 0, 0
        Am, Bm = gen(rs, (R, M)), gen(rs, (R, N))
        fa = np.full((R + 2, lda), np.nan, np.float32); fa[:R, :M] = Am
        fb = np.full((R + 2, ldb), np.nan, np.float32); fb[:R, :N] = Bm
    c0 = gen(rs, (M, N)) if acc else None
    cs0 = gen(rs, M) if (acc and cs) else None
    return dict(spec=spec, fa=fa.reshape(-1), fb=fb.reshape(-1), Am=Am, Bm=Bm, lda=lda, ldb=ldb, a_gs=a_gs, b_gs=b_gs, c0=c0, cs0=cs0)


def _multi_bufs(b):
    M, N, R, ag, bg, x3, cs, acc, what = b["spec"]
    a, bb = torch.from_numpy(b["fa"]).to(dev), torch.from_numpy(b["fb"]).to(dev)
    c = _out(M, N, N + 5, F32, b["c0"])
    csv = _vec(M, b["cs0"]) if cs else None
    q = _tnf_problem(a, bb, M, N, R, b["lda"], b["ldb"], N + 5, c, csv, x3=x3, acc=acc, cs_acc=acc and cs, a_group=ag, a_gs=b["a_gs"],
                     b_group=bg, b_gs=b["b_gs"])
    return q, (a, bb, c, csv)


def _multi_check(b, c, csv, kind):
    M, N, R, ag, bg, x3, cs, acc, what = b["spec"]
    assert _guard_ok(c, M, N) and (csv is None or bool((csv[M:] == SENT).all()))
    if kind == "int":
        _exact(_np(c[:M, :N]), G.tn(b["Am"], b["Bm"], b["c0"]), what)
        if cs:
            _exact(_np(csv[:M]), G.colsum(b["Am"], b["cs0"]), what + ": column sums")
    else:
        ref, bound, rho = G.tn_bound(b["Am"], b["Bm"], 32, c0=b["c0"], x3=x3)
        _close(_np(c[:M, :N]), ref, bound, rho, what)
        if cs:
            ref, bound, rho = G.colsum_bound(b["Am"], 32, c0=b["cs0"], x3=x3)
            _close(_np(csv[:M]), ref, bound, rho, what + ": column sums")


@pytest.mark.parametrize("kind", ["int", "float"])
def test_tn_f32_multi_launch_row_groups_x3_and_column_sums(kind):
    """mvae_gemm_tn_f32_multi: the four instantiations of gemm_tn_f32_body (x3 x column sums), grouped A and B with group smaller than, equal
    to and larger than the 32-row stage, a split problem (9 slabs: asserted through mvae_gemm_tn_f32_multi_workspace, which is 0 for every
    other problem) and two with R = 0 -- each alone (n = 1: a problem of a multi launch of one gets target 768, the single launcher's plan)
    and all mixed in one launch (target 1536 / 8 = 192 each).  Integers: both exact, hence equal; floats: both inside
    the bound (x3: the x3 bound)."""
    built = [_multi_build(s, kind, i) for i, s in enumerate(MULTI_SPECS)]
    for b in built:                                        # single launches
        for _ in range(2):
            q, (a, bb, c, csv) = _multi_bufs(b)
            assert _multi([q], want_ws=_multi_ws(b["spec"])) == 0
            _multi_check(b, c, csv, kind)
    runs = []
    for _ in range(2):                                     # mixed
        qs, bufs = zip(*[_multi_bufs(b) for b in built])
        assert _multi(list(qs), want_ws=sum(_multi_ws(s_) for s_ in MULTI_SPECS)) == 0
        for b, (a, bb, c, csv) in zip(built, bufs):
            _multi_check(b, c, csv, kind)
        runs.append(bufs)
    for u, v in zip(*runs):
        assert torch.equal(_bits(u[2]), _bits(v[2])) and (u[3] is None or torch.equal(_bits(u[3]), _bits(v[3])))


def test_tn_f32_multi_launch_limits():
    """n == MVAE_TN_F32_MULTI_MAX (16) problems in one launch (target clamps at 96 each); n = 17, n = 0 and a problem with M <= 0 are refused
    with MVAE_ERR_INVALID before anything is launched or written."""
    assert ops.TnF32Batch.MAX == 16
    built = [_multi_build((5 + 4 * i, 70 - 3 * i, 40 + 9 * i, 0, 0, i % 2 == 1, i % 3 == 0, False, f"problem {i} of 16"), "int", i) for i in range(16)]
    qs, bufs = zip(*[_multi_bufs(b) for b in built])
    assert _multi(list(qs)) == 0
    for b, (a, bb, c, csv) in zip(built, bufs):
        _multi_check(b, c, csv, "int")
    for bad in ("n17", "n0", "m0"):
        qs, bufs = zip(*[_multi_bufs(b) for b in built])
        qs = list(qs)
        if bad == "m0":
            qs[3].M = 0
            lib = L.load()
            arr = (L.GemmTnF32Problem * 16)(*qs)
            rc = lib.mvae_gemm_tn_f32_multi(16, arr, L.ptr(ops.Scratch.get(1 << 20, dev, tag="tn_f32_multi")), 1 << 20, L.stream_ptr())
        else:
            n = 17 if bad == "n17" else 0
            lib = L.load()
            arr = (L.GemmTnF32Problem * 17)(*(qs + [qs[0]]))
            rc = lib.mvae_gemm_tn_f32_multi(n, arr, L.ptr(ops.Scratch.get(1 << 20, dev, tag="tn_f32_multi")), 1 << 20, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == -1, bad
        for b, (a, bb, c, csv) in zip(built, bufs):
            M, N = b["spec"][0], b["spec"][1]
            assert bool(torch.isnan(c[:M, :N]).all()) and _guard_ok(c, M, N), bad
