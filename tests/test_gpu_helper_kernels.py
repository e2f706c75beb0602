"""GPU tests (pytest -m gpu) of the helper kernels that the model tests reach only inside whole-model checks: the MOSES cross-entropy and
latent kernels, the column / row / time reductions, cast / transpose and the multi-job pack, permutes, masks, one-hots, the input pipeline,
the activation backwards and the ReLU conv.  Each entry is called directly and compared with a float64 restatement on the CPU, at the
shapes where its launcher changes branch (chunk caps, vector tails, alignment fallbacks, grid-stride loops, partial-sum blocks).

Three kinds of check:
  data movement (permutes, masks, one-hots, copies, casts)  bit-exact; casts against torch's own .to(torch.bfloat16);
  reductions      small integers (exact in bf16 and fp32, so every partial sum is exact): the float64 sum bit for bit, whatever the
                  order; random floats within 2e-6 * sum|x| per output; two runs bitwise identical (the reductions are deterministic);
  math kernels    float64 references with autograd; losses <= 1e-6 relative, gradients bounded per element by the size of their terms.
Destinations start as NaN or a sentinel, so a missing or a stray write is visible.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gpu_helpers import O                       # noqa: E402
from molecular_vae_amd import ops, _lib as L    # noqa: E402

dev = torch.device("cuda")
SENT = -12345.0                                 # f32 sentinel; bf16 sentinel bits below
SENT_BF16 = -0x1235                             # int16 view of the bf16 sentinel (0xEDCB, a finite value near -7.9e27)


def g32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def host(x):
    torch.cuda.synchronize()
    return x.detach().cpu()


def ints(rs, shape, lo=-8, hi=8):
    """small integers: exact in bf16 and fp32, and every partial sum of up to 2^20 of them is exact in fp32"""
    return rs.randint(lo, hi + 1, size=shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------ MOSES token cross-entropy
def _ce_ref(logits_tm, ldl, x, pad, B, T, V, g, dy_ext):
    """float64 F.cross_entropy(y[:, :-1], x[:, 1:], ignore_index=pad) (mosesvae.py:193-197) on y[b, t] = logits row t*B+b, and the
    gradient of g * loss + sum(y * dy_ext) w.r.t. y, returned time-major [T*B, V]."""
    y = torch.from_numpy(logits_tm[:, :V].astype(np.float64).reshape(T, B, V).transpose(1, 0, 2).copy()).requires_grad_(True)
    xt = torch.from_numpy(x)
    loss = F.cross_entropy(y[:, :-1].reshape(-1, V), xt[:, 1:].reshape(-1), ignore_index=pad)
    obj = g * loss
    if dy_ext is not None:
        obj = obj + (y * torch.from_numpy(dy_ext.astype(np.float64))).sum()
    obj.backward()
    count = int((xt[:, 1:] != pad).sum())
    return float(loss.detach()), count, y.grad.numpy().transpose(1, 0, 2).reshape(T * B, V)


def _ce_run(logits_tm, ldl, x, pad, B, T, V, g, dy_ext, dt, ldd):
    tl = g32(logits_tm)
    tx = torch.from_numpy(x).to(dev)
    loss2 = torch.full((2,), float("nan"), device=dev)
    ops.ce_loss_fwd(tl, ldl, tx, pad, loss2, B, T, V)
    gout = None if g == 1.0 else torch.tensor([g], dtype=torch.float32, device=dev)
    dl = torch.full((T * B, ldd), float("nan"), device=dev).to(dt)
    ops.ce_loss_bwd(tl, ldl, tx, pad, loss2, gout, None if dy_ext is None else g32(dy_ext), dl, B, T, V)
    return host(loss2).numpy().astype(np.float64), host(dl).float().numpy().astype(np.float64)


def _ce_inputs(B, T, V, ldl, pad, seed, all_pad_seq=True):
    rs = np.random.RandomState(seed)
    logits = (2.0 * rs.standard_normal((T * B, ldl))).astype(np.float32)
    logits[:, V:] = rs.choice([np.nan, np.inf, -1e30, 7.0], size=(T * B, ldl - V))        # the kernel must never read the pad columns
    x = rs.randint(0, V, size=(B, T)).astype(np.int64)
    x[rs.random_sample((B, T)) < 0.15] = pad                                                 # scattered pad targets
    if all_pad_seq and B > 1 and T > 1:
        x[B // 2, 1:] = pad                                                                  # a sequence that is all pad after its first token
    return logits, x


CE_CASES = [   # B, T, V, ldl, ldd, g, with dy_ext
    (7, 9, 5, 5, 8, 1.0, False),           # B*T = 63: one partial block, not full
    (8, 8, 30, 33, 32, 0.37, True),        # B*T = 64: exactly one block; ldl > V with garbage
    (13, 5, 65, 65, 72, -1.75, False),     # B*T = 65: a second block holding one row; V = 65: lane 0 holds a second column
    (3, 21, 64, 64, 64, 2.5, True),        # V = 64: one column per lane, ldd == V
    (5, 13, 130, 136, 136, 1.0, True),     # V = 130: up to three columns per lane
    (1024, 100, 30, 32, 32, 0.5, True),    # 1600 partials: the final kernel's strided walk over more than 1000 blocks
]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,V,ldl,ldd,g,ext", CE_CASES, ids=[f"B{c[0]}T{c[1]}V{c[2]}" for c in CE_CASES])
def test_ce_loss_matches_float64_cross_entropy(B, T, V, ldl, ldd, g, ext, dt):
    pad = min(3, V - 1)
    logits, x = _ce_inputs(B, T, V, ldl, pad, seed=B * T + V)
    dy_ext = (0.01 * np.random.RandomState(V).standard_normal((B, T, V))).astype(np.float32) if ext else None
    loss, count, dref = _ce_ref(logits, ldl, x, pad, B, T, V, g, dy_ext)
    loss2, dl = _ce_run(logits, ldl, x, pad, B, T, V, g, dy_ext, dt, ldd)
    assert loss2[1] == count
    assert abs(loss2[0] - loss) <= 1e-6 * abs(loss), (loss2, loss)
    assert not dl[:, V:].any(), "pad columns V..ldd-1 must be zero"
    counted = np.zeros((T, B), bool)
    counted[:-1] = (x[:, 1:] != pad).T
    bound = 4e-6 * abs(g) / count * counted.reshape(T * B, 1) + 1e-6 * (np.abs(dy_ext).transpose(1, 0, 2).reshape(T * B, V) if ext else 0.0)
    if dt == torch.bfloat16:
        bound = bound + 2.0 ** -8 * np.abs(dref)                 # one bf16 rounding of the value
    err = np.abs(dl[:, :V] - dref)
    assert (err <= bound).all(), (err.max(), np.unravel_index(np.argmax(err - bound), err.shape))
    if not ext:
        assert not dl[~counted.reshape(-1)].any(), "rows without a counted target must be exactly zero"


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_ce_loss_single_step_counts_nothing(dt):
    """T = 1: no row has a target -- NaN loss, zero count and zero gradients (what torch gives for an empty mean)."""
    B, T, V = 4, 1, 30
    logits, x = _ce_inputs(B, T, V, 32, 0, seed=11)
    loss, count, dref = _ce_ref(logits, 32, x, 0, B, T, V, 1.0, None)
    loss2, dl = _ce_run(logits, 32, x, 0, B, T, V, 1.0, None, dt, 32)
    assert np.isnan(loss) and np.isnan(loss2[0]) and loss2[1] == 0 == count
    assert not dref.any() and not dl.any()


def test_ce_loss_is_deterministic():
    B, T, V = 1024, 100, 30
    logits, x = _ce_inputs(B, T, V, 32, 3, seed=5)
    a = _ce_run(logits, 32, x, 3, B, T, V, 1.0, None, torch.float32, 32)
    b = _ce_run(logits, 32, x, 3, B, T, V, 1.0, None, torch.float32, 32)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_ce_loss_out_of_range_target_gives_nan_and_is_never_read(dt):
    """An id < 0 or >= V that is not pad: NaN loss (as mvae_ce_rows_fwd and the fused ELBO), not counted, and a zero CE gradient for its
    row, so dlogits stays finite; the external dy is still added.  The bad ids sit at interior rows (their neighbours' logits exist), so
    a kernel that used them as addresses would still read inside the buffer -- and return a finite loss."""
    B, T, V, pad = 4, 6, 30, 0
    logits, x = _ce_inputs(B, T, V, V, pad, seed=21, all_pad_seq=False)
    x[x == pad] = 1
    bad = {(1, 2): -1, (2, 3): V, (1, 4): V + 1}                 # (b, t + 1): rows t*B + b = 5, 10, 13 of 24
    for k, v in bad.items():
        x[k] = v
    dy_ext = (0.01 * np.random.RandomState(2).standard_normal((B, T, V))).astype(np.float32)
    loss2, dl = _ce_run(logits, V, x, pad, B, T, V, 0.5, dy_ext, dt, 32)
    assert np.isnan(loss2[0]), f"finite loss {loss2[0]} from out-of-range targets"
    xs = x.copy()
    for k in bad:
        xs[k] = pad                                              # the valid targets alone
    _, count, dref = _ce_ref(logits, V, xs, pad, B, T, V, 0.5, dy_ext)
    assert loss2[1] == count == B * (T - 1) - len(bad)
    assert np.isfinite(dl).all() and not dl[:, V:].any()
    tol = 4e-6 * 0.5 / count + 1e-6 * np.abs(dy_ext).transpose(1, 0, 2).reshape(T * B, V)
    if dt == torch.bfloat16:
        tol = tol + 2.0 ** -8 * np.abs(dref)
    assert (np.abs(dl[:, :V] - dref) <= tol).all()
    for (b, t1) in bad:                                          # those rows: dy_ext alone
        row = (t1 - 1) * B + b
        ext_row = dy_ext[b, t1 - 1].astype(np.float64)
        if dt == torch.float32:
            assert np.array_equal(dl[row, :V], ext_row)
        else:
            assert np.array_equal(dl[row, :V], torch.from_numpy(dy_ext[b, t1 - 1]).to(torch.bfloat16).double().numpy())


# ------------------------------------------------------------------------------------------------ MOSES latent (reparameterisation + KL)
def _latent_ref(mu, lv, eps, dz_in, dkl, dlv_ext):
    m = torch.from_numpy(mu.astype(np.float64)).requires_grad_(True)
    v = torch.from_numpy(lv.astype(np.float64)).requires_grad_(True)
    e = torch.from_numpy(eps.astype(np.float64))
    z = m + torch.exp(v / 2) * e
    kl = 0.5 * (torch.exp(v) + m ** 2 - 1 - v).sum(1).mean()
    obj = kl * (dkl if dkl is not None else 0.0)
    if dz_in is not None:
        obj = obj + (z * torch.from_numpy(dz_in.astype(np.float64))).sum()
    if dlv_ext is not None:
        obj = obj + (v * torch.from_numpy(dlv_ext.astype(np.float64))).sum()
    if obj.requires_grad:
        obj.backward()
    gm = m.grad.numpy() if m.grad is not None else np.zeros_like(mu, np.float64)
    gv = v.grad.numpy() if v.grad is not None else np.zeros_like(lv, np.float64)
    return z.detach().numpy(), float(kl), gm, gv


@pytest.mark.parametrize("B,dz", [(1, 1), (3, 63), (5, 64), (3, 65), (1, 128), (5, 300), (1024, 64), (1024, 65)])
def test_moses_latent_matches_float64(B, dz):
    rs = np.random.RandomState(B * 1000 + dz)
    mu = rs.standard_normal((B, dz)).astype(np.float32)
    lv = (0.8 * rs.standard_normal((B, dz))).astype(np.float32)
    lv.flat[:: 7] = 0.0
    eps = rs.standard_normal((B, dz)).astype(np.float32)
    tmu, tlv, teps = g32(mu), g32(lv), g32(eps)
    z = torch.full((B, dz), float("nan"), device=dev); kl = torch.full((1,), float("nan"), device=dev)
    ops.moses_latent_fwd(tmu, tlv, teps, z, kl, B, dz)
    zr, klr, _, _ = _latent_ref(mu, lv, eps, None, None, None)
    zh = host(z).numpy().astype(np.float64)
    assert (np.abs(zh - zr) <= 1e-6 * (np.abs(mu) + np.abs(np.exp(lv / 2.0) * eps)) + 1e-30).all()
    # 1e-6 relative to the size of the summed terms: each term exp(lv) + mu^2 - 1 - lv cancels to ~mu^2 where lv ~ 0
    kl_mag = 0.5 * (np.exp(lv.astype(np.float64)) + mu.astype(np.float64) ** 2 + 1.0 + np.abs(lv)).sum(1).mean()
    assert abs(float(kl) - klr) <= 1e-6 * kl_mag, (float(kl), klr)
    z2 = torch.empty_like(z); kl2 = torch.empty_like(kl)
    ops.moses_latent_fwd(tmu, tlv, teps, z2, kl2, B, dz)
    assert torch.equal(z, z2) and torch.equal(kl, kl2)
    # backward with each optional input given or absent
    dz_in = rs.standard_normal((B, dz)).astype(np.float32)
    dlv_ext = rs.standard_normal((B, dz)).astype(np.float32)
    dkl = np.float32(1.3)
    for mask in range(8):
        a = dz_in if mask & 1 else None
        k = dkl if mask & 2 else None
        c = dlv_ext if mask & 4 else None
        dmu = torch.full((B, dz), float("nan"), device=dev); dlv = torch.full((B, dz), float("nan"), device=dev)
        ops.moses_latent_bwd(tmu, tlv, teps, None if a is None else g32(a), None if k is None else g32(np.array([k])),
                             None if c is None else g32(c), dmu, dlv, B, dz)
        _, _, gm, gv = _latent_ref(mu, lv, eps, a, None if k is None else float(k), c)
        kk = float(k) if k is not None else 0.0
        aa = np.abs(a) if a is not None else 0.0
        bm = 1e-6 * (aa + abs(kk) * np.abs(mu) / B) + 1e-30
        bv = 1e-6 * (aa * np.abs(eps) * 0.5 * np.exp(lv / 2.0) + abs(kk) * 0.5 * (np.exp(lv) + 1.0) / B + (np.abs(c) if c is not None else 0.0)) + 1e-30
        assert (np.abs(host(dmu).numpy() - gm) <= bm).all(), mask
        assert (np.abs(host(dlv).numpy() - gv) <= bv).all(), mask


# ------------------------------------------------------------------------------------------------ reductions
def _padded(X, ld, dt, fill=float("nan")):
    """X [M, N] into a [M, ld] device buffer of dtype dt whose columns N..ld-1 hold `fill`"""
    M, N = X.shape
    buf = torch.full((max(M, 1), ld), fill, dtype=torch.float32)
    buf[:M, :N] = torch.from_numpy(X)
    return buf.to(dt).to(dev)


def _check_sum(got, X64, exact, axis):
    ref = X64.sum(axis)
    if exact:
        assert np.array_equal(got, ref), np.flatnonzero(got != ref)[:8]
    else:
        assert (np.abs(got - ref) <= 2e-6 * np.abs(X64).sum(axis)).all()


@pytest.mark.parametrize("M", [0, 1, 127, 128, 129, 40000])
@pytest.mark.parametrize("kind", ["colsum_f32", "colsum_t_f32", "colsum_t_bf16"])
def test_colsum_exact_integers_random_floats_and_determinism(kind, M):
    dt = torch.bfloat16 if kind.endswith("bf16") else torch.float32
    fn = ops.colsum if kind == "colsum_f32" else ops.colsum_t
    rs = np.random.RandomState(M + len(kind))
    for N in (1, 7, 9, 300):
        ld = N + (5 if kind == "colsum_f32" else 8 - N % 8 + 8)    # colsum_t needs ldx % 8 == 0; always some garbage pad
        for exact in (True, False):
            X = ints(rs, (M, N)) if exact else rs.standard_normal((M, N)).astype(np.float32)
            Xd = _padded(X, ld, dt)
            X64 = Xd[:M, :N].float().cpu().numpy().astype(np.float64)      # the values as stored (bf16-rounded for the random pass)
            out = torch.full((N + 3,), float("nan"), device=dev)
            fn(Xd, M, N, out, ldx=ld)
            got = host(out).numpy()
            assert np.isnan(got[N:]).all(), "written past N"
            if M == 0:
                assert np.array_equal(got[:N], np.zeros(N)), "M = 0 must give zeros"
            _check_sum(got[:N].astype(np.float64), X64, exact, 0)
            out2 = torch.full((N + 3,), float("nan"), device=dev)
            fn(Xd, M, N, out2, ldx=ld)
            assert torch.equal(out[:N], out2[:N])


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [1, 7, 8, 1000])
def test_rowsum_aligned_and_unaligned_rows_with_and_without_accumulate(C, dt):
    rs = np.random.RandomState(C)
    R = 37
    epc = 4 if dt == torch.float32 else 8
    for ld in (C + (-C) % epc + epc, C + 1 + (C % 2)):              # 16-byte aligned rows; then an odd pitch (rows alternate alignment)
        for exact in (True, False):
            X = ints(rs, (R, C)) if exact else rs.standard_normal((R, C)).astype(np.float32)
            Xd = _padded(X, ld, dt)
            X64 = Xd[:, :C].float().cpu().numpy().astype(np.float64)
            init = ints(rs, (R,))
            for acc in (False, True):
                out = torch.full((R + 2,), float("nan"), device=dev)
                if acc:
                    out[:R] = g32(init)
                ops.rowsum(Xd, R, C, out, ldx=ld, accumulate=acc)
                got = host(out).numpy()
                assert np.isnan(got[R:]).all()
                ref = X64.sum(1) + (init.astype(np.float64) if acc else 0.0)
                if exact:
                    assert np.array_equal(got[:R], ref), (ld, acc)
                else:
                    assert (np.abs(got[:R] - ref) <= 2e-6 * (np.abs(X64).sum(1) + (np.abs(init) if acc else 0.0))).all(), (ld, acc)
                out2 = torch.full((R + 2,), float("nan"), device=dev)
                if acc:
                    out2[:R] = g32(init)
                ops.rowsum(Xd, R, C, out2, ldx=ld, accumulate=acc)
                assert torch.equal(out[:R], out2[:R])


@pytest.mark.parametrize("T", [1, 3, 4, 7, 120])
@pytest.mark.parametrize("path", ["f32", "bf16_vec", "bf16_odd_bw", "bf16_unaligned_out"])
def test_timesum_vector_path_and_its_fallbacks(path, T):
    dt = torch.float32 if path == "f32" else torch.bfloat16
    B, W = (6, 40) if path != "bf16_odd_bw" else (5, 13)           # B*W % 8 != 0 forces the scalar fallback
    rs = np.random.RandomState(T)
    for exact in (True, False):
        X = ints(rs, (T, B, W)) if exact else rs.standard_normal((T, B, W)).astype(np.float32)
        Xd = torch.from_numpy(X).to(dt).to(dev)
        X64 = Xd.float().cpu().numpy().astype(np.float64)
        off = 1 if path == "bf16_unaligned_out" else 0              # out one float past a 16-byte boundary: the scalar fallback
        runs = []
        for _ in range(2):
            buf = torch.full((B * W + 2,), float("nan"), device=dev)
            ops.timesum(Xd, T, B, W, buf[off:off + B * W])
            runs.append(host(buf).numpy())
        got = runs[0]
        assert np.isnan(got[:off]).all() and np.isnan(got[off + B * W:]).all()
        _check_sum(got[off:off + B * W].reshape(B, W).astype(np.float64), X64, exact, 0)
        assert np.array_equal(runs[0], runs[1], equal_nan=True)


# ------------------------------------------------------------------------------------------------ casts, transposes, the pack table
def _bits(x):
    return x.view(torch.int16) if x.dtype == torch.bfloat16 else x.view(torch.int32)


def _sentinel(shape, dt):
    if dt == torch.bfloat16:
        return torch.full(shape, SENT_BF16, dtype=torch.int16, device=dev).view(torch.bfloat16)
    return torch.full(shape, SENT, dtype=torch.float32, device=dev)


def _special_f32():
    """values where a float -> bf16 conversion goes wrong: exact ties (half an ulp above values with even and odd last bits), just off a
    tie, +-inf, the largest finite f32 and bf16 values, the smallest normal, f32 subnormals, signed zeros, and NaN"""
    v = [1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, -(1.0 + 2 ** -8), -(1.0 + 3 * 2 ** -8), 3.0 + 2 ** -7, 256.0 + 1.0, 257.0 + 2.0,
         1.0 + 2 ** -8 + 2 ** -20, 1.0 + 2 ** -8 - 2 ** -20, np.inf, -np.inf, 3.4028234663852886e38, -3.4028234663852886e38,
         3.3895313892515355e38, 3.3961775292304e38, 1.1754943508222875e-38, 1e-40, -1e-40, 9.2e-41, 2 ** -133, 2 ** -149,
         2 ** -133 + 2 ** -141, 0.0, -0.0, np.nan]
    return np.array(v, np.float32)


def _expect_cast(src_f32_or_bf16, dt):
    return src_f32_or_bf16.cpu().to(dt)


def _assert_cast_equal(got, want):
    """bit-exact, except that any NaN only has to stay a NaN (its payload is the converter's choice)"""
    got, want = got.cpu(), want.cpu()
    nan = torch.isnan(want.float())
    assert torch.equal(torch.isnan(got.float()), nan)
    assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), (got[~nan], want[~nan])


PAIRS = [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32)]


@pytest.mark.parametrize("sdt,ddt", PAIRS, ids=["f32-f32", "f32-bf16", "bf16-bf16", "bf16-f32"])
def test_cast_transpose_all_dtype_pairs_with_zero_filled_pads(sdt, ddt):
    rs = np.random.RandomState(7)
    for R in (1, 31, 32, 33, 100):
        for C_ in (1, 31, 32, 33, 100):
            lds, ldd, ldt = C_ + 3, C_ + 5, R + 6
            src = torch.from_numpy(rs.standard_normal((R, lds)).astype(np.float32) * 3).to(sdt).to(dev)
            dst_full, dstT_full = _sentinel((R + 2, ldd), ddt), _sentinel((C_ + 2, ldt), ddt)
            ops.cast_transpose(src, R, C_, dst=dst_full[:R], dstT=dstT_full[:C_], lds=lds)
            want = _expect_cast(src[:, :C_], ddt)
            dst, dstT = host(dst_full), host(dstT_full)
            assert torch.equal(_bits(dst[:R, :C_]), _bits(want)), (R, C_)
            assert torch.equal(_bits(dstT[:C_, :R]), _bits(want.t().contiguous())), (R, C_)
            assert not dst[:R, C_:].float().any() and not dstT[:C_, R:].float().any(), "pad columns must be zero-filled"
            assert torch.equal(_bits(dst[R:]), _bits(_sentinel((2, ldd), ddt).cpu())), "rows past R touched"
            assert torch.equal(_bits(dstT[C_:]), _bits(_sentinel((2, ldt), ddt).cpu())), "rows past C touched"
    # dstT alone
    src = torch.from_numpy(rs.standard_normal((33, 40)).astype(np.float32)).to(sdt).to(dev)
    only_t = _sentinel((33, 36), ddt)
    ops.cast_transpose(src, 33, 33, dstT=only_t, lds=40)
    assert torch.equal(_bits(host(only_t)[:, :33]), _bits(_expect_cast(src[:, :33], ddt).t().contiguous()))
    assert not host(only_t)[:, 33:].float().any()


def test_bf16_stores_round_to_nearest_even_like_torch():
    """f2bf: ties to even, +-inf, the largest finite values (the f32 maximum rounds up to inf), subnormals, and NaN staying NaN -- through
    mvae_cast_transpose (dst and dstT) and through kind 0 of mvae_pack_multi."""
    v = torch.from_numpy(_special_f32())
    want = v.to(torch.bfloat16)
    n = v.numel()
    src = v.reshape(1, n).to(dev)
    dst, dstT = _sentinel((1, n + 3), torch.bfloat16), _sentinel((n, 8), torch.bfloat16)
    ops.cast_transpose(src, 1, n, dst=dst, dstT=dstT)
    _assert_cast_equal(host(dst)[0, :n], want)
    _assert_cast_equal(host(dstT)[:, 0], want)
    pk = ops.PackList()
    d2 = _sentinel((1, n), torch.bfloat16)
    pk.cast_transpose(src, 1, n, dst=d2)
    pk.run()
    _assert_cast_equal(host(d2)[0], want)
    # random fp32 values with every low-bit pattern: each is rounded exactly as torch rounds it
    rs = np.random.RandomState(1)
    r = (rs.standard_normal((64, 257)) * np.exp2(rs.randint(-30, 30, (64, 257)))).astype(np.float32)
    r.view(np.uint32)[:, :32] = (r.view(np.uint32)[:, :32] & 0xFFFF0000) | 0x8000      # exact ties
    tr = torch.from_numpy(r).to(dev)
    out = _sentinel((64, 257), torch.bfloat16)
    ops.cast_transpose(tr, 64, 257, dst=out)
    assert torch.equal(_bits(host(out)), _bits(torch.from_numpy(r).to(torch.bfloat16)))


def test_pack_multi_mixed_table_touches_only_its_blocks():
    rs = np.random.RandomState(3)

    def f(*shape):
        return torch.from_numpy(rs.standard_normal(shape).astype(np.float32)).to(dev)

    # kind 0: f32 -> bf16, dst and dstT as sub-blocks of larger buffers
    s0 = f(33, 104)
    d0_full, t0_full = _sentinel((40, 120), torch.bfloat16), _sentinel((110, 48), torch.bfloat16)
    d0, t0 = d0_full[2:35, 3:103], t0_full[1:101, 5:38]
    # kind 1: out = a + b over 2500 elements (three blocks, the last partial), and a zero-element add between two other jobs
    a1, b1 = f(2500), f(2500)
    o1_full = torch.full((2600,), SENT, device=dev); o1 = o1_full[40:2540]
    e_a, e_b, e_o = torch.empty(0, device=dev), torch.empty(0, device=dev), torch.empty(0, device=dev)
    # kind 2: f32 block copy with leading dimensions
    s2_full = f(31, 50)
    d2_full = torch.full((36, 60), SENT, device=dev); d2 = d2_full[4:35, 7:47]
    # kind 0: f32 -> f32, dstT only, one row
    s3 = f(1, 31)
    t3_full = torch.full((33, 4), SENT, device=dev); t3 = t3_full[1:32, 1:2]
    # kind 0: bf16 -> bf16 and bf16 -> f32
    s4 = f(32, 32).to(torch.bfloat16)
    d4_full = _sentinel((34, 40), torch.bfloat16); d4 = d4_full[1:33, 4:36]
    s5 = f(7, 65).to(torch.bfloat16)
    d5_full = torch.full((9, 70), SENT, device=dev); d5 = d5_full[1:8, 2:67]
    pk = ops.PackList()
    pk.cast_transpose(s0, 33, 100, dst=d0, dstT=t0)
    pk.add(a1, b1, o1)
    pk.add(e_a, e_b, e_o)
    pk.copy(s2_full[:, 3:43], d2)
    pk.cast_transpose(s3, 1, 31, dstT=t3)
    pk.cast_transpose(s4, 32, 32, dst=d4)
    pk.cast_transpose(s5, 7, 65, dst=d5)
    assert [L.load().mvae_pack_job_blocks(j) for j in pk.jobs] == [4 * 2, 3, 0, 2 * 1, 1, 1, 3]
    pk.run()
    torch.cuda.synchronize()

    def outside(full, r0, r1, c0, c1, sentinel_full):
        m = torch.ones(full.shape, dtype=torch.bool)
        m[r0:r1, c0:c1] = False
        return torch.equal(_bits(full.cpu())[m], _bits(sentinel_full.cpu())[m])

    want0 = s0[:, :100].cpu().to(torch.bfloat16)
    assert torch.equal(_bits(d0.cpu()), _bits(want0)) and torch.equal(_bits(t0.cpu()), _bits(want0.t().contiguous()))
    assert outside(d0_full, 2, 35, 3, 103, _sentinel((40, 120), torch.bfloat16))
    assert outside(t0_full, 1, 101, 5, 38, _sentinel((110, 48), torch.bfloat16))
    assert torch.equal(o1.cpu(), a1.cpu() + b1.cpu())
    assert (o1_full[:40].cpu() == SENT).all() and (o1_full[2540:].cpu() == SENT).all()
    assert torch.equal(d2.cpu(), s2_full[:, 3:43].cpu()) and outside(d2_full, 4, 35, 7, 47, torch.full((36, 60), SENT))
    assert torch.equal(t3.cpu(), s3.cpu().t()) and outside(t3_full, 1, 32, 1, 2, torch.full((33, 4), SENT))
    assert torch.equal(_bits(d4.cpu()), _bits(s4.cpu())) and outside(d4_full, 1, 33, 4, 36, _sentinel((34, 40), torch.bfloat16))
    assert torch.equal(d5.cpu(), s5.cpu().float()) and outside(d5_full, 1, 8, 2, 67, torch.full((9, 70), SENT))
    # run again: the same table, the same result
    before = [x.clone() for x in (d0_full, t0_full, o1_full, d2_full, t3_full, d4_full, d5_full)]
    pk.run()
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(before, (d0_full, t0_full, o1_full, d2_full, t3_full, d4_full, d5_full)))


# ------------------------------------------------------------------------------------------------ permutes, masks, one-hots, input pipeline
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 7, 5), (2, 33, 65), (3, 400, 501)])
def test_permute021_and_permute102_bit_exact(shape):
    N, A, Bd = shape
    rs = np.random.RandomState(A)
    x = rs.standard_normal(shape).astype(np.float32)
    out = torch.full((N * A * Bd + 4,), float("nan"), device=dev)
    ops.permute021(g32(x), out, N, A, Bd)
    o = host(out)
    assert torch.equal(o[:N * A * Bd], torch.from_numpy(x.transpose(0, 2, 1).reshape(-1).copy())) and torch.isnan(o[N * A * Bd:]).all()
    T, B, V = shape
    out = torch.full((T * B * V + 4,), float("nan"), device=dev)
    ops.permute102(g32(x), out, T, B, V)
    o = host(out)
    assert torch.equal(o[:T * B * V], torch.from_numpy(x.transpose(1, 0, 2).reshape(-1).copy())) and torch.isnan(o[T * B * V:]).all()


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_mask_rows_tb_clears_exactly_the_finished_rows(dt):
    T, B = 9, 7
    rs = np.random.RandomState(0)
    lengths = np.array([9, 0, 4, 1, 8, 9, 5], np.int32)              # 0 and T included
    for ld in ((40, 24) if dt == torch.float32 else (40, 24, 8)):
        x = torch.from_numpy(rs.standard_normal((T * B, ld)).astype(np.float32)).to(dt).to(dev)
        keep = torch.from_numpy((np.arange(T)[:, None] < lengths[None, :]).reshape(-1))          # row t*B + b kept iff t < lengths[b]
        before = host(x).clone()
        ops.mask_rows_tb(x, T, B, torch.from_numpy(lengths).to(dev))
        after = host(x)
        assert torch.equal(_bits(after[keep]), _bits(before[keep])), "a kept row changed"
        assert torch.equal(_bits(after[~keep]), torch.zeros_like(_bits(after[~keep]))), "a finished row is not +0"


def test_onehot_f32_pads_and_clamped_ids():
    rs = np.random.RandomState(1)
    nrows, ld, n = 35, 44, 1001
    idx = rs.randint(0, nrows, n).astype(np.int64)
    idx[[3, 50, 999]] = [-1, nrows, 1 << 40]                        # out-of-range ids are clamped to [0, nrows)
    full = torch.full((n + 2, ld), float("nan"), device=dev)
    ops.onehot_f32(torch.from_numpy(idx).to(dev), full[:n], nrows)
    want = np.zeros((n, ld), np.float32)
    want[np.arange(n), np.clip(idx, 0, nrows - 1)] = 1.0
    got = host(full)
    assert torch.equal(got[:n], torch.from_numpy(want)) and torch.isnan(got[n:]).all()


@pytest.mark.parametrize("with_ohe", [True, False])
def test_expand_indices_permuted_and_repeated_rows(with_ohe):
    rs = np.random.RandomState(2)
    N, Lq, C_, B = 50, 120, 35, 300
    store = rs.randint(0, C_, (N, Lq)).astype(np.uint8)
    rows = rs.randint(0, N, B).astype(np.int64)
    rows[:5] = [49, 0, 49, 7, 7]
    idx = torch.full((B, Lq), -7, dtype=torch.int64, device=dev)
    ohe = torch.full((B, Lq, C_), float("nan"), device=dev) if with_ohe else None
    ops.expand_indices(torch.from_numpy(store).to(dev), torch.from_numpy(rows).to(dev), idx, ohe, B, Lq, C_)
    want = store[rows].astype(np.int64)
    assert torch.equal(host(idx), torch.from_numpy(want))
    if with_ohe:
        assert torch.equal(host(ohe), torch.from_numpy(np.eye(C_, dtype=np.float32)[want]))


# ------------------------------------------------------------------------------------------------ activation backwards (grid-stride loops)
N_BIG = 600_007                 # > 2048 blocks * 256 threads: the grid-stride loops run a second round; not a multiple of 256


def _pre_with_edges(rs, n):
    x = rs.standard_normal(n) * 2.0
    x[rs.choice(n, 5000, replace=False)] = 0.0                       # y exactly 0
    x[:8] = [0.0, -0.0, 1e-30, -1e-30, -30.0, 30.0, -1e-7, 1e-7]
    return x


def test_relu_bwd_bit_exact():
    rs = np.random.RandomState(4)
    y = np.maximum(_pre_with_edges(rs, N_BIG), 0.0).astype(np.float32)
    y[1::3] = -np.abs(y[1::3]) - 1.0                                   # negative values too (an arbitrary input, not only relu outputs)
    dy = rs.standard_normal(N_BIG).astype(np.float32)
    d = g32(dy)
    ops.relu_bwd(d, g32(y))
    assert torch.equal(host(d), torch.from_numpy(np.where(y > 0, dy, np.float32(0.0))))


def test_selu_bwd_matches_float64_autograd():
    """dy * selu'(x) through the forward output y = selu(x): at x = 0 the reference (scale * ELU) has derivative scale * alpha"""
    rs = np.random.RandomState(5)
    x = torch.from_numpy(_pre_with_edges(rs, N_BIG)).requires_grad_(True)
    y64 = torch.selu(x)
    dy = rs.standard_normal(N_BIG).astype(np.float32)
    y64.backward(torch.from_numpy(dy.astype(np.float64)))
    ref = x.grad.numpy()
    y32 = y64.detach().numpy().astype(np.float32)
    d = g32(dy)
    ops.selu_bwd(d, g32(y32))
    got = host(d).numpy().astype(np.float64)
    sa = 1.0507009873554804934193349852946 * 1.6732632423543772848170429916717
    bound = 1e-6 * np.abs(dy) * (np.abs(y32) + sa)
    assert (np.abs(got - ref) <= bound).all()
    zero = y32 == 0
    assert zero.sum() >= 4990 and np.allclose(got[zero], dy[zero] * sa, rtol=1e-6, atol=0)


def test_lambda_bwd_matches_float64_autograd():
    rs = np.random.RandomState(6)
    B, o = 1031, 520                                                  # B*o = 536120 > 524288, not a multiple of 256
    mu = rs.standard_normal((B, o)).astype(np.float32)
    lv = rs.standard_normal((B, o)).astype(np.float32)
    lv[:, ::5] = 0.0
    lv[:, 1::5] = -np.abs(lv[:, 1::5])
    eps = rs.standard_normal((B, o)).astype(np.float32)
    dz, dmu, dlv = (rs.standard_normal((B, o)).astype(np.float32) for _ in range(3))
    mulv = g32(np.concatenate([mu, lv], 1))
    for mask in (7, 1, 2, 4, 0):
        a, b, c = (dz if mask & 1 else None), (dmu if mask & 2 else None), (dlv if mask & 4 else None)
        out = torch.full((B, 2 * o), float("nan"), device=dev)
        ops.lambda_bwd(mulv, g32(eps), *(None if v is None else g32(v) for v in (a, b, c)), out, B, o)
        m = torch.from_numpy(mu.astype(np.float64)).requires_grad_(True)
        v_ = torch.from_numpy(lv.astype(np.float64)).requires_grad_(True)
        z = m + torch.exp(v_ / 2) * torch.from_numpy(eps.astype(np.float64))
        obj = (z * 0).sum()
        for term, val in ((z, a), (m, b), (v_, c)):
            if val is not None:
                obj = obj + (term * torch.from_numpy(val.astype(np.float64))).sum()
        obj.backward()
        got = host(out).numpy().astype(np.float64)
        aa = np.abs(a) if a is not None else 0.0
        bm = 1e-6 * (aa + (np.abs(b) if b is not None else 0.0)) + 1e-30
        bv = 1e-6 * (aa * np.abs(eps) * 0.5 * np.exp(lv / 2.0) + (np.abs(c) if c is not None else 0.0)) + 1e-30
        assert (np.abs(got[:, :o] - m.grad.numpy()) <= bm).all(), mask
        assert (np.abs(got[:, o:] - v_.grad.numpy()) <= bv).all(), mask


# ------------------------------------------------------------------------------------------------ Conv1d + ReLU (models2d)
@pytest.mark.parametrize("case", [
    (3, 7, 23, 5, 4, 8, 8, 29, True),          # ragged: nothing aligned to a K-step
    (64, 120, 35, 9, 9, 120, 12, 35, False),   # models2d conv1d1: one-hot block, no dx, no wq
    (64, 9, 27, 9, 9, 12, 12, 27, True),       # conv1d2
    (64, 9, 19, 10, 11, 12, 12, 19, True),     # conv1d3
])
def test_conv1d_relu_vs_oracle(case):
    B, Cin, W, Cout, k, ldx, ldo, Wbuf, want_dx = case
    rs = np.random.RandomState(B + Cin + W)
    x = rs.standard_normal((B, Cin, W)) * 0.5
    w = rs.standard_normal((Cout, Cin, k)) * (1.0 / np.sqrt(Cin * k)); b = rs.standard_normal(Cout) * 0.1
    y_ref, cache = O.conv_relu_fwd(x, w, b)
    Wout = W - k + 1
    xd = torch.zeros(B, Wbuf, ldx, device=dev); xd[:, :W, :Cin] = g32(x.transpose(0, 2, 1))
    wd, bd = g32(w), g32(b)
    wp = torch.full((Cout, k * ldx), 7.0, device=dev)
    wq = torch.full((Cin, k * ldo), 7.0, device=dev) if want_dx else None
    ops.conv1d_pack_weights(wd, Cin, Cout, k, ldx, wp, ldo if want_dx else 0, wq)
    y = torch.full((B * Wout, ldo), float("nan"), device=dev)
    ops.conv1d_selu_fwd(xd, B, W, ldx, Wbuf * ldx, Cout, k, wp, bd, y, ldo, act=L.ACT_RELU)
    yh = host(y).numpy()
    yk = yh.reshape(B, Wout, ldo)[:, :, :Cout].transpose(0, 2, 1)
    assert np.abs(yk - y_ref).max() <= 1e-5 * np.abs(y_ref).max() and (yk >= 0).all()
    assert np.isnan(yh[:, Cout:]).all(), "columns Cout..ldo-1 of y are not written"
    # the kernel takes the derivative from y: where the pre-activation is within fp32 rounding of 0, its sign is the forward's (checked above)
    pre = cache[2]
    pre = np.where(np.abs(pre) <= 1e-6 * np.abs(pre).max(), np.where(yk > 0, 1.0, -1.0), pre)
    cache = (cache[0], cache[1], pre, cache[3])
    dy = rs.standard_normal(y_ref.shape)
    dx_ref, dw_ref, db_ref = O.conv_relu_bwd(dy, cache)
    dyd = torch.zeros(B * Wout, ldo, device=dev); dyd[:, :Cout] = g32(dy.transpose(0, 2, 1).reshape(B * Wout, Cout))
    dzp = torch.full((B * (Wout + 2 * k - 2), ldo), 3.0, device=dev)
    dw = torch.full((Cout, Cin, k), float("nan"), device=dev); db = torch.full((Cout,), float("nan"), device=dev)
    dx = torch.zeros(B * W, ldx, device=dev) if want_dx else None
    ops.conv1d_selu_bwd(B, W, Cin, ldx, Wbuf * ldx, Cout, ldo, k, dyd, y, xd, wq, dzp, dw, db, dx, ldx if want_dx else 0, act=L.ACT_RELU)
    dwh, dbh = host(dw).numpy(), host(db).numpy()
    assert np.abs(dwh - dw_ref).max() <= 1e-5 * np.abs(dw_ref).max() and np.abs(dbh - db_ref).max() <= 1e-5 * np.abs(db_ref).max()
    if want_dx:
        dxh = host(dx).numpy().reshape(B, W, ldx)
        assert np.abs(dxh[:, :, :Cin].transpose(0, 2, 1) - dx_ref).max() <= 1e-5 * np.abs(dx_ref).max()
        assert not dxh[:, :, Cin:].any()
