"""float64 references, input recipes and per-element error bounds for the GEMM entries (csrc/gemm.hip): numpy only, no GPU, nothing imported
from the package.  test_gemm_ref_host.py checks this file against numpy.matmul on explicit im2col and shows that the bounds reject every
planted mutant; test_gpu_gemm_kernels.py holds the kernels to it.

Operations
  nt(A, B, bias, act, c0)      C = act(A . B^T + bias) (+ c0: accumulate), A [M, K], B [N, K]
  tn(A, B, c0)                 C = A^T . B (+ c0), A [K, M], B [K, N];  colsum(A, c0) = sum_k A[k, :] (+ c0)
  rows(buf, R, L, ld, group, gstride)
                               the operand matrix a kernel sees in a flat buffer: row r is the L elements that start at
                               (r // group) * gstride + (r % group) * ld when group > 0, at r * ld otherwise.  Rows of one group may overlap
                               (ld < L): the channels-last Conv1d reads its im2col matrix this way.

Inputs
  ints(rs, shape)   integers in [-8, 8].  |a b| <= 64, so every partial sum of up to K = 2^17 products is an integer of magnitude <= 2^23:
                    exact in fp32 whatever the order, tile or split, and the operands are exact in bf16 (8 significant bits).  The three
                    bf16 products of the x3 form are exact too (hi = the value, lo = 0).  A kernel must therefore return the integer
                    result bit for bit (ACT_NONE / ACT_RELU; a bf16 C: that integer rounded once to bf16).  No tolerance.
  floats(rs, shape, bf16)
                    standard normals rounded to the storage type first, so that the check isolates the kernel.

Bounds (per element, from the CPU alone).  Scale  s_ij = sum_k |a_ik b_jk| (+ |bias_j|).
  f32 / bf16 operands, fp32 accumulate:  |got - ref| <= 4 rho s_ij + 2^-23 s_ij,  rho = max_ij |C_f32numpy - C_f64| / s_ij  with the numpy
      float32 product summed in K-steps of ke (32 elements for f32, 64 for bf16: 128 bytes, KB / sizeof(T) in csrc/common.hpp).  The
      factor 4 is the argument of test_gpu_gru_kernels.py / test_gpu_lstm_kernels.py: the kernel sums in MFMA-tile and split order, a
      different sample of the same rounding noise.  2^-23 s_ij is one fp32 ulp of the scale: the final rounding (and the floor for tiny K,
      where rho can be 0).
  x3 (fp32 operands as three bf16 products, split_x3 in csrc/tile_pipe.hpp):  x = hi + lo + d  with  hi = x truncated to bf16 (8 significant
      bits: |x - hi| < 2^-7 |x|, and x - hi is exact in fp32: it is the low 16 mantissa bits), lo = bf16(x - hi) rounded to nearest
      (unit roundoff 2^-8), so |lo| <= 2^-7 (1 + 2^-8) |x| and |d| <= 2^-8 . 2^-7 |x| = 2^-15 |x|.  The kernel adds ah bh + ah bl + al bh
      (each product of two bf16 is exact in fp32); against a b it lacks  al bl + da b + a db + da db:
          |al bl| <= 2^-14 (1 + 2^-8)^2 |a b| = 4.032 . 2^-16 |a b|,   |da b| + |a db| <= 2 . 2^-15 |a b| = 4 . 2^-16 |a b|,   |da db| <= 2^-30 |a b|
      i.e. at most 8.04 . 2^-16 |a b| per product: X3_C = 8.04, bound = X3_C . 2^-16 s_ij on top of the fp32-accumulate bound.
  bf16 C:  one bf16 ulp of |ref_ij| on top (ulp = 2^(e - 7), 2^e <= |ref| < 2^(e + 1)).
  accumulate (C += result, fp32 C):  the scale does not take c0 in; the one fp32 add onto C costs half an ulp of its result, and c0 is itself
      a rounded fp32 value: 2^-24 |ref_ij| + 2^-23 |c0_ij| on top (nt_bound).
  activations:  the bound on the pre-activation z passes through act with act's global Lipschitz constant -- 1 for ReLU, scale . alpha =
      1.7581 for SELU (the slope at 0-) -- which holds ACROSS the kink at 0, so inputs need not be kept away from it (this is the "widen by
      the slope difference" choice, taken everywhere); SELU adds test_gpu_helper_kernels.py's 1e-6 (|ref| + scale . alpha) for expm1f.
"""
import numpy as np

ACT_NONE, ACT_SELU, ACT_RELU = 0, 1, 2          # include/mvae.h
KE = {"f32": 32, "bf16": 64}
SELU_ALPHA = 1.6732632423543772848170429916717
SELU_SCALE = 1.0507009873554804934193349852946
SELU_SA = SELU_SCALE * SELU_ALPHA
X3_C = 8.04


def bf16_round(x):
    """x (any float array) rounded to nearest-even bf16, returned as float32 (finite inputs)."""
    u = np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def bf16_ulp(x):
    """One bf16 ulp of |x| (float64): 2^(e - 7) for 2^e <= |x| < 2^(e + 1); the smallest normal's ulp at 0."""
    ax = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return np.exp2(np.floor(np.log2(ax)) - 7)


def ints(rs, shape, lo=-8, hi=8):
    return rs.randint(lo, hi + 1, size=shape).astype(np.float32)


def floats(rs, shape, bf16=False):
    x = rs.standard_normal(shape).astype(np.float32)
    return bf16_round(x) if bf16 else x


def row_starts(R, ld, group=0, gstride=0):
    r = np.arange(R, dtype=np.int64)
    return (r // group) * gstride + (r % group) * ld if group > 0 else r * ld


def rows(buf, R, L, ld, group=0, gstride=0):
    """[R, L] operand matrix out of the flat buffer (a copy; rows may overlap in the buffer)."""
    buf = np.asarray(buf).reshape(-1)
    idx = row_starts(R, ld, group, gstride)[:, None] + np.arange(L, dtype=np.int64)[None, :]
    return buf[idx]


def act_fn(z, act):
    z = np.asarray(z, np.float64)
    if act == ACT_RELU:
        return np.maximum(z, 0.0)
    if act == ACT_SELU:
        return np.where(z > 0, SELU_SCALE * z, SELU_SA * np.expm1(np.minimum(z, 0.0)))
    return z


def nt_pre(A, B, bias=None):
    z = np.asarray(A, np.float64) @ np.asarray(B, np.float64).T
    return z if bias is None else z + np.asarray(bias, np.float64)[None, :]


def nt(A, B, bias=None, act=ACT_NONE, c0=None):
    c = act_fn(nt_pre(A, B, bias), act)
    return c if c0 is None else c + np.asarray(c0, np.float64)


def tn(A, B, c0=None):
    c = np.asarray(A, np.float64).T @ np.asarray(B, np.float64)
    return c if c0 is None else c + np.asarray(c0, np.float64)


def colsum(A, c0=None):
    c = np.asarray(A, np.float64).sum(0)
    return c if c0 is None else c + np.asarray(c0, np.float64)


def nt_scale(A, B, bias=None, c0=None):
    s = np.abs(np.asarray(A, np.float64)) @ np.abs(np.asarray(B, np.float64)).T
    if bias is not None:
        s = s + np.abs(np.asarray(bias, np.float64))[None, :]
    return s if c0 is None else s + np.abs(np.asarray(c0, np.float64))


def nt_f32(A, B, ke, bias=None):
    """The same product in numpy float32, summed in K-steps of ke (then the bias, in float32)."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    c = np.zeros((A.shape[0], B.shape[0]), np.float32)
    for k0 in range(0, A.shape[1], ke):
        c = c + A[:, k0:k0 + ke] @ B[:, k0:k0 + ke].T
    return c if bias is None else c + np.asarray(bias, np.float32)[None, :]


def nt_rho(A, B, ke, bias=None):
    """rho = max_ij |C_f32numpy - C_f64| / s_ij: the CPU's own fp32-accumulate floor, in units of the scale."""
    s = nt_scale(A, B, bias)
    d = np.abs(nt_f32(A, B, ke, bias).astype(np.float64) - nt_pre(A, B, bias))
    ok = s > 0
    return float((d[ok] / s[ok]).max()) if ok.any() else 0.0


def bound_pre(s, rho, x3=False):
    b = 4.0 * rho * s + 2.0 ** -23 * s
    return b + X3_C * 2.0 ** -16 * s if x3 else b


def bound_out(bpre, ref, act=ACT_NONE, c_bf16=False):
    """Bound on the stored output given the bound on the pre-activation (ref: the float64 output, WITHOUT any accumulated c0 for bf16)."""
    b = bpre
    if act == ACT_SELU:
        b = SELU_SA * bpre + 1e-6 * (np.abs(ref) + SELU_SA)
    if c_bf16:
        b = b + bf16_ulp(ref)
    return b


def nt_bound(A, B, ke, bias=None, act=ACT_NONE, c0=None, c_bf16=False, x3=False):
    """(ref, bound, rho) for C = act(A . B^T + bias) (+ c0)."""
    rho = nt_rho(A, B, ke, bias)
    ref = nt(A, B, bias, act)
    b = bound_out(bound_pre(nt_scale(A, B, bias), rho, x3), ref, act, c_bf16)
    if c0 is not None:
        ref = ref + np.asarray(c0, np.float64)
        b = b + 2.0 ** -23 * np.abs(np.asarray(c0, np.float64)) + 2.0 ** -24 * np.abs(ref)     # the add onto C: one more fp32 rounding
    return ref, b, rho


def tn_bound(A, B, ke, c0=None, x3=False, bias=None, act=ACT_NONE, c_bf16=False):
    """The TN form is the NT form of the transposes: C = A^T . B = nt(A^T, B^T)."""
    return nt_bound(np.asarray(A).T, np.asarray(B).T, ke, bias=bias, act=act, c0=c0, c_bf16=c_bf16, x3=x3)


def colsum_bound(A, ke, c0=None, x3=False):
    """Column sums of A [K, M] as the product with a column of ones: (ref [M], bound [M], rho)."""
    ones = np.ones((1, np.asarray(A).shape[0]), np.float32)
    ref, b, rho = nt_bound(np.asarray(A).T, ones, ke, c0=None if c0 is None else np.asarray(c0)[:, None], x3=x3)
    return ref[:, 0], b[:, 0], rho


def exact_out(ref, c_bf16=False):
    """The integer recipe's expected output as float32: the float64 integer result, rounded once to bf16 for a bf16 C."""
    r32 = np.asarray(ref, np.float64).astype(np.float32)
    assert (r32.astype(np.float64) == ref).all(), "integer result not representable in fp32: K too large for the recipe"
    return bf16_round(r32) if c_bf16 else r32


def within(got, ref, bound):
    """(ok, worst |got - ref| / bound, its index).  NaN / inf in got fail."""
    got = np.asarray(got, np.float64)
    d = np.abs(got - ref)
    bad = ~(d <= bound)                          # NaN compares false: bad
    ratio = np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d == 0, 0.0, np.inf))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else ()
    return (not bad.any()), (float(ratio[i]) if ratio.size else 0.0), i


def im2col(x, B, W, Cin, k):
    """Explicit im2col of channels-last x [B, W, Cin]: row (b, w) = x[b, w : w + k, :] flattened, [B * Wout, k * Cin]."""
    Wout = W - k + 1
    x = np.asarray(x).reshape(B, W, Cin)
    return np.stack([x[b, w:w + k, :].reshape(-1) for b in range(B) for w in range(Wout)])
