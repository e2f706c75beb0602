"""tests/gemm_ref.py checked without a GPU: the grouped (row-group) reference against numpy.matmul on an explicit im2col, the integer recipe's
exactness at the largest K the GPU suite uses, the x3 constant against a float64 emulation of split_x3, and the bound machinery against
planted mutants of a correct result -- each must be rejected by the float bound AND by the bitwise integer comparison."""
import numpy as np
import pytest

import gemm_ref as G

K_MAX = 1 << 17          # the integer recipe's limit; test_gpu_gemm_kernels.py stays below it (its longest operand, the 2 GiB case, has 245 non-zero rows)


def test_row_groups_are_the_explicit_im2col():
    """rows() with group = Wout, gstride = x_bs, ld = ldx on a channels-last buffer with a gap behind every batch IS the im2col matrix, and
    nt / tn on it are numpy.matmul on that matrix; group == 0 is the plain row-major operand."""
    rs = np.random.RandomState(0)
    B, W, ldx, k, Cout, gap = 3, 9, 8, 4, 5, 12
    Wout, x_bs = W - k + 1, W * ldx + gap
    buf = np.full(B * x_bs, np.nan, np.float32)
    x = G.floats(rs, (B, W, ldx))
    for b in range(B):
        buf[b * x_bs:b * x_bs + W * ldx] = x[b].reshape(-1)
    col = G.im2col(x, B, W, ldx, k)
    got = G.rows(buf, B * Wout, k * ldx, ldx, Wout, x_bs)
    assert got.shape == (B * Wout, k * ldx) and np.array_equal(got, col)
    wp, bias = G.floats(rs, (Cout, k * ldx)), G.floats(rs, Cout)
    assert np.array_equal(G.nt(got, wp, bias), np.matmul(col.astype(np.float64), wp.astype(np.float64).T) + bias.astype(np.float64))
    dz = G.floats(rs, (B * Wout, Cout))
    assert np.array_equal(G.tn(dz, got), np.matmul(dz.astype(np.float64).T, col.astype(np.float64)))
    assert np.array_equal(G.colsum(dz), dz.astype(np.float64).sum(0))
    plain = np.arange(24, dtype=np.float32)
    assert np.array_equal(G.rows(plain, 3, 5, 8), plain.reshape(3, 8)[:, :5])
    assert list(G.row_starts(5, 4, 2, 100)) == [0, 4, 100, 104, 200]


def test_integer_recipe_is_exact_at_the_largest_k():
    """|sum| <= 64 K = 2^23 at K = 2^17: every partial sum is an fp32 integer in any order -- shown for the worst case (all products 64, summed
    sequentially in float32) and for random operands summed by numpy in float32 in K-steps of 32 and of 64."""
    worst = np.cumsum(np.full(K_MAX, 64.0, np.float32), dtype=np.float32)
    assert np.array_equal(worst.astype(np.float64), 64.0 * np.arange(1, K_MAX + 1))
    rs = np.random.RandomState(1)
    A, B = G.ints(rs, (4, K_MAX)), G.ints(rs, (3, K_MAX))
    assert A.min() == -8 and A.max() == 8 and np.array_equal(G.bf16_round(A), A)          # exact in bf16 too
    ref = G.nt(A, B)
    for ke in (32, 64):
        assert np.array_equal(G.nt_f32(A, B, ke).astype(np.float64), ref)
        assert G.nt_rho(A, B, ke) == 0.0
    assert np.array_equal(G.exact_out(ref).astype(np.float64), ref)
    big = np.array([[257.0, -1027.0, 65535.0]])                                           # a bf16 C: rounded once, to nearest even
    assert np.array_equal(G.exact_out(big, c_bf16=True), np.array([[256.0, -1024.0, 65536.0]], np.float32))
    with pytest.raises(AssertionError):
        G.exact_out(np.array([2.0 ** 24 + 1]))


def test_bf16_rounding_and_ulp():
    x = np.array([1.0, 1.00390625, 1.01171875, -3.0, 0.1], np.float32)      # 1 + 2^-8: tie to even (down); 1 + 3 . 2^-8: tie to even (up)
    assert np.array_equal(G.bf16_round(x)[:4], np.array([1.0, 1.0, 1.015625, -3.0], np.float32))
    assert np.array_equal(G.bf16_ulp(np.array([1.0, 1.99, 2.0, -0.75])), np.array([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8]))


def _split_x3(x):
    """split_x3 of csrc/tile_pipe.hpp restated: hi = x truncated to bf16, lo = bf16(x - hi) rounded to nearest even."""
    x = np.asarray(x, np.float32)
    hi = (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    return hi, G.bf16_round(x - hi)


def test_x3_constant_covers_the_emulated_three_product_form():
    """The three products of split_x3, summed in float64 (so that only the dropped terms remain), stay inside X3_C . 2^-16 s_ij -- and use a
    good part of it, i.e. the constant is not slack by an order of magnitude."""
    rs = np.random.RandomState(2)
    A, B = G.floats(rs, (40, 64)), G.floats(rs, (24, 64))
    ah, al = _split_x3(A); bh, bl = _split_x3(B)
    f = lambda a: a.astype(np.float64)
    c3 = f(ah) @ f(bh).T + f(ah) @ f(bl).T + f(al) @ f(bh).T
    per_product = np.abs((f(ah) * f(bh[0]) + f(ah) * f(bl[0]) + f(al) * f(bh[0])) - f(A) * f(B[0])) / np.abs(f(A) * f(B[0]))
    assert per_product.max() <= G.X3_C * 2.0 ** -16 and per_product.max() > 0.2 * G.X3_C * 2.0 ** -16
    ok, worst, _ = G.within(c3, G.nt(A, B), G.X3_C * 2.0 ** -16 * G.nt_scale(A, B))
    assert ok and worst < 1.0


# ---- mutants: each takes the correct pieces and returns a wrong result of the same shape
def _case(kind, act):
    rs = np.random.RandomState(7)
    M = N = 48; K = 96
    gen = G.ints if kind == "int" else (lambda r, s: G.floats(r, s))
    A, B, bias, c0 = gen(rs, (M, K)), gen(rs, (N, K)), gen(rs, N), gen(rs, (M, N))
    return A, B, bias, c0, act


def _correct(A, B, bias, c0, act):
    return G.nt(A, B, bias, act, c0)


def _m_last_k_dropped(A, B, bias, c0, act):
    return G.nt(A[:, :-1], B[:, :-1], bias, act, c0)


def _m_one_term_doubled(A, B, bias, c0, act):
    z = G.nt_pre(A, B, bias)
    i, j = 5, 7
    k = int(np.argmax(np.abs(A[i].astype(np.float64) * B[j])))          # a term that is there (an integer operand may be 0)
    z[i, j] += float(A[i, k]) * float(B[j, k])
    return G.act_fn(z, act) + c0


def _m_subtiles_swapped(A, B, bias, c0, act):
    c = _correct(A, B, bias, c0, act).copy()
    t = c[0:16, 16:32].copy(); c[0:16, 16:32] = c[16:32, 0:16]; c[16:32, 0:16] = t
    return c


def _m_bias_wrong_axis(A, B, bias, c0, act):
    return G.act_fn(G.nt_pre(A, B) + bias.astype(np.float64)[:, None], act) + c0


def _m_act_before_bias(A, B, bias, c0, act):
    return G.act_fn(G.nt_pre(A, B), act) + bias.astype(np.float64)[None, :] + c0


def _m_accumulate_ignored(A, B, bias, c0, act):
    return G.nt(A, B, bias, act)


def _m_pad_column_leaked(A, B, bias, c0, act):
    """K + 1 columns: the pad behind K (3.0 in A, -2.0 in B, the finite pads of the older GEMM tests) joins the sum."""
    Ap = np.concatenate([A, np.full((A.shape[0], 1), 3.0, np.float32)], 1)
    Bp = np.concatenate([B, np.full((B.shape[0], 1), -2.0, np.float32)], 1)
    return G.nt(Ap, Bp, bias, act, c0)


MUTANTS = [_m_last_k_dropped, _m_one_term_doubled, _m_subtiles_swapped, _m_bias_wrong_axis, _m_act_before_bias, _m_accumulate_ignored,
           _m_pad_column_leaked]


_ACT_IDS = {G.ACT_NONE: "none", G.ACT_RELU: "relu", G.ACT_SELU: "selu"}


def _pairs(acts):
    """(mutant, act) pairs; without an activation 'activation before the bias' is the same function, so that pair does not exist."""
    return [pytest.param(m, a, id=f"{m.__name__[3:]}-{_ACT_IDS[a]}") for m in MUTANTS for a in acts
            if not (m is _m_act_before_bias and a == G.ACT_NONE)]


@pytest.mark.parametrize("mutant,act", _pairs([G.ACT_NONE, G.ACT_RELU, G.ACT_SELU]))
def test_float_bound_rejects_mutant(mutant, act):
    A, B, bias, c0, act = _case("float", act)
    for ke in (32, 64):
        ref, bound, rho = G.nt_bound(A, B, ke, bias=bias, act=act, c0=c0)
        assert 0 < rho < 2.0 ** -22, rho
        good32 = (G.act_fn(G.nt_f32(A, B, ke, bias).astype(np.float64), act) + c0).astype(np.float32)      # an honest fp32 result passes
        ok, worst, _ = G.within(good32, ref, bound)
        assert ok and worst < 1.0, worst
        ok, worst, where = G.within(mutant(A, B, bias, c0, act), ref, bound)
        print(f"{mutant.__name__[3:]} act={act} ke={ke}: rho = {rho:.3g}, mutant's worst error = {worst:.3g} bounds at {where}")
        assert not ok and worst > 10.0, worst
    nan = ref.copy(); nan[3, 3] = np.nan                                    # a missing write (the output starts as NaN) is rejected too
    assert not G.within(nan, ref, bound)[0]


@pytest.mark.parametrize("mutant,act", _pairs([G.ACT_NONE, G.ACT_RELU]))
def test_integer_recipe_rejects_mutant_bitwise(mutant, act):
    A, B, bias, c0, act = _case("int", act)
    want = G.exact_out(_correct(A, B, bias, c0, act))
    assert np.array_equal(want, (G.act_fn(G.nt_f32(A, B, 32, bias), act) + c0).astype(np.float32))
    got = mutant(A, B, bias, c0, act).astype(np.float32)
    assert not np.array_equal(got, want)
    # the bf16-C form keeps the difference visible wherever the integer moves by more than an ulp; at least one element does
    assert not np.array_equal(G.bf16_round(got), G.exact_out(_correct(A, B, bias, c0, act), c_bf16=True))


def test_bf16_c_and_x3_bounds_have_the_stated_size():
    rs = np.random.RandomState(3)
    A, B = G.floats(rs, (20, 128), bf16=True), G.floats(rs, (12, 128), bf16=True)
    ref, b, rho = G.nt_bound(A, B, 64)
    _, b16, _ = G.nt_bound(A, B, 64, c_bf16=True)
    _, b3, _ = G.nt_bound(A, B, 64, x3=True)
    assert np.array_equal(b16 - b, G.bf16_ulp(ref)) or np.allclose(b16 - b, G.bf16_ulp(ref), rtol=1e-9, atol=0)
    assert np.allclose(b3 - b, G.X3_C * 2.0 ** -16 * G.nt_scale(A, B), rtol=1e-9, atol=0)
    assert G.within(G.bf16_round(ref.astype(np.float32)), ref, b16)[0]              # the correctly rounded bf16 result passes
    # TN and column sums are the NT machinery on the transposes
    At, Bt = np.ascontiguousarray(A.T), np.ascontiguousarray(B.T)
    rt, bt, _ = G.tn_bound(At, Bt, 64)
    assert np.array_equal(rt, ref) and bt.shape == b.shape and (bt >= 2.0 ** -23 * G.nt_scale(A, B)).all()      # (rho is numpy's order: it may differ)
    rc, bc, _ = G.colsum_bound(At, 64)
    assert np.array_equal(rc, At.astype(np.float64).sum(0)) and bc.shape == (20,) and (bc > 0).all()
