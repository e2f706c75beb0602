"""float64 references, input recipes, case lists and per-element error bounds for the optimiser, token-table and loss-head kernels of
csrc/elementwise.hip (mvae_sumsq, mvae_clip_adam, mvae_gather_rows_tb, mvae_scatter_rows_tb, mvae_onehot_tb, mvae_bce_kl_loss_fwd / _bwd,
mvae_softmax_tb_fwd / _bwd): numpy only, no GPU, nothing imported from the package.  test_optim_head_ref_host.py checks this file against
torch in float64, shows that the bounds reject every planted mutant and derives the K constants below; test_gpu_optim_head_kernels.py holds
the kernels to it.

Every reference takes the float32 arrays (bf16 data: as float32) and the float32 scalars the kernel gets and computes in float64.

Inputs
  ints(rs, shape, lo, hi)   small integers: exact in bf16 and fp32, and (the callers keep count * max|x| below 2^24) every partial sum is an
                            exact fp32 integer in any order.  A reduction must then return the float64 sum bit for bit: no tolerance.
  floats(rs, shape, bf16)   standard normals, rounded to the storage type first.

Bounds
  reductions (sumsq partials, scatter cells)   |got - ref| <= RED_BOUND * sum |terms| per output: test_gpu_helper_kernels.py's value, kept.
  math kernels                                 assert_within(got, ref, scale, K): per element |got - ref| <= K * 2^-24 * scale, where scale is
      the size of the terms the element is made of (each function below returns it beside the value) and K is ONE constant per kernel:
      8 x the worst err / (2^-24 * scale) of the float32 numpy restatement of the kernel's own formula (the dt = np.float32 form of the same
      function) against the float64 reference over ALL cases of the GPU test, rounded up to a power of two.  The 8: the kernel may sum in
      another order and uses hardware log2 / rcp / exp of 1 to 2 ulp; a wrong formula misses by orders of magnitude more.
      test_optim_head_ref_host.py recomputes the ratios and asserts K >= 8 x ratio.
  bf16 outputs                                 the float64 result rounded to bf16 (nearest even), one bf16 ulp of it plus the f32 bound.

K constants: value, the CPU ratio it derives from, and the worst ratio the kernels showed on an MI355X (test_gpu_optim_head_kernels.py).
"""
import functools

import numpy as np

U = 2.0 ** -24
CHUNK = 1 << 16                  # SUMSQ_CHUNK: elements per partial sum
RED_BOUND = 2e-6                 # reductions: times the sum of |terms| per output (tests/test_gpu_helper_kernels.py)
FLT_MAX = float(np.finfo(np.float32).max)

K_ADAM = 64.0                    # mvae_clip_adam: p, m, v and the norm.        CPU ratio 6.97    worst on the GPU: 6.35
K_BCE_FWD = 32.0                 # mvae_bce_kl_loss_fwd: out[0..2].             CPU ratio 3.05    worst on the GPU: 2.20
K_BCE_BWD = 64.0                 # mvae_bce_kl_loss_bwd: drecon, dmu, dlogvar.  CPU ratio 4.36    worst on the GPU: 4.36
K_SOFTMAX_BWD = 32.0             # mvae_softmax_tb_bwd (f32): dl and dlT.       CPU ratio 3.09    worst on the GPU: 2.46


def bf16_round(x):
    """x rounded to nearest-even bf16, returned as float32 (finite inputs)."""
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


# ------------------------------------------------------------------------------------------------ comparisons
def ratio(got, ref, scale):
    """Worst |got - ref| / (2^-24 * scale) over the elements; inf for a NaN / inf in got and for a non-zero error where scale is 0."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.broadcast_to(np.asarray(scale, np.float64), ref.shape)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(got - ref)
        r = np.where(scale > 0, d / (U * np.where(scale > 0, scale, 1.0)), np.where(d == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


def assert_within(got, ref, scale, K, what=""):
    """Per element |got - ref| <= K * 2^-24 * scale.  Returns the worst ratio err / (2^-24 * scale)."""
    r = ratio(got, ref, scale)
    assert r <= K, f"{what}: worst err / (2^-24 * scale) = {r:.4g} > K = {K}"
    return r


def assert_within_bf16(got, ref, scale, K, what=""):
    """A bf16 output (given as float32): the float64 result rounded to bf16, one bf16 ulp of it plus the f32 bound."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    want = bf16_round(ref.astype(np.float32)).astype(np.float64)
    bound = bf16_ulp(ref) + K * U * np.broadcast_to(np.asarray(scale, np.float64), ref.shape)
    bad = ~(np.abs(got - want) <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} bf16 elements beyond one ulp + the f32 bound, first at {np.argwhere(bad)[0]}"


def assert_sum_within(got, ref, sumabs, what=""):
    """A reduction of floats: |got - ref| <= RED_BOUND * sum |terms| per output."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bad = ~(np.abs(got - ref) <= RED_BOUND * np.asarray(sumabs, np.float64))
    assert not bad.any(), f"{what}: {int(bad.sum())} sums beyond {RED_BOUND} * sum|x|, first at {np.argwhere(bad)[0]}"


def assert_exact(got, ref, what=""):
    """The integer recipe: the float64 result bit for bit (as a value: the results are integers, -0 does not occur)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.abs(ref).max(initial=0.0) < 2.0 ** 24, "integer result not representable in fp32"
    bad = ~(got == ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} integer results differ, first at {np.argwhere(bad)[0]}"


# ------------------------------------------------------------------------------------------------ mvae_sumsq + mvae_clip_adam
def sumsq_partials(g, dt=np.float64):
    """Per 65536-element chunk, the sum of squares of g (the last chunk may be short).  A square beyond float32's range counts as inf in the
    float64 form too: the kernel forms the squares in float32."""
    x = np.asarray(g).astype(dt).reshape(-1)
    nch = (x.size + CHUNK - 1) // CHUNK
    with np.errstate(over="ignore", invalid="ignore"):
        sq = x * x
        if dt is np.float64:
            sq = np.where(sq > FLT_MAX, np.inf, sq)
        pad = np.zeros(nch * CHUNK, dt)
        pad[:x.size] = sq
        return pad.reshape(nch, CHUNK).sum(1, dtype=dt)


def adam_step(p, g, m, v, grad_scale, max_norm, lr, b1, b2, eps, step, dt=np.float64):
    """One clip_grad_norm_ + Adam step as include/mvae.h states it, in dtype dt: float64 is the reference, float32 the restatement of
    clip_adam_kernel's own operation order.  g may be longer than p: the surplus (the optimiser's poison slot) enters the norm alone.
    Returns a dict: p, m, v, norm, coef, skipped (bool), and the scales sp, sm, sv of the bound."""
    f = dt
    gs, mx, lr, b1, b2, eps = (f(np.float32(x)) for x in (grad_scale, max_norm, lr, b1, b2, eps))
    p, m, v, g = (np.asarray(a).astype(f) for a in (p, m, v, g))      # float32 arrays; a float64 trajectory keeps its own state
    n = p.size
    with np.errstate(over="ignore", invalid="ignore"):
        ss = sumsq_partials(g, dt).sum(dtype=f)
        ss = f(np.inf) if ss > FLT_MAX else ss
        norm = np.sqrt(ss) * gs
    if not np.isfinite(norm):
        z = np.zeros(n)
        return dict(p=p, m=m, v=v, norm=norm, coef=f(np.nan), skipped=True, sp=z, sm=z, sv=z)
    coef = f(1.0)
    if mx > 0:
        coef = min(f(1.0), mx / (norm + f(np.float32(1e-6))))
    bc1 = 1.0 - float(b1) ** step                          # the launcher: in double, handed to the kernel as float
    bc2s = np.sqrt(1.0 - float(b2) ** step)
    if f is np.float32:
        bc1, bc2s = np.float32(bc1), np.float32(bc2s)
    gi = g[:n] * (coef * gs)
    one = f(1.0)
    mi = b1 * m + (one - b1) * gi
    vi = b2 * v + (one - b2) * gi * gi
    denom = np.sqrt(vi) / f(bc2s) + eps
    with np.errstate(invalid="ignore", divide="ignore"):
        upd = (lr / f(bc1)) * (mi / denom)
    pn = p - upd
    a = lambda x: np.abs(np.asarray(x, np.float64))
    return dict(p=pn, m=mi, v=vi, norm=norm, coef=coef, skipped=False, sp=a(p) + a(upd), sm=a(b1 * m) + a((one - b1) * gi),
                sv=a(b2 * v) + a((one - b2) * gi * gi))


def clip_adam_steps(p, gs, m, v, grad_scale, max_norm, lr, b1, b2, eps, step0, dt=np.float64):
    """len(gs) steps from (p, m, v), step numbers step0, step0 + 1, ...  A step whose norm is not finite leaves p, m, v as they are and is
    counted.  Returns one adam_step dict per step, each with `nskipped` = the skipped count after that step."""
    out, k = [], 0
    for i, g in enumerate(gs):
        s = adam_step(p, g, m, v, grad_scale, max_norm, lr, b1, b2, eps, step0 + i, dt)
        k += int(s["skipped"])
        s["nskipped"] = k
        p, m, v = s["p"], s["m"], s["v"]
        out.append(s)
    return out


ADAM_NS = (1, 257, 70001, 4096 * 256 + 257)                # the last wraps the grid-stride loop of grid_for(n, 256, 4096)
ADAM_NORMS = (10.0, 2.0, 8.0, 3.0)                         # against max_norm = 5: the clip binds on steps 1 and 3 only
ADAM_DEFAULT = dict(grad_scale=1.0, max_norm=5.0, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, step0=1)
ADAM_CASES = {                                             # name -> (hyper-parameter overrides, zero fraction of g, element offset)
    "defaults": ({}, 0.0, 0),
    "grad_scale": (dict(grad_scale=0.5), 0.0, 0),
    "no_clip": (dict(max_norm=0.0), 0.0, 0),
    "betas_eps": (dict(b1=0.5, b2=0.9, eps=1e-3), 0.0, 0),
    "late_step": (dict(step0=100000), 0.0, 0),
    "zero_grads": ({}, 0.3, 0),
    "offset4": ({}, 0.0, 1),
}


def adam_hp(case):
    return dict(ADAM_DEFAULT, **ADAM_CASES[case][0])


def adam_inputs(n, case):
    """p, m, v and four different gradients whose norms x grad_scale are about ADAM_NORMS.  Non-zero |g| stay above 1e-6 (no denormal
    term); `zero_grads` mixes exact zeros in.  Every fifth element (n > 1) starts with m = v = 0 and has a gradient of 2e-6 .. 1e-5 on every
    step: sqrt(v_hat) stays near eps = 1e-8's size there, so where eps enters the denominator shows in p."""
    hp, zero_frac = adam_hp(case), ADAM_CASES[case][1]
    rs = np.random.RandomState(1000 + n % 9973 + 7 * sorted(ADAM_CASES).index(case))
    p = (rs.uniform(0.05, 0.15, size=n) * rs.choice([-1.0, 1.0], size=n)).astype(np.float32)      # |p| well above lr * |update|: see sp
    m = (0.01 * rs.standard_normal(n)).astype(np.float32)
    v = (1e-4 * rs.standard_normal(n) ** 2).astype(np.float32)
    tiny = (np.arange(n) % 5 == 0) & (n > 1)
    m[tiny] = v[tiny] = 0.0
    gs = []
    for target in ADAM_NORMS:
        g = rs.standard_normal(n)
        if zero_frac and n > 1:
            g[rs.random_sample(n) < zero_frac] = 0.0
        g = g * (target / hp["grad_scale"] / max(np.sqrt((g * g).sum()), 1e-30))
        small = (g != 0) & (np.abs(g) < 2e-6)
        g[small] = np.where(g[small] < 0, -2e-6, 2e-6)
        g[tiny] = rs.uniform(2e-6, 1e-5, size=int(tiny.sum())) * rs.choice([-1.0, 1.0], size=int(tiny.sum()))
        gs.append(g.astype(np.float32))
    return p, gs, m, v


# ------------------------------------------------------------------------------------------------ token table
def _ids_tb(idx, B, L, nrows):
    """ids of the time-major rows t*B + b out of the batch-major idx [B, L], clamped to [0, nrows)."""
    idx = np.asarray(idx, np.int64).reshape(B, L)
    return np.clip(idx.T.reshape(-1), 0, nrows - 1)


def gather_rows_tb(idx, B, L, nrows, table, base=None):
    """out[t*B + b, :] = table[idx[b, t], :] (+ base[b, :]) as float32: one float32 add, so the kernel must match bit for bit."""
    table = np.asarray(table, np.float32)
    out = table[_ids_tb(idx, B, L, nrows)]
    add = np.tile(np.asarray(base, np.float32), (L, 1)) if base is not None else np.float32(0.0)
    return (out + add).astype(np.float32)


def scatter_rows_tb(idx, B, L, nrows, d, W):
    """(dtable [nrows, W], sum of |terms| per cell): dtable[c, :] = sum over the rows t*B + b with idx[b, t] == c of d[t*B + b, :W]."""
    d = np.asarray(d, np.float32).astype(np.float64)[:B * L, :W]
    ids = _ids_tb(idx, B, L, nrows)
    out, sa = np.zeros((nrows, W)), np.zeros((nrows, W))
    np.add.at(out, ids, d)
    np.add.at(sa, ids, np.abs(d))
    return out, sa


def onehot_tb(idx, B, L, nrows, ld):
    """out[t*B + b, c] = (idx[b, t] == c) for c < ld."""
    out = np.zeros((B * L, ld), np.float32)
    out[np.arange(B * L), _ids_tb(idx, B, L, nrows)] = 1.0
    return out


def token_ids(rs, B, L, V):
    """Batch-major ids with one id that never occurs (V >= 3) and, where there is room, the out-of-range ids -4 and V + 9."""
    never = V // 2 if V >= 3 else -1
    pool = np.array([i for i in range(V) if i != never], np.int64)
    idx = pool[rs.randint(0, pool.size, size=(B, L))]
    flat = idx.reshape(-1)
    if flat.size >= 4:
        flat[flat.size // 3] = -4
        flat[(2 * flat.size) // 3] = V + 9
    return idx, never


# ------------------------------------------------------------------------------------------------ ELBO
LN2_F32 = np.float32(0.693147180559945309)


def _bce_logs(p, dt):
    """max(log p, -100), max(log(1 - p), -100).  float32: fast_log / fast_log1m of elementwise.hip restated (log2 times ln 2; Kahan's log1p)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        if dt is np.float64:
            lp, l1p = np.log(p), np.log1p(-p)
        else:
            one = np.float32(1.0)
            lp = np.log2(p) * LN2_F32
            u = one - p
            d = u - one
            l1p = np.where(d == 0, -p, (np.log2(u) * LN2_F32) * (-p) * (one / np.where(d == 0, one, d)))
    return np.maximum(lp, dt(-100.0)), np.maximum(l1p, dt(-100.0))


def bce_kl_fwd(recon, target, mu, logvar, max_len, dt=np.float64):
    """(out [3], scale [3]): out = [total, xent, kl] with xent = max_len * mean BCE(recon, target) (both logs clamped at -100) and
    kl = -0.5 * mean(1 + mu - logvar^2 - exp(mu)) (mu / logvar swapped, as include/mvae.h says).  scale: the same with every term's parts
    taken as absolute values (sum |terms| / n)."""
    p, t, a, b = (np.asarray(x, np.float32).astype(dt).reshape(-1) for x in (recon, target, mu, logvar))
    ml, one = dt(np.float32(max_len)), dt(1.0)
    lp, l1p = _bce_logs(p, dt)
    terms = t * lp + (one - t) * l1p
    ea = np.exp(a)
    kt = one + a - b * b - ea
    xent = ml * (-terms.sum(dtype=dt) / dt(p.size))
    kl = dt(-0.5) * (kt.sum(dtype=dt) / dt(a.size))
    sx = float(ml) * float(np.abs(terms.astype(np.float64)).sum()) / p.size
    sk = 0.5 * float((1.0 + np.abs(a) + b * b + ea).astype(np.float64).sum()) / a.size
    return np.array([xent + kl, xent, kl], dt), np.array([sx + sk, sx, sk])


def bce_kl_bwd(recon, target, mu, logvar, max_len, grad_out=None, dt=np.float64):
    """drecon = g (max_len / n) (p - t) / max(p (1 - p), 1e-12), dmu = g (-0.5 / m)(1 - exp(mu)), dlogvar = g (0.5 / m) 2 logvar, g = grad_out or 1.
    Returns (drecon, dmu, dlogvar) and their scales (|drecon|, |sl| (1 + exp(mu)), |dlogvar|)."""
    p, t, a, b = (np.asarray(x, np.float32).astype(dt).reshape(-1) for x in (recon, target, mu, logvar))
    g = dt(1.0) if grad_out is None else dt(np.float32(grad_out))
    one = dt(1.0)
    sr = g * dt(np.float32(max_len)) / dt(p.size)
    sl = g * dt(-0.5) / dt(a.size)
    dr = sr * (p - t) / np.maximum((one - p) * p, dt(np.float32(1e-12)))
    ea = np.exp(a)
    dmu = sl * (one - ea)
    dlv = sl * (dt(-2.0) * b)
    ab = lambda x: np.abs(np.asarray(x, np.float64))
    return (dr, dmu, dlv), (ab(dr), abs(float(sl)) * (1.0 + ab(ea)), ab(dlv))


BCE_SHAPES = ((1, 1), (5, 3000), (21, 64), (10500, 18688), (10503, 7), (8 * 1024 * 1024 + 3, 64))    # (n, m); the last: the 1024-block cap
BCE_CLAMP_P = np.array([0.0, 1.0, 1.0, 0.0, 0.5], np.float32)
BCE_CLAMP_T = np.array([1.0, 0.0, 1.0, 0.0, 1.0], np.float32)
BCE_EDGE_P = np.array([0.0, 1e-30, 1e-7, 0.5, 1.0 - 2.0 ** -24, 1.0], np.float32)
MAX_LEN = 120.0


@functools.lru_cache(maxsize=4)
def bce_inputs(n, m, soft):
    """recon in (0, 1), hard (one in ten is 1) or soft targets, mu and logvar."""
    rs = np.random.RandomState(n % 100003 + 31 * m + int(soft))
    recon = rs.uniform(1e-4, 1.0 - 1e-4, size=n).astype(np.float32)
    target = rs.random_sample(n).astype(np.float32) if soft else (rs.random_sample(n) < 0.1).astype(np.float32)
    mu, logvar = (0.5 * rs.standard_normal(m)).astype(np.float32), (0.5 * rs.standard_normal(m)).astype(np.float32)
    for x in (recon, target, mu, logvar):
        x.setflags(write=False)
    return recon, target, mu, logvar


# ------------------------------------------------------------------------------------------------ softmax head
def softmax_fwd(logits, B, L, C):
    """recon [B, L, C] (batch-major) from the time-major logits rows t*B + b (the first C columns)."""
    x = np.asarray(logits, np.float32).astype(np.float64)[:B * L, :C].reshape(L, B, C)
    e = np.exp(x - x.max(2, keepdims=True))
    return (e / e.sum(2, keepdims=True)).transpose(1, 0, 2)


def softmax_bwd(p, dp, dt=np.float64):
    """(dl [L*B, C] time-major, dlT [C, L*B], scale [L*B, C]) from batch-major p, dp [B, L, C]: dl = p (dp - sum_c dp p)."""
    p, dp = (np.asarray(x, np.float32).astype(dt) for x in (p, dp))
    B, L, C = p.shape
    s = (dp * p).sum(2, keepdims=True, dtype=dt)
    dl = (p * (dp - s)).transpose(1, 0, 2).reshape(L * B, C)
    p64, dp64 = np.abs(p.astype(np.float64)), np.abs(dp.astype(np.float64))
    scale = (p64 * (dp64 + (dp64 * p64).sum(2, keepdims=True))).transpose(1, 0, 2).reshape(L * B, C)
    return dl, dl.T.copy(), scale


SOFTMAX_BWD_SHAPES = ((1, 1, 1, 1), (5, 7, 3, 8), (37, 13, 35, 40), (9, 6, 65, 128), (3, 5, 128, 128))    # B, L, C, ldd
SOFTMAX_FWD_SHAPES = ((5, 7, 3), (37, 13, 35))


def softmax_inputs(B, L, C):
    rs = np.random.RandomState(B * 1000 + L * 10 + C)
    p = softmax_fwd(2.0 * rs.standard_normal((L * B, C)), B, L, C).astype(np.float32)
    return p, rs.standard_normal((B, L, C)).astype(np.float32)
