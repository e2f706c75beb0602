"""Reference of the latent k-NN (mvae_latent_knn, ops.latent_knn): a float64 brute force sorted by (d2, row), the checker every output goes
through, the f32 direct-difference emulation the host test runs through that checker, and the inputs the GPU test uses (so that the host
test can run the emulation on every one of them).  numpy only."""
import numpy as np

K_MAX = 32                                   # include/mvae.h: k <= 32
DZ_MAX = 192


def rel_bound(dz):
    """Relative error a f32 sum of dz squares of f32 differences may have against float64, derived: per summand one rounding in the
    difference, which the square doubles, plus one for the square, and at most dz for the sum of non-negative terms -- (dz + 4) * 2^-24
    with room for the final adds."""
    return (dz + 4) * 2.0 ** -24


def dist64(q, t):
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    out = np.empty((q.shape[0], t.shape[0]))
    for i in range(q.shape[0]):              # row by row: no [Q, N, dz] array
        out[i] = ((q[i][None, :] - t) ** 2).sum(1)
    return out


def eligible(d64_row, ex):
    ok = ~np.isnan(d64_row)
    if ex is not None and 0 <= ex < ok.shape[0]:
        ok[ex] = False
    return ok


def knn(q, t, k, exclude=None):
    """(dist float64 [Q, k], idx int64 [Q, k]): the k eligible rows with the smallest (d2, row), ascending; the tail (+inf, -1)."""
    d = dist64(q, t)
    Q, N = d.shape
    dist, idx = np.full((Q, k), np.inf), np.full((Q, k), -1, np.int64)
    for i in range(Q):
        ok = eligible(d[i], None if exclude is None else int(exclude[i]))
        rows = np.nonzero(ok)[0]
        order = rows[np.lexsort((rows, d[i][rows]))][:k]
        dist[i, :order.size], idx[i, :order.size] = d[i][order], order
    return dist, idx


def check(dist, idx, q, t, k, exclude=None):
    """Asserts, per query, what include/mvae.h promises of (dist f32 [Q, k], idx int64 [Q, k]); see the numbered comments."""
    dist, idx = np.asarray(dist), np.asarray(idx)
    q, t = np.asarray(q), np.asarray(t)
    Q, dz = q.shape
    N = t.shape[0]
    assert dist.shape == (Q, k) and idx.shape == (Q, k) and dist.dtype == np.float32 and idx.dtype == np.int64
    rel = rel_bound(dz)
    d64 = dist64(q, t)
    for i in range(Q):
        ex = None if exclude is None else int(exclude[i])
        ok = eligible(d64[i], ex)
        n_el = int(ok.sum())
        n = min(k, n_el)
        got_j, got_d = idx[i], dist[i]
        # 1. indices: distinct rows of the table, -1 only in a tail of exactly k - (eligible rows) entries (its distances +inf), never the
        #    excluded row or a row at a NaN distance
        assert np.all(got_j[n:] == -1) and np.all(got_d[n:] == np.inf), (i, got_j, got_d)
        head = got_j[:n]
        assert np.all((head >= 0) & (head < N)), (i, head)
        assert np.unique(head).size == n, (i, "duplicate row", head)
        assert np.all(ok[head]), (i, "ineligible row returned", head[~ok[head]])
        # 2. each distance is the float64 distance of its row to within the derived bound
        ref = d64[i][head]
        assert np.all(np.abs(got_d[:n].astype(np.float64) - ref) <= rel * ref), (i, got_d[:n], ref)
        # 3. strictly increasing in (distance, row), in the returned f32 values
        for m in range(1, n):
            assert got_d[m - 1] < got_d[m] or (got_d[m - 1] == got_d[m] and head[m - 1] < head[m]), (i, m, got_d[:n], head)
        # 4. nothing nearer was left out
        if n == k:
            left = ok.copy()
            left[head] = False
            if left.any():
                assert d64[i][left].min() >= float(got_d[k - 1]) * (1 - rel), (i, d64[i][left].min(), got_d[k - 1])


def emulate_f32(q, t, k, exclude=None):
    """What a correct kernel may return: f32 differences, f32 squares, an f32 sum (numpy's order), ranked by (d2, row) in those values."""
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    Q, N = q.shape[0], t.shape[0]
    dist, idx = np.full((Q, k), np.inf, np.float32), np.full((Q, k), -1, np.int64)
    for i in range(Q):
        diff = q[i][None, :] - t
        d = (diff * diff).sum(1, dtype=np.float32)
        ok = eligible(d, None if exclude is None else int(exclude[i]))
        rows = np.nonzero(ok)[0]
        order = rows[np.lexsort((rows, d[rows]))][:k]
        dist[i, :order.size], idx[i, :order.size] = d[order], order
    return dist, idx


def expanded_f32(q, t, k):
    """The GEMM form |q|^2 + |t|^2 - 2 q.t in f32: what the kernel must NOT compute."""
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    d = ((q * q).sum(1, dtype=np.float32)[:, None] + (t * t).sum(1, dtype=np.float32)[None, :]) - np.float32(2) * (q @ t.T)
    idx = np.stack([np.lexsort((np.arange(t.shape[0]), d[i]))[:k] for i in range(q.shape[0])])
    return np.take_along_axis(d, idx, 1).astype(np.float32), idx.astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------- inputs
def _clip(x):
    """Magnitudes in [1e-3, 1e3]: no square of a value or of a representable difference underflows or overflows."""
    s = np.where(x < 0, -1.0, 1.0)
    return (s * np.clip(np.abs(x), 1e-3, 1e3)).astype(np.float32)


def random_inputs(Q, N, dz, seed, scale=1.0):
    rs = np.random.RandomState(seed)
    return _clip(rs.standard_normal((Q, dz)) * scale), _clip(rs.standard_normal((N, dz)) * scale)


def clustered_inputs(Q, N, dz, seed, offset, spread):
    """Latents clustered at offset +- spread; the first min(Q, N) // 2 queries ARE table rows (their distance to themselves is 0)."""
    rs = np.random.RandomState(seed)
    t = (offset + spread * rs.standard_normal((N, dz))).astype(np.float32)
    q = (offset + spread * rs.standard_normal((Q, dz))).astype(np.float32)
    n_self = min(Q, N) // 2
    q[:n_self] = t[rs.permutation(N)[:n_self]]
    return q, t


def lattice_inputs(Q=130, N=2000, dz=8, seed=11):
    """Integer latents in [-3, 3] with repeated rows: every f32 sum is exact in any order, so the answer is unique bit for bit."""
    rs = np.random.RandomState(seed)
    base = rs.randint(-3, 4, (N // 4, dz))
    t = base[rs.randint(0, base.shape[0], N)].astype(np.float32)
    q = np.concatenate([t[rs.randint(0, N, Q // 2)], rs.randint(-3, 4, (Q - Q // 2, dz)).astype(np.float32)])
    return q, t


K = K_MAX
# (Q, N, dz, k, kind, with exclude): Q in {1, 2, 63, 64, 65, 257}, N in {1, k - 1, k, k + 1, 255, 256, 257, 4099}, dz in {1, 31, 32, 33, 160,
# 192}, k in {1, 2, 8, K_MAX}.  Dispatcher paths: one slot (N <= 256) / split and merge (N > 256), a lane of the merge owning one list or
# several (N = 20000: 79 slots; N = 65500: 256), whole-row loads (dz a multiple of 32, aligned rows) / the guarded path (other dz; the
# strided test adds dz = 160 with unaligned rows), a short last query tile (Q = 1, 2, 63, 65, 257) / full ones.
CASES = [
    (1, 1, 1, 1, "random", False), (1, 1, 160, K, "random", True), (2, 1, 32, 2, "random", True), (1, 7, 31, 8, "random", False),
    (2, 8, 33, 8, "random", True), (63, 9, 160, 8, "random", False), (64, K - 1, 192, K, "random", True), (65, K, 160, K, "random", False),
    (2, K + 1, 31, K, "random", True), (257, 255, 32, 1, "random", False), (64, 256, 160, 2, "random", True), (65, 257, 33, 8, "random", False),
    (63, 4099, 160, K, "random", True), (1, 4099, 192, 8, "random", False), (2, 4099, 1, 2, "random", False), (257, 4099, 31, 2, "random", True),
    (64, 255, 1, K, "random", False), (1, 256, 33, 1, "random", True), (65, 1, 192, 1, "random", False), (2, 257, 192, K, "random", True),
    (1, 20000, 160, 16, "random", False), (2, 65500, 32, 8, "random", True), (257, 257, 160, 8, "random", False),
    (63, 2, 32, 1, "random", True), (64, 4099, 32, K, "random", False), (1, 1, 33, 2, "random", False),
    (65, 4099, 160, 8, "cluster30", False), (64, 257, 160, K, "cluster30", True), (2, 255, 31, 8, "cluster30", False),
    (65, 4099, 160, 8, "cluster5", False), (63, 256, 192, K, "cluster5", True), (257, 300, 33, 2, "cluster5", False),
]


def case_inputs(case, n):
    """(q, t, exclude) of CASES[n]; random cases take a scale from 1e-2 to 1e2 in turn."""
    Q, N, dz, k, kind, with_ex = case
    if kind == "random":
        q, t = random_inputs(Q, N, dz, 1000 + n, scale=(1e-2, 1.0, 1e2)[n % 3])
    elif kind == "cluster30":
        q, t = clustered_inputs(Q, N, dz, 1000 + n, 30.0, 1e-3)
    else:
        q, t = clustered_inputs(Q, N, dz, 1000 + n, 5.0, 1.0)
    ex = None
    if with_ex:                              # the true nearest row for even queries, none (-1) for the others
        ex = np.full(Q, -1, np.int64)
        near = knn(q, t, 1)[1][:, 0]
        ex[::2] = near[::2]
    return q, t, ex
