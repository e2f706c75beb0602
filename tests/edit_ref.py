"""Reference of the token-level Levenshtein kernels (mvae_edit_distance_rows, mvae_edit_knn; ops.edit_distance_rows / ops.edit_knn): the
plain three-term dynamic program, a pairs-vectorised form of it for the search, the brute-force k-NN sorted by (distance, row), the checker
every output goes through (integers: exact equality), a CPU emulation of the kernels' bit-vector recurrence (one and two 64-bit words) that
the host test runs through that checker, and the inputs the GPU tests use (so that the host test can run the emulation on every one of
them).  numpy only."""
import functools

import numpy as np

K_MAX = 32                                   # include/mvae.h: k <= 32
PATTERN_MAX = 128                            # MVAE_EDIT_PATTERN_MAX
NONE = 2147483647                            # MVAE_EDIT_NONE
PAD, BOS, EOS = 0, 1, 2                      # the specials of the test vocabulary; V ids in all
V = 12
ALPHABET = np.arange(4, 10)                  # six ordinary tokens, so that distances are not just lengths
T_MAX = PATTERN_MAX + 1                      # the widest query tensor


# ---------------------------------------------------------------------------------------------------------------------- the distance
def content(row, eos=EOS):
    """row[1:] up to, and not including, the first `eos`; to the last column without one.  Column 0 never takes part."""
    r = np.asarray(row).reshape(-1)[1:]
    hit = np.nonzero(r == eos)[0]
    return r[:hit[0]] if hit.size else r


def lev(a, b, V=V):
    """Plain Levenshtein distance by the three-term DP; tokens are equal iff they are the same id inside [0, V)."""
    a, b = [int(t) for t in a], [int(t) for t in b]
    prev = list(range(len(b) + 1))
    for i, p in enumerate(a, 1):
        cur = [i] + [0] * len(b)
        for j, t in enumerate(b, 1):
            same = p == t and 0 <= p < V
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (0 if same else 1))
        prev = cur
    return prev[len(b)]


def pad_rows(rows, dtype=np.int64, fill=-1):
    lens = np.array([len(r) for r in rows], np.int64)
    out = np.full((len(rows), max(int(lens.max()) if len(rows) else 0, 1)), fill, dtype)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out, lens


def lev_block(p, texts, lens, V=V):
    """One pattern against a padded [P, n] block of texts (row i holds lens[i] tokens), one numpy step per pattern token: the row of the
    DP table is x[j] = min(up + 1, diagonal + mismatch) followed by the horizontal term D[j] = min_{j' <= j} (x[j'] + j - j'), which is
    minimum.accumulate(x - j) + j.  Returns int64 [P]."""
    texts = np.asarray(texts, np.int64)
    P, n = texts.shape
    j = np.arange(n + 1, dtype=np.int64)
    D = np.broadcast_to(j, (P, n + 1)).copy()
    for i, tok in enumerate(p, 1):
        tok = int(tok)
        x = np.empty_like(D)
        x[:, 0] = i
        miss = np.ones((P, n), np.int64) if not 0 <= tok < V else (texts != tok).astype(np.int64)
        np.minimum(D[:, 1:] + 1, D[:, :-1] + miss, out=x[:, 1:])
        D = np.minimum.accumulate(x - j, axis=1) + j
    return D[np.arange(P), np.asarray(lens, np.int64)]


def distances(p, corpus, V=V):
    """The distance from pattern p to every corpus row (a list of 1-D arrays): int64 [N].  Short and long rows go through lev_block apart,
    so that a few long rows do not widen the block of the many short ones."""
    lens = np.array([len(r) for r in corpus], np.int64)
    out = np.empty(len(corpus), np.int64)
    for sel in (np.nonzero(lens <= 72)[0], np.nonzero(lens > 72)[0]):
        if sel.size:
            texts, ln = pad_rows([corpus[i] for i in sel])
            out[sel] = lev_block(p, texts, ln, V)
    return out


def knn(queries, corpus, k, exclude=None, V=V, dist_fn=None, higher_row_first=False):
    """(dist int32 [Q, k], idx int64 [Q, k]) for query CONTENTS (a list of 1-D arrays): the k eligible rows with the smallest
    (distance, row), ascending; the tail (NONE, -1).  dist_fn / higher_row_first: the wrong kernels of the host test."""
    Q, N = len(queries), len(corpus)
    dist, idx = np.full((Q, k), NONE, np.int32), np.full((Q, k), -1, np.int64)
    for i, p in enumerate(queries):
        d = distances(p, corpus, V) if dist_fn is None else np.array([dist_fn(p, r) for r in corpus], np.int64)
        ok = np.ones(N, bool)
        if exclude is not None and 0 <= int(exclude[i]) < N:
            ok[int(exclude[i])] = False
        rows = np.nonzero(ok)[0]
        order = rows[np.lexsort((-rows if higher_row_first else rows, d[rows]))][:k]
        dist[i, :order.size], idx[i, :order.size] = d[order], order
    return dist, idx


def check(dist, idx, queries, corpus, k, exclude=None, V=V, ref=None):
    """Asserts what include/mvae.h promises of (dist int32 [Q, k], idx int64 [Q, k]): exactly the reference, tail included."""
    dist, idx = np.asarray(dist), np.asarray(idx)
    Q, N = len(queries), len(corpus)
    assert dist.shape == (Q, k) and idx.shape == (Q, k) and dist.dtype == np.int32 and idx.dtype == np.int64, (dist.shape, dist.dtype, idx.dtype)
    ref_d, ref_j = knn(queries, corpus, k, exclude, V) if ref is None else ref
    for i in range(Q):
        n = min(k, N - (1 if exclude is not None and 0 <= int(exclude[i]) < N else 0))
        assert np.all(idx[i, n:] == -1) and np.all(dist[i, n:] == NONE), (i, "tail", idx[i], dist[i])
        assert np.all((idx[i, :n] >= 0) & (idx[i, :n] < N)), (i, idx[i])
        assert np.array_equal(idx[i], ref_j[i]), (i, "rows", idx[i], ref_j[i], dist[i], ref_d[i])
        assert np.array_equal(dist[i], ref_d[i]), (i, "distances", dist[i], ref_d[i])


# ---------------------------------------------------------------------------------------------------------------------- the kernels' recurrence
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
ONE, ZERO, TOP = np.uint64(1), np.uint64(0), np.uint64(1 << 63)


def _block(Eq, hin, Pv, Mv):
    """One text token in one 64-row block for a vector of texts (csrc/edit_distance.hip: ed_block).  hin int64 [P] in {-1, 0, 1}."""
    neg, pos = (hin < 0).astype(np.uint64), (hin > 0).astype(np.uint64)
    Xv = Eq | Mv
    Eq = Eq | neg
    Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq
    Ph = Mv | ~(Xh | Pv)
    Mh = Pv & Xh
    Phs, Mhs = (Ph << ONE) | pos, (Mh << ONE) | neg
    return Mhs | ~(Xv | Phs), Phs & Xv, Ph, Mh


def _delta(Ph, Mh, bit):
    return ((Ph & bit) != 0).astype(np.int64) - ((Mh & bit) != 0).astype(np.int64)


def bitvector_block(p, texts, lens, V=V, cut_at_64=False):
    """lev_block by the bit-vector recurrence of the kernels: match vectors of the pattern in one (m <= 64) or two 64-bit words, the
    horizontal delta leaving word 0 at its top bit entering word 1.  cut_at_64: the wrong kernel that drops word 1."""
    p = [int(t) for t in p]
    m = len(p)
    texts, lens = np.asarray(texts, np.int64), np.asarray(lens, np.int64)
    P, n = texts.shape
    if m == 0:
        return lens.copy()
    peq = np.zeros((V + 1, 2), np.uint64)                      # row V: a token that equals nothing
    for i, tok in enumerate(p):
        if 0 <= tok < V:
            peq[tok, i >> 6] |= np.uint64(1 << (i & 63))
    if cut_at_64 and m > 64:
        m = 64
    two = m > 64
    bit = np.uint64(1 << ((m - 1) & 63))
    tt = np.where((texts >= 0) & (texts < V), texts, V)
    Pv0 = np.full(P, M64); Mv0 = np.zeros(P, np.uint64)
    Pv1 = np.full(P, M64); Mv1 = np.zeros(P, np.uint64)
    score = np.full(P, m, np.int64)
    plus = np.ones(P, np.int64)
    for j in range(int(lens.max()) if P else 0):
        Pv0, Mv0, Ph, Mh = _block(peq[tt[:, j], 0], plus, Pv0, Mv0)
        if two:
            Pv1, Mv1, Ph, Mh = _block(peq[tt[:, j], 1], _delta(Ph, Mh, TOP), Pv1, Mv1)
        score += np.where(j < lens, _delta(Ph, Mh, bit), 0)
    return score


def bitvector_knn(queries, corpus, k, exclude=None, V=V):
    """What a correct kernel returns: the bit-vector distances ranked by (distance, row)."""
    Q, N = len(queries), len(corpus)
    texts, lens = pad_rows(corpus)
    dist, idx = np.full((Q, k), NONE, np.int32), np.full((Q, k), -1, np.int64)
    for i, p in enumerate(queries):
        d = bitvector_block(p, texts, lens, V)
        ok = np.ones(N, bool)
        if exclude is not None and 0 <= int(exclude[i]) < N:
            ok[int(exclude[i])] = False
        rows = np.nonzero(ok)[0]
        order = rows[np.lexsort((rows, d[rows]))][:k]
        dist[i, :order.size], idx[i, :order.size] = d[order], order
    return dist, idx


# ---------------------------------------------------------------------------------------------------------------------- inputs
def mutate(s, n_edits, rs):
    s = list(s)
    for _ in range(n_edits):
        op = rs.randint(4)
        if op == 0 and s:
            s[rs.randint(len(s))] = int(rs.choice(ALPHABET))
        elif op == 1 and s:
            del s[rs.randint(len(s))]
        elif op == 2 and len(s) > 1:                           # a transposition: two edits for Levenshtein
            i = rs.randint(len(s) - 1)
            s[i], s[i + 1] = s[i + 1], s[i]
        else:
            s.insert(rs.randint(len(s) + 1), int(rs.choice(ALPHABET)))
    return np.array(s, np.int64)


def seeds_corpus(N, seed, n_seeds=5, lo=12, hi=40, extras=True):
    """A "mutated seeds" corpus: a few seed strings over six tokens, each copied many times with 0 to 4 random edits -- neighbours are
    close, ties are frequent, exact duplicates exist.  extras: empty rows, rows of 150 to 300 tokens and tokens >= V among them."""
    rs = np.random.RandomState(seed)
    seeds = [rs.choice(ALPHABET, rs.randint(lo, hi + 1)) for _ in range(n_seeds)]
    rows = [mutate(seeds[rs.randint(n_seeds)], rs.randint(5), rs) for _ in range(N)]
    if extras:
        for i in range(N):
            u = rs.rand()
            if u < 0.03:
                rows[i] = np.zeros(0, np.int64)
            elif u < 0.06:
                rows[i] = rs.choice(ALPHABET, rs.randint(150, 301))
            elif u < 0.12 and len(rows[i]):
                rows[i] = rows[i].copy()
                rows[i][rs.randint(len(rows[i]))] = (V, 200, 255, 63)[rs.randint(4)]
    return rows


def csr(rows):
    """(tokens uint8 [total], offsets int64 [N + 1]): the last row ends at the last byte of the buffer."""
    offsets = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=offsets[1:])
    tokens = np.concatenate([np.asarray(r, np.uint8) for r in rows]) if offsets[-1] else np.zeros(0, np.uint8)
    return tokens, offsets


def query_tensor(contents, T, seed=0, garbage=True):
    """int64 [Q, T]: <bos>, the content, <eos> where there is room, then garbage far outside int32 (or <pad>); the bos column itself holds
    garbage in every other row -- its value does not matter."""
    rs = np.random.RandomState(seed)
    x = np.full((len(contents), T), PAD, np.int64)
    for i, c in enumerate(contents):
        assert len(c) <= T - 1, (len(c), T)
        if garbage:
            x[i] = rs.randint(-2 ** 40, 2 ** 40, T)
            x[i, ::3] = rs.choice(ALPHABET, x[i, ::3].shape[0])            # ordinary tokens and stray <eos> behind the end as well
            x[i, 5::7] = EOS
        x[i, 0] = BOS if i % 2 == 0 else -7
        x[i, 1:1 + len(c)] = c
        if 1 + len(c) < T:
            x[i, 1 + len(c)] = EOS
    return x


def queries_for(corpus, Q, seed):
    """Q query contents: corpus rows with 0 to 3 edits (every fourth an exact copy), and -- from Q = 3 on -- contents of length (0,) 64, 65
    and 128 in the same batch (the empty one from Q = 4 on), one token of a long one outside [0, V)."""
    rs = np.random.RandomState(seed)
    short = [i for i, r in enumerate(corpus) if len(r) <= PATTERN_MAX] or [None]
    out = []
    for i in range(Q):
        src = short[rs.randint(len(short))]
        base = np.zeros(0, np.int64) if src is None else np.asarray(corpus[src], np.int64)
        out.append(base.copy() if i % 4 == 0 else mutate(base, rs.randint(4), rs)[:PATTERN_MAX])
    if Q >= 3:
        for slot, n in zip(rs.permutation(Q)[:4], (0, 64, 65, 128) if Q >= 4 else (64, 65, 128)):
            c = rs.choice(ALPHABET, n).astype(np.int64)
            if n == 65:
                c[40] = -3
            if n == 128:
                c[100] = 2 ** 35 + 4
            out[slot] = c
    return out


# (Q, N, k, with exclude): Q in {1, 3, 64, 65}, N in {1, 63, 64, 65, 256, 257, 1000, 5000}, k in {1, 5, 32}; k > N exercises the tail; N <= 256 is
# one slot (no workspace), N > 256 splits the corpus and runs the merge launch; the largest case has Q = 16.
CASES = [
    (1, 1, 1, False), (3, 1, 5, True), (3, 63, 5, False), (64, 64, 32, True), (65, 65, 1, False), (3, 256, 32, False), (1, 257, 5, False),
    (64, 257, 1, True), (65, 1000, 5, False), (3, 1000, 32, True), (1, 5000, 32, False), (16, 5000, 5, True), (65, 5, 32, False),
]


@functools.lru_cache(maxsize=None)
def case_inputs(n):
    """(corpus rows, query contents, x int64 [Q, 129], exclude or None, reference (dist, idx)) of CASES[n]; computed once per process."""
    Q, N, k, with_ex = CASES[n]
    corpus = seeds_corpus(N, 100 + n)
    queries = queries_for(corpus, Q, 200 + n)
    x = query_tensor(queries, T_MAX, 300 + n)
    ex = None
    if with_ex:                              # the true nearest row for even queries, none (-1) for the others
        ex = np.full(Q, -1, np.int64)
        ex[::2] = knn(queries, corpus, 1)[1][::2, 0]
    return corpus, queries, x, ex, knn(queries, corpus, k, ex)


@functools.lru_cache(maxsize=None)
def ties_inputs(N=600, Q=65, seed=7):
    """The mutated-seeds corpus without extras, each of its first 40 rows copied again further down (exact duplicates), and queries of
    which the first 40 ARE those rows: (corpus, queries, x, the rows the first 40 queries were taken from)."""
    corpus = seeds_corpus(N, seed, extras=False)
    for i in range(40):
        corpus[N // 2 + i] = corpus[i].copy()
    rs = np.random.RandomState(seed + 1)
    src = np.concatenate([np.arange(20), N // 2 + np.arange(20, 40)])
    queries = [corpus[i].copy() for i in src] + [mutate(corpus[rs.randint(N)], rs.randint(1, 4), rs) for _ in range(Q - 40)]
    return corpus, queries, query_tensor(queries, 60, seed), src


# ---------------------------------------------------------------------------------------------------------------------- the rows test
ROWS_PATTERN_LENS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 66, 100, 127, 128)
ROWS_TEXT_LENS = (0, 1, 63, 64, 65, 128, 129, 200, 300)


@functools.lru_cache(maxsize=None)
def rows_inputs(seed=5):
    """About 300 pairs for mvae_edit_distance_rows: (a int64 [B, 129], b int64 [B, 302], reference int32 [B]).  Every pattern length
    crossed with every text length, twice (a random text, and a text derived from the pattern by a few edits, so that the distance is not
    just the length difference); equal strings; one-edit neighbours at the first, the 64th, the 65th and the last position; rows without
    <eos> that run to T - 1 on either side; <eos> in column 1; garbage behind the <eos> with ids far outside int32; ids >= V and negative
    ids inside the content on each side."""
    rs = np.random.RandomState(seed)
    Ta, Tb = T_MAX, 302
    pa, pb = [], []
    for m in ROWS_PATTERN_LENS:
        for n in ROWS_TEXT_LENS:
            p = rs.choice(ALPHABET, m).astype(np.int64)
            pa.append(p); pb.append(rs.choice(ALPHABET, n).astype(np.int64))
            t = mutate(p, rs.randint(1, 6), rs)                # the pattern with a few edits, cut or filled up to n tokens
            pa.append(p); pb.append(np.concatenate([t, rs.choice(ALPHABET, max(n - len(t), 0))])[:n].astype(np.int64))
    for m in (1, 64, 65, 100, 128):                            # equal strings and one-edit neighbours
        p = rs.choice(ALPHABET, m).astype(np.int64)
        pa.append(p); pb.append(p.copy())
        for pos in (0, 63, 64, m - 1):
            if pos < m:
                t = p.copy(); t[pos] = 4 + (t[pos] - 4 + 1) % 6
                pa.append(p); pb.append(t)
                pa.append(p); pb.append(np.delete(p, pos))
                pa.append(p); pb.append(np.insert(p, pos, 9))
    for m, n in ((40, 45), (70, 60), (128, 300), (10, 10)):    # ids outside [0, V) inside the content, on each side and on both
        p = rs.choice(ALPHABET, m).astype(np.int64)
        t = mutate(p, 2, rs)
        t = np.concatenate([t, rs.choice(ALPHABET, max(n - len(t), 0))])
        p2, t2 = p.copy(), t.copy()
        p2[m // 2] = -5; p2[m - 1] = V
        t2[len(t) // 2] = 2 ** 33 + 5; t2[0] = -1
        pa += [p2, p, p2]; pb += [t, t2, t2]
        same = p.copy(); same[3] = 77                          # equal ids outside the vocabulary still differ
        pa.append(same); pb.append(same.copy())
    a = query_tensor(pa, Ta, seed + 1)
    b = query_tensor(pb, Tb, seed + 2)
    ref = np.array([lev_block(content(a[i]), content(b[i])[None, :] if len(content(b[i])) else np.zeros((1, 1), np.int64),
                              [len(content(b[i]))])[0] for i in range(len(pa))], np.int32)
    assert all(np.array_equal(content(a[i]), pa[i]) and np.array_equal(content(b[i]), pb[i]) for i in range(len(pa)))
    return a, b, ref
