"""CPU tests of the Levenshtein reference and checker (tests/edit_ref.py) and of the host surface of mvae_edit_distance_rows / mvae_edit_knn:
the reference agrees with an independent pure-Python DP and with known values, a CPU emulation of the kernels' bit-vector recurrence passes
the checker on every input the GPU tests use, the checker refuses eight wrong kernels, and the new entry points are declared, bound, exported
and refuse bad arguments before anything is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from molecular_vae_amd import _lib as L, data as D, mosesvae as MV, ops, train as TR, vocab as VC
import edit_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dp(a, b, V=ER.V):
    """An independent full-table DP, written apart from edit_ref.lev."""
    m, n = len(a), len(b)
    D_ = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(m + 1):
        for j in range(n + 1):
            if i == 0 or j == 0:
                D_[i][j] = i + j
            else:
                eq = int(a[i - 1]) == int(b[j - 1]) and 0 <= int(a[i - 1]) < V
                D_[i][j] = min(D_[i - 1][j] + 1, D_[i][j - 1] + 1, D_[i - 1][j - 1] + (not eq))
    return D_[m][n]


def _ids(s):
    return np.array([ord(c) - ord("a") for c in s], np.int64)


def test_reference_known_values_and_metric_properties():
    V = 26
    assert ER.lev(_ids("kitten"), _ids("sitting"), V) == 3 and ER.lev(_ids("flaw"), _ids("lawn"), V) == 2
    assert ER.lev(_ids("ab"), _ids("ba"), V) == 2                               # no transposition
    rs = np.random.RandomState(0)
    for n in (0, 1, 7, 70):
        s = rs.choice(ER.ALPHABET, n)
        assert ER.lev([], s) == n and ER.lev(s, []) == n and ER.lev(s, s) == 0
    assert ER.lev([77, 4], [77, 4]) == 1 and ER.lev([-1], [-1]) == 1            # ids outside [0, V) equal nothing
    strings = [rs.choice(ER.ALPHABET, rs.randint(0, 25)) for _ in range(12)]
    strings += [ER.mutate(strings[i], 2, rs) for i in range(6)]
    d = np.array([[ER.lev(a, b) for b in strings] for a in strings])
    assert np.array_equal(d, d.T) and (np.diag(d) == 0).all()
    lens = np.array([len(s) for s in strings])
    assert (d >= np.abs(lens[:, None] - lens[None, :])).all() and (d <= np.maximum(lens[:, None], lens[None, :])).all()
    assert (d[:, None, :] <= d[:, :, None] + d[None, :, :]).all()               # triangle inequality on every triple


def test_reference_forms_agree_with_an_independent_dp_on_random_pairs():
    rs = np.random.RandomState(1)
    for _ in range(60):
        a = rs.choice(ER.ALPHABET, rs.randint(0, 131))[:ER.PATTERN_MAX]
        b = ER.mutate(a, rs.randint(6), rs) if rs.rand() < 0.5 else rs.choice(ER.ALPHABET, rs.randint(0, 90))
        if rs.rand() < 0.3 and len(a) and len(b):
            a, b = a.copy(), b.copy()
            a[rs.randint(len(a))] = (-2, ER.V, 200)[rs.randint(3)]
            b[rs.randint(len(b))] = (-2, ER.V, 200)[rs.randint(3)]
        want = _dp(a, b)
        texts, lens = ER.pad_rows([b])
        assert ER.lev(a, b) == want and ER.lev_block(a, texts, lens)[0] == want and ER.bitvector_block(a, texts, lens)[0] == want, (a, b)
    corpus = ER.seeds_corpus(40, 3)
    q = ER.queries_for(corpus, 5, 4)
    dist, idx = ER.knn(q, corpus, 8, exclude=np.array([0, -1, 3, -1, -1]))
    for i in range(5):
        d = np.array([_dp(q[i], r) for r in corpus])
        ok = np.ones(40, bool)
        if i in (0, 2):
            ok[(0, -1, 3)[i]] = False
        rows = np.nonzero(ok)[0]
        order = rows[np.lexsort((rows, d[rows]))][:8]
        assert np.array_equal(idx[i], order) and np.array_equal(dist[i], d[order])
    dist, idx = ER.knn(q[:2], corpus[:3], 5, exclude=np.array([1, -1]))       # fewer rows than k, one excluded: the tail
    assert (idx[0, 2:] == -1).all() and (dist[0, 2:] == ER.NONE).all() and 1 not in idx[0] and (idx[1, 3:] == -1).all()


@pytest.mark.parametrize("n", range(len(ER.CASES)))
def test_bit_vector_recurrence_passes_the_checker_on_every_gpu_input(n):
    corpus, queries, x, ex, ref = ER.case_inputs(n)
    Q, N, k, _ = ER.CASES[n]
    assert all(np.array_equal(ER.content(x[i]), queries[i]) for i in range(Q))
    if Q >= 3:
        assert ({0, 64, 65, 128} if Q >= 4 else {64, 65, 128}) <= {len(q) for q in queries}
    ER.check(*ER.bitvector_knn(queries, corpus, k, ex), queries, corpus, k, ex, ref=ref)


def test_bit_vector_recurrence_passes_on_the_rows_and_ties_inputs():
    a, b, ref = ER.rows_inputs()
    assert 250 <= a.shape[0] <= 350
    got = []
    for i in range(a.shape[0]):
        texts, lens = ER.pad_rows([ER.content(b[i])])
        got.append(ER.bitvector_block(ER.content(a[i]), texts, lens)[0])
    assert np.array_equal(np.array(got, np.int32), ref)
    for i in range(0, a.shape[0], 7):                                           # the vectorised reference against the independent DP
        assert ref[i] == _dp(ER.content(a[i]), ER.content(b[i]))
    lens_a = {len(ER.content(r)) for r in a}
    lens_b = {len(ER.content(r)) for r in b}
    assert set(ER.ROWS_PATTERN_LENS) <= lens_a and set(ER.ROWS_TEXT_LENS) <= lens_b
    corpus, queries, x, src = ER.ties_inputs()
    ER.check(*ER.bitvector_knn(queries, corpus, 8), queries, corpus, 8)


def _refused(dist, idx, queries, corpus, k, exclude=None):
    with pytest.raises(AssertionError):
        ER.check(dist, idx, queries, corpus, k, exclude)


def _hamming(p, r):
    n = min(len(p), len(r))
    return int(sum(int(p[i]) != int(r[i]) or not 0 <= int(p[i]) < ER.V for i in range(n))) + abs(len(p) - len(r))


def _indel(p, r):
    m, n = len(p), len(r)
    Lc = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(m):
        for j in range(n):
            Lc[i + 1][j + 1] = Lc[i][j] + 1 if int(p[i]) == int(r[j]) and 0 <= int(p[i]) < ER.V else max(Lc[i][j + 1], Lc[i + 1][j])
    return m + n - 2 * Lc[m][n]


def _osa(p, r):
    m, n = len(p), len(r)
    D_ = [[i + j if i == 0 or j == 0 else 0 for j in range(n + 1)] for i in range(m + 1)]
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            D_[i][j] = min(D_[i - 1][j] + 1, D_[i][j - 1] + 1, D_[i - 1][j - 1] + (int(p[i - 1]) != int(r[j - 1])))
            if i > 1 and j > 1 and int(p[i - 1]) == int(r[j - 2]) and int(p[i - 2]) == int(r[j - 1]):
                D_[i][j] = min(D_[i][j], D_[i - 2][j - 2] + 1)
    return D_[m][n]


@pytest.mark.parametrize("wrong", [_hamming, _indel, _osa], ids=["hamming_plus_length", "indel_only", "transposition_as_one_edit"])
def test_checker_refuses_another_distance(wrong):
    corpus = ER.seeds_corpus(150, 21, n_seeds=4, lo=8, hi=14, extras=False)
    rs = np.random.RandomState(22)
    queries = [ER.mutate(corpus[rs.randint(150)], rs.randint(1, 4), rs) for _ in range(8)]
    k = 5
    ER.check(*ER.bitvector_knn(queries, corpus, k), queries, corpus, k)
    _refused(*ER.knn(queries, corpus, k, dist_fn=wrong), queries, corpus, k)


def test_checker_refuses_five_more_wrong_kernels():
    # the pattern cut at 64 tokens (a dropped carry): a case whose batch holds contents of 65 and 128 tokens
    n = 3
    corpus, queries, x, ex, ref = ER.case_inputs(n)
    k = ER.CASES[n][2]
    texts, lens = ER.pad_rows(corpus)
    d = np.stack([ER.bitvector_block(p, texts, lens, cut_at_64=True) for p in queries])
    rows = np.arange(len(corpus))
    cut_d, cut_j = np.full((len(queries), k), ER.NONE, np.int32), np.full((len(queries), k), -1, np.int64)
    for i in range(len(queries)):
        order = rows[np.lexsort((rows, d[i]))][:k]
        cut_d[i, :order.size], cut_j[i, :order.size] = d[i][order], order
    _refused(cut_d, cut_j, queries, corpus, k)
    # content that runs past the <eos>
    past = [np.asarray(x[i, 1:])[:ER.PATTERN_MAX] for i in range(len(queries))]
    _refused(*ER.knn(past, corpus, k), queries, corpus, k)
    # exclude ignored
    assert ex is not None
    _refused(*ER.knn(queries, corpus, k), queries, corpus, k, exclude=ex)
    # out-of-range ids that equal each other: the query IS a corpus row holding a byte >= V, whose true distance to it is 1, not 0
    n = 8
    corpus, queries, x, ex, ref = ER.case_inputs(n)
    k = ER.CASES[n][2]
    row = next(i for i, r in enumerate(corpus) if len(r) and len(r) <= 64 and (np.asarray(r) >= ER.V).any())
    q2 = [np.asarray(corpus[row], np.int64)] + list(queries[1:4])
    good = ER.knn(q2, corpus, k)
    assert good[0][0, 0] >= 1
    ER.check(*good, q2, corpus, k)
    _refused(*ER.knn(q2, corpus, k, dist_fn=lambda p, r: ER.lev(p, r, V=1 << 62)), q2, corpus, k)
    # ties by the higher row, on the corpus with exact duplicates
    corpus, queries, x, src = ER.ties_inputs()
    ref_d, ref_j = ER.knn(queries[:12], corpus, 4)
    assert (ref_d[:, 0] == 0).all() and (ref_d[:, 1] == 0).all()
    _refused(*ER.knn(queries[:12], corpus, 4, higher_row_first=True), queries[:12], corpus, 4)


# ---------------------------------------------------------------------------------------------------------------------- host surface
def test_edit_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "mvae.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.load()
    for name in ("mvae_edit_distance_rows", "mvae_edit_knn_workspace", "mvae_edit_knn"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define\s+MVAE_EDIT_NONE\s+2147483647\b", header) and re.search(r"#define\s+MVAE_EDIT_PATTERN_MAX\s+128\b", header)
    assert re.search(r"#define\s+MVAE_ABI_VERSION\s+12\b", header)
    assert (ops.EDIT_NONE, ops.EDIT_PATTERN_MAX, ops.EDIT_K_MAX, ops.EDIT_V_MAX) == (ER.NONE, ER.PATTERN_MAX, ER.K_MAX, 64)
    assert callable(ops.edit_distance_rows) and callable(ops.edit_knn) and callable(MV.VAE.edit_distance)
    assert callable(D.MosesDeviceDataset.nearest_strings)
    build = open(os.path.join(ROOT, "molecular-vae_amd", "csrc", "build.sh")).read()
    assert build.count("elementwise edit_distance latent_knn corpus_index conv latent capi; do") == 2
    assert "build/edit_distance.o" in build and "build/tune/edit_distance.o" in build
    usage = os.path.join(ROOT, "molecular-vae_amd", "csrc", "build", "edit_distance.usage.txt")
    if os.path.exists(usage):                                                    # written by the build: no kernel of the file uses scratch
        sizes = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", open(usage).read())
        assert len(sizes) >= 3 and set(sizes) == {"0"}, sizes


def test_edit_entries_refuse_bad_arguments_before_launching_and_plan_by_shape():
    """Everything below returns before any HIP call (no device needed)."""
    lib = L.load()
    fake = ctypes.c_void_p(256)                               # never dereferenced: every call below is refused first

    def rows(B=4, V=30, eos=2, a=fake, a_ld=100, Ta=100, b=fake, b_ld=300, Tb=300, dist=fake):
        return lib.mvae_edit_distance_rows(B, V, eos, a, a_ld, Ta, b, b_ld, Tb, dist, None)
    assert rows(B=0) == -1 and rows(Ta=0, a_ld=0) == -1 and rows(Tb=0) == -1 and rows(a_ld=99) == -1 and rows(b_ld=299) == -1
    assert rows(a=None) == -1 and rows(b=None) == -1 and rows(dist=None) == -1
    assert rows(eos=-1) == -1 and rows(eos=65536) == -1 and rows(V=0) == -1 and rows(V=65) == -1
    assert rows(Ta=130, a_ld=130) == -3 and rows(Ta=1000, a_ld=1000) == -3

    def knn(Q=1, T=100, V=30, eos=2, x=fake, x_ld=100, tokens=fake, offsets=fake, N=20000, k=16, dist=fake, idx=fake, ws=None, nb=0):
        return lib.mvae_edit_knn(Q, T, V, eos, x, x_ld, tokens, offsets, N, k, None, dist, idx, ws, nb, None)
    assert knn(Q=0) == -1 and knn(N=0) == -1 and knn(k=0) == -1 and knn(T=0) == -1 and knn(x_ld=99) == -1
    assert knn(x=None) == -1 and knn(tokens=None) == -1 and knn(offsets=None) == -1 and knn(dist=None) == -1 and knn(idx=None) == -1
    assert knn(eos=-1) == -1 and knn(eos=65536) == -1 and knn(V=0) == -1 and knn(V=65) == -1
    assert knn(k=ER.K_MAX + 1) == -3 and knn(T=130, x_ld=130) == -3
    need = lib.mvae_edit_knn_workspace(1, 20000, 16)
    assert need > 0 and need % (16 * 12) == 0 and 2 <= need // (16 * 12) <= 256       # slots * Q * k * 12 bytes
    assert knn() == -2 and knn(ws=fake, nb=need - 1) == -2 and knn(ws=ctypes.c_void_p(260), nb=need) == -1
    # the workspace depends on (Q, N, k) alone -- the signature has nothing else -- and is O(Q k slots), never Q x N
    for Q in (1, 64, 1024, 4096):
        nb = lib.mvae_edit_knn_workspace(Q, 1_600_000, 32)
        assert 0 < nb <= 256 * Q * 32 * 12 and nb <= 64 << 20, (Q, nb)
        assert nb == lib.mvae_edit_knn_workspace(Q, 1_600_000, 32)
    assert lib.mvae_edit_knn_workspace(64, 256, 32) == 0 and lib.mvae_edit_knn_workspace(1, 1, 1) == 0
    assert lib.mvae_edit_knn_workspace(3, 257, 5) > 0
    assert lib.mvae_edit_knn_workspace(0, 10, 1) == 0 and lib.mvae_edit_knn_workspace(1, 300, 33) == 0 and lib.mvae_edit_knn_workspace(1, 0, 1) == 0


def test_python_surface_raises_before_device_work():
    vocab = VC.OneHotVocab(list("abc"))
    ds = D.MosesDeviceDataset(["ab", "c", "abc"], vocab, device="cpu")
    for k in (0, 33, 1.5):
        with pytest.raises(ValueError, match="k must be"):
            ds.nearest_strings(["ab"], k=k)
    with pytest.raises(ValueError, match="columns"):
        ds.nearest_strings(["a" * 128])                                           # bos + 128 + eos = 130 columns
    with pytest.raises(ValueError, match="columns"):
        ds.nearest_strings(torch.zeros(2, 130, dtype=torch.long))
    with pytest.raises(ValueError, match="at least one"):
        ds.nearest_strings([])
    big = VC.OneHotVocab([chr(ord("0") + i) for i in range(70)])
    assert len(big) > 64
    with pytest.raises(ValueError, match="at most 64"):
        D.MosesDeviceDataset(["01", "2"], big, device="cpu").nearest_strings(["01"])
    torch.manual_seed(0)
    model = MV.VAE(vocab, dtype=torch.float32)
    with pytest.raises(ValueError, match="rows against"):
        model.edit_distance(["ab", "c"], ["ab"])
    with pytest.raises(ValueError, match="columns"):
        model.edit_distance(torch.zeros(2, 130, dtype=torch.long), torch.zeros(2, 131, dtype=torch.long))
    with pytest.raises(ValueError, match="at least one"):
        model.edit_distance([], [])
    with pytest.raises(ValueError, match="at most 64"):
        MV.VAE(big, dtype=torch.float32).edit_distance(["01"], ["2"])
    with pytest.raises(ValueError, match="columns"):
        ops.edit_distance_rows(torch.zeros(2, 130, dtype=torch.long), torch.zeros(2, 140, dtype=torch.long), 2, 12)
    with pytest.raises(ValueError, match="needs novel_against"):
        TR.moses_generate(model, 4, nearest=True)
    with pytest.raises(ValueError, match="max_len"):
        TR.moses_generate(model, 4, max_len=131, novel_against=ds, nearest=True)
    # lookup's messages are what they were
    with pytest.raises(ValueError, match="lookup: needs at least one row"):
        ds.lookup([])
    with pytest.raises(ValueError, match=r"lookup: x must be \[B, T\]"):
        ds.lookup(torch.zeros(3, dtype=torch.long))
