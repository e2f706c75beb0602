"""GPU tests of mvae_edit_distance_rows / mvae_edit_knn (ops.edit_distance_rows / ops.edit_knn) against the numpy reference of
tests/edit_ref.py, with exact equality: the pair kernel at the word boundaries of the bit-vector recurrence, the search at its edge shapes
through both dispatcher paths, the tie rule on a corpus with exact duplicates, independence of the batch, determinism, write coverage and the
error codes."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from molecular_vae_amd import _lib as L, ops    # noqa: E402
import edit_ref as ER                           # noqa: E402

dev = torch.device("cuda")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _corpus(rows):
    """The CSR on the device, the token buffer exactly as long as the corpus: the last row ends at the last byte."""
    tokens, offsets = ER.csr(rows)
    if tokens.size == 0:
        tokens = np.zeros(1, np.uint8)           # a pointer to pass; no byte of it belongs to a row
    return _t(tokens), _t(offsets)


def _knn(x, rows, k, ex=None, **kw):
    tokens, offsets = _corpus(rows)
    dist, idx = ops.edit_knn(_t(x), tokens, offsets, len(rows), k, ER.EOS, ER.V, exclude=None if ex is None else _t(ex), **kw)
    return dist.cpu().numpy(), idx.cpu().numpy()


def test_rows_at_the_word_boundaries_with_strides_and_guards():
    a, b, ref = ER.rows_inputs()
    B, Ta, Tb = a.shape[0], a.shape[1], b.shape[1]
    lib = L.load()
    big = 2 ** 40 + 3                            # what stands in the padding of the leading dimensions: never loaded, never compared
    ap = torch.full((B, Ta + 5), big, dtype=torch.long, device=dev)
    bp = torch.full((B, Tb + 3), big, dtype=torch.long, device=dev)
    ap[:, :Ta], bp[:, :Tb] = _t(a), _t(b)
    guard = 4
    dist = torch.full((B + guard,), -7, dtype=torch.int32, device=dev)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.mvae_edit_distance_rows(B, ER.V, ER.EOS, p(ap), Ta + 5, Ta, p(bp), Tb + 3, Tb, p(dist), st) == 0
    got = dist.cpu().numpy()
    print("rows: pairs", B, "mismatches", int((got[:B] != ref).sum()))
    assert (got[B:] == -7).all()
    assert np.array_equal(got[:B], ref), np.nonzero(got[:B] != ref)[0][:10]
    # a pattern side of 130 columns is refused and nothing runs; the wrapper puts the narrower tensor there and agrees
    wide = torch.zeros((B, 130), dtype=torch.long, device=dev)
    assert lib.mvae_edit_distance_rows(B, ER.V, ER.EOS, p(wide), 130, 130, p(bp), Tb + 3, Tb, p(dist), st) == -3
    torch.cuda.synchronize()
    assert np.array_equal(dist.cpu().numpy(), got)
    assert np.array_equal(ops.edit_distance_rows(ap[:, :Ta], bp[:, :Tb], ER.EOS, ER.V).cpu().numpy(), ref)
    assert np.array_equal(ops.edit_distance_rows(bp[:, :Tb], ap[:, :Ta], ER.EOS, ER.V).cpu().numpy(), ref)
    with pytest.raises(ValueError):
        ops.edit_distance_rows(bp[:, :Tb], bp[:, :Tb], ER.EOS, ER.V)
    # a row without <eos> runs to T - 1: the same pairs cut to narrower tensors
    cut = np.array([lev for lev in (ER.lev(ER.content(a[i, :40]), ER.content(b[i, :70])) for i in range(0, B, 9))], np.int32)
    assert np.array_equal(ops.edit_distance_rows(ap[::9, :40], bp[::9, :70], ER.EOS, ER.V).cpu().numpy(), cut)
    one = ops.edit_distance_rows(ap[:5, :1], bp[:5, :Tb], ER.EOS, ER.V).cpu().numpy()       # T = 1: the empty content
    assert np.array_equal(one, [len(ER.content(b[i])) for i in range(5)])


@pytest.mark.parametrize("n", range(len(ER.CASES)))
def test_knn_edge_shapes_match_the_reference(n):
    Q, N, k, _ = ER.CASES[n]
    corpus, queries, x, ex, ref = ER.case_inputs(n)
    need = L.load().mvae_edit_knn_workspace(Q, N, k)
    assert (need > 0) == (N > 256)               # more than one workgroup of corpus rows: the split-and-merge path runs
    dist, idx = _knn(x, corpus, k, ex)
    ER.check(dist, idx, queries, corpus, k, ex, ref=ref)


def test_ties_and_duplicates_rank_by_the_lower_row():
    corpus, queries, x, src = ER.ties_inputs()
    N, k = len(corpus), 8
    ref = ER.knn(queries, corpus, k)
    dist, idx = _knn(x, corpus, k)
    assert np.array_equal(idx, ref[1]) and np.array_equal(dist, ref[0])
    copies = [[j for j, r in enumerate(corpus) if np.array_equal(r, corpus[i])] for i in src]      # every row with the query's content
    first, second = np.array([c[0] for c in copies]), np.array([c[1] for c in copies])
    assert all(len(c) >= 2 for c in copies) and (first != src).any()
    assert (dist[:40, :2] == 0).all() and np.array_equal(idx[:40, 0], first) and np.array_equal(idx[:40, 1], second)
    ex = np.full(len(queries), -1, np.int64)
    ex[:40] = first
    dist, idx = _knn(x, corpus, k, ex)
    ER.check(dist, idx, queries, corpus, k, ex)
    assert (dist[:40, 0] == 0).all() and np.array_equal(idx[:40, 0], second) and not (idx[:40] == first[:, None]).any()


def test_a_query_does_not_depend_on_its_batch_and_runs_are_equal():
    n = 8                                         # Q = 65, N = 1000
    Q, N, k, _ = ER.CASES[n]
    corpus, queries, x, ex, ref = ER.case_inputs(n)
    tokens, offsets = _corpus(corpus)
    xt = _t(x)
    guard = 3
    dist = torch.full((Q + guard, k), -7, dtype=torch.int32, device=dev)
    idx = torch.full((Q + guard, k), -7, dtype=torch.long, device=dev)
    ops.edit_knn(xt, tokens, offsets, N, k, ER.EOS, ER.V, dist=dist[:Q], idx=idx[:Q])
    assert (dist[Q:] == -7).all() and (idx[Q:] == -7).all()
    d2, j2 = ops.edit_knn(xt, tokens, offsets, N, k, ER.EOS, ER.V)
    assert torch.equal(dist[:Q], d2) and torch.equal(idx[:Q], j2)
    for i in (0, 31, 32, 64):                     # alone: another query tile, another split of the corpus
        d1, j1 = ops.edit_knn(xt[i:i + 1], tokens, offsets, N, k, ER.EOS, ER.V)
        assert torch.equal(d1[0], dist[i]) and torch.equal(j1[0], idx[i]), i
    d3, j3 = ops.edit_knn(xt[:, :ER.T_MAX], tokens[:int(offsets[300])], offsets[:301], 300, k, ER.EOS, ER.V)      # a prefix of the corpus
    ER.check(d3.cpu().numpy(), j3.cpu().numpy(), queries, corpus[:300], k)


def test_error_codes_come_back_without_a_launch():
    lib = L.load()
    corpus, queries, x, ex, ref = ER.case_inputs(6)                                    # Q = 1, N = 257: needs a workspace
    tokens, offsets = _corpus(corpus)
    xt = _t(np.concatenate([x, np.zeros((1, 1), np.int64)], 1))                         # 130 columns to offer
    dist = torch.full((1, 5), -7, dtype=torch.int32, device=dev)
    idx = torch.full((1, 5), -7, dtype=torch.long, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(Q=1, T=129, V=ER.V, eos=ER.EOS, ld=130, N=257, k=5, ws=None, nb=0):
        return lib.mvae_edit_knn(Q, T, V, eos, p(xt), ld, p(tokens), p(offsets), N, k, None, p(dist), p(idx), ws, nb, st)
    assert call(T=130) == -3 and call(k=33) == -3
    assert call(Q=0) == -1 and call(N=0) == -1 and call(k=0) == -1 and call(T=0) == -1 and call(ld=128) == -1 and call(V=65) == -1 and call(eos=-1) == -1
    need = lib.mvae_edit_knn_workspace(1, 257, 5)
    assert need > 0 and call() == -2
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    assert call(ws=p(ws), nb=need - 1) == -2
    torch.cuda.synchronize()
    assert (dist == -7).all() and (idx == -7).all()                                     # nothing ran
    assert call(ws=p(ws), nb=need) == 0
    torch.cuda.synchronize()
    ER.check(dist.cpu().numpy(), idx.cpu().numpy(), queries, corpus, 5)
