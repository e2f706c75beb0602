"""CPU tests of the latent k-NN's reference and checker (tests/knn_ref.py) and of its host surface: the float64 brute force agrees with torch,
a f32 direct-difference emulation passes the checker on every input the GPU test uses, the checker refuses seven wrong kernels, and the new
entry points are declared, bound, exported and refuse bad arguments before anything is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import molecular_vae_amd as mv
from molecular_vae_amd import _lib as L, data as D, mosesvae as MV, ops
import knn_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_agrees_with_torch_cdist_and_sort():
    for n, (Q, N, dz, k) in enumerate(((5, 300, 160, 8), (3, 40, 1, 4), (7, 33, 33, 32))):
        q, t = KR.random_inputs(Q, N, dz, 50 + n)
        dist, idx = KR.knn(q, t, k)
        d = torch.cdist(torch.from_numpy(q).double(), torch.from_numpy(t).double()) ** 2
        order = torch.argsort(d, dim=1, stable=True)[:, :k]
        assert np.array_equal(idx, order.numpy())
        assert np.allclose(dist, torch.gather(d, 1, order).numpy(), rtol=1e-12, atol=0)
    q, t = KR.random_inputs(2, 5, 4, 9)                       # fewer rows than k, one excluded: the tail
    dist, idx = KR.knn(q, t, 8, exclude=np.array([3, -1]))
    assert (idx[0, 4:] == -1).all() and (idx[1, 5:] == -1).all() and 3 not in idx[0] and np.isinf(dist[0, 4:]).all()
    assert sorted(idx[1, :5].tolist()) == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("n", range(len(KR.CASES)))
def test_f32_direct_difference_passes_the_checker_on_every_gpu_input(n):
    case = KR.CASES[n]
    q, t, ex = KR.case_inputs(case, n)
    assert 1e-3 <= np.abs(q).min() and np.abs(q).max() <= 1e3 and 1e-3 <= np.abs(t).min() and np.abs(t).max() <= 1e3
    dist, idx = KR.emulate_f32(q, t, case[3], ex)
    KR.check(dist, idx, q, t, case[3], ex)


def test_f32_direct_difference_is_exact_on_the_lattice():
    q, t = KR.lattice_inputs()
    dist, idx = KR.emulate_f32(q, t, KR.K_MAX)
    ref_d, ref_j = KR.knn(q, t, KR.K_MAX)
    assert np.array_equal(idx, ref_j) and np.array_equal(dist.astype(np.float64), ref_d)
    assert (np.diff(ref_d, axis=1) == 0).any(), "the lattice must produce ties"
    KR.check(dist, idx, q, t, KR.K_MAX)


def _refused(dist, idx, q, t, k, exclude=None):
    with pytest.raises(AssertionError):
        KR.check(dist, idx, q, t, k, exclude)


def test_checker_refuses_ties_broken_towards_the_higher_row():
    q, t = KR.lattice_inputs()
    k = KR.K_MAX
    d = KR.dist64(q, t).astype(np.float32)
    rows = np.arange(t.shape[0])
    idx = np.stack([np.lexsort((-rows, d[i]))[:k] for i in range(q.shape[0])]).astype(np.int64)
    _refused(np.take_along_axis(d, idx, 1), idx, q, t, k)


def test_checker_refuses_five_more_wrong_kernels():
    q, t = KR.random_inputs(9, 300, 33, 77)
    k = 8
    dist, idx = KR.emulate_f32(q, t, k + 1)
    KR.check(dist[:, :k].copy(), idx[:, :k].copy(), q, t, k)
    # the k-th neighbour replaced by the (k + 1)-th
    _refused(np.delete(dist, k - 1, 1), np.delete(idx, k - 1, 1), q, t, k)
    # unsorted output
    d2, j2 = dist[:, :k].copy(), idx[:, :k].copy()
    d2[:, [2, 5]], j2[:, [2, 5]] = d2[:, [5, 2]], j2[:, [5, 2]]
    _refused(d2, j2, q, t, k)
    # a duplicated index
    d2, j2 = dist[:, :k].copy(), idx[:, :k].copy()
    d2[:, 1], j2[:, 1] = d2[:, 0], j2[:, 0]
    _refused(d2, j2, q, t, k)
    # the excluded row returned
    _refused(dist[:, :k].copy(), idx[:, :k].copy(), q, t, k, exclude=idx[:, 0].copy())
    # a row at a NaN distance returned: row 5 holds a NaN, the wrong kernel ranks it as if the NaN were the query's own value
    t_nan = t.copy()
    t_nan[5, 7] = np.nan
    t_fill = t.copy()
    t_fill[5] = q[0]
    t_fill[5, 7] = q[0, 7]
    d2, j2 = KR.emulate_f32(q, t_fill, k)
    assert 5 in j2[0]
    _refused(d2, j2, q, t_nan, k)
    d3, j3 = KR.emulate_f32(q, t_nan, k)                      # the right answer on that table passes
    assert not (j3 == 5).any()
    KR.check(d3, j3, q, t_nan, k)


@pytest.mark.parametrize("offset,spread", [(30.0, 1e-3), (5.0, 1.0)])
def test_checker_refuses_the_norm_expansion_on_clustered_latents(offset, spread):
    q, t = KR.clustered_inputs(65, 4099, 160, 5, offset, spread)
    k = 8
    KR.check(*KR.emulate_f32(q, t, k), q, t, k)
    _refused(*KR.expanded_f32(q, t, k), q, t, k)


# ---------------------------------------------------------------------------------------------------------------------- host surface
def test_knn_entry_points_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvae.h")).read(), flags=re.S)
    lib = L.load()
    for name in ("mvae_latent_knn", "mvae_latent_knn_workspace"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert callable(ops.latent_knn) and callable(MV.VAE.encode)
    assert "MosesLatentIndex" in mv.__all__ and mv.MosesLatentIndex is D.MosesLatentIndex
    assert callable(D.MosesDeviceDataset.encode_latents) and callable(D.MosesDeviceDataset.smiles)
    assert callable(D.MosesLatentIndex.search) and callable(D.MosesLatentIndex.neighbors)
    build = open(os.path.join(ROOT, "molecular-vae_amd", "csrc", "build.sh")).read()
    assert build.count("latent_knn corpus_index conv latent capi; do") == 2
    assert "build/latent_knn.o" in build and "build/tune/latent_knn.o" in build


def test_knn_refuses_bad_arguments_before_launching_and_plans_by_shape():
    """Everything below returns before any HIP call (no device needed)."""
    lib = L.load()
    fake = ctypes.c_void_p(256)                               # never dereferenced: every call below is refused first

    def knn(Q=1, N=20000, dz=160, k=16, q=fake, ldq=160, t=fake, ldt=160, dist=fake, idx=fake, ws=None, nb=0):
        return lib.mvae_latent_knn(Q, N, dz, k, q, ldq, t, ldt, None, dist, idx, ws, nb, None)
    assert knn(Q=0) == -1 and knn(N=0) == -1 and knn(k=0) == -1 and knn(dz=0) == -1 and knn(ldq=159) == -1 and knn(ldt=159) == -1
    assert knn(q=None) == -1 and knn(t=None) == -1 and knn(dist=None) == -1 and knn(idx=None) == -1
    assert knn(dz=KR.DZ_MAX + 1, ldq=200, ldt=200) == -3 and knn(k=KR.K_MAX + 1) == -3
    need = lib.mvae_latent_knn_workspace(1, 20000, 160, 16)
    assert need > 0 and need % (16 * 12) == 0 and 2 <= need // (16 * 12) <= 256       # slots * Q * k * 12 bytes
    assert knn() == -2 and knn(ws=fake, nb=need - 1) == -2 and knn(ws=ctypes.c_void_p(260), nb=need) == -1
    # the workspace is O(Q k slots) at the target shapes, never Q x N
    for Q in (1, 64, 1024, 4096):
        nb = lib.mvae_latent_knn_workspace(Q, 1_600_000, 160, 32)
        assert 0 < nb <= 256 * Q * 32 * 12 and nb <= 64 << 20, (Q, nb)
    assert lib.mvae_latent_knn_workspace(64, 256, 160, 32) == 0 and lib.mvae_latent_knn_workspace(1, 1, 1, 1) == 0
    assert lib.mvae_latent_knn_workspace(0, 10, 4, 1) == 0 and lib.mvae_latent_knn_workspace(1, 300, 193, 1) == 0


def test_latent_index_refuses_a_foreign_vocabulary_and_a_bad_table():
    from molecular_vae_amd import vocab as VC
    vocab = VC.OneHotVocab(list("abc"))
    ds = D.MosesDeviceDataset(["ab", "c", "abc"], vocab, device="cpu")
    torch.manual_seed(0)
    other = MV.VAE(VC.OneHotVocab(list("abd")), dtype=torch.float32)
    with pytest.raises(ValueError, match="another vocabulary"):
        ds.encode_latents(other)
    with pytest.raises(ValueError, match="batch_size"):
        ds.encode_latents(MV.VAE(vocab, dtype=torch.float32), batch_size=0)
    with pytest.raises(ValueError, match="mu must be"):
        D.MosesLatentIndex(torch.zeros(2, 4), ds)
    index = D.MosesLatentIndex(torch.zeros(3, 4), ds)
    with pytest.raises(ValueError, match="z must be"):
        index.search(torch.zeros(2, 5), 1)
    with pytest.raises(ValueError, match="another vocabulary"):
        index.neighbors(["ab"], 1, other)
    assert ds.smiles([2, 0, -1, 1]) == ["abc", "ab", None, "c"] and ds.smiles(np.array([[1], [2]])) == ["c", "abc"]
    with pytest.raises(ValueError, match="outside"):
        ds.smiles([3])
