"""CPU tests of the MOSES decoding / scoring surface (mosesvae.VAE.decode, VAE.score, train.moses_reconstruction): the C entry points are
declared, bound and exported at ABI 12, the names are exported by the package, argument checks refuse before anything is launched, and
the float64 reference beam search (tests/beam_ref.py) equals exhaustive enumeration on a tiny random GRU."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import molecular_vae_amd as mv
from molecular_vae_amd import _lib as L, mosesvae as MV, vocab as VC
import beam_ref as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mvae_moses_beam_step", "mvae_moses_beam_finalize", "mvae_ce_rows_fwd")


def test_decode_entry_points_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvae.h")).read(), flags=re.S)
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", header).group(1)) == 12 == L.ABI_VERSION
    lib = L.load()
    assert lib.mvae_abi_version() == 12
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert "moses_reconstruction" in mv.__all__ and mv.moses_reconstruction is mv.train.moses_reconstruction
    assert callable(MV.VAE.decode) and callable(MV.VAE.score)
    from molecular_vae_amd import ops
    assert all(callable(getattr(ops, n)) for n in ("moses_beam_step", "moses_beam_finalize", "ce_rows"))


def test_decode_entry_points_refuse_bad_arguments_before_launching():
    """Everything below returns before any HIP call (no device needed)."""
    lib = L.load()
    fake = ctypes.c_void_p(256)                                  # never dereferenced: every call below is refused first

    def step(K=4, V=30, H=512, dtype=L.MVAE_F32, eos=1, pad=2, W=2048, stp=1, state=fake, table=fake):
        return lib.mvae_moses_beam_step(dtype, 8, K, V, H, 3, state, 0, 0, H + 8, fake, H + 8, None, stp, eos, pad, table, W, fake, fake,
                                        fake, fake, fake, fake, fake, None)
    assert step(K=0) == -1 and step(K=17) == -1 and step(K=5, V=4) == -1          # K outside [1, 16] or K > V
    assert step(V=65, K=1) == -3 and step(V=64, H=1024) == -3                     # V > 64; the head does not fit the LDS
    assert step(state=None) == -1 and step(table=None) == -1 and step(dtype=7) == -1
    assert step(eos=30) == -1 and step(pad=-1) == -1 and step(W=6) == -1 and step(stp=0) == -1
    fin = lambda K=4, max_len=10, ids=fake: lib.mvae_moses_beam_finalize(8, K, max_len, 0, fake, fake, fake, fake, ids, None, None, None)
    assert fin(K=0) == -1 and fin(K=17) == -1 and fin(max_len=0) == -1 and fin(ids=None) == -1
    rows = lambda B=4, V=30, ldl=30, out=fake: lib.mvae_ce_rows_fwd(B, 8, V, fake, ldl, fake, 2, out, None)
    assert rows(B=0) == -1 and rows(ldl=29) == -1 and rows(out=None) == -1


def _cpu_model():
    torch.manual_seed(0)
    return MV.VAE(VC.OneHotVocab(list("abc")), dtype=torch.float32)              # V = 7 (3 symbols + 4 specials)


def test_decode_and_score_refuse_bad_arguments():
    model = _cpu_model()
    V, dz = model.x_emb.num_embeddings, model.d_z
    z = torch.zeros(3, dz)
    for k in (0, 17, V + 1):
        with pytest.raises(ValueError, match="beam_width"):
            model.decode(z, beam_width=k)
    with pytest.raises(ValueError, match="max_len"):
        model.decode(z, max_len=0)
    with pytest.raises(ValueError, match="z must be"):
        model.decode(torch.zeros(3, dz + 1))
    with pytest.raises(ValueError, match="z must be"):
        model.score(["ab", "c", "a"], torch.zeros(3, dz - 1))
    with pytest.raises(L.MvaeError, match="MI355X only"):                       # a CPU model: no fallback
        model.decode(z, beam_width=2)
    with pytest.raises(L.MvaeError, match="MI355X only"):
        model.score(["ab", "c", "a"], z)


def _tiny_params(V, H=8, dz=3, n_layers=2, seed=5):
    rs = np.random.RandomState(seed)
    p = {"x_emb.weight": np.eye(V)}
    for l in range(n_layers):
        p[f"decoder_rnn.weight_ih_l{l}"] = rs.standard_normal((3 * H, V + dz if l == 0 else H))
        p[f"decoder_rnn.weight_hh_l{l}"] = rs.standard_normal((3 * H, H)) * 0.5
        p[f"decoder_rnn.bias_ih_l{l}"] = rs.standard_normal(3 * H) * 0.1
        p[f"decoder_rnn.bias_hh_l{l}"] = rs.standard_normal(3 * H) * 0.1
    p["decoder_lat.weight"] = rs.standard_normal((H, dz)); p["decoder_lat.bias"] = rs.standard_normal(H) * 0.1
    p["decoder_fc.weight"] = rs.standard_normal((V, H)) * 2.0; p["decoder_fc.bias"] = rs.standard_normal(V) * 0.1
    return p, rs.standard_normal(dz)


@pytest.mark.parametrize("seed", [5, 6, 7])
def test_reference_beam_search_equals_exhaustive_enumeration(seed):
    """V = 4, max_len = 4, K = V^3: the beam keeps every hypothesis, so it must return every sequence the decoder can emit (tokens after
    an <eos> are pad), sorted by its summed log-probability, with the reference's end rule -- and -inf for the beams left over."""
    V, max_len, bos, eos, pad = 4, 4, 0, 1, 2
    K = V ** 3
    p, z = _tiny_params(V, seed=seed)
    ids, ends, scores, _ = BR.beam_search(p, z, K, max_len, bos, eos, pad, n_layers=2)
    want = []
    for toks in itertools.product(range(V), repeat=max_len - 1):
        seq = [bos]
        for t in toks:
            seq.append(t)
            if t == eos:
                break
        if len(seq) < max_len and seq[-1] != eos:
            continue
        if tuple(seq) in {tuple(w[1]) for w in want}:
            continue
        lp, _, _ = BR.teacher_forced(p, z, seq, n_layers=2)
        want.append((float(lp.sum()), seq))
    want.sort(key=lambda w: -w[0])
    n = len(want)
    assert n == 1 + 3 + 9 + 27                                    # <eos> first at step 1, 2, 3, or never
    assert np.isfinite(scores[:n]).all() and np.isneginf(scores[n:]).all()
    for k, (s, seq) in enumerate(want):
        assert abs(scores[k] - s) < 1e-10, k
        assert ends[k] == len(seq) and list(ids[k, :ends[k]]) == seq and (ids[k, ends[k]:] == pad).all(), k
    assert (np.diff(scores[:n]) <= 0).all()


def test_reference_greedy_is_the_argmax_chain():
    """K = 1: the reference beam search is greedy decoding (each token the arg-max of its teacher-forced log p)."""
    V, max_len, bos, eos, pad = 6, 8, 0, 1, 2
    p, z = _tiny_params(V, seed=11)
    ids, ends, scores, _ = BR.beam_search(p, z, 1, max_len, bos, eos, pad, n_layers=2)
    seq = list(ids[0, :ends[0]])
    lp, best, _ = BR.teacher_forced(p, z, seq, n_layers=2)
    assert list(best) == seq[1:] and abs(lp.sum() - scores[0]) < 1e-12
