"""CPU tests of syntax-constrained decoding (mvae_moses_beam_syntax_step, VAE.decode(syntax=True), moses_reconstruction(syntax=True)): the
entry point is declared, bound and exported at ABI 12 and refuses bad arguments before anything is launched; the Python surface refuses
max_len < 3 on a CPU model; the float64 reference of tests/beam_syntax_ref.py is beam_ref.beam_search when the constraint is off, and
with it on every finite hypothesis is accepted by the independently written validator of tests/syntax_ref.py and ends in <eos>."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import molecular_vae_amd as mv
from molecular_vae_amd import _lib as L, mosesvae as MV, vocab as VC, ops
from oracle import initparams as ip
import beam_ref as BR
import beam_syntax_ref as BS
import syntax_ref as SY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mvae_moses_beam_syntax_step"
ALPHABET = "CNOSFcnos()=#123[]@H+-lBr"          # data.synthetic_smiles' alphabet: V = 29 with the four specials
N_ATOMS = 10                                     # C N O S F c n o s B


def _vocab():
    return VC.OneHotVocab(set(ALPHABET))


_CACHE = {}


def _params():
    if "p" not in _CACHE:
        params = ip.init_params(ip.moses_shapes(len(_vocab())), 303, 1.5, np.float32)
        _CACHE["p"] = {k: p.astype(np.float64) for k, p in params.items()}
    return _CACHE["p"]


def _latents(B, seed, scale):
    rs = np.random.RandomState(seed)
    return (rs.standard_normal((B, 160)) * scale).astype(np.float32).astype(np.float64)


def test_entry_is_declared_bound_and_exported_at_abi_12():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvae.h")).read(), flags=re.S)
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", header).group(1)) == 12 == L.ABI_VERSION
    lib = L.load()
    assert lib.mvae_abi_version() == 12
    assert re.search(r"\b" + NAME + r"\s*\(", header)
    assert NAME in L.SIGNATURES and hasattr(lib, NAME)
    assert len(L.SIGNATURES[NAME][1]) == len(L.SIGNATURES["mvae_moses_beam_step"][1]) + 3          # tok_info, gstate, max_len
    assert L.SIGNATURES[NAME][1][:-4] == L.SIGNATURES["mvae_moses_beam_step"][1][:-1]
    assert callable(ops.moses_beam_syntax_step)


def test_entry_refuses_bad_arguments_before_launching():
    """Everything below returns before any HIP call (no device needed)."""
    lib = L.load()
    fake = ctypes.c_void_p(256)                                  # never dereferenced: every call below is refused first

    def step(K=4, V=30, H=512, dtype=L.MVAE_F32, eos=1, pad=2, W=2048, stp=1, state=fake, table=fake, tok=fake, gs=fake, max_len=10):
        return getattr(lib, NAME)(dtype, 8, K, V, H, 3, state, 0, 0, H + 8, fake, H + 8, None, stp, eos, pad, table, W, fake, fake, fake, fake,
                                  fake, fake, fake, tok, gs, max_len, None)
    # what mvae_moses_beam_step refuses, with its codes
    assert step(K=0) == -1 and step(K=17) == -1 and step(K=5, V=4) == -1
    assert step(V=65, K=1) == -3 and step(V=64, H=1024) == -3
    assert step(state=None) == -1 and step(table=None) == -1 and step(dtype=7) == -1
    assert step(eos=30) == -1 and step(pad=-1) == -1 and step(W=6) == -1 and step(stp=0) == -1
    # and its own
    assert step(tok=None) == -1 and step(gs=None) == -1
    assert step(max_len=2) == -1 and step(max_len=0) == -1
    assert step(stp=-1) == -1 and step(stp=10) == -1 and step(stp=11) == -1
    assert step(eos=-1) == -1


def test_decode_refuses_bad_syntax_arguments_and_has_no_cpu_fallback():
    torch.manual_seed(0)
    model = MV.VAE(VC.OneHotVocab(list("CNO(=)1")), dtype=torch.float32)
    z = torch.zeros(2, model.d_z)
    for n in (2, 1):
        with pytest.raises(ValueError, match="max_len >= 3"):
            model.decode(z, syntax=True, max_len=n)
        with pytest.raises(ValueError, match="max_len >= 3"):
            model._beam_search(z, 2, n, syntax=True)
    with pytest.raises(ValueError, match="max_len >= 3"):
        mv.moses_reconstruction(model, [[model.string2tensor("CO", device="cpu")]], max_len=2, syntax=True)
    with pytest.raises(L.MvaeError, match="MI355X only"):                            # a CPU model: no fallback
        model.decode(z, syntax=True, max_len=3)
    no_atoms = MV.VAE(VC.OneHotVocab(list("xyz")), dtype=torch.float32)
    with pytest.raises(ValueError, match="no atom token"):
        no_atoms.decode(torch.zeros(2, no_atoms.d_z), syntax=True, max_len=8)


@pytest.mark.parametrize("K,max_len", [(1, 9), (3, 7), (4, 2)])
def test_reference_without_the_constraint_is_the_plain_reference(K, max_len):
    v, p = _vocab(), _params()
    for z in _latents(2, seed=2, scale=0.7):
        a = BS.beam_search(p, z, K, max_len, v, syntax=False)
        b = BR.beam_search(p, z, K, max_len, v.bos, v.eos, v.pad)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


@pytest.mark.parametrize("K", [1, 4, 16])
@pytest.mark.parametrize("max_len", [3, 5, 20])
def test_reference_hypotheses_are_well_formed_and_end_in_eos(K, max_len):
    """Every finite hypothesis of the float64 reference passes the independent validator and ends in <eos> with pad after it; beam 0 is
    always finite; scores are sorted with -inf last; at K = 16, max_len = 3 exactly the alphabet's 10 atoms give a hypothesis."""
    v, p = _vocab(), _params()
    for z in _latents(3, seed=2, scale=0.7):
        ids, ends, scores, _ = BS.beam_search(p, z, K, max_len, v)
        assert np.isfinite(scores[0])
        s = np.where(np.isfinite(scores), scores, -1e300)
        assert (np.diff(s) <= 0).all()
        for k in range(K):
            if not np.isfinite(scores[k]):
                continue
            assert SY.row_valid(ids[k], v), (k, ids[k])
            assert 3 <= ends[k] <= max_len and ids[k, ends[k] - 1] == v.eos and (ids[k, ends[k]:] == v.pad).all()
        if K == 16 and max_len == 3:
            assert np.isfinite(scores).sum() == N_ATOMS
