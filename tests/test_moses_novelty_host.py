"""CPU tests of the corpus index surface (mvae_corpus_index_build / mvae_corpus_index_probe, MosesDeviceDataset.lookup / contains /
n_distinct, moses_generate(novel_against=)): the entries are declared, bound and exported at ABI 12 and refuse bad arguments before
anything is launched; the reference tests/novelty_ref.py equals plain ``in`` on a set of strings; and moses_generate refuses a wrong
``novel_against`` before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import molecular_vae_amd as mv
from molecular_vae_amd import _lib as L, data as D, mosesvae as MV, vocab as VC, ops
import novelty_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD, PROBE = "mvae_corpus_index_build", "mvae_corpus_index_probe"


def test_entries_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvae.h")).read(), flags=re.S)
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", header).group(1)) == 12 == L.ABI_VERSION
    lib = L.load()
    assert lib.mvae_abi_version() == 12
    for name, nargs in ((BUILD, 7), (PROBE, 12)):
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl and decl.group(1).count(",") + 1 == nargs, name
        assert name in L.SIGNATURES and hasattr(lib, name), name
        assert len(L.SIGNATURES[name][1]) == nargs, name
    assert callable(ops.corpus_index_build) and callable(ops.corpus_index_probe)
    for name in ("build_index", "lookup", "contains"):
        assert callable(getattr(D.MosesDeviceDataset, name))
    assert isinstance(D.MosesDeviceDataset.n_distinct, property)
    build = open(os.path.join(ROOT, "molecular-vae_amd", "csrc", "build.sh")).read()
    assert build.count("corpus_index conv latent capi; do") == 2 and "build/corpus_index.o" in build and "build/tune/corpus_index.o" in build


def test_entries_refuse_bad_arguments_before_launching():
    """Everything below returns before any HIP call (no device needed)."""
    lib = L.load()
    fake = ctypes.c_void_p(256)                                  # never dereferenced: every call below is refused first

    def build(tokens=fake, offsets=fake, N=10, slots=fake, n_slots=16, n_distinct=None):
        return lib.mvae_corpus_index_build(tokens, offsets, N, slots, n_slots, n_distinct, None)

    def probe(tokens=fake, offsets=fake, N=10, slots=fake, n_slots=16, B=4, T=9, x=fake, x_ld=9, eos=4, match=fake):
        return lib.mvae_corpus_index_probe(tokens, offsets, N, slots, n_slots, B, T, x, x_ld, eos, match, None)
    table = (dict(tokens=None), dict(offsets=None), dict(slots=None), dict(N=0), dict(N=-1), dict(n_slots=15), dict(n_slots=24),
             dict(n_slots=8), dict(N=16), dict(N=17), dict(n_slots=0), dict(n_slots=-16))      # not a power of two / not greater than N
    for bad in table:
        assert build(**bad) == -1, bad
        assert build(n_distinct=fake, **bad) == -1, bad
        assert probe(**bad) == -1, bad
    for bad in (dict(x=None), dict(match=None), dict(B=0), dict(B=-1), dict(T=0), dict(T=-1), dict(x_ld=8), dict(eos=-1), dict(eos=65536)):
        assert probe(**bad) == -1, bad


def _strings(n, seed, alphabet="CNO()=c1", longest=9):
    rs = np.random.RandomState(seed)
    return ["".join(rs.choice(list(alphabet), size=int(k))) for k in rs.randint(0, longest + 1, size=n)]


def test_reference_equals_membership_in_a_set_of_strings():
    """For a corpus without specials token equality is string equality: the dict of tests/novelty_ref.py answers what ``in`` answers, and
    names the first row that holds the string."""
    corpus = _strings(300, seed=1, longest=4)                                # short strings over 8 characters: many repeats, some empty
    vocab = VC.CharVocab.from_data(corpus + ["CNO()=c1"])
    table = NR.index([vocab.string2ids(s) for s in corpus])
    assert NR.n_distinct(table) == len(set(corpus)) < len(corpus) and "" in corpus
    queries = _strings(400, seed=2, longest=5) + corpus[:20]
    rows = [vocab.string2ids(s, add_bos=True, add_eos=True) + [vocab.pad] * k for k, s in zip(range(len(queries)), queries)]
    got = NR.lookup(table, rows, vocab.eos)
    assert [g >= 0 for g in got] == [s in set(corpus) for s in queries]
    assert 0 < sum(g >= 0 for g in got) < len(got)
    assert all(g == corpus.index(s) for g, s in zip(got, queries) if g >= 0)
    # the cut: nothing at or behind the first <eos> counts; without one the row runs to its end
    e = vocab.eos
    assert NR.content([vocab.bos, 1, 2, e, 3, e], e) == (1, 2) and NR.content([vocab.bos, 1, 2, 3], e) == (1, 2, 3)
    assert NR.content([vocab.bos], e) == () and NR.content([vocab.bos, e, 5], e) == ()
    assert NR.lookup(NR.index([[1, 2], [], [1, 2]]), [[9, 1, 2, e], [9, e], [9, 1, 2], [9, 1, 300, e], [9, 1, -1, e]], e) == [0, 1, 0, -1, -1]


def _cpu_model(chars="abc"):
    torch.manual_seed(0)
    return MV.VAE(VC.OneHotVocab(list(chars)), dtype=torch.float32)


def test_moses_generate_refuses_a_wrong_novel_against_before_any_device_work():
    model = _cpu_model()
    same = D.MosesDeviceDataset(["ab", "c"], VC.OneHotVocab(list("abc")), device="cpu")
    other = D.MosesDeviceDataset(["ab", "c"], VC.OneHotVocab(list("abcd")), device="cpu")     # every special one id further on
    renamed = D.MosesDeviceDataset(["ab", "c"], VC.OneHotVocab(list("abd")), device="cpu")    # same size, id 2 another character
    for ds in (other, renamed):
        with pytest.raises(ValueError, match="vocabulary"):
            mv.moses_generate(model, 4, max_len=4, novel_against=ds)
    for thing in ({"ab", "c"}, ["ab"], "ab", same.tokens):
        with pytest.raises(ValueError, match="MosesDeviceDataset"):
            mv.moses_generate(model, 4, max_len=4, novel_against=thing)
    with pytest.raises(L.MvaeError, match="MI355X only"):                                      # accepted; then a CPU model has no fallback
        mv.moses_generate(model, 4, max_len=4, novel_against=same)
    assert same._slots is None                                                                # nothing was built on the way


def test_lookup_refuses_bad_input_and_has_no_cpu_fallback():
    ds = D.MosesDeviceDataset(["ab", "c"], VC.OneHotVocab(list("abc")), device="cpu")
    with pytest.raises(ValueError, match="at least one row"):
        ds.lookup([])
    for x in (torch.zeros(3, dtype=torch.long), torch.zeros(2, 3, 4, dtype=torch.long), torch.zeros(0, 3, dtype=torch.long)):
        with pytest.raises(ValueError, match=r"\[B, T\]"):
            ds.lookup(x)
    for call in (ds.build_index, lambda: ds.lookup(["ab"]), lambda: ds.contains(["ab"]), lambda: ds.n_distinct):
        with pytest.raises(L.MvaeError, match="MI355X only"):
            call()
