"""CPU tests of prefix-constrained sampling and decoding (mvae_moses_sample_forced_step, mvae_moses_beam_forced_step,
mvae_smiles_prefix_state; VAE.sample / decode / moses_generate with prefix=): the entry points are declared, bound and exported at ABI 12
and refuse bad arguments before anything is launched; every ValueError of the Python surface is raised by a CPU model; the table builder
handles broadcast, an empty prefix and the P = max_len - 2 edge; the float64 reference of tests/prefix_ref.py is
beam_syntax_ref.beam_search when no prefix is given, and its prefix walk agrees with syntax_ref's automaton."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import molecular_vae_amd as mv
from molecular_vae_amd import _lib as L, mosesvae as MV, vocab as VC, ops
import beam_syntax_ref as BS
import prefix_ref as PR
import syntax_ref as SY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE, BEAM, WALK = "mvae_moses_sample_forced_step", "mvae_moses_beam_forced_step", "mvae_smiles_prefix_state"


def test_entries_are_declared_bound_and_exported_at_abi_12():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvae.h")).read(), flags=re.S)
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", header).group(1)) == 12 == L.ABI_VERSION
    lib = L.load()
    for name in (SAMPLE, BEAM, WALK):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    # the arguments of the *_syntax_step entries plus (forced, forced_ld) in front of the stream
    for forced, sibling in ((SAMPLE, "mvae_moses_sample_syntax_step"), (BEAM, "mvae_moses_beam_syntax_step")):
        a, b = L.SIGNATURES[forced][1], L.SIGNATURES[sibling][1]
        assert len(a) == len(b) + 2 and a[:-3] == b[:-1] and a[-1] == b[-1]
    assert callable(ops.moses_sample_forced_step) and callable(ops.moses_beam_forced_step) and callable(ops.smiles_prefix_state)


def test_entries_refuse_bad_arguments_before_launching():
    """Everything below returns before any HIP call (no device needed)."""
    lib = L.load()
    fake = ctypes.c_void_p(256)                                  # never dereferenced: every call below is refused first

    def smp(V=30, H=512, dtype=L.MVAE_F32, temp=1.0, top_k=0, top_p=1.0, stp=1, eos=1, W=2048, h=fake, tok=fake, gs=fake, max_len=10,
            forced=fake, fld=10):
        return getattr(lib, SAMPLE)(dtype, 8, V, H, h, H + 8, fake, H + 8, None, temp, top_k, top_p, 7, stp, eos, fake, W, fake, fake, fake, 10,
                                    fake, fake, fake, None, None, tok, gs, max_len, forced, fld, None)
    # what the filtered / syntax entries refuse
    assert smp(h=None) == -1 and smp(dtype=7) == -1 and smp(V=65) == -1 and smp(W=6) == -1 and smp(temp=0.0) == -1
    assert smp(top_k=31) == -1 and smp(top_p=0.0) == -1 and smp(top_p=float("nan")) == -1
    assert smp(max_len=2) == -1 and smp(stp=0) == -1 and smp(stp=10, fld=11) == -1 and smp(eos=30) == -1
    assert smp(V=64, H=1024) == -3
    # its own
    assert smp(forced=None) == -1 and smp(stp=3, fld=3) == -1 and smp(fld=0) == -1
    assert smp(tok=None) == -1 and smp(gs=None) == -1                       # both or neither

    def beam(K=4, V=30, H=512, dtype=L.MVAE_F32, eos=1, pad=2, W=2048, stp=1, state=fake, tok=fake, gs=fake, max_len=10, forced=fake, fld=10):
        return getattr(lib, BEAM)(dtype, 8, K, V, H, 3, state, 0, 0, H + 8, fake, H + 8, None, stp, eos, pad, fake, W, fake, fake, fake, fake,
                                  fake, fake, fake, tok, gs, max_len, forced, fld, None)
    assert beam(K=0) == -1 and beam(K=17) == -1 and beam(K=5, V=4) == -1 and beam(state=None) == -1 and beam(dtype=7) == -1
    assert beam(eos=30) == -1 and beam(pad=-1) == -1 and beam(W=6) == -1 and beam(stp=0) == -1
    assert beam(V=65, K=1) == -3 and beam(V=64, H=1024) == -3
    assert beam(V=65, K=1, tok=None, gs=None) == -3
    assert beam(max_len=2) == -1 and beam(stp=10, fld=11) == -1
    assert beam(forced=None) == -1 and beam(stp=3, fld=3) == -1 and beam(fld=0) == -1
    assert beam(tok=None) == -1 and beam(gs=None) == -1

    def walk(B=4, P=5, V=30, ids=fake, ld=5, lens=fake, info=fake, st=fake, need=fake, bad=fake):
        return getattr(lib, WALK)(B, P, V, ids, ld, lens, info, st, need, bad, None)
    for name in ("ids", "lens", "info", "st", "need", "bad"):
        assert walk(**{name: None}) == -1, name
    assert walk(B=0) == -1 and walk(P=-1) == -1 and walk(V=0) == -1 and walk(V=65) == -1 and walk(ld=4) == -1


def _cpu_model():
    torch.manual_seed(0)
    return MV.VAE(VC.OneHotVocab(list("CNO(=)1")), dtype=torch.float32)


def test_every_prefix_error_is_raised_by_a_cpu_model():
    model = _cpu_model()
    v = model.vocabulary
    z = torch.zeros(3, model.d_z)
    calls = {
        "sample": lambda prefix, max_len=10: model.sample(3, max_len=max_len, z=z, prefix=prefix),
        "sample_syntax": lambda prefix, max_len=10: model.sample(3, max_len=max_len, z=z, prefix=prefix, syntax=True, top_k=3),
        "decode": lambda prefix, max_len=10: model.decode(z, beam_width=2, max_len=max_len, prefix=prefix),
        "beam": lambda prefix, max_len=10: model._beam_search(z, 2, max_len, syntax=True, prefix=prefix),
        "generate": lambda prefix, max_len=10: mv.moses_generate(model, 3, batch_size=2, max_len=max_len, prefix=prefix),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="list of 3"):
            call(["C", "N"])
        with pytest.raises(ValueError, match="list of 3"):
            call(["C", "N", "O", "C"])
        with pytest.raises(ValueError, match=r"row 1: character 'x' is not in the vocabulary"):
            call(["C", "Cx", "O"])
        with pytest.raises(ValueError, match="not in the vocabulary"):
            call("Cl")
        for bad in (-1, len(v), v.bos, v.eos, v.pad):
            with pytest.raises(ValueError, match=rf"row 0, position 1: id {bad} "):
                call(torch.tensor([v.c2i["C"], bad]))
            with pytest.raises(ValueError, match=rf"row 2, position 0: id {bad} "):
                call(["C", "", torch.tensor([bad])])
        with pytest.raises(ValueError, match="row 0 has 9 tokens, max_len = 10"):
            call("C" * 9)
        with pytest.raises(ValueError, match="row 1 has 3 tokens, max_len = 4"):
            call(["", "CCC", "C"], max_len=4)
        with pytest.raises(ValueError, match="1-D integer id tensor"):
            call(torch.zeros(2, 2, dtype=torch.long))
        with pytest.raises(ValueError, match="1-D integer id tensor"):
            call(torch.tensor([0.0, 1.0]))
        with pytest.raises(L.MvaeError, match="MI355X only"):                          # a valid prefix on a CPU model: no fallback
            call("C" * 8)
        with pytest.raises(L.MvaeError, match="MI355X only"):
            call(["", "CC", torch.tensor([v.unk])])                                    # <unk> is an id like another
    with pytest.raises(L.MvaeError, match="MI355X only"):                              # prefix=None: what it always did
        model.sample(3, max_len=10, z=z)


def test_prefix_table_layout():
    model = _cpu_model()
    v = model.vocabulary
    C, N, O = v.c2i["C"], v.c2i["N"], v.c2i["O"]
    assert model._prefix_table(None, 5, 10, "t") is None
    tab, lens = model._prefix_table("CN", 5, 6, "t")                                  # one prefix: a single row, broadcast later
    assert tab.dtype == torch.int32 and lens.dtype == torch.int32
    assert tab.tolist() == [[-1, C, N, -1, -1, -1]] and lens.tolist() == [2]
    tab, lens = model._prefix_table(torch.tensor([O, O, C, N]), 5, 6, "t")            # P = max_len - 2: the last step stays free
    assert tab.tolist() == [[-1, O, O, C, N, -1]] and lens.tolist() == [4]
    tab, lens = model._prefix_table(["", "C", torch.tensor([N, O], dtype=torch.int32), [C, C, C]], 4, 5, "t")
    assert tab.tolist() == [[-1] * 5, [-1, C, -1, -1, -1], [-1, N, O, -1, -1], [-1, C, C, C, -1]] and lens.tolist() == [0, 1, 2, 3]
    tab, lens = model._prefix_table("", 3, 2, "t")                                    # nothing forced at all
    assert tab.tolist() == [[-1, -1]] and lens.tolist() == [0]
    tab, lens = model._prefix_table([torch.empty(0, dtype=torch.long)] * 2, 2, 3, "t")
    assert tab.tolist() == [[-1] * 3] * 2 and lens.tolist() == [0, 0]


@pytest.mark.parametrize("syntax", [False, True])
@pytest.mark.parametrize("K,max_len", [(1, 9), (3, 7), (4, 4)])
def test_reference_without_prefixes_is_the_syntax_reference(K, max_len, syntax):
    v = PR.vocab()
    _, p = PR.model(torch.float32)
    for z in PR.latents(2, seed=2, scale=0.7).double().numpy():
        a = PR.beam_search(p, z, K, max_len, v, prefix=(), syntax=syntax)
        b = BS.beam_search(p, z, K, max_len, v, syntax=syntax)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


def test_reference_with_a_prefix_keeps_it_and_scores_the_whole_string():
    """K = 3, prefix "CC(": every hypothesis starts with it, beams 1 .. K-1 are alive after the first free step, and beam 0's score is the
    teacher-forced log p of its whole row; with syntax every finite hypothesis is well-formed."""
    import beam_ref as BR
    v = PR.vocab()
    _, p = PR.model(torch.float32)
    pre = PR.string_ids("CC(", v)
    z = PR.latents(1, seed=2, scale=0.7).double().numpy()[0]
    for syntax in (False, True):
        ids, ends, sc, _ = PR.beam_search(p, z, 3, 12, v, prefix=pre, syntax=syntax)
        assert np.isfinite(sc).all() and (ids[:, 1:4] == np.array(pre)).all()
        lp, _, _ = BR.teacher_forced(p, z, ids[0, :ends[0]])
        assert abs(lp.sum() - sc[0]) < 1e-9
        if syntax:
            assert all(SY.row_valid(r, v) for r in ids)


def test_prefix_walk_follows_the_automaton():
    v = PR.vocab()
    chars = SY.token_chars(v)
    rs = np.random.RandomState(3)
    for n in range(0, 21):
        st, ids = SY.random_prefix(chars, n, rs)
        words, need, bad = PR.prefix_walk(ids, v)
        assert bad == -1 and words == SY.pack_state(st, v) and need == SY.need(st)
    words, need, bad = PR.prefix_walk(PR.string_ids("C)", v), v)
    assert bad == 1 and need == 0 and words[0] & 0xFF == SY.ERROR and (words[0] >> 16) & 0xFF == v.c2i["C"]
    assert PR.prefix_walk([v.c2i["C"], 99], v)[2] == 1 and PR.prefix_walk([v.bos], v)[2] == 0
    assert PR.prefix_walk(PR.string_ids("C((", v), v)[2] == 2                       # '(' after '(' is refused
    assert PR.prefix_walk(PR.string_ids("C=", v), v)[1:] == (2, -1)                 # an atom and <eos> are owed
