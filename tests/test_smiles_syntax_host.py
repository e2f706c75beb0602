"""CPU tests of the SMILES syntax surface (vocab.smiles_token_table, mvae_moses_sample_syntax_step, mvae_smiles_syntax_check,
VAE.sample(syntax=), VAE.syntax_valid, moses_generate(syntax=, count_valid=)): the token table, the two formulations of the accepted
language in tests/syntax_ref.py (the automaton of the specification and an independently written validator) on hand-made strings and
on random constrained walks, the argument checks of the entry points (refused before anything is launched), and the ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import molecular_vae_amd as mv
from molecular_vae_amd import _lib as L, data as D, mosesvae as MV, vocab as VC, ops
import syntax_ref as SY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP, CHECK = "mvae_moses_sample_syntax_step", "mvae_smiles_syntax_check"
G5 = ["CCO", "c1ccccc1", "CC(=O)Oc1ccccc1C(=O)O", "CN1CCC[C@H]1c2cccnc2", "O=C(O)c1ccccc1", "C1CC1", "N#Cc1ccc(Br)cc1",
      "CC(C)Cc1ccc(cc1)[C@@H](C)C(=O)O"]
GOOD = G5 + ["C[N+](C)(C)C", "[O-]C", "ClC(Cl)Cl"]
BAD = ["C(", "C)", "C1CC", "C11", "C()", "C(=)", "=C", "C=", "C[", "[]C", "C(C)1CC1", "Cr", "Bl", "CH", ""]
MAX_LENS = (3, 4, 5, 6, 8, 12, 20, 40, 100)


def _g5_vocab(golden_dir):
    g = np.load(os.path.join(golden_dir, "g5_vocab.npz"))
    v = VC.CharVocab.from_data(G5)
    assert [v.i2c[i] for i in range(len(v))] == [str(s) for s in g["symbols"]]
    return v


def _synth_vocab(extra=""):
    return VC.OneHotVocab(set("CNOSFcnos()=#123[]@H+-lBr") | set(extra))


def test_entries_are_declared_bound_and_exported_at_abi_12():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvae.h")).read(), flags=re.S)
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", header).group(1)) == 12 == L.ABI_VERSION
    lib = L.load()
    assert lib.mvae_abi_version() == 12
    for name in (STEP, CHECK):
        assert re.search(r"\b" + name + r"\s*\(", header)
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert len(L.SIGNATURES[STEP][1]) == len(L.SIGNATURES["mvae_moses_sample_filtered_step"][1]) + 3      # tok_info, gstate, max_len
    assert callable(ops.moses_sample_syntax_step) and callable(ops.smiles_syntax_check)
    assert callable(VC.smiles_token_table) and callable(MV.VAE.syntax_valid)


def test_token_table_of_the_g5_vocabulary(golden_dir):
    v = _g5_vocab(golden_dir)
    t = VC.smiles_token_table(v)
    assert t.dtype == torch.int32 and tuple(t.shape) == (len(v),)
    t = t.tolist()
    cls = {ch: t[i] & 0xFF for ch, i in v.c2i.items()}
    for ch in "CNOBcn":
        assert cls[ch] == VC.SMI_ATOM and t[v.c2i[ch]] == VC.SMI_ATOM
    assert cls["#"] == cls["="] == VC.SMI_BOND and cls["("] == VC.SMI_LPAR and cls[")"] == VC.SMI_RPAR
    assert cls["["] == VC.SMI_LBRK and cls["]"] == VC.SMI_RBRK and cls["@"] == VC.SMI_AT and cls["H"] == VC.SMI_H
    assert t[v.c2i["1"]] == VC.SMI_DIGIT | 1 << 16 and t[v.c2i["2"]] == VC.SMI_DIGIT | 2 << 16
    assert t[v.c2i["r"]] == VC.SMI_TAIL | (v.c2i["B"] + 1) << 8
    assert t[v.eos] == VC.SMI_EOS and t[v.bos] == t[v.pad] == t[v.unk] == VC.SMI_OTHER
    assert "l" not in v.c2i


def test_token_table_of_the_synthetic_alphabet_is_the_vocabulary_of_synthetic_smiles():
    v = _synth_vocab()
    w = VC.OneHotVocab.from_data(D.synthetic_smiles(2048, seed=0))
    assert v.c2i == w.c2i and len(v) == 29
    t = VC.smiles_token_table(v).tolist()
    want = {"l": VC.SMI_TAIL | (v.c2i["C"] + 1) << 8, "r": VC.SMI_TAIL | (v.c2i["B"] + 1) << 8, "-": VC.SMI_MINUS, "+": VC.SMI_PLUS,
            "3": VC.SMI_DIGIT | 3 << 16, "S": VC.SMI_ATOM, "s": VC.SMI_ATOM, "F": VC.SMI_ATOM}
    for ch, word in want.items():
        assert t[v.c2i[ch]] == word, ch
    assert sum(1 for x in t if x & 0xFF == VC.SMI_OTHER) == 3                      # bos, pad, unk
    # characters outside the grammar are OTHER; '0' is a ring digit, the bonds / \ : are bonds
    x = _synth_vocab("0/\\.%:I")
    tx = VC.smiles_token_table(x).tolist()
    assert tx[x.c2i["."]] == tx[x.c2i["%"]] == VC.SMI_OTHER and tx[x.c2i["0"]] == VC.SMI_DIGIT
    assert tx[x.c2i["/"]] == tx[x.c2i["\\"]] == tx[x.c2i[":"]] == VC.SMI_BOND and tx[x.c2i["I"]] == VC.SMI_ATOM


def test_token_table_pairing_and_tail_rules():
    t = lambda chars: (lambda v: {ch: w & 0xFF for ch, w in zip([v.i2c[i] for i in range(len(v))], VC.smiles_token_table(v).tolist())})(
        VC.CharVocab(set(chars)))
    assert t("Cl")["l"] == VC.SMI_TAIL and t("Nl")["l"] == VC.SMI_OTHER               # Cl needs its C
    assert t("Br")["r"] == VC.SMI_TAIL and t("Cr")["r"] == VC.SMI_OTHER               # Br needs its B
    assert t("C()")["("] == VC.SMI_LPAR and t("C()")[")"] == VC.SMI_RPAR
    assert t("C(")["("] == VC.SMI_OTHER and t("C)")[")"] == VC.SMI_OTHER
    assert t("C[]")["["] == VC.SMI_LBRK and t("C[]")["]"] == VC.SMI_RBRK
    assert t("C[")["["] == VC.SMI_OTHER and t("C]")["]"] == VC.SMI_OTHER
    for chars in ("", "()=1", "H+-", "lr"):
        with pytest.raises(ValueError, match="no atom token"):
            VC.smiles_token_table(VC.CharVocab(set(chars)))
    # token_chars (the test helper) draws the same lines
    v = VC.CharVocab(set("Nl(C"))
    ch = SY.token_chars(v)
    assert ch[v.c2i["l"]] == "l" and ch[v.c2i["("]] is None and ch[v.eos] == "$" and ch[v.bos] is None


@pytest.mark.parametrize("s", GOOD)
def test_both_formulations_accept(s):
    assert SY.accepts(s) and SY.valid_smiles(s)


@pytest.mark.parametrize("s", BAD)
def test_both_formulations_reject(s):
    assert not SY.accepts(s) and not SY.valid_smiles(s)


def test_need_counts_the_tokens_a_shortest_completion_takes():
    """need() on a few states by hand: START needs an atom and <eos>; an open ring on the current atom needs another atom, its digit and
    <eos>; inside a bracket the symbol, ']' and the rest."""
    def state(s):
        st = SY.S0
        for ch in s:
            st = SY.step(st, ch)
            assert st is not None, s
        return st
    assert SY.need(SY.S0) == 2 and SY.need(state("C")) == 1 and SY.need(state("C=")) == 2
    assert SY.need(state("C1")) == 3 and SY.need(state("C1C")) == 2 and SY.need(state("C1C(")) == 4
    assert SY.need(state("C1C(C)")) == 3                                             # an atom, the digit, <eos>: no digit after ')'
    assert SY.need(state("C[")) == 3 and SY.need(state("C[N")) == 2 and SY.need(state("C[N+]")) == 1
    assert SY.need(state("C(C(C")) == 3


@pytest.mark.parametrize("name", ["g5", "synthetic+"])
def test_random_constrained_walks_finish_and_are_well_formed(golden_dir, name):
    """2,000 uniformly random constrained walks per max_len: every allowed set is non-empty, every walk ends in <eos> within max_len, and
    the independently written validator accepts the string.  (Unconstrained uniform strings over the same alphabet are accepted at about
    2 %: printed.)"""
    v = _g5_vocab(golden_dir) if name == "g5" else _synth_vocab("0/\\.%")
    chars = SY.token_chars(v)
    rs = np.random.RandomState(7)
    longest = 0
    for max_len in MAX_LENS:
        for _ in range(2000):
            ids, states = SY.random_walk(chars, max_len, rs)
            assert states[-1][0] == SY.END and ids[-1] == v.eos and len(ids) <= max_len - 1, (max_len, ids)
            s = "".join(chars[t] for t in ids[:-1])
            assert SY.valid_smiles(s), (max_len, s)
            longest = max(longest, len(ids))
    assert longest == 99                                                             # the budget is used, not just respected
    sym = [c for c in chars if c is not None and c != "$"]
    hits = sum(SY.valid_smiles("".join(rs.choice(sym, size=rs.randint(1, 12)))) for _ in range(4000))
    print(f"{name}: unconstrained uniform strings accepted: {hits / 4000:.3f}")
    assert hits / 4000 < 0.25


def test_validator_and_automaton_agree_on_random_strings():
    """The two formulations decide the same language: random strings biased towards short, plausible ones."""
    rs = np.random.RandomState(11)
    sym = list("CCCNOcn()()==#1212[]@H+-lBr")
    n_ok = 0
    for _ in range(20000):
        s = "".join(rs.choice(sym, size=rs.randint(1, 9)))
        a, b = SY.accepts(s), SY.valid_smiles(s)
        assert a == b, s
        n_ok += a
    assert n_ok > 200


def test_entry_points_refuse_bad_arguments_before_launching():
    """Everything below returns before any HIP call (no device needed)."""
    lib = L.load()
    fake = ctypes.c_void_p(256)                                  # never dereferenced: every call below is refused first

    def step(top_k=0, top_p=1.0, V=29, dtype=L.MVAE_F32, temp=1.0, x=fake, W=2048, tok=fake, gs=fake, max_len=10, step=1, eos=1):
        return getattr(lib, STEP)(dtype, 8, V, 512, fake, 520, fake, 520, None, temp, top_k, top_p, 1, step, eos, fake, W, fake, fake, x, 16, fake,
                                  fake, fake, None, None, tok, gs, max_len, None)
    # what the filtered entry refuses
    assert step(top_k=-1) == -1 and step(top_k=30) == -1 and step(top_p=0.0) == -1 and step(top_p=float("nan")) == -1
    assert step(V=65) == -1 and step(x=None) == -1 and step(dtype=7) == -1 and step(temp=0.0) == -1 and step(W=6) == -1
    # and its own
    assert step(tok=None) == -1 and step(gs=None) == -1
    assert step(max_len=2) == -1 and step(max_len=0) == -1
    assert step(step=0) == -1 and step(step=-1) == -1 and step(step=10) == -1 and step(step=11) == -1
    assert step(eos=-1) == -1 and step(eos=29) == -1

    def chk(B=4, T=8, V=29, x=fake, ld=8, tok=fake, eos=1, valid=fake):
        return getattr(lib, CHECK)(B, T, V, x, ld, tok, eos, valid, None, None)
    assert chk(B=0) == -1 and chk(T=0) == -1 and chk(V=0) == -1 and chk(V=65) == -1 and chk(x=None) == -1 and chk(tok=None) == -1
    assert chk(valid=None) == -1 and chk(ld=7) == -1 and chk(eos=29) == -1 and chk(eos=-1) == -1


def test_sample_and_generate_refuse_bad_syntax_arguments_and_have_no_cpu_fallback():
    torch.manual_seed(0)
    model = MV.VAE(VC.OneHotVocab(list("CNO(=)1")), dtype=torch.float32)
    for n in (2, 1, 0):
        with pytest.raises(ValueError, match="max_len >= 3"):
            model.sample(2, max_len=n, syntax=True)
        with pytest.raises(ValueError, match="max_len >= 3"):
            model._sample_tokens(torch.zeros(2, model.d_z), n, 1.0, 0, syntax=True)
    with pytest.raises(ValueError, match="max_len >= 3"):
        mv.moses_generate(model, 4, max_len=2, syntax=True)
    with pytest.raises(L.MvaeError, match="MI355X only"):                            # a CPU model: no fallback
        model.sample(2, max_len=3, syntax=True)
    with pytest.raises(L.MvaeError, match="MI355X only"):
        model.syntax_valid(["CCO"])
    with pytest.raises(L.MvaeError, match="MI355X only"):
        mv.moses_generate(model, 4, max_len=8, syntax=True, count_valid=True)
    no_atoms = MV.VAE(VC.OneHotVocab(list("xyz")), dtype=torch.float32)
    with pytest.raises(ValueError, match="no atom token"):
        no_atoms.sample(2, max_len=8, syntax=True)
