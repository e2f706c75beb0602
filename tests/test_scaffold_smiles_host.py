"""CPU tests of the scaffold SMILES (mvae_smiles_scaffold_smiles_rows / _corpus / _host): the host entry (csrc/scaffold_smiles.hip on
the shared writer and the shared ranks, compiled for the CPU) against the reference of tests/scaffold_smiles_ref.py, byte for byte in
tokens, lengths, statuses and info on canon_ref.corpus() + canon_ref.CAGES; what the definition promises, through entries that know
nothing of the new reference -- the graph, scaffold, kekule and substructure entries --, idempotence, invariance under respelling, one
string whichever member is taken at every tie; three deliberately broken references that named checks must catch; every refusal; the
argument checks; the declarations and the compiler's resource remarks; the header's worked examples as literal strings."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from molecular_vae_amd import _lib as L, vocab as VC, ops
import canon_ref as CN
import chem_ref as CR
import rewrite_ref as RR
import scaffold_smiles_ref as SS
from test_smiles_rewrite_host import LADDER                      # a constant: the P ladder that needs eleven ring digits at once

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mvae_smiles_scaffold_smiles_rows", "mvae_smiles_scaffold_smiles_corpus", "mvae_smiles_scaffold_smiles_host")
SPELLINGS = 8
SEED = 5
# rows that reach the spelling's refusals on the scaffold itself (chosen with the reference alone).  RING_MULTI: the allene centre is the
# only unbracketed atom, so it has the lowest invariant and is the root, and the ring closes on its second double bond.  DEPTH: the S
# chain is a linker between two rings, every =I is Exo, and S ranks below I, so each S opens a branch for the next.
MULTI = "[CH]1=C=[CH][CH2][CH2][CH2]1"
DEEP = "C1CC1" + "=S(=I)" * 17 + "=C1CC1"
WORKED = (("Cn1cccc1", "c1cc[nH]c1"), ("C[n+]1ccccc1", "c1cc[nH+]cc1"), ("C[N+]1(C)CCCC1", "C1CC[NH2+]C1"), ("O=C1CCCCC1C", "C1CCC(=O)CC1"),
          ("N#Cc1ccc(Br)=c1", "c1cc=[cH]c1"), ("Clc1ccccc1", "c1ccccc1"), ("CP1(=O)CCCC1", "C1CCP(=O)C1"))


def _tables(v):
    return VC.smiles_token_table(v), VC.smiles_chem_table(v), VC.smiles_emit_table(v)


def _host(strings, max_content=127, T=None, T_out=None, v=None, **kw):
    v = CR.vocabulary() if v is None else v
    x = torch.from_numpy(CR.token_rows(strings, v, T))
    out = ops.smiles_scaffold_smiles_host(x, *_tables(v), v.bos, v.eos, v.pad, max_content, T_out, **kw)
    return tuple(None if t is None else t.numpy() for t in out)


def _decode(out, out_len, v):
    return ["".join(v.i2c[int(i)] for i in row[1:n - 1]) for row, n in zip(out, out_len)]


def _want(refs, v, T_out):
    """The reference's (status, string, info) per row as the arrays the entries write."""
    B = len(refs)
    rows, lens = np.full((B, T_out), v.pad, np.int64), np.zeros(B, np.int32)
    status, info = np.zeros(B, np.int32), np.zeros((B, 4), np.int32)
    for b, (st, s, inf) in enumerate(refs):
        ids = v.string2ids(s, add_bos=True, add_eos=True)
        rows[b, :min(len(ids), T_out)] = ids[:T_out]
        lens[b], status[b] = len(ids), st
        if inf is not None and st in (0, 9, 10, 11, 12, 13):
            info[b] = inf
    return rows, lens, status, info


def _equal(got, want):
    return [name for g, w, name in zip(got, want, ("out", "out_len", "status", "info")) if not np.array_equal(g, w)]


_CASES = {}


def cases():
    """(rows, the reference's result per row, the host entry's outputs, its rows decoded) of canon_ref.corpus() + canon_ref.CAGES:
    computed once per process and shared; callers leave it unchanged."""
    if "c" not in _CASES:
        rows = CN.corpus() + CN.CAGES
        got = _host(rows, T=131)
        _CASES["c"] = (rows, [SS.scaffold(s) for s in rows], got, _decode(got[0], got[1], CR.vocabulary()))
    return _CASES["c"]


def _older(strings):
    """What the entries that existed before say of the strings: graph status, scaffold (status, mask, desc, key), kekule (status, desc)."""
    v = CR.vocabulary()
    tok, chem = VC.smiles_token_table(v), VC.smiles_chem_table(v)
    x = torch.from_numpy(CR.token_rows([s if 0 < len(s) <= 127 else "C(" for s in strings], v))
    g = ops.smiles_graph_host(x, tok, chem, v.eos)[0].numpy()
    s = [t.numpy() for t in ops.smiles_scaffold_host(x, tok, chem, v.eos)]
    k = [t.numpy() for t in ops.smiles_kekule_host(x, tok, chem, v.eos, mate=False)[:2]]
    return g, s, k


# ------------------------------------------------------------------------------------------------ the properties, as functions of
# (input strings, output strings, info or None): each returns the indices of the rows that break it, so that the sensitivity test can
# hand them a broken reference's output.  Only rows with a non-empty output are judged.
def breaks_graph_status(rows, outs, info=None):
    g = _older(outs)[0]
    return [i for i, o in enumerate(outs) if o and g[i] != 0]


def breaks_scaffold_entry(rows, outs, info=None):
    """The older scaffold entry on the output: S is all of its atoms; desc[0:2] and the scaffold key are the input's; desc[0:2] is info[0:2]."""
    _, si, _ = _older(rows)
    _, so, _ = _older(outs)
    bad = []
    for i, o in enumerate(outs):
        if not o:
            continue
        n = len(RR.atoms_of(o))
        whole = so[1][i].view(np.uint64).tolist() == [((1 << n) - 1) & (2 ** 64 - 1), ((1 << n) - 1) >> 64]
        same = so[2][i, :2].tolist() == si[2][i, :2].tolist() and so[3][i, 1] == si[3][i, 1]
        told = info is None or so[2][i, :2].tolist() == list(info[i][:2])
        if not (so[0][i] == 0 and whole and same and told):
            bad.append(i)
    return bad


def breaks_kekule(rows, outs, info=None):
    _, _, ki = _older(rows)
    _, _, ko = _older(outs)
    return [i for i, o in enumerate(outs) if o and ki[0][i] == 0 and (ko[0][i] != 0 or ko[1][i].tolist() != ki[1][i].tolist())]


def breaks_empty_on_refusal(status, outs):
    return [i for i, (st, o) in enumerate(zip(status, outs)) if st != 0 and o]


def test_entries_are_declared_bound_and_exported_at_abi_12():
    text = open(os.path.join(ROOT, "include", "mvae.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", header).group(1)) == 12 == L.ABI_VERSION
    lib = L.load()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    # the canon entries' arguments without rank
    for mine, canon in zip(ENTRIES, ("mvae_smiles_canon_rows", "mvae_smiles_canon_corpus", "mvae_smiles_canon_host")):
        assert len(L.SIGNATURES[mine][1]) == len(L.SIGNATURES[canon][1]) - 1
    assert ops.SCAFFOLD_SMILES_STATUS_NAMES == ops.REWRITE_STATUS_NAMES + ("no_ring",) and len(ops.REWRITE_STATUS_NAMES) == 14
    assert int(re.search(r"#define\s+MVAE_SMILES_NO_RING\s+(\d+)", header).group(1)) == ops.SMILES_STATUS_NO_RING == SS.NO_RING == 14
    assert int(re.search(r"#define\s+MVAE_SCAFFOLD_SMILES_INFO\s+(\d+)", header).group(1)) == len(ops.SCAFFOLD_SMILES_INFO) == 4
    for phrase in ("Scaffold SMILES", "not rdkit's MurckoScaffoldSmiles", "Nothing is sanitised", "no aromaticity is perceived",
                   "C1CCC(CC1)CCCCCC1CCCCC1", "NOT proved in general"):
        assert phrase in text, phrase
    build = open(os.path.join(ROOT, "molecular-vae_amd", "csrc", "build.sh")).read()
    assert build.count(" scaffold_smiles smiles_substruct ") == 2 and "build/scaffold_smiles.o build/smiles_substruct.o" in build
    assert "build/tune/scaffold_smiles.o build/tune/smiles_substruct.o" in build
    assert "smiles_canon.hpp -nt build/$f.o" in build and "scaffold_sets.hpp -nt build/$f.o" in build
    # the sets, the ranks and the writer are shared, not copied
    csrc = os.path.join(ROOT, "molecular-vae_amd", "csrc")
    src = open(os.path.join(csrc, "scaffold_smiles.hip")).read()
    for name in ("scaffold_sets.hpp", "smiles_canon.hpp", "smiles_writer.hpp"):
        assert f'#include "{name}"' in src, name
    assert "EM_LPAR" not in src and "Writer<" not in src and "run_end" not in src and "Sets scaffold_sets" not in src
    assert '#include "scaffold_sets.hpp"' in open(os.path.join(csrc, "scaffold.hip")).read()
    assert '#include "smiles_canon.hpp"' in open(os.path.join(csrc, "smiles_canon.hip")).read()


def test_new_kernels_use_no_scratch(tmp_path):
    """The compiler's resource remarks for the two kernels of scaffold_smiles.hip, cross-compiled for gfx950: scratch 0, no spills, and
    the LDS per block that include/mvae.h states -- the rewrite's 80 KiB with nothing added."""
    csrc = os.path.join(ROOT, "molecular-vae_amd", "csrc")
    usage = os.path.join(csrc, "build", "scaffold_smiles.usage.txt")
    sources = ("scaffold_smiles.hip", "scaffold_sets.hpp", "smiles_canon.hpp", "smiles_writer.hpp", "smiles_rounds.hpp", "smiles_graph.hpp",
               "smiles_syntax.hpp", "common.hpp", "../../include/mvae.h")
    if os.path.exists(usage) and os.path.getmtime(usage) >= max(os.path.getmtime(os.path.join(csrc, f)) for f in sources):
        text = open(usage, errors="replace").read()
    else:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                              "-c", os.path.join(csrc, "scaffold_smiles.hip"), "-o", str(tmp_path / "scaffold_smiles.dev.o")],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert run.returncode == 0, run.stderr[-2000:]
        text = run.stderr
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 2 and all(any(k in n for n in names) for k in ("smiles_scaffold_smiles_rows_kernel", "smiles_scaffold_smiles_corpus_kernel")), names
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 2
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 2 and re.findall(r"SGPRs Spill: (\d+)", text) == ["0"] * 2
    header = open(os.path.join(ROOT, "include", "mvae.h")).read()
    stated = int(re.search(r"#define\s+MVAE_SCAFFOLD_SMILES_LDS_BYTES\s+(\d+)", header).group(1))
    assert list(map(int, re.findall(r"LDS Size \[bytes/block\]: (\d+)", text))) == [stated] * 2 == [81920] * 2
    assert stated == int(re.search(r"#define\s+MVAE_REWRITE_LDS_BYTES\s+(\d+)", header).group(1))
    assert all(int(n) <= 128 for n in re.findall(r" VGPRs: (\d+)", text))


def test_host_entry_equals_the_reference_byte_for_byte():
    """Tokens, lengths, statuses and info of all 1,017 rows; the same with max_content 20 and 1, with T_out = 2 and without info.  The
    input is not degenerate (asserted on the reference alone, as floors)."""
    rows, refs, got, _ = cases()
    v = CR.vocabulary()
    written = [r for r in refs if r[0] == 0]
    print("rows:", len(rows), "written:", len(written), "no ring:", sum(r[0] == SS.NO_RING for r in refs), "new bracket:",
          sum(r[2][2] > 0 for r in written), "distinct:", len({r[1] for r in written}), "longest:", max(len(r[1]) for r in written))
    assert len(rows) >= 1000 and len(written) >= 700 and sum(r[0] == SS.NO_RING for r in refs) >= 150
    assert sum(r[2][2] > 0 for r in written) >= 50 and len({r[1] for r in written}) >= 400 and max(len(r[1]) for r in written) >= 100
    assert sum(r[2][3] > 0 for r in written) >= 400               # rows that lose a substituent
    wrong = _equal(got, _want(refs, v, 131))
    assert not wrong, wrong
    for mc in (20, 1):
        cut = [SS.scaffold(s, max_content=mc) for s in rows]
        assert sum(r[0] == RR.LONG for r in cut) >= (100 if mc == 20 else 700) and all(r[1] == "" for r in cut if r[0])
        wrong = _equal(_host(rows, max_content=mc, T=131), _want(cut, v, 131))
        assert not wrong, (mc, wrong)
    two = _host(rows, T=131, T_out=2, info=False)
    assert two[3] is None and np.array_equal(two[0], got[0][:, :2]) and np.array_equal(two[1], got[1]) and np.array_equal(two[2], got[2])
    assert (got[1] > 2).sum() == len(written)                      # out_len > T_out tells a cut row: every written one


def test_worked_examples():
    v = CR.vocabulary()
    out, out_len, status, info = _host([w[0] for w in WORKED])
    assert not status.any() and _decode(out, out_len, v) == [w[1] for w in WORKED]
    assert info[:, 2].tolist() == [1, 0, 0, 0, 1, 0, 0] and info[:, 3].tolist() == [1, 1, 2, 1, 2, 1, 1]
    assert [SS.scaffold(w[0])[1] for w in WORKED] == [w[1] for w in WORKED]


def test_outputs_are_valid_scaffolds_of_the_same_kekule_system():
    """The output under the graph, scaffold and kekule entries, none of which knows the new reference."""
    rows, refs, got, outs = cases()
    assert breaks_graph_status(rows, outs) == []
    bad = breaks_scaffold_entry(rows, outs, got[3])
    assert bad == [], [(rows[i], outs[i]) for i in bad[:3]]
    bad = breaks_kekule(rows, outs)
    assert bad == [], [(rows[i], outs[i]) for i in bad[:3]]
    assert sum(1 for s, o in zip(rows, outs) if o and any(c in o for c in "cnos")) >= 300       # aromatic scaffolds are there to judge


def test_scaffolds_are_fixed_points():
    rows, refs, got, outs = cases()
    written = [o for o in outs if o]
    again = _host(written, T=131)
    assert not again[2].any() and _decode(again[0], again[1], CR.vocabulary()) == written
    assert (again[3][:, 2:] == 0).all()                            # nothing is lost and no atom changes


def test_respellings_give_one_scaffold():
    """Eight spellings of every row by the device's own rule: the same scaffold row.  Skipped: spellings of more than 127 tokens, which
    the walk itself refuses as TOO_LONG."""
    rows, refs, got, outs = cases()
    origin, spelled, skipped = [], [], set()
    for i, s in enumerate(rows):
        for d in range(SPELLINGS):
            t = RR.respell(s, SEED, 1000 * i + d, max_content=10 ** 6)[1]
            if len(t) > 127:
                skipped.add(i)
                continue
            origin.append(i)
            spelled.append(t)
    print("spellings:", len(spelled), "changed:", sum(t != rows[i] for i, t in zip(origin, spelled)), "rows with a skip:", sorted(skipped))
    assert len(skipped) <= len(rows) // 100 and sum(t != rows[i] for i, t in zip(origin, spelled)) >= 6000
    out, out_len, status, info = _host(spelled, T=131)
    same = (out == got[0][origin]).all(1) & (out_len == got[1][origin]) & (status == got[2][origin]) & (info == got[3][origin]).all(1)
    assert same.all(), [(rows[origin[k]], spelled[k]) for k in np.nonzero(~same)[0][:3]]


def test_every_choice_at_every_tie_gives_one_string():
    rows, refs, got, outs = cases()
    for s, o in zip(rows, outs):
        if o:
            assert CN.all_choices(o) == {o}, (s, o)
    assert len(CN.all_choices("C1CCC(CC1)CCCCCC1CCCCC1")) == 2      # the known instance of the canon section's limit; not in the corpus


def test_the_scaffold_is_a_substructure_of_its_row():
    """Scaffolds of at most 32 atoms, compiled as queries, hit their own rows within 65536 steps; none is undecided."""
    rows, refs, got, outs = cases()
    v = CR.vocabulary()
    tok, chem, emit = _tables(v)
    pick = [i for i, o in enumerate(outs) if o and got[3][i, 0] <= 32]
    assert len(pick) >= 700
    most = 0
    for lo in range(0, len(pick), 64):
        idx = pick[lo:lo + 64]
        table, qstatus = ops.smiles_substruct_compile(torch.from_numpy(CR.token_rows([outs[i] for i in idx], v)), tok, chem, emit, v.eos)
        assert not qstatus.any()
        x = torch.from_numpy(CR.token_rows([rows[i] for i in idx], v))
        status, hit, undecided, _, steps = ops.smiles_substruct_host(x, tok, chem, v.eos, table, max_steps=65536)
        q = torch.arange(len(idx))
        assert not status.any() and ops.substruct_bits(hit, len(idx))[q, q].all(), [rows[i] for i in idx]
        assert not ops.substruct_bits(undecided, len(idx))[q, q].any()
        most = max(most, int(steps[q, q].max()))
    print("most steps:", most)


def test_equal_strings_have_equal_keys():
    """The strings refine the scaffold keys: rows with one scaffold string have one scaffold key, and here the strings tell more apart."""
    rows, refs, got, outs = cases()
    keys = _older(rows)[1][3][:, 1]
    by_string = {}
    for o, k in zip(outs, keys):
        if o:
            by_string.setdefault(o, set()).add(int(k))
    assert all(len(k) == 1 for k in by_string.values())
    n_keys = len({k for ks in by_string.values() for k in ks})
    print("strings:", len(by_string), "keys:", n_keys)
    assert len(by_string) > n_keys >= 400


def test_broken_references_are_caught():
    """no_h by the kekule check (Cn1cccc1 -> c1ccnc1 gains an atom of N) and by the worked examples; keep_leaf by the scaffold-entry check
    (the kept leaf is not in S of the output) and by idempotence; copy_on_refusal by the empty-row check."""
    rows = cases()[0][::4]
    res = {b: [SS.scaffold(s, broken=b) for s in rows] for b in SS.BROKEN}
    outs = {b: [r[1] for r in res[b]] for b in SS.BROKEN}
    assert breaks_kekule(rows, outs["no_h"]) and [SS.scaffold(w[0], broken="no_h")[1] for w in WORKED] != [w[1] for w in WORKED]
    assert breaks_scaffold_entry(rows, outs["keep_leaf"])
    assert any(SS.scaffold(o)[1] != o for o in outs["keep_leaf"] if o)
    assert breaks_empty_on_refusal([r[0] for r in res["copy_on_refusal"]], outs["copy_on_refusal"])
    good = [SS.scaffold(s) for s in rows]
    assert not breaks_kekule(rows, [r[1] for r in good]) and not breaks_scaffold_entry(rows, [r[1] for r in good])
    assert not breaks_empty_on_refusal([r[0] for r in good], [r[1] for r in good])


def test_every_refusal_gives_the_empty_row():
    """One row of every status 1 - 6 and 8 - 14: bos, eos, pad..., out_len 2; info zeros unless the ranks were computed (9 - 13)."""
    v = CR.vocabulary()
    rejected = [s for s, st, _ in CR.REJECTED if st != CR.OK and s] + ["C" * 128]
    rows = rejected + ["C[C@H]1CC1", "F/C=C/C1CC1", MULTI, LADDER, DEEP, "CCO", "C" * 127]
    refs = [SS.scaffold(s) for s in rows]
    assert {r[0] for r in refs[:len(rejected)]} == {1, 2, 3, 4, 5, 6}
    assert [r[0] for r in refs[len(rejected):]] == [RR.STEREO, RR.STEREO, RR.RING_MULTI, RR.RING_DIGITS, RR.DEPTH, SS.NO_RING, SS.NO_RING]
    assert all(len(s) <= 127 for s in rows[len(rejected):]) and [r[2] is not None for r in refs[-5:]] == [True, True, True, False, False]
    got = _host(rows, T=140)
    wrong = _equal(got, _want(refs, v, 140))
    assert not wrong, wrong
    assert (got[1] == 2).all() and (got[0][:, 0] == v.bos).all() and (got[0][:, 1] == v.eos).all() and (got[0][:, 2:] == v.pad).all()
    assert breaks_empty_on_refusal(got[2], _decode(got[0], got[1], v)) == []
    # LONG: the scaffold of 4-methylbiphenyl takes 15 tokens
    long_rows = ["Cc1ccc(cc1)c1ccccc1", "Cc1ccccc1"]
    refs = [SS.scaffold(s, max_content=14) for s in long_rows]
    assert [r[0] for r in refs] == [RR.LONG, 0] and refs[0][2] == [12, 13, 0, 1]
    got = _host(long_rows, max_content=14)
    wrong = _equal(got, _want(refs, v, got[0].shape[1]))
    assert not wrong, wrong
    # NO_TOKEN: the scaffold of N-methylpyrrole needs an H the vocabulary lacks
    small = VC.OneHotVocab(set(CR.ALPHABET) - {"H"})
    refs = [SS.scaffold(s, have=set(CR.ALPHABET) - {"H"}) for s in ("Cn1cccc1", "Cc1ccccc1")]
    assert [r[0] for r in refs] == [RR.NO_TOKEN, 0] and refs[0][1] == ""
    wrong = _equal(_host(["Cn1cccc1", "Cc1ccccc1"], v=small, T_out=129), _want(refs, small, 129))
    assert not wrong, wrong


def test_edge_rows_strided_input_and_prefilled_outputs():
    """A strided view (x_ld > T), rows without <eos> and with ids outside the vocabulary; every element of prefilled outputs is written."""
    v = CR.vocabulary()
    tabs = _tables(v)
    x = torch.from_numpy(CR.token_rows(["c1cccn1", "c1ccccc1", "C=F", "c1ccncc1", "CC(C)CO", "Cc1ccccc1"], v, T=12))
    x[0, 8] = v.pad                                                # no <eos>
    x[1, 3] = -1
    x[3, 2] = len(v)
    wide = torch.full((6, 40), v.eos, dtype=torch.long)
    wide[:, :12] = x
    pre = (torch.full((6, 20), 0x7f7f7f7f, dtype=torch.int64), torch.full((6,), 0x7f7f7f7f, dtype=torch.int32),
           torch.full((6,), 0x7f7f7f7f, dtype=torch.int32), torch.full((6, 4), 0x7f7f7f7f, dtype=torch.int32))
    got = ops.smiles_scaffold_smiles_host(wide[:, :12], *tabs, v.bos, v.eos, v.pad, 127, 20, *pre)
    assert got[2].tolist() == [1, 1, 2, 1, 14, 0] and got[1].tolist() == [2, 2, 2, 2, 2, 10]
    assert got[0][:5].tolist() == [[v.bos, v.eos] + [v.pad] * 18] * 5 and got[3].tolist() == [[0] * 4] * 5 + [[6, 6, 0, 1]]
    assert got[0][5].tolist() == v.string2ids("c1ccccc1", add_bos=True, add_eos=True) + [v.pad] * 10
    fresh = ops.smiles_scaffold_smiles_host(wide[:, :12], *tabs, v.bos, v.eos, v.pad, 127, 20)
    assert all(torch.equal(a, b) for a, b in zip(fresh, got))


def test_entries_refuse_bad_arguments_before_launching():
    """Everything below returns before any HIP call (no device needed): exactly what the canon entries refuse."""
    lib = L.load()
    fake = ctypes.c_void_p(256)                                  # never dereferenced: every call below is refused first

    def rows(name, B=4, T=8, V=29, x=fake, ld=8, tok=fake, chem=fake, emit=fake, bos=0, eos=1, pad=2, mc=127, T_out=129, out=fake,
             out_len=fake, status=fake):
        tail = (None, None, None) if name == ENTRIES[0] else (None,)
        return getattr(lib, name)(B, T, V, x, ld, tok, chem, emit, bos, eos, pad, mc, T_out, out, out_len, status, *tail)
    for name in (ENTRIES[0], ENTRIES[2]):
        assert rows(name, B=0) == -1 and rows(name, T=0, ld=0) == -1 and rows(name, V=0, eos=0) == -1 and rows(name, V=65) == -3
        assert rows(name, x=None) == -1 and rows(name, tok=None) == -1 and rows(name, chem=None) == -1 and rows(name, status=None) == -1
        assert rows(name, emit=None) == -1 and rows(name, out=None) == -1 and rows(name, out_len=None) == -1 and rows(name, ld=7) == -1
        assert rows(name, eos=29) == -1 and rows(name, eos=-1) == -1 and rows(name, mc=0) == -1 and rows(name, mc=128) == -1
        assert rows(name, T_out=1) == -1 and rows(name, bos=-1) == -1 and rows(name, pad=65536) == -1 and rows(name, V=65, out=None) == -3

    def corpus(tokens=fake, offsets=fake, N=100, rows=fake, B=4, V=29, tok=fake, chem=fake, emit=fake, mc=100, stride=100, tokens_out=fake,
               offsets_out=fake, status=fake):
        return lib.mvae_smiles_scaffold_smiles_corpus(tokens, offsets, N, rows, B, V, tok, chem, emit, mc, stride, tokens_out, offsets_out,
                                                      status, None, None, None, None)
    assert corpus(N=0) == -1 and corpus(B=0) == -1 and corpus(V=0) == -1 and corpus(V=65) == -3 and corpus(rows=None) == -1
    assert corpus(tokens=None) == -1 and corpus(offsets=None) == -1 and corpus(tok=None) == -1 and corpus(chem=None) == -1
    assert corpus(emit=None) == -1 and corpus(status=None) == -1 and corpus(tokens_out=None) == -1 and corpus(offsets_out=None) == -1
    assert corpus(mc=0) == -1 and corpus(mc=128, stride=128) == -1 and corpus(stride=99) == -1
    with pytest.raises(ValueError, match=r"max_content must be in \[1, 127\]"):
        _host(["CCO"], max_content=128)


def test_python_surface():
    """data.scaffold_smiles through the host entry equals the reference; the device-only surfaces raise on a CPU model or corpus before
    any device work: no fallback; top_scaffolds defaults to 0 and is refused without scaffolds=True."""
    import inspect
    from molecular_vae_amd import data as D, mosesvae as MV, train as TR
    v = CR.vocabulary()
    strings = RR.fragment_corpus(12, seed=2) + [w[0] for w in WORKED] + ["CCO", "C[C@H]1CC1", "C("]
    got, status = D.scaffold_smiles(strings, v, device="cpu", return_status=True)
    ref = [SS.scaffold(s) for s in strings]
    assert got == [r[1] for r in ref] and status.tolist() == [r[0] for r in ref]
    assert got[-3:] == ["", "", ""] and status.tolist()[-3:] == [SS.NO_RING, RR.STEREO, 1] and got[12:19] == [w[1] for w in WORKED]
    assert D.scaffold_smiles(strings, v, device="cpu") == got
    with pytest.raises(ValueError, match="at least one string"):
        D.scaffold_smiles([], v, device="cpu")
    torch.manual_seed(0)
    model = MV.VAE(VC.OneHotVocab(list("CNOc(=)1")), dtype=torch.float32)
    ds = D.MosesDeviceDataset(["CCO", "c1ccccc1"], model.vocabulary, device="cpu")
    with pytest.raises(L.MvaeError, match="MI355X only"):
        model.scaffold_smiles(["CCO"])
    with pytest.raises(L.MvaeError, match="MI355X only"):
        ds.scaffold_smiles()
    with pytest.raises(L.MvaeError, match="MI355X only"):
        ds.scaffold_smiles_status
    with pytest.raises(L.MvaeError, match="MI355X only"):
        ds.scaffold_smiles_counts
    assert inspect.signature(TR.moses_generate).parameters["top_scaffolds"].default == 0
    with pytest.raises(ValueError, match="top_scaffolds needs scaffolds=True"):
        TR.moses_generate(model, 4, top_scaffolds=3)
    with pytest.raises(ValueError, match="top_scaffolds supports max_len <= 129"):
        TR.moses_generate(model, 4, max_len=130, scaffolds=True, top_scaffolds=3)
