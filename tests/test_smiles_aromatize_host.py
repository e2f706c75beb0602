"""CPU tests of the aromatic normal form (mvae_smiles_aromatize_rows / _corpus / _host): the host entry (csrc/smiles_aromatize.hip on the
matching of csrc/kekule.hpp and the writer driver of csrc/smiles_writer.hpp, compiled for the CPU) against the reference of
tests/arom_ref.py, byte for byte in tokens, lengths, statuses, info and arom; a hand-stated table of Kekule and aromatic spellings that
must give one row; the rows that must stay Kekule, the refusals and their precedence; what the definition promises on the corpora the
reference is compared on -- the same molecule by the graph and kekule entries, idempotence, invariance under respelling and under the
choice of Kekule structure --; four deliberately broken references that these checks must catch; the edge and argument cases; the
declarations and the compiler's resource remarks."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from molecular_vae_amd import _lib as L, vocab as VC, ops
import arom_ref as AR
import canon_ref as CN
import chem_ref as CR
import kekule_ref as KR
import rewrite_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mvae_smiles_aromatize_rows", "mvae_smiles_aromatize_corpus", "mvae_smiles_aromatize_host")
SEED = 11

# (molecule, Kekule spellings, aromatic spelling, aromatic atoms): stated by hand from the rule of include/mvae.h
TABLE = [
    ("benzene", ["C1=CC=CC=C1"], "c1ccccc1", 6),
    ("pyridine", ["C1=CC=NC=C1"], "c1ccncc1", 6),
    ("pyrrole", ["C1=CNC=C1"], "c1cc[nH]c1", 5),
    ("N-methylpyrrole", ["CN1C=CC=C1"], "Cn1cccc1", 5),
    ("furan", ["C1=COC=C1"], "c1ccoc1", 5),
    ("thiophene", ["C1=CSC=C1"], "c1ccsc1", 5),
    ("thiazole", ["C1=CSC=N1"], "c1cscn1", 5),
    ("imidazole", ["C1=CN=CN1"], "c1cnc[nH]1", 5),
    ("naphthalene", ["C1=CC=C2C=CC=CC2=C1"], "c1ccc2ccccc2c1", 10),
    ("indole", ["C1=CC=C2C(=C1)C=CN2"], "c1ccc2c(c1)cc[nH]2", 9),
    ("biphenyl", ["C1=CC=C(C=C1)C1=CC=CC=C1"], "c1ccc(cc1)c1ccccc1", 12),
    ("o-xylene", ["CC1=C(C)C=CC=C1", "CC1=CC=CC=C1C"], "Cc1ccccc1C", 6),
    ("styrene", ["C=CC1=CC=CC=C1"], "C=Cc1ccccc1", 6),
    ("indene", ["C1C=CC2=CC=CC=C12"], "C1C=Cc2ccccc12", 6),
    ("fluorene", ["C1C2=CC=CC=C2C2=CC=CC=C12"], "C1c2ccccc2-c2ccccc12", 12),
    ("2-pyridone", ["O=C1C=CC=CN1"], "O=c1cccc[nH]1", 6),
    ("uracil", ["O=C1C=CNC(=O)N1"], "O=c1cc[nH]c(=O)[nH]1", 6),
    ("tropone", ["O=C1C=CC=CC=C1"], "O=c1cccccc1", 7),
    ("caffeine", ["CN1C=NC2=C1C(=O)N(C)C(=O)N2C"], "Cn1cnc2c1c(=O)n(C)c(=O)n2C", 9),
    ("pyridinium", ["C[N+]1=CC=CC=C1"], "C[n+]1ccccc1", 6),
    ("pyrylium", ["C1=CC=[O+]C=C1"], "c1cc[o+]cc1", 6),
    ("cyclopentadienyl anion", ["[CH-]1C=CC=C1"], "[cH-]1cccc1", 5),
]
STAY_KEKULE = ["O=C1C=CC(=O)C=C1", "C1=CCC=C1", "C1=CC=C1", "C1=CC=CC=CC=C1", "C=C1C=CC=C1", "O=C1C=CC(=O)N1", "C1=CC2=CC=CC=CC2=C1", "CCO"]
NOT_AROMATIC = ["c1ccc1", "c1ccccccc1", "O=c1ccc(=O)cc1", "c1cc2cccccc2c1", "c1ccpcc1"]
NOT_KEKULE = ["c1cccn1", "c1cccc1"]
EIGHT_RING = "N1C=CC=CNC=C1"                  # 1,4-dihydro-1,4-diazocine: eight candidates with 10 electrons, and no cycle of 5 - 7


def _tables(v):
    return VC.smiles_token_table(v), VC.smiles_chem_table(v), VC.smiles_emit_table(v)


def _host(strings, max_content=127, T=None, T_out=None, v=None, **kw):
    v = CR.vocabulary() if v is None else v
    x = torch.from_numpy(CR.token_rows(strings, v, T))
    out = ops.smiles_aromatize_host(x, *_tables(v), v.bos, v.eos, v.pad, max_content, T_out, **kw)
    return tuple(t.numpy() for t in out)


def _decode(out, out_len, v=None):
    v = CR.vocabulary() if v is None else v
    return ["".join(v.i2c[int(i)] for i in row[1:n - 1]) for row, n in zip(out, out_len)]


def _want(refs, v, T_out):
    """The reference's (status, string, info, arom) per row as the arrays the entries write."""
    B = len(refs)
    rows, lens = np.full((B, T_out), v.pad, np.int64), np.zeros(B, np.int32)
    status, info, arom = np.zeros(B, np.int32), np.zeros((B, 4), np.int32), np.full((B, 128), 0xFF, np.uint8)
    for b, (st, s, inf, ar) in enumerate(refs):
        ids = v.string2ids(s, add_bos=True, add_eos=True)
        rows[b, :len(ids)] = ids
        lens[b], status[b] = len(ids), st
        if inf is not None:
            info[b], arom[b, :len(ar)] = inf, ar
    return rows, lens, status, info, arom


def _equal(got, want):
    return [name for g, w, name in zip(got, want, ("out", "out_len", "status", "info", "arom")) if not np.array_equal(g, w)]


_CASES = {}


def corpus():
    """The rows the entry is compared on: kekule_ref's ring systems and edge rows, rewrite_ref's hand rows and fragment corpus, the cage
    rows, a 1000-row slice of the mutation corpus, and the hand table above.  Distinct, at most 127 characters, none empty."""
    if "rows" not in _CASES:
        rows = (KR.ring_system_corpus() + [r[0] for r in KR.edge_rows()] + RR.HAND_ROWS + RR.fragment_corpus(300, seed=1) + CN.CAGES
                + CR.mutation_corpus()[::4][:1000] + [s for _, ks, a, _ in TABLE for s in ks + [a]] + STAY_KEKULE + NOT_AROMATIC + NOT_KEKULE + [EIGHT_RING])
        _CASES["rows"] = [s for s in dict.fromkeys(rows) if 0 < len(s) <= 127]
    return _CASES["rows"]


def cases():
    """(rows, the reference's result per row, the host entry's outputs): computed once per process and shared; callers leave it unchanged."""
    if "c" not in _CASES:
        rows = corpus()
        _CASES["c"] = (rows, [AR.aromatize(s) for s in rows], _host(rows, T=131))
    return _CASES["c"]


def written():
    """the indices of the status-0 rows"""
    return [i for i, r in enumerate(cases()[1]) if r[0] == 0]


def test_entries_are_declared_bound_and_exported_at_abi_12():
    text = open(os.path.join(ROOT, "include", "mvae.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", header).group(1)) == 12 == L.ABI_VERSION
    lib = L.load()
    for name, canon in zip(ENTRIES, ("mvae_smiles_canon_rows", "mvae_smiles_canon_corpus", "mvae_smiles_canon_host")):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
        assert L.SIGNATURES[name] == L.SIGNATURES[canon]               # the canon entries' arguments, arom in the place of rank
    assert int(re.search(r"#define\s+MVAE_SMILES_NOT_AROMATIC\s+(\d+)", header).group(1)) == ops.SMILES_STATUS_NOT_AROMATIC == 17
    assert len(ops.AROMATIZE_STATUS_NAMES) == 18 and ops.AROMATIZE_STATUS_NAMES[17] == "not_aromatic" and ops.AROMATIZE_STATUS_NAMES[7] == "kekule"
    assert int(re.search(r"#define\s+MVAE_AROMATIZE_INFO\s+(\d+)", header).group(1)) == len(ops.AROMATIZE_INFO) == 4
    assert int(re.search(r"#define\s+MVAE_AROMATIZE_COUNTS\s+(\d+)", header).group(1)) == ops.AROMATIZE_COUNTS == 32
    assert "Aromatic normal form" in text and "What this is NOT: the rule is this library's own" in text
    build = open(os.path.join(ROOT, "molecular-vae_amd", "csrc", "build.sh")).read()
    assert build.count(" smiles_aromatize fragment_smiles ") == 2 and "build/smiles_aromatize.o build/fragment_smiles.o" in build
    assert "build/tune/smiles_aromatize.o" in build and "kekule.hpp -nt build/$f.o" in build
    # the matching, the ranks and the writer are shared, not copied
    csrc = os.path.join(ROOT, "molecular-vae_amd", "csrc")
    src = open(os.path.join(csrc, "smiles_aromatize.hip")).read()
    assert all(f'#include "{h}"' in src for h in ("kekule.hpp", "smiles_canon.hpp", "smiles_writer.hpp"))
    assert "common_base" not in src and "EM_LPAR" not in src and "run_end" not in src
    kek = open(os.path.join(csrc, "kekule.hip")).read()
    assert '#include "kekule.hpp"' in kek and "common_base" not in kek and "struct Forest" not in kek


def test_new_kernels_use_no_scratch(tmp_path):
    """The compiler's resource remarks for the two kernels of smiles_aromatize.hip: scratch 0, no spills, and the LDS per block that
    include/mvae.h states, at most 80 KiB so that two blocks fit a CU.  The build leaves the remarks in
    csrc/build/smiles_aromatize.usage.txt; on a tree whose library was built another way the test compiles the device code itself."""
    csrc = os.path.join(ROOT, "molecular-vae_amd", "csrc")
    usage = os.path.join(csrc, "build", "smiles_aromatize.usage.txt")
    sources = ("smiles_aromatize.hip", "kekule.hpp", "smiles_canon.hpp", "smiles_writer.hpp", "smiles_rounds.hpp", "smiles_graph.hpp",
               "smiles_syntax.hpp", "common.hpp", "../../include/mvae.h")
    if os.path.exists(usage) and os.path.getmtime(usage) >= max(os.path.getmtime(os.path.join(csrc, f)) for f in sources):
        text = open(usage, errors="replace").read()
    else:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                              "-c", os.path.join(csrc, "smiles_aromatize.hip"), "-o", str(tmp_path / "smiles_aromatize.dev.o")],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert run.returncode == 0, run.stderr[-2000:]
        text = run.stderr
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 2 and all(any(k in n for n in names) for k in ("smiles_aromatize_rows_kernel", "smiles_aromatize_corpus_kernel")), names
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 2
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 2 and re.findall(r"SGPRs Spill: (\d+)", text) == ["0"] * 2
    header = open(os.path.join(ROOT, "include", "mvae.h")).read()
    stated = int(re.search(r"#define\s+MVAE_AROMATIZE_LDS_BYTES\s+(\d+)", header).group(1))
    assert list(map(int, re.findall(r"LDS Size \[bytes/block\]: (\d+)", text))) == [stated] * 2
    assert f"MVAE_AROMATIZE_LDS_BYTES = {stated} B" in header and stated <= 81920
    assert all(int(n) <= 128 for n in re.findall(r" VGPRs: (\d+)", text))


def test_hand_table_kekule_and_aromatic_spellings_give_one_row():
    """Every row of the table is status 0 with the stated number of aromatic atoms in info[1] and in arom, and all its spellings give
    the identical output row, which is the reference's."""
    for name, kekules, aromatic, n_arom in TABLE:
        rows = kekules + [aromatic]
        out, out_len, status, info, arom = _host(rows, T_out=40)
        assert not status.any(), (name, status)
        assert (info[:, 1] == n_arom).all() and ((arom == 1).sum(1) == n_arom).all(), (name, info)
        assert (out == out[0]).all() and (out_len == out_len[0]).all(), (name, _decode(out, out_len))
        atoms = info[0, 0]
        assert (info[:, 0] == atoms).all() and ((arom <= 1).sum(1) == atoms).all() and (arom[:, atoms:] == 0xFF).all()
        # an aromatic spelling has nothing raised and nothing lowered; a Kekule spelling has every aromatic atom raised
        assert info[-1, 2:].tolist() == [0, 0] and (info[:-1, 2] == n_arom).all() and (info[:-1, 3] >= 1).all(), (name, info)
        assert AR.aromatize(aromatic)[1] == _decode(out, out_len)[0], name
    v = CR.vocabulary()
    spelled = dict(zip([t[0] for t in TABLE], _decode(*_host([t[2] for t in TABLE])[:2], v)))
    assert spelled["pyrrole"] == "c1cc[nH]c1" and spelled["benzene"] == "c1ccccc1" and "[nH]" in spelled["indole"]
    assert "=" in spelled["indene"] and spelled["indene"].count("c") == 6                 # the five-ring double bond stays
    assert spelled["styrene"].count("C=C") == 1 and "=O" in spelled["tropone"] and spelled["caffeine"].count("=O") == 2


def test_rows_without_aromatic_atoms_come_out_as_canon_writes_them():
    v = CR.vocabulary()
    out, out_len, status, info, arom = _host(STAY_KEKULE, T_out=40)
    x = torch.from_numpy(CR.token_rows(STAY_KEKULE, v))
    canon = ops.smiles_canon_host(x, *_tables(v), v.bos, v.eos, v.pad, 127, 40, info=False, rank=False)
    assert not status.any() and not info[:, 1:].any() and not (arom == 1).any()
    assert np.array_equal(out, canon[0].numpy()) and np.array_equal(out_len, canon[1].numpy())


def test_every_refusal_is_copied_through_unchanged_in_its_precedence():
    """NOT_AROMATIC and KEKULE rows; one row of every walk status; two stereo rows; a stereo row that would not kekulise (STEREO wins),
    a row that neither kekulises nor is aromatic by the rule (KEKULE wins); LONG through a small max_content; NO_TOKEN through a
    vocabulary without the token the normal form needs.  info and arom are there exactly where the output graph was made."""
    v = CR.vocabulary()
    rejected = [s for s, st, _ in CR.REJECTED if st != CR.OK and s] + ["C" * 128]
    stereo = ["C[C@H](N)O", "F/C=C/F"]
    mixed = ["F/C=C/c1cccn1", "c1cccc1c1ccc1", "C1=CC=CC=C1c1ccc1"]
    rows = rejected + stereo + NOT_AROMATIC + NOT_KEKULE + mixed
    refs = [AR.aromatize(s) for s in rows]
    k = len(rejected)
    assert {r[0] for r in refs[:k]} == {1, 2, 3, 4, 5, 6} and [r[0] for r in refs[k:k + 2]] == [RR.STEREO] * 2
    assert [r[0] for r in refs[k + 2:k + 9]] == [17] * 5 + [7] * 2 and [r[0] for r in refs[k + 9:]] == [RR.STEREO, 7, 17]
    assert all(r[2] is None and r[1] == s for r, s in zip(refs, rows))
    got = _host(rows, T=140)
    wrong = _equal(got, _want(refs, v, 140))
    assert not wrong, wrong
    assert (got[0] == CR.token_rows(rows, v, 140)[:, :got[0].shape[1]])[:-1].all() and not got[3].any() and (got[4] == 0xFF).all()
    # LONG: pyrrole's normal form takes 10 tokens where its Kekule spelling takes 9
    long_rows = ["N1C=CC=C1", "C1=COC=C1", "C1=CC=CC=C1"]
    refs = [AR.aromatize(s, max_content=9) for s in long_rows]
    assert [r[0] for r in refs] == [RR.LONG, 0, 0] and refs[0][2] == [5, 5, 5, 2] and refs[0][1] == "N1C=CC=C1"
    got = _host(long_rows, max_content=9)
    wrong = _equal(got, _want(refs, v, got[0].shape[1]))
    assert not wrong, wrong
    # NO_TOKEN: the vocabulary cannot write a lower-case c
    have = set(CR.ALPHABET) - {"c"}
    small = VC.OneHotVocab(have)
    refs = [AR.aromatize(s, have=have) for s in ("C1=CC=CC=C1", "C1=CCC=C1")]
    assert [r[0] for r in refs] == [RR.NO_TOKEN, 0] and refs[0][1] == "C1=CC=CC=C1" and refs[0][2] == [6, 6, 6, 3]
    wrong = _equal(_host(["C1=CC=CC=C1", "C1=CCC=C1"], v=small, T_out=129), _want(refs, small, 129))
    assert not wrong, wrong


def test_host_entry_equals_the_reference_byte_for_byte():
    """Tokens, lengths, statuses, info and arom of every row of the corpora.  The input is not degenerate (asserted on the reference
    alone)."""
    rows, refs, got = cases()
    v = CR.vocabulary()
    by_status = {st: sum(r[0] == st for r in refs) for st in sorted({r[0] for r in refs})}
    raised = sum(r[0] == 0 and r[2][2] > 0 for r in refs)
    partly = sum(r[0] == 0 and 0 < r[2][1] < r[2][0] for r in refs)
    print("rows:", len(rows), "by status:", by_status, "with atoms raised:", raised, "partly aromatic:", partly,
          "distinct normal forms:", len({r[1] for r in refs if r[0] == 0}))
    assert by_status[0] >= 600 and by_status.get(7, 0) >= 300 and by_status.get(17, 0) >= 300 and raised >= 20 and partly >= 200
    wrong = _equal(got, _want(refs, v, 131))
    if wrong:
        st = _want(refs, v, 131)
        bad = [i for i in range(len(rows)) if any(not np.array_equal(g[i], w[i]) for g, w in zip(got, st))]
        print([(rows[i], refs[i][:3], int(got[2][i]), _decode(got[0][i:i + 1], got[1][i:i + 1], v), got[3][i].tolist()) for i in bad[:5]])
    assert not wrong, wrong


def test_broken_references_are_told_from_the_right_one():
    """Each deliberately wrong variant of the reference disagrees with the host entry on the hand table or the corpora."""
    rows, refs, got = cases()
    v = CR.vocabulary()
    mine = _decode(got[0], got[1], v)
    table = [s for _, ks, a, _ in TABLE for s in ks + [a]] + STAY_KEKULE + [EIGHT_RING]
    probe = table + [rows[i] for i in written()[::3]]
    entry = dict(zip(rows, zip(got[2].tolist(), mine)))
    for broken in AR.BROKEN:
        caught = [s for s in probe if AR.aromatize(s, broken=broken)[:2] != entry[s]]
        print(broken, "caught on", len(caught), caught[:3])
        assert caught, broken
    assert AR.aromatize(EIGHT_RING)[2] == [8, 0, 0, 0] and AR.aromatize(EIGHT_RING, broken="eight_rings")[2] == [8, 8, 8, 3]
    assert AR.aromatize("N1C=CC=C1", broken="no_nh")[1] == "c1ccnc1"
    assert AR.aromatize("O=C1C=CC=CN1", broken="no_c_o")[2][1] == 0
    assert AR.aromatize("C1=CC=C2C=CC=CC2=C1", broken="inside_doubles")[2][1] == 6


def test_normal_forms_are_the_same_molecule_and_kekulise():
    """(a) the graph entry, which knows nothing of the new code, gives the output status 0 and the input's formula (hydrogens are
    conserved), heavy atoms, bonds and rings; (b) the kekule entry gives it status 0."""
    rows, refs, got = cases()
    v = CR.vocabulary()
    tok, chem = VC.smiles_token_table(v), VC.smiles_chem_table(v)
    idx = written()
    before = torch.from_numpy(CR.token_rows([rows[i] for i in idx], v))
    after = torch.from_numpy(got[0][idx])
    g0, g1 = ops.smiles_graph_host(before, tok, chem, v.eos), ops.smiles_graph_host(after, tok, chem, v.eos)
    assert not g0[0].any() and not g1[0].any()
    assert torch.equal(g0[3], g1[3]) and torch.equal(g0[2][:, :3], g1[2][:, :3]) and torch.equal(g0[2][:, 5:], g1[2][:, 5:])
    assert (g1[2][:, 4].numpy() == got[3][idx, 1]).all()               # the aromatic atoms the walk counts in the output are info[1]
    assert not ops.smiles_kekule_host(after, tok, chem, v.eos, mate=False)[0].any()


def test_normal_forms_are_fixed_points():
    """(c) aromatize(out) == out, with nothing raised and nothing lowered"""
    rows, refs, got = cases()
    idx = written()
    v = CR.vocabulary()
    x = torch.from_numpy(got[0][idx])
    again = ops.smiles_aromatize_host(x, *_tables(v), v.bos, v.eos, v.pad, 127, 131)
    assert not again[2].any() and np.array_equal(again[0].numpy(), got[0][idx]) and np.array_equal(again[1].numpy(), got[1][idx])
    assert not again[3][:, 2:].any() and np.array_equal(again[3][:, :2].numpy(), got[3][idx, :2])


def test_respellings_give_one_normal_form():
    """(d) four smiles_rewrite_host draws of every status-0 row give the row's normal form, wherever smiles_canon_host itself is
    invariant under those draws (the canon section's caveat about ties carries over): those left out are at most 1 % of the rows."""
    rows, refs, got = cases()
    idx = written()
    v = CR.vocabulary()
    tabs = _tables(v)
    x = torch.from_numpy(CR.token_rows([rows[i] for i in idx], v, 131))
    canon0 = ops.smiles_canon_host(x, *tabs, v.bos, v.eos, v.pad, 127, 131, info=False, rank=False)
    same_canon, same_normal, respelled = np.ones(len(idx), bool), np.ones(len(idx), bool), np.ones(len(idx), bool)
    for d in range(4):
        draw = ops.draw_words(torch.arange(len(idx)) * 4 + d)
        y, _, st = ops.smiles_rewrite_host(x, *tabs, v.bos, v.eos, v.pad, SEED, draw, 127, 131)
        ok = (st == 0).numpy()
        respelled &= ok
        c = ops.smiles_canon_host(y, *tabs, v.bos, v.eos, v.pad, 127, 131, info=False, rank=False)
        a = ops.smiles_aromatize_host(y, *tabs, v.bos, v.eos, v.pad, 127, 131, info=False, arom=False)
        same_canon &= ~ok | ((c[0] == canon0[0]).all(1) & (c[2] == 0)).numpy()
        same_normal &= ~ok | ((a[0].numpy() == got[0][idx]).all(1) & (a[2] == 0).numpy())
    enter = respelled & same_canon
    left_out = int((respelled & ~same_canon).sum())
    print("status-0 rows:", len(idx), "respelled four times:", int(respelled.sum()), "canon not invariant:", left_out, "enter:", int(enter.sum()))
    assert left_out <= len(idx) // 100 and enter.sum() >= 500
    bad = np.nonzero(enter & ~same_normal)[0]
    assert bad.size == 0, [rows[idx[k]] for k in bad[:5]]


def test_kekule_spellings_give_the_normal_form_of_the_row():
    """(e) every status-0 row with an aromatic atom in the input, written in upper case with '=' on the bonds of the kekule entry's
    matching and respelled from a random root, has the row's normal form."""
    rows, refs, got = cases()
    v = CR.vocabulary()
    idx = [i for i in written() if any(ch in rows[i] for ch in "cnos")]
    x = torch.from_numpy(CR.token_rows([rows[i] for i in idx], v))
    status, _, mate = ops.smiles_kekule_host(x, VC.smiles_token_table(v), VC.smiles_chem_table(v), v.eos)
    assert not status.any()
    spelled = [AR.kekule_spelling(rows[i], mate[k].tolist(), SEED, k) for k, i in enumerate(idx)]
    keep = [k for k, s in enumerate(spelled) if s is not None and len(s) <= 127]
    print("rows with aromatic atoms:", len(idx), "Kekule spellings written:", len(keep))
    assert len(keep) >= 200
    assert all(not any(ch in spelled[k] for ch in "cnos") for k in keep)
    out, out_len, st, info, _ = _host([spelled[k] for k in keep], T=131)
    assert not st.any()
    rows_of = [idx[k] for k in keep]
    same = (out == got[0][rows_of]).all(1) & (out_len == got[1][rows_of])
    assert same.all(), [(rows[rows_of[k]], spelled[keep[k]]) for k in np.nonzero(~same)[0][:3]]
    assert (info[:, 1] == got[3][rows_of, 1]).all() and (info[:, 2] == info[:, 1]).all()


def test_edge_rows_strided_input_and_prefilled_outputs():
    """A strided view (x_ld > T), rows without <eos> and with ids outside the vocabulary, T_out smaller than needed; every element of
    prefilled outputs is written and info / arom may be left out."""
    v = CR.vocabulary()
    tabs = _tables(v)
    x = torch.from_numpy(CR.token_rows(["c1cccn1", "c1ccccc1", "C=F", "c1ccncc1", "N1C=CC=C1"], v, T=12))
    x[0, 8] = v.pad                                                # no <eos>
    x[1, 3] = -1
    x[3, 2] = len(v)
    wide = torch.full((5, 40), v.eos, dtype=torch.long)
    wide[:, :12] = x
    pre = (torch.full((5, 20), 0x7f7f7f7f, dtype=torch.int64), torch.full((5,), 0x7f7f7f7f, dtype=torch.int32),
           torch.full((5,), 0x7f7f7f7f, dtype=torch.int32), torch.full((5, 4), 0x7f7f7f7f, dtype=torch.int32),
           torch.full((5, 128), 0x7f, dtype=torch.uint8))
    got = ops.smiles_aromatize_host(wide[:, :12], *tabs, v.bos, v.eos, v.pad, 127, 20, *pre)
    assert got[2].tolist() == [1, 1, 2, 1, 0] and got[1].tolist() == [12, 10, 5, 10, 12]
    assert (got[0][:4, :12] == x[:4]).all() and (got[0][:, 12:] == v.pad).all()
    assert _decode(got[0][4:].numpy(), got[1][4:].numpy(), v) == ["c1cc[nH]c1"]
    assert got[3].tolist() == [[0] * 4] * 4 + [[5, 5, 5, 2]] and (got[4][:4] == 0xFF).all()
    assert got[4][4].tolist() == [1] * 5 + [0xFF] * 123
    fresh = ops.smiles_aromatize_host(wide[:, :12], *tabs, v.bos, v.eos, v.pad, 127, 20)
    assert all(torch.equal(a, b) for a, b in zip(fresh, got))
    cut = ops.smiles_aromatize_host(wide[:, :12], *tabs, v.bos, v.eos, v.pad, 127, 4, info=False, arom=False)
    assert torch.equal(cut[0], got[0][:, :4]) and torch.equal(cut[1], got[1]) and torch.equal(cut[2], got[2]) and cut[3] is None and cut[4] is None


def test_entries_refuse_bad_arguments_before_launching():
    """Everything below returns before any HIP call (no device needed)."""
    lib = L.load()
    fake = ctypes.c_void_p(256)                                  # never dereferenced: every call below is refused first

    def rows(name, B=4, T=8, V=29, x=fake, ld=8, tok=fake, chem=fake, emit=fake, bos=0, eos=1, pad=2, mc=127, T_out=129, out=fake,
             out_len=fake, status=fake):
        tail = (None, None, None, None) if name == ENTRIES[0] else (None, None)
        return getattr(lib, name)(B, T, V, x, ld, tok, chem, emit, bos, eos, pad, mc, T_out, out, out_len, status, *tail)
    for name in (ENTRIES[0], ENTRIES[2]):
        assert rows(name, B=0) == -1 and rows(name, T=0, ld=0) == -1 and rows(name, V=0, eos=0) == -1 and rows(name, V=65) == -3
        assert rows(name, x=None) == -1 and rows(name, tok=None) == -1 and rows(name, chem=None) == -1 and rows(name, status=None) == -1
        assert rows(name, emit=None) == -1 and rows(name, out=None) == -1 and rows(name, out_len=None) == -1 and rows(name, ld=7) == -1
        assert rows(name, eos=29) == -1 and rows(name, eos=-1) == -1 and rows(name, mc=0) == -1 and rows(name, mc=128) == -1
        assert rows(name, T_out=1) == -1 and rows(name, bos=-1) == -1 and rows(name, pad=65536) == -1 and rows(name, V=65, out=None) == -3

    def corpus_(tokens=fake, offsets=fake, N=100, rows=fake, B=4, V=29, tok=fake, chem=fake, emit=fake, mc=100, stride=100, tokens_out=fake,
                offsets_out=fake, status=fake):
        return lib.mvae_smiles_aromatize_corpus(tokens, offsets, N, rows, B, V, tok, chem, emit, mc, stride, tokens_out, offsets_out, status,
                                                None, None, None, None, None)
    assert corpus_(N=0) == -1 and corpus_(B=0) == -1 and corpus_(V=0) == -1 and corpus_(V=65) == -3 and corpus_(rows=None) == -1
    assert corpus_(tokens=None) == -1 and corpus_(offsets=None) == -1 and corpus_(tok=None) == -1 and corpus_(chem=None) == -1
    assert corpus_(emit=None) == -1 and corpus_(status=None) == -1 and corpus_(tokens_out=None) == -1 and corpus_(offsets_out=None) == -1
    assert corpus_(mc=0) == -1 and corpus_(mc=128, stride=128) == -1 and corpus_(stride=99) == -1
    with pytest.raises(ValueError, match=r"max_content must be in \[1, 127\]"):
        _host(["CCO"], max_content=128)


def test_python_surface():
    """data.normal_smiles through the host entry equals the reference; the device-only surfaces raise on a CPU model or corpus before any
    device work: no fallback; moses_generate refuses what normal=True cannot take before any device work."""
    import inspect
    from molecular_vae_amd import data as D, mosesvae as MV, train as TR
    v = CR.vocabulary()
    strings = RR.fragment_corpus(12, seed=2) + ["C1=CC=CC=C1", "c1ccccc1", "C[C@H](N)O", "c1ccc1", "C("]
    got, status = D.normal_smiles(strings, v, device="cpu", return_status=True)
    ref = [AR.aromatize(s) for s in strings]
    assert got == [r[1] for r in ref] and status.tolist() == [r[0] for r in ref]
    assert got[-5] == got[-4] == "c1ccccc1" and status[-3] == RR.STEREO and status[-2] == 17 and got[-1] == "C("
    with pytest.raises(ValueError, match="at least one string"):
        D.normal_smiles([], v, device="cpu")
    torch.manual_seed(0)
    model = MV.VAE(VC.OneHotVocab(list("CNOc(=)1")), dtype=torch.float32)
    ds = D.MosesDeviceDataset(["CCO", "c1ccccc1"], model.vocabulary, device="cpu")
    with pytest.raises(L.MvaeError, match="MI355X only"):
        model.normal_form(["CCO"])
    with pytest.raises(L.MvaeError, match="MI355X only"):
        ds.normal_form()
    with pytest.raises(L.MvaeError, match="MI355X only"):
        ds.normal_status()
    with pytest.raises(L.MvaeError, match="MI355X only"):
        ds.normal_counts()
    assert inspect.signature(TR.moses_generate).parameters["normal"].default is False
    with pytest.raises(ValueError, match="normal=True supports max_len <= 129"):
        TR.moses_generate(model, 4, max_len=130, normal=True)
    big = MV.VAE(VC.OneHotVocab([chr(0x100 + i) for i in range(70)]), dtype=torch.float32)
    with pytest.raises(ValueError, match="normal=True supports at most 64 ids"):
        TR.moses_generate(big, 4, normal=True)
