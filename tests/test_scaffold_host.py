"""CPU tests of the scaffold surface (mvae_smiles_scaffold_rows / _corpus / _host, ops.key_histogram / histogram_cosine /
scaffold_split_rows, VAE.scaffolds, MosesDeviceDataset.scaffolds / scaffold_histogram / rows_with_scaffold / scaffold_split,
moses_generate(scaffolds=)): the host entry (the walk of csrc/smiles_graph.hpp with the recorder of csrc/smiles_rounds.hpp and the sets
and rounds of csrc/scaffold.hip, compiled for the CPU) against the reference of tests/scaffold_ref.py on the mutation corpus, hand-stated
scaffolds, invariance under re-spelling, the lists of graphs the keys are known to separate, the histogram helpers against
collections.Counter, the argument checks of the new entries (refused before anything is launched), the ABI, and the compiler's resource
remarks for the new kernels."""
import collections
import ctypes
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import molecular_vae_amd as mv
from molecular_vae_amd import _lib as L, data as D, mosesvae as MV, vocab as VC, ops
import chem_ref as CR
import scaffold_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mvae_smiles_scaffold_rows", "mvae_smiles_scaffold_corpus", "mvae_smiles_scaffold_host")

# scaffolds the scaffold keys are known to tell apart, pairwise
SCAFFOLDS = {
    "decalin": "C1CCC2CCCCC2C1", "bicyclopentyl": "C1CCCC1C1CCCC1", "o-terphenyl": "c1ccccc1c1ccccc1c1ccccc1",
    "m-terphenyl": "c1ccccc1c1cccc(c1)c1ccccc1", "p-terphenyl": "c1ccccc1c1ccc(cc1)c1ccccc1", "biphenyl": "c1ccccc1c1ccccc1",
    "diphenylmethane": "c1ccccc1Cc1ccccc1", "bibenzyl": "c1ccccc1CCc1ccccc1", "pyridine": "c1ccncc1", "benzene": "c1ccccc1",
    "cyclohexane": "C1CCCCC1", "cyclohexene": "C1=CCCCC1", "cyclopentane": "C1CCCC1", "indole": "c1ccc2[nH]ccc2c1",
    "benzofuran": "c1ccc2occc2c1", "benzimidazole": "c1ccc2[nH]cnc2c1", "naphthalene": "c1ccc2ccccc2c1", "azulene-like 5-7": "c1ccc2cccc2cc1",
    "2-phenylpyridine": "c1ccccc1c1ccccn1", "3-phenylpyridine": "c1ccccc1c1cccnc1", "4-phenylpyridine": "c1ccccc1c1ccncc1",
    "cyclohexanone": "O=C1CCCCC1", "spiro[5.5]": "C1CCCCC12CCCCC2", "spiro[4.5]": "C1CCCC12CCCCC2", "bicyclobutane": "C12CC1C2",
    "benzophenone": "O=C(c1ccccc1)c1ccccc1", "diphenyl sulfone": "c1ccccc1S(=O)(=O)c1ccccc1", "diphenyl sulfide": "c1ccccc1Sc1ccccc1",
    "tetralin": "c1ccc2CCCCc2c1", "indane": "c1ccc2CCCc2c1", "cubane": "C12C3C4C1C5C2C3C45", "thiophene": "c1ccsc1", "furan": "c1ccoc1",
    "pyrrole": "c1cc[nH]c1",
}


def _host(strings, T=None):
    v = CR.vocabulary()
    x = torch.from_numpy(CR.token_rows(strings, v, T))
    return tuple(t.numpy() for t in ops.smiles_scaffold_host(x, VC.smiles_token_table(v), VC.smiles_chem_table(v), v.eos))


def _atoms(mask_row):
    """The atom set of one mask row."""
    return {a for a in range(128) if (int(mask_row[a >> 6]) >> (a & 63)) & 1}


def test_entries_are_declared_bound_and_exported_at_abi_12():
    text = open(os.path.join(ROOT, "include", "mvae.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", header).group(1)) == 12 == L.ABI_VERSION
    lib = L.load()
    assert lib.mvae_abi_version() == 12
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert len(L.SIGNATURES[ENTRIES[0]][1]) == len(L.SIGNATURES[ENTRIES[2]][1]) + 1 == 13       # the host entry: no stream
    assert len(L.SIGNATURES[ENTRIES[1]][1]) == 11
    assert re.search(r"#define\s+MVAE_GRAPH_KEY_ROUNDS\s+8\b", header) and ops.GRAPH_KEY_ROUNDS == 8 == SR.ROUNDS
    assert "Murcko scaffold" in text and "Graph key" in text and "NOT rdkit's MurckoScaffold" in text and "nothing is kekulised" in text
    for fn in (ops.smiles_scaffold_rows, ops.smiles_scaffold_corpus, ops.smiles_scaffold_host, ops.key_histogram, ops.histogram_cosine,
               MV.VAE.scaffolds, D.MosesDeviceDataset.scaffolds, D.MosesDeviceDataset.scaffold_histogram,
               D.MosesDeviceDataset.rows_with_scaffold, D.MosesDeviceDataset.scaffold_split):
        assert callable(fn)
    assert inspect.signature(mv.moses_generate).parameters["scaffolds"].default is False
    build = open(os.path.join(ROOT, "molecular-vae_amd", "csrc", "build.sh")).read()
    assert build.count("moses_decode scaffold fingerprint smiles_graph elementwise") == 2
    assert "build/scaffold.o build/fingerprint.o build/smiles_graph.o" in build
    assert "build/tune/scaffold.o build/tune/fingerprint.o build/tune/smiles_graph.o" in build
    assert "smiles_rounds.hpp -nt build/$f.o" in build                                  # the shared header is part of the staleness test
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        body = open(os.path.join(ROOT, doc)).read()
        assert "not rdkit's MurckoScaffold" in body, doc


def test_new_kernels_use_no_scratch(tmp_path):
    """The compiler's resource remarks for the two kernels of scaffold.hip: scratch 0, no spills (nothing indexed at run time is a
    private array), and the LDS per block include/mvae.h states, at most 160 KiB.  The build leaves the remarks in
    csrc/build/scaffold.usage.txt; on a tree whose library was built another way the test compiles the device code itself."""
    csrc = os.path.join(ROOT, "molecular-vae_amd", "csrc")
    usage = os.path.join(csrc, "build", "scaffold.usage.txt")
    sources = ("scaffold.hip", "smiles_rounds.hpp", "smiles_graph.hpp", "smiles_syntax.hpp")
    if os.path.exists(usage) and os.path.getmtime(usage) >= max(os.path.getmtime(os.path.join(csrc, f)) for f in sources):
        text = open(usage, errors="replace").read()
    else:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                              "-c", os.path.join(csrc, "scaffold.hip"), "-o", str(tmp_path / "scaffold.dev.o")],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert run.returncode == 0, run.stderr[-2000:]
        text = run.stderr
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 2 and all(any(k in n for n in names) for k in ("rows_kernelIN3scf8ScaffoldE", "corpus_kernelIN3scf8ScaffoldE")), names
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 2
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 2 and re.findall(r"SGPRs Spill: (\d+)", text) == ["0"] * 2
    header = open(os.path.join(ROOT, "include", "mvae.h")).read()
    stated = int(re.search(r"#define\s+MVAE_SCAFFOLD_LDS_BYTES\s+(\d+)", header).group(1))
    assert list(map(int, re.findall(r"LDS Size \[bytes/block\]: (\d+)", text))) == [stated] * 2 and stated <= 160 * 1024
    assert f"{stated} B" in header
    assert all(int(v) <= 128 for v in re.findall(r" VGPRs: (\d+)", text))


def test_host_entry_equals_the_reference_on_the_mutation_corpus():
    """All four outputs, every one of the 4 250 rows; rows that are not ok are zero.  The input is not degenerate: at least 800 rows
    with status 0, at least 500 of them with a scaffold, at least 200 distinct scaffold keys and 600 distinct molecule keys (asserted on
    the reference alone)."""
    strings, want = SR.corpus_expected()
    ok = want[0] == 0
    has = want[3][:, 1] != 0
    n_scaf, n_mol = len(set(want[3][has, 1].tolist())), len(set(want[3][ok, 0].tolist()))
    print("rows:", len(strings), "status 0:", int(ok.sum()), "with a scaffold:", int(has.sum()), "distinct scaffold keys:", n_scaf,
          "distinct molecule keys:", n_mol, "linker rows:", int((want[2][:, 2] > 0).sum()), "exo rows:", int((want[2][:, 3] > 0).sum()))
    assert ok.sum() >= 800 and has.sum() >= 500 and n_scaf >= 200 and n_mol >= 600
    assert (want[2][:, 3] > 0).sum() >= 50                            # no row of this corpus has a linker: the next test is about those
    assert (want[3][ok, 0] != 0).all() and not has[~ok].any()
    got = _host(strings)
    for g, w, name in zip(got, want, ("status", "mask", "desc", "key")):
        wrong = np.nonzero((g != w).reshape(len(strings), -1).any(1))[0]
        assert wrong.size == 0, (name, [(strings[i], g[i].tolist(), w[i].tolist()) for i in wrong[:3]])
    for g in got[1:]:
        assert not g[~ok].any()
    v = CR.vocabulary()
    graph_status = ops.smiles_graph_host(torch.from_numpy(CR.token_rows(strings, v)), VC.smiles_token_table(v), VC.smiles_chem_table(v), v.eos)[0]
    assert (graph_status.numpy() == got[0]).all()


LINKED = ["c1ccccc1CC(=O)Cc1ccccc1", "c1ccccc1S(=O)(=O)c1ccccc1", "C1CC1CCC(C)CC1CC1", "O=C(c1ccccc1)c1ccccc1", "c1ccccc1CCc1ccccc1",
          "C1CC1C(CC)(C1CC1)CC1CCC1", "CC(C)(C)c1ccc(cc1)C(=O)NCCc1ccc(O)cc1", "C1CCCCC1=CC=C1CCCC1", "c1ccccc1OC(C)COc1ccncc1", "O=S(=O)(N1CCCC1)c1ccc(F)cc1",
          "C1CC1C(C2CC2)(C3CC3)CCCC", "c1ccccc1C(=O)C(=O)c1ccccc1", "N(C1CC1)(C1CC1)CCN(C)C", "C(C1CC1)(C1CC1)(C1CC1)C1CC1", "CCC(CC1CC1)CC(C)CC1CCC1CC"]


def test_host_entry_equals_the_reference_on_linkers_from_every_root():
    """Molecules with linkers, branched linkers and exocyclic double bonds, each in its own spelling and in eight re-spellings from random
    roots, so that rings, linkers and substituents hang off the spanning tree in every arrangement: all four outputs equal the
    reference's, which finds Core by the component criterion."""
    rng = np.random.RandomState(23)
    strings = list(LINKED) + [SR.rewrite(s, rng)[0] for s in LINKED for _ in range(8)]
    want = SR.expected(strings)
    print("rows:", len(strings), "distinct strings:", len(set(strings)), "with linker atoms:", int((want[2][:, 2] > 0).sum()),
          "with exo atoms:", int((want[2][:, 3] > 0).sum()))
    assert (want[0] == 0).all() and (want[2][:, 2] > 0).sum() >= 100 and (want[2][:, 3] > 0).sum() >= 40 and len(set(strings)) >= 100
    got = _host(strings)
    for g, w, name in zip(got, want, ("status", "mask", "desc", "key")):
        wrong = np.nonzero((g != w).reshape(len(strings), -1).any(1))[0]
        assert wrong.size == 0, (name, [(strings[i], g[i].tolist(), w[i].tolist()) for i in wrong[:3]])
    for i in range(len(LINKED)):                                      # and a re-spelling keeps both keys and the counts
        rows = [i] + list(range(len(LINKED) + 8 * i, len(LINKED) + 8 * i + 8))
        assert (got[3][rows] == got[3][i]).all() and (got[2][rows] == got[2][i]).all(), LINKED[i]


def test_hand_stated_scaffolds():
    """Atom sets and counts stated by hand (atoms are numbered in string order)."""
    cases = [
        ("CC(=O)Oc1ccccc1C(=O)O", set(range(4, 10)), [6, 6, 0, 0]),                        # aspirin: the six ring atoms only
        ("Cn1cnc2c1c(=O)n(C)c(=O)n2C", set(range(1, 13)) - {9}, [11, 12, 0, 2]),           # caffeine: both rings and both =O, no methyl
        ("c1ccccc1CC(=O)Cc1ccccc1", set(range(16)), [16, 17, 3, 1]),                        # a linker of three and its =O
        ("c1ccccc1S(=O)(=O)c1ccccc1", set(range(15)), [15, 16, 1, 2]),                      # the sulfonyl linker keeps both =O
        ("C1CCCCC1=CC", set(range(7)), [7, 7, 0, 1]),                                        # the ring plus the exocyclic =C, not its methyl
        ("OC(=O)C1CCCCC1", set(range(3, 9)), [6, 6, 0, 0]),                                  # a =O on a substituent is not kept
        ("C12CC1C2", set(range(4)), [4, 5, 0, 0]),
        ("C1CCCC12CCCCC2", set(range(10)), [10, 11, 0, 0]),                                  # a spiro pair shares one atom
        ("C1CC1CCC(C)CC1CC1", {0, 1, 2, 3, 4, 5, 7, 8, 9, 10}, [10, 11, 4, 0]),              # the branch on the linker is dropped
    ]
    status, mask, desc, key = _host([c[0] for c in cases])
    assert (status == 0).all()
    for i, (s, atoms, d) in enumerate(cases):
        assert _atoms(mask[i]) == atoms and desc[i].tolist() == d, (s, sorted(_atoms(mask[i])), desc[i].tolist())
        assert key[i, 0] != 0 and key[i, 1] != 0
    status, mask, desc, key = _host(["CCCC", "CC(=O)O", "C", "[NH4+]"])
    assert (status == 0).all() and not mask.any() and not desc.any() and not key[:, 1].any() and (key[:, 0] != 0).all()
    rejected = [s for s, st, _ in CR.REJECTED if st != CR.OK] + ["C" * 128]
    out = _host(rejected)
    assert set(out[0].tolist()) == {1, 2, 3, 4, 5, 6} and not any(t.any() for t in out[1:])


def test_keys_do_not_depend_on_the_spelling():
    """Every FORMULAS string and six rewrites of each: the rewriter is checked first (status 0, the original's formula), then both keys
    and desc are equal and the mask is the same atom set under the renumbering."""
    rng = np.random.RandomState(11)
    originals = [s for s, _ in CR.FORMULAS]
    rewrites = [[SR.rewrite(s, rng) for _ in range(6)] for s in originals]
    changed = 0
    for (s, formula), group in zip(CR.FORMULAS, rewrites):
        for t, old in group:
            a = CR.analyse(t)
            assert a[0] == CR.OK and CR.hill(a[3], a[2][6]) == formula and sorted(old) == list(range(len(old))), (s, t, a)
            changed += t != s
    assert changed >= 3 * len(originals)                              # the rewrites are other strings, not copies
    flat = [t for group in rewrites for t, _ in group]
    st0, mask0, desc0, key0 = _host(originals)
    st1, mask1, desc1, key1 = _host(flat)
    assert (st0 == 0).all() and (st1 == 0).all()
    for i, group in enumerate(rewrites):
        for j, (t, old) in enumerate(group):
            r = i * 6 + j
            assert key1[r].tolist() == key0[i].tolist() and desc1[r].tolist() == desc0[i].tolist(), (originals[i], t)
            assert _atoms(mask1[r]) == SR.renumbered(_atoms(mask0[i]), old), (originals[i], t)
    # a few by hand
    for same in (("CCO", "OCC", "C(O)C"), ("c1ccccc1C", "Cc1ccccc1", "c1(C)ccccc1"), ("C1CCC2CCCCC2C1", "C12CCCCC1CCCC2")):
        key = _host(list(same))[3]
        assert (key == key[0]).all() and key[0, 0] != 0, same


def test_scaffold_key_ignores_substituents_and_molecule_key_does_not():
    status, _, desc, key = _host(["c1ccccc1", "Cc1ccccc1", "Oc1ccccc1", "CC(=O)Oc1ccccc1C(=O)O"])
    assert (status == 0).all() and (key[:, 1] == key[0, 1]).all() and key[0, 1] != 0 and (desc == desc[0]).all()
    assert len(set(key[:, 0].tolist())) == 4


def test_keys_separate_the_hand_lists():
    """Pairwise distinct scaffold keys over SCAFFOLDS (decalin / bicyclopentyl need the ring-bond bit), pairwise distinct molecule keys
    over FORMULAS; the reference agrees."""
    names, strings = list(SCAFFOLDS), list(SCAFFOLDS.values())
    assert len(strings) >= 20
    status, _, desc, key = _host(strings)
    assert (status == 0).all() and (key[:, 1] != 0).all()
    seen = {}
    for name, k in zip(names, key[:, 1].tolist()):
        assert k not in seen, (name, seen[k])
        seen[k] = name
    assert (key == SR.expected(strings)[3]).all()
    by = dict(zip(names, desc.tolist()))
    assert by["decalin"] == by["bicyclopentyl"] == [10, 11, 0, 0] and by["benzophenone"] == [14, 15, 1, 1]
    formulas = [s for s, _ in CR.FORMULAS]
    status, _, _, key = _host(formulas)
    assert (status == 0).all() and len(set(key[:, 0].tolist())) == len(formulas) and (key[:, 0] != 0).all()


def _counter(keys, weights=None):
    c = collections.Counter()
    for i, k in enumerate(keys):
        if k:
            c[k] += 1 if weights is None else weights[i]
    return c


def test_key_histogram_and_cosine_against_a_counter():
    """Integer sums are exact; the cosine is within 8 x 2^-53 relative of the Counter's (three roundings on each side); empty -> NaN."""
    rs = np.random.RandomState(5)
    pool = np.concatenate([rs.randint(-2 ** 62, 2 ** 62, size=40), [0, -1, 1, -2 ** 63, 2 ** 63 - 1]]).astype(np.int64)
    a, b = pool[rs.randint(len(pool), size=3000)], pool[rs.randint(len(pool) - 10, size=500)]
    wa = rs.randint(1, 1000, size=a.size).astype(np.int64)
    for keys, w in ((a, None), (a, wa), (b, None), (a.reshape(60, 50), wa.reshape(60, 50))):
        k, c = ops.key_histogram(torch.from_numpy(keys), None if w is None else torch.from_numpy(w))
        want = _counter(keys.reshape(-1).tolist(), None if w is None else w.reshape(-1).tolist())
        assert k.dtype == c.dtype == torch.int64 and k.tolist() == sorted(want) and c.tolist() == [want[x] for x in sorted(want)]
        assert 0 not in k.tolist()
    ha, hb = ops.key_histogram(torch.from_numpy(a), torch.from_numpy(wa)), ops.key_histogram(torch.from_numpy(b))
    for x, y, cx, cy in ((ha, hb, _counter(a.tolist(), wa.tolist()), _counter(b.tolist())), (hb, ha, _counter(b.tolist()), _counter(a.tolist(), wa.tolist())),
                         (ha, ha, _counter(a.tolist(), wa.tolist()), _counter(a.tolist(), wa.tolist()))):
        got = ops.histogram_cosine(*x, *y)
        want = SR.cosine(cx, cy)
        print("cosine", float(got), "Counter", want, "relative difference", abs(float(got) - want) / want)
        assert got.dtype == torch.float64 and got.dim() == 0 and 0 < want <= 1 and abs(float(got) - want) <= 8 * 2.0 ** -53 * want
    assert abs(float(ops.histogram_cosine(*ha, *ha)) - 1.0) <= 8 * 2.0 ** -53
    only = ops.key_histogram(torch.tensor([7, 7, 9])), ops.key_histogram(torch.tensor([8, 10, 10]))
    assert float(ops.histogram_cosine(*only[0], *only[1])) == 0.0                          # disjoint keys
    assert float(ops.histogram_cosine(*ops.key_histogram(torch.tensor([3, 3, 5])), *ops.key_histogram(torch.tensor([3, 5, 5])))) == \
        pytest.approx(4 / 5, rel=8 * 2.0 ** -53)
    empty = ops.key_histogram(torch.zeros(4, dtype=torch.int64))
    none = ops.key_histogram(torch.zeros(0, dtype=torch.int64))
    assert empty[0].numel() == empty[1].numel() == none[0].numel() == 0
    for x, y in ((empty, ha), (ha, empty), (none, none)):
        assert math.isnan(float(ops.histogram_cosine(*x, *y)))
    assert math.isnan(SR.cosine(collections.Counter(), _counter(a.tolist())))
    assert ops.keys_in(ha[0], torch.tensor([int(ha[0][3]), 12345, 0])).tolist() == [True, False, False]


def test_scaffold_split_on_cpu_tensors():
    """ops.scaffold_split_rows on the host entry's scaffold keys of the mutation corpus: the two sides are disjoint and cover every row,
    share no non-zero key, rows without a scaffold stay in train, at least the asked fraction of the ring-bearing rows is held out and
    no more than one scaffold beyond it, the same seed gives the same split and another seed another one."""
    strings, want = SR.corpus_expected()
    keys = torch.from_numpy(want[3][:, 1].copy())
    ringed = int((keys != 0).sum())
    largest = max(collections.Counter(k for k in keys.tolist() if k).values())
    for fraction in (0.0, 0.1, 0.5, 1.0):
        train, test = ops.scaffold_split_rows(keys, fraction, seed=3)
        assert train.dtype == test.dtype == torch.int64
        assert sorted(train.tolist() + test.tolist()) == list(range(len(strings))) and train.tolist() == sorted(train.tolist())
        assert test.tolist() == sorted(test.tolist())
        ktrain, ktest = set(keys[train].tolist()) - {0}, set(keys[test].tolist())
        assert not ktrain & ktest and 0 not in ktest
        assert fraction * ringed <= test.numel() < fraction * ringed + largest + (fraction == 0.0)
        again = ops.scaffold_split_rows(keys, fraction, seed=3)
        assert torch.equal(again[0], train) and torch.equal(again[1], test)
        if fraction == 0.0:
            assert test.numel() == 0
        if fraction == 1.0:
            assert test.numel() == ringed
    assert not torch.equal(ops.scaffold_split_rows(keys, 0.5, seed=4)[1], ops.scaffold_split_rows(keys, 0.5, seed=3)[1])
    none = ops.scaffold_split_rows(torch.zeros(5, dtype=torch.int64), 0.5)
    assert none[0].tolist() == [0, 1, 2, 3, 4] and none[1].numel() == 0
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="test_fraction must be in"):
            ops.scaffold_split_rows(keys, bad)


def test_host_entry_edge_rows_and_prefilled_outputs():
    """127 tokens in ring-bearing rows (two rings and a 117-atom linker; one ring of 125 atoms), the 128-token row, a ring and a linker that straddle atom 64, 25 rings in one row, a cage, a
    strided view, a row without <eos>, ids outside the vocabulary; every element of prefilled outputs is written; mask may be left out."""
    v = CR.vocabulary()
    tok, chem = VC.smiles_token_table(v), VC.smiles_chem_table(v)
    strings = ["C1CC1" + "C" * 117 + "C1CC1", "C" * 128, "C" * 60 + "C1CCCCCCC1", "c1ccccc1" + "C" * 62 + "c1ccccc1", "C1CC1" * 25 + "CC",
               "C12C3C4C1C5C2C3C45" + "C" * 100, "CCC1" + "C" * 66 + "1"]
    strings.append("C1" + "C" * 124 + "1")                           # 127 tokens: the most atoms a ring-bearing row can have, all in the ring
    assert len(strings[0]) == len(strings[-1]) == 127 and len(strings[3]) < 127
    got = _host(strings, T=140)
    want = SR.expected(strings)
    assert got[0].tolist() == [0, CR.TOO_LONG, 0, 0, 0, 0, 0, 0] == want[0].tolist()
    for g, w in zip(got, want):
        assert (g == w).all()
    assert got[2][0].tolist() == [123, 124, 117, 0] and got[2][7].tolist() == [125, 125, 0, 0] and got[2][3].tolist() == [74, 75, 62, 0] and got[2][4].tolist() == [75, 99, 0, 0]
    assert _atoms(got[1][2]) == set(range(60, 68)) and got[1][2, 0] != 0 and got[1][2, 1] != 0          # a ring in both mask words
    x = torch.from_numpy(CR.token_rows(["C1CC1O", "CC(=O)O", "C=F", "CCN", "C1CC1O"], v, T=12))
    x[0, 7] = v.pad                                                # no <eos>
    x[1, 3] = -1
    x[3, 2] = len(v)
    wide = torch.full((5, 40), v.eos, dtype=torch.long)
    wide[:, :12] = x
    status = torch.full((5,), 0x7f7f7f7f, dtype=torch.int32)
    mask = torch.full((5, 2), 0x7f7f7f7f7f7f7f7f, dtype=torch.int64)
    desc = torch.full((5, 4), 0x7f7f7f7f, dtype=torch.int32)
    key = torch.full((5, 2), 0x7f7f7f7f7f7f7f7f, dtype=torch.int64)
    ops.smiles_scaffold_host(wide[:, :12], tok, chem, v.eos, status, mask, desc, key)
    assert status.tolist() == [1, 1, 2, 1, 0] and not mask[:4].any() and not desc[:4].any() and not key[:4].any()
    one = SR.expected(["C1CC1O"])
    assert mask[4].tolist() == one[1][0].tolist() == [7, 0] and desc[4].tolist() == [3, 3, 0, 0] and key[4].tolist() == one[3][0].tolist()
    without = ops.smiles_scaffold_host(wide[:, :12], tok, chem, v.eos, mask=False)
    assert without[1] is None and torch.equal(without[0], status) and torch.equal(without[2], desc) and torch.equal(without[3], key)


def test_entries_refuse_bad_arguments_before_launching():
    """Everything below returns before any HIP call (no device needed)."""
    lib = L.load()
    fake = ctypes.c_void_p(256)                                  # never dereferenced: every call below is refused first

    def rows(name, B=4, T=8, V=29, x=fake, ld=8, tok=fake, chem=fake, eos=1, status=fake, mask=fake, desc=fake, key=fake):
        tail = (None,) if name == ENTRIES[0] else ()
        return getattr(lib, name)(B, T, V, x, ld, tok, chem, eos, status, mask, desc, key, *tail)
    for name in (ENTRIES[0], ENTRIES[2]):
        assert rows(name, B=0) == -1 and rows(name, T=0, ld=0) == -1 and rows(name, V=0, eos=0) == -1 and rows(name, V=65) == -3
        assert rows(name, x=None) == -1 and rows(name, tok=None) == -1 and rows(name, chem=None) == -1 and rows(name, status=None) == -1
        assert rows(name, desc=None) == -1 and rows(name, key=None) == -1 and rows(name, ld=7) == -1 and rows(name, eos=29) == -1
        assert rows(name, eos=-1) == -1 and rows(name, V=65, mask=None) == -3

    def corpus(tokens=fake, offsets=fake, N=100, V=29, tok=fake, chem=fake, status=fake, mask=fake, desc=fake, key=fake):
        return lib.mvae_smiles_scaffold_corpus(tokens, offsets, N, V, tok, chem, status, mask, desc, key, None)
    assert corpus(N=0) == -1 and corpus(N=-3) == -1 and corpus(V=0) == -1 and corpus(V=65) == -3
    assert corpus(tokens=None) == -1 and corpus(offsets=None) == -1 and corpus(tok=None) == -1 and corpus(chem=None) == -1
    assert corpus(status=None) == -1 and corpus(desc=None) == -1 and corpus(key=None) == -1


def test_python_surface_raises_before_device_work():
    torch.manual_seed(0)
    model = MV.VAE(VC.OneHotVocab(list("CNO(=)1")), dtype=torch.float32)
    big = MV.VAE(VC.OneHotVocab([chr(65 + i) for i in range(61)]), dtype=torch.float32)
    ds = D.MosesDeviceDataset(["CCO", "CC"], model.vocabulary, device="cpu")
    with pytest.raises(ValueError, match="scaffolds=True supports at most 64 ids"):
        mv.moses_generate(big, 4, max_len=8, scaffolds=True)
    with pytest.raises(ValueError, match="at most 64"):
        D.MosesDeviceDataset(["AB"], big.vocabulary, device="cpu").scaffolds()
    with pytest.raises(ValueError, match="at most 64"):
        D.MosesDeviceDataset(["AB"], big.vocabulary, device="cpu").rows_with_scaffold(["AB"])
    with pytest.raises(ValueError, match="test_fraction must be in"):
        ds.scaffold_split(1.5)
    with pytest.raises(L.MvaeError, match="MI355X only"):                            # a CPU model: no fallback
        mv.moses_generate(model, 4, max_len=8, scaffolds=True)
    with pytest.raises(L.MvaeError, match="MI355X only"):
        model.scaffolds(["CCO"])
    for call in (ds.scaffolds, ds.scaffold_histogram, lambda: ds.rows_with_scaffold(["CCO"]), lambda: ds.scaffold_split(0.1)):
        with pytest.raises(L.MvaeError, match="MI355X only"):
            call()
