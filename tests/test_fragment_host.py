"""CPU tests of the fragment feature (mvae_smiles_fragment_rows / _corpus / _host, mvae_smiles_fragment_smiles_rows / _corpus / _host):
the host entries (csrc/fragment.hip and csrc/fragment_smiles.hip compiled for the CPU) against the reference of tests/frag_ref.py,
element for element and token row for token row, on the mutation corpus and the header's worked examples; what the definition promises
-- a partition, invariance under re-spelling, conservation of atoms and hydrogens as the older graph entry counts them --; the Frag
figure against collections.Counter; the boundary at 16 fragments; every refusal; the declarations and the compiler's resource remarks."""
import collections
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import molecular_vae_amd as mv
from molecular_vae_amd import _lib as L, data as D, mosesvae as MV, vocab as VC, ops
import chem_ref as CR
import frag_ref as FG
import rewrite_ref as RR
import scaffold_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS_ENTRIES = ("mvae_smiles_fragment_rows", "mvae_smiles_fragment_corpus", "mvae_smiles_fragment_host")
SMILES_ENTRIES = ("mvae_smiles_fragment_smiles_rows", "mvae_smiles_fragment_smiles_corpus", "mvae_smiles_fragment_smiles_host")
# (row, cuts, cuts by rule A alone, the fragments as strings in this library's canonical spelling); the header spells the last fragment
# of aspirin O=CO, which is the same graph
WORKED = (("CC(=O)Oc1ccccc1C(=O)O", 3, 1, ["CC=O", "O", "c1ccccc1", "C(=O)O"]), ("Cc1ccccc1", 0, 0, ["Cc1ccccc1"]), ("CCOCC", 0, 0, ["CCOCC"]),
          ("c1ccccc1c1ccccc1", 1, 0, ["c1ccccc1", "c1ccccc1"]), ("CC(=O)NC", 1, 1, ["CC=O", "CN"]), ("CCn1cccc1", 1, 0, ["CC", "c1cc[nH]c1"]))
RINGS16, RINGS17 = "C1CC1" * 16, "C1CC1" * 17


def _tables(v):
    return VC.smiles_token_table(v), VC.smiles_chem_table(v), VC.smiles_emit_table(v)


def _host(strings, T=None, **kw):
    v = CR.vocabulary()
    x = torch.from_numpy(CR.token_rows(strings, v, T))
    return tuple(None if t is None else t.numpy() for t in ops.smiles_fragment_host(x, *_tables(v)[:2], v.eos, **kw))


def _host_smiles(strings, frag, max_content=127, T=None, T_out=131, v=None, **kw):
    v = CR.vocabulary() if v is None else v
    x = torch.from_numpy(CR.token_rows(strings, v, T))
    out = ops.smiles_fragment_smiles_host(x, *_tables(v), v.bos, v.eos, v.pad, frag, max_content, T_out, **kw)
    return tuple(None if t is None else t.numpy() for t in out)


def _decode(out, out_len, v):
    return ["".join(v.i2c[int(i)] for i in row[1:n - 1]) for row, n in zip(out, out_len)]


def _atoms(words):
    return {a for a in range(128) if (int(words[a >> 6]) >> (a & 63)) & 1}


def _want_smiles(refs, v, T_out):
    """The reference's (status, string, info) per row as the arrays the string entries write."""
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


_CASES = {}


def cases():
    """(strings, the reference's arrays, the host entry's arrays) of the mutation corpus + the worked examples + the two ring rows:
    computed once per process and shared; callers leave it unchanged."""
    if "c" not in _CASES:
        strings = CR.mutation_corpus() + [w[0] for w in WORKED] + [RINGS16, RINGS17]
        _CASES["c"] = (strings, FG.expected(strings), _host(strings))
    return _CASES["c"]


def test_entries_are_declared_bound_and_exported_at_abi_12():
    text = open(os.path.join(ROOT, "include", "mvae.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", header).group(1)) == 12 == L.ABI_VERSION
    lib = L.load()
    for name in KEYS_ENTRIES + SMILES_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    # the scaffold entries' arguments; the string entries take frag in front of info
    for mine, theirs in zip(KEYS_ENTRIES, ("mvae_smiles_scaffold_rows", "mvae_smiles_scaffold_corpus", "mvae_smiles_scaffold_host")):
        assert L.SIGNATURES[mine] == L.SIGNATURES[theirs]
    for mine, theirs in zip(SMILES_ENTRIES, ("mvae_smiles_scaffold_smiles_rows", "mvae_smiles_scaffold_smiles_corpus", "mvae_smiles_scaffold_smiles_host")):
        assert len(L.SIGNATURES[mine][1]) == len(L.SIGNATURES[theirs][1]) + 1

    def define(name):
        return int(re.search(r"#define\s+" + name + r"\s+(\d+)", header).group(1))
    assert define("MVAE_FRAGMENT_MAX") == ops.FRAGMENT_MAX == FG.F == 16 and define("MVAE_FRAGMENT_DESC") == len(ops.FRAGMENT_DESC) == 4
    assert define("MVAE_SMILES_FRAG_MANY") == ops.SMILES_STATUS_FRAG_MANY == FG.FRAG_MANY == 15
    assert define("MVAE_SMILES_NO_FRAGMENT") == ops.SMILES_STATUS_NO_FRAGMENT == FG.NO_FRAGMENT == 16
    assert define("MVAE_FRAGMENT_SMILES_COUNTS") == ops.FRAGMENT_SMILES_COUNTS == 32 and define("MVAE_FRAGMENT_SMILES_INFO") == 4
    assert define("MVAE_FRAGMENT_LDS_BYTES") == define("MVAE_FRAGMENT_SMILES_LDS_BYTES") == 81920
    assert ops.FRAGMENT_STATUS_NAMES[15] == "frag_many" and ops.FRAGMENT_SMILES_STATUS_NAMES[16] == "no_fragment"
    assert ops.FRAGMENT_SMILES_STATUS_NAMES[:15] == ops.SCAFFOLD_SMILES_STATUS_NAMES
    for phrase in ("Fragments (an addition", "not BRICS, not RECAP", "agreement with any toolkit is", "CC(=O)Oc1ccccc1C(=O)O"):
        assert phrase in text, phrase
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        body = open(os.path.join(ROOT, doc)).read()
        assert "not BRICS" in body and "mvae_smiles_fragment" in body, doc
    for fn in (ops.smiles_fragment_rows, ops.smiles_fragment_corpus, ops.smiles_fragment_host, ops.fragment_dict, ops.smiles_fragment_smiles_rows,
               ops.smiles_fragment_smiles_corpus, ops.smiles_fragment_smiles_host, MV.VAE.fragments, MV.VAE.fragment_smiles, D.fragment_smiles,
               D.MosesDeviceDataset.fragments, D.MosesDeviceDataset.fragment_histogram, D.MosesDeviceDataset.rows_with_fragment):
        assert callable(fn)
    assert inspect.signature(mv.moses_generate).parameters["fragments"].default is False
    build = open(os.path.join(ROOT, "molecular-vae_amd", "csrc", "build.sh")).read()
    assert build.count(" fragment_smiles fragment scaffold_smiles ") == 2 and "build/fragment_smiles.o build/fragment.o" in build
    assert "build/tune/fragment_smiles.o build/tune/fragment.o" in build
    for h in ("fragment_sets.hpp", "graph_key.hpp", "smiles_cut.hpp"):
        assert h + " -nt build/$f.o" in build, h
    # the cut set and the labels, the key and the cut are shared, not copied
    csrc = os.path.join(ROOT, "molecular-vae_amd", "csrc")
    src = {f: open(os.path.join(csrc, f)).read() for f in ("fragment.hip", "fragment_smiles.hip", "scaffold.hip", "scaffold_smiles.hip")}
    assert '#include "fragment_sets.hpp"' in src["fragment.hip"] and '#include "fragment_sets.hpp"' in src["fragment_smiles.hip"]
    assert '#include "graph_key.hpp"' in src["fragment.hip"] and '#include "graph_key.hpp"' in src["scaffold.hip"]
    assert '#include "smiles_cut.hpp"' in src["fragment_smiles.hip"] and '#include "smiles_cut.hpp"' in src["scaffold_smiles.hip"]
    assert all("Cuts cut_bonds" not in s and "int labels(" not in s and "int hydrogens(" not in s and "0x7FEB352D" not in s for s in src.values())


@pytest.mark.parametrize("name", ["fragment", "fragment_smiles"])
def test_new_kernels_use_no_scratch(tmp_path, name):
    """The compiler's resource remarks for the two kernels of each new file, cross-compiled for gfx950: scratch 0, no spills, and the
    LDS per block that include/mvae.h states, 80 KiB, so that two blocks fit a CU."""
    csrc = os.path.join(ROOT, "molecular-vae_amd", "csrc")
    usage = os.path.join(csrc, "build", name + ".usage.txt")
    sources = (name + ".hip", "fragment_sets.hpp", "graph_key.hpp", "smiles_cut.hpp", "smiles_canon.hpp", "smiles_writer.hpp", "smiles_rounds.hpp",
               "smiles_graph.hpp", "smiles_syntax.hpp", "common.hpp", "../../include/mvae.h")
    if os.path.exists(usage) and os.path.getmtime(usage) >= max(os.path.getmtime(os.path.join(csrc, f)) for f in sources):
        text = open(usage, errors="replace").read()
    else:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                              "-c", os.path.join(csrc, name + ".hip"), "-o", str(tmp_path / (name + ".dev.o"))],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert run.returncode == 0, run.stderr[-2000:]
        text = run.stderr
    names = re.findall(r"Function Name: (\S+)", text)
    kernels = ("rows_kernelIN3frg8FragmentE", "corpus_kernelIN3frg8FragmentE") if name == "fragment" else \
        ("smiles_fragment_smiles_rows_kernel", "smiles_fragment_smiles_corpus_kernel")
    assert len(names) == 2 and all(any(k in n for n in names) for k in kernels), names
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 2
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 2 and re.findall(r"SGPRs Spill: (\d+)", text) == ["0"] * 2
    assert list(map(int, re.findall(r"LDS Size \[bytes/block\]: (\d+)", text))) == [81920] * 2
    assert all(int(n) <= 128 for n in re.findall(r" VGPRs: (\d+)", text))


def test_keys_entry_equals_the_reference_element_for_element():
    """All four outputs of all 4,258 rows; rows that are not ok are zero.  The input is not degenerate, asserted on the reference alone
    BEFORE anything is compared: at least 3 statuses, at least 25 % of the status-0 rows with 2 or more fragments, at least 20 rows with
    a cut that only rule A makes."""
    strings, want, got = cases()
    ok = want[0] == 0
    n_multi, n_acyl = int((want[2][ok, 0] >= 2).sum()), int((want[2][:, 2] > 0).sum())
    print("rows:", len(strings), "statuses:", np.bincount(want[0]).tolist(), "status 0 with >= 2 fragments:", n_multi, "of", int(ok.sum()),
          "rows with a rule-A-only cut:", n_acyl, "distinct keys:", len(set(want[3][want[3] != 0].tolist())))
    assert len(strings) == 4258 and len(set(want[0].tolist())) >= 3
    assert n_multi >= 0.25 * ok.sum() and n_acyl >= 20
    for g, w, name in zip(got, want, ("status", "mask", "desc", "key")):
        wrong = np.nonzero((g != w).reshape(len(strings), -1).any(1))[0]
        assert g.shape == w.shape and g.dtype == w.dtype and wrong.size == 0, (name, [(strings[i], g[i].tolist(), w[i].tolist()) for i in wrong[:3]])
    bad = ~ok & (want[0] != FG.FRAG_MANY)
    for g in got[1:]:
        assert not g[bad].any()
    v = CR.vocabulary()
    graph_status = ops.smiles_graph_host(torch.from_numpy(CR.token_rows(strings, v)), *_tables(v)[:2], v.eos)[0].numpy()
    assert ((graph_status == got[0]) | (got[0] == FG.FRAG_MANY)).all() and (graph_status[got[0] == FG.FRAG_MANY] == 0).all()
    without = _host(strings, mask=False)
    assert without[1] is None and all((a == b).all() for a, b in zip(without[::2] + without[3:], got[::2] + got[3:]))


def test_worked_examples():
    v = CR.vocabulary()
    rows = [w[0] for w in WORKED]
    status, mask, desc, key = _host(rows)
    assert not status.any() and desc[:, :3].tolist() == [[len(w[3]), w[1], w[2]] for w in WORKED]
    assert desc[:, 3].tolist() == [6, 7, 5, 6, 3, 5]
    most = max(len(w[3]) for w in WORKED)
    for f in range(most + 1):
        out, out_len, st, info = _host_smiles(rows, f)
        want = [w[3][f] if f < len(w[3]) else "" for w in WORKED]
        assert _decode(out, out_len, v) == want == [FG.fragment_smiles(s, f)[1] for s in rows]
        assert st.tolist() == [0 if f < len(w[3]) else FG.NO_FRAGMENT for w in WORKED]
    assert D.fragment_smiles(rows, v, device="cpu") == [w[3] for w in WORKED]
    # the ring of every worked example that has one is benzene's scaffold key; the two halves of biphenyl are one key
    benzene = SR.scaffold("c1ccccc1")[3][1]
    assert key[0, 2] == key[3, 0] == key[3, 1] == benzene and key[0, 0] == key[4, 0] and (key[1, 1:] == 0).all()
    # the fragments compile as substructure queries and hit their own row
    tok, chem, emit = _tables(v)
    for row, _, _, parts in WORKED:
        table, qstatus = ops.smiles_substruct_compile(torch.from_numpy(CR.token_rows(parts, v)), tok, chem, emit, v.eos)
        assert not qstatus.any()
        x = torch.from_numpy(CR.token_rows([row], v))
        st, hit, undecided, _, _ = ops.smiles_substruct_host(x, tok, chem, v.eos, table)
        assert st.tolist() == [0] and ops.substruct_bits(hit, len(parts)).all() and not ops.substruct_bits(undecided, len(parts)).any()


def test_string_entry_equals_the_reference_token_row_for_token_row():
    """Every fragment number up to the most any row has, and one beyond, over the whole stretch: tokens, lengths, statuses and info."""
    strings, want, got = cases()
    v = CR.vocabulary()
    most = int(want[2][:, 0].max())
    assert most == 17
    n_written, new_brackets = 0, 0
    for f in range(most + 1):
        refs = [FG.fragment_smiles(s, f) for s in strings]
        res = _host_smiles(strings, f)
        wrong = [name for g, w, name in zip(res, _want_smiles(refs, v, 131), ("out", "out_len", "status", "info")) if not np.array_equal(g, w)]
        assert not wrong, (f, wrong)
        n_written += sum(r[0] == 0 for r in refs)
        new_brackets += sum(r[0] == 0 and r[2][2] > 0 for r in refs)
        # the string entry knows no limit of 16: it says NO_FRAGMENT exactly where the row has f or fewer fragments
        stereo_free = np.array([not any(c in s for c in "@/\\") for s in strings])
        told = (want[0] == 0) | (want[0] == FG.FRAG_MANY)
        assert ((res[2] == FG.NO_FRAGMENT) == (told & stereo_free & (want[2][:, 0] <= f))).all()
    print("fragments written:", n_written, "with an atom that became a bracket atom:", new_brackets)
    assert n_written >= 1000 and new_brackets >= 20
    assert (res[2] != 0).all() and (res[1] == 2).all()               # f = 17: no row has an 18th fragment
    small = _host_smiles(strings, 1, max_content=3, info=False)
    refs = [FG.fragment_smiles(s, 1, max_content=3) for s in strings]
    assert small[3] is None and sum(r[0] == RR.LONG for r in refs) >= 50
    assert not [n for g, w, n in zip(small[:3], _want_smiles(refs, v, 131)[:3], "abc") if not np.array_equal(g, w)]


def test_fragments_partition_the_atoms():
    strings, want, got = cases()
    status, mask, desc, key = got
    checked = 0
    for b in np.nonzero(status == 0)[0]:
        n = len(FG.FR.molecule(strings[b]))
        sets = [_atoms(mask[b, f]) for f in range(16)]
        used = [s for s in sets if s]
        assert len(used) == desc[b, 0] == desc[b, 1] + 1 and all(sets[:len(used)]) and not any(sets[len(used):])
        assert sum(len(s) for s in used) == n == len(set().union(*used)) and set().union(*used) == set(range(n))
        assert max(len(s) for s in used) == desc[b, 3] and [min(s) for s in used] == sorted(min(s) for s in used)
        assert (key[b, :len(used)] != 0).all() and not key[b, len(used):].any() and 0 <= desc[b, 2] <= desc[b, 1]
        checked += 1
    assert checked >= 800


def test_key_lists_do_not_depend_on_the_spelling():
    """Three re-spellings of 300 status-0 rows from random roots: the sorted list of fragment keys and desc are equal, and the atom sets
    are the same sets under the renumbering."""
    strings, want, got = cases()
    rng = np.random.RandomState(11)
    fine = [b for b in np.nonzero(want[0] == 0)[0] if not any(c in strings[b] for c in "@/\\")]       # the rewriter knows no stereo
    pick = [fine[i] for i in rng.choice(len(fine), size=300, replace=False)]
    assert sum(want[2][b, 0] >= 2 for b in pick) >= 100
    spelled = [[SR.rewrite(strings[b], rng) for _ in range(3)] for b in pick]
    flat = [t for group in spelled for t, _ in group]
    assert sum(t != strings[b] for b, group in zip(pick, spelled) for t, _ in group) >= 600
    st, mask, desc, key = _host(flat)
    assert not st.any()
    for i, b in enumerate(pick):
        for j, (t, old) in enumerate(spelled[i]):
            r = 3 * i + j
            assert sorted(key[r].tolist()) == sorted(got[3][b].tolist()) and desc[r].tolist() == got[2][b].tolist(), (strings[b], t)
            mine = {frozenset(_atoms(mask[r, f])) for f in range(desc[r, 0])}
            theirs = {frozenset(SR.renumbered(_atoms(got[1][b, f]), old)) for f in range(desc[r, 0])}
            assert mine == theirs, (strings[b], t)


def test_fragments_conserve_atoms_and_hydrogens():
    """Through the older graph entry, which knows nothing of fragments: every fragment string is valence-consistent; its heavy atoms are
    the popcount of its mask; the element counts summed over the fragments are the row's; the hydrogens are the row's plus two per cut."""
    strings, want, got = cases()
    v = CR.vocabulary()
    tok, chem = _tables(v)[:2]
    rows = [b for b in np.nonzero(got[0] == 0)[0] if not any(c in strings[b] for c in "@/\\")]
    assert len(rows) >= 600
    own = ops.smiles_graph_host(torch.from_numpy(CR.token_rows([strings[b] for b in rows], v)), tok, chem, v.eos)
    parts = D.fragment_smiles([strings[b] for b in rows], v, device="cpu")
    flat = [p for ps in parts for p in ps]
    st, _, desc, formula = (t.numpy() for t in ops.smiles_graph_host(torch.from_numpy(CR.token_rows(flat, v)), tok, chem, v.eos))
    assert not st.any()
    at = 0
    for i, b in enumerate(rows):
        k = len(parts[i])
        assert k == got[2][b, 0]
        total = formula[at:at + k].sum(0)
        row_formula = own[3][i].numpy().copy()
        hydrogens = int(got[2][b, 1]) * 2
        assert total[1:].tolist() == row_formula[1:].tolist(), strings[b]
        assert total[0] == row_formula[0] + hydrogens, (strings[b], parts[i])
        for f in range(k):
            # heavy_atoms leaves explicit [H] atoms out; the mask holds them
            explicit_h = sum(1 for a in _atoms(got[1][b, f]) if FG.FR.molecule(strings[b])[a]["el"] == "H")
            assert desc[at + f, 0] == len(_atoms(got[1][b, f])) - explicit_h, (strings[b], parts[i])
        at += k
    assert at == len(flat) >= 1000


def test_frag_figure_against_a_counter():
    """ops.key_histogram + histogram_cosine on the [N, 16] keys equal scaffold_ref.cosine of the reference's Counters to the last bit:
    exact integer dot product and squared norms, the product of the norms, one sqrt, one division -- the order histogram_cosine
    documents.  A set against itself is 1.0."""
    strings, want, got = cases()
    half = len(strings) // 2
    a, b = got[3][:half], got[3][half:]
    ca = collections.Counter(k for s in strings[:half] for k in FG.fragments(s)[3])
    cb = collections.Counter(k for s in strings[half:] for k in FG.fragments(s)[3])
    assert len(ca) >= 100 and len(cb) >= 100 and set(ca) & set(cb) and max(ca.values()) >= 50
    ha, hb = ops.key_histogram(torch.from_numpy(a.copy())), ops.key_histogram(torch.from_numpy(b.copy()))
    assert ha[0].tolist() == sorted(ca) and ha[1].tolist() == [ca[k] for k in sorted(ca)]
    cos = ops.histogram_cosine(*ha, *hb)
    ref = SR.cosine(ca, cb)
    print("frag", float(cos), "Counter", ref)
    assert cos.dtype == torch.float64 and 0 < ref < 1 and float(cos) == ref == float(ops.histogram_cosine(*hb, *ha))
    assert float(ops.histogram_cosine(*ha, *ha)) == 1.0 == SR.cosine(ca, ca)
    # multiplicity counts: a weight doubles a row's fragments
    w = torch.ones(a.shape, dtype=torch.int64)
    w[::2] = 2
    cw = collections.Counter()
    for i, s in enumerate(strings[:half]):
        for k in FG.fragments(s)[3]:
            cw[k] += 2 if i % 2 == 0 else 1
    assert float(ops.histogram_cosine(*ops.key_histogram(torch.from_numpy(a.copy()), w), *hb)) == SR.cosine(cw, cb)


def test_the_boundary_at_sixteen_fragments():
    v = CR.vocabulary()
    status, mask, desc, key = _host([RINGS16, RINGS17])
    assert status.tolist() == [0, FG.FRAG_MANY] and desc.tolist() == [[16, 15, 0, 3], [17, 16, 0, 3]]
    assert (key[0] == SR.scaffold("C1CC1")[3][1]).all() and [sorted(_atoms(mask[0, f])) for f in range(16)] == [[3 * f, 3 * f + 1, 3 * f + 2] for f in range(16)]
    assert not mask[1].any() and not key[1].any()
    out, out_len, st, info = _host_smiles([RINGS16, RINGS17], 16)
    assert st.tolist() == [FG.NO_FRAGMENT, 0] and out_len.tolist() == [2, 7] and _decode(out, out_len, v) == ["", "C1CC1"]
    assert out[0].tolist() == [v.bos, v.eos] + [v.pad] * 129 and info.tolist() == [[0] * 4, [3, 3, 0, 1]]
    out, out_len, st, info = _host_smiles([RINGS16, RINGS17], 15)
    assert st.tolist() == [0, 0] and _decode(out, out_len, v) == ["C1CC1"] * 2 and info.tolist() == [[3, 3, 0, 1], [3, 3, 0, 2]]
    parts, first = D.fragment_smiles([RINGS16, RINGS17, "C("], v, device="cpu", return_status=True)
    assert [len(p) for p in parts] == [16, 17, 0] and first.tolist() == [0, 0, 1]


def test_every_refusal_of_the_string_entry_gives_the_empty_row():
    """One row of every walk status, stereo rows, a fragment too long for max_content, a fragment that needs a token the vocabulary
    lacks: bos, eos, pad..., out_len 2, never a copy."""
    v = CR.vocabulary()
    rejected = [s for s, st, _ in CR.REJECTED if st != CR.OK and s] + ["C" * 128]
    rows = rejected + ["C[C@H]1CC1", "F/C=C/C1CC1", "CCO"]
    for f in (0, 1):
        refs = [FG.fragment_smiles(s, f) for s in rows]
        assert {r[0] for r in refs[:len(rejected)]} == {1, 2, 3, 4, 5, 6}
        assert [r[0] for r in refs[len(rejected):]] == [RR.STEREO, RR.STEREO, 0 if f == 0 else FG.NO_FRAGMENT]
        got = _host_smiles(rows, f, T=140, T_out=140)
        wrong = [n for g, w, n in zip(got, _want_smiles(refs, v, 140), ("out", "out_len", "status", "info")) if not np.array_equal(g, w)]
        assert not wrong, (f, wrong)
        empty = got[2] != 0
        assert (got[1][empty] == 2).all() and (got[0][empty, 0] == v.bos).all() and (got[0][empty, 1] == v.eos).all() and (got[0][empty, 2:] == v.pad).all()
    refs = [FG.fragment_smiles(s, 1, max_content=5) for s in ("Cc1ccc(cc1)c1ccccc1", "CCn1cccc1")]
    assert [r[0] for r in refs] == [RR.LONG, RR.LONG] and refs[0][2] == [6, 6, 0, 1]
    got = _host_smiles(["Cc1ccc(cc1)c1ccccc1", "CCn1cccc1"], 1, max_content=5)
    assert not [n for g, w, n in zip(got, _want_smiles(refs, v, 131), "abcd") if not np.array_equal(g, w)]
    small = VC.OneHotVocab(set(CR.ALPHABET) - {"H"})
    refs = [FG.fragment_smiles(s, 1, have=set(CR.ALPHABET) - {"H"}) for s in ("CCn1cccc1", "CCc1ccccc1")]
    assert [r[0] for r in refs] == [RR.NO_TOKEN, 0] and refs[0][1] == ""
    got = _host_smiles(["CCn1cccc1", "CCc1ccccc1"], 1, v=small, T_out=129)
    assert not [n for g, w, n in zip(got, _want_smiles(refs, small, 129), "abcd") if not np.array_equal(g, w)]


def test_edge_rows_strided_input_and_prefilled_outputs():
    """127-token rows, the 128-token row, a fragment that straddles atom 64, a cage, a strided view, a row without <eos>, ids outside the
    vocabulary; every element of prefilled outputs is written."""
    v = CR.vocabulary()
    tok, chem, emit = _tables(v)
    strings = ["C1CC1" + "C" * 117 + "C1CC1", "C" * 128, "C1CC1" + "C" * 58 + "C1CCCCCCC1", "c1ccccc1" + "C" * 62 + "c1ccccc1",
               "C12C3C4C1C5C2C3C45" + "C" * 100, "C" * 127]
    got = _host(strings, T=140)
    want = FG.expected(strings)
    assert got[0].tolist() == [0, CR.TOO_LONG, 0, 0, 0, 0] == want[0].tolist()
    for g, w in zip(got, want):
        assert (g == w).all()
    assert got[2].tolist() == [[3, 2, 0, 117], [0] * 4, [3, 2, 0, 58], [3, 2, 0, 62], [2, 1, 0, 100], [1, 0, 0, 127]]
    assert _atoms(got[1][0, 1]) == set(range(3, 120)) and (got[1][0, 1] != 0).all() and _atoms(got[1][2, 2]) == set(range(61, 69))
    assert (got[1][2, 2] != 0).all()                               # a ring in both mask words
    x = torch.from_numpy(CR.token_rows(["C1CC1OCC", "CC(=O)O", "C=F", "CCN", "C1CC1OCC"], v, T=12))
    x[0, 9] = v.pad                                                # no <eos>
    x[1, 3] = -1
    x[3, 2] = len(v)
    wide = torch.full((5, 40), v.eos, dtype=torch.long)
    wide[:, :12] = x
    pre = (torch.full((5,), 0x7f7f7f7f, dtype=torch.int32), torch.full((5, 16, 2), 0x7f7f7f7f7f7f7f7f, dtype=torch.int64),
           torch.full((5, 4), 0x7f7f7f7f, dtype=torch.int32), torch.full((5, 16), 0x7f7f7f7f7f7f7f7f, dtype=torch.int64))
    ops.smiles_fragment_host(wide[:, :12], tok, chem, v.eos, *pre)
    status, mask, desc, key = pre
    assert status.tolist() == [1, 1, 2, 1, 0] and not mask[:4].any() and not desc[:4].any() and not key[:4].any()
    one = FG.expected(["C1CC1OCC"])
    assert desc[4].tolist() == [2, 1, 0, 3] and (mask[4].numpy() == one[1][0]).all() and (key[4].numpy() == one[3][0]).all()
    pre = (torch.full((5, 20), 0x7f7f7f7f, dtype=torch.int64), torch.full((5,), 0x7f7f7f7f, dtype=torch.int32),
           torch.full((5,), 0x7f7f7f7f, dtype=torch.int32), torch.full((5, 4), 0x7f7f7f7f, dtype=torch.int32))
    got = ops.smiles_fragment_smiles_host(wide[:, :12], tok, chem, emit, v.bos, v.eos, v.pad, 1, 127, 20, *pre)
    assert got[2].tolist() == [1, 1, 2, 1, 0] and got[1].tolist() == [2, 2, 2, 2, 5] and got[3].tolist() == [[0] * 4] * 4 + [[3, 2, 0, 1]]
    assert got[0][:4].tolist() == [[v.bos, v.eos] + [v.pad] * 18] * 4
    assert got[0][4].tolist() == v.string2ids("CCO", add_bos=True, add_eos=True) + [v.pad] * 15


def test_entries_refuse_bad_arguments_before_launching():
    """Everything below returns before any HIP call (no device needed): the matrices of the scaffold entries, and frag < 0."""
    lib = L.load()
    fake = ctypes.c_void_p(256)                                  # never dereferenced: every call below is refused first

    def rows(name, B=4, T=8, V=29, x=fake, ld=8, tok=fake, chem=fake, eos=1, status=fake, mask=fake, desc=fake, key=fake):
        tail = (None,) if name == KEYS_ENTRIES[0] else ()
        return getattr(lib, name)(B, T, V, x, ld, tok, chem, eos, status, mask, desc, key, *tail)
    for name in (KEYS_ENTRIES[0], KEYS_ENTRIES[2]):
        assert rows(name, B=0) == -1 and rows(name, T=0, ld=0) == -1 and rows(name, V=0, eos=0) == -1 and rows(name, V=65) == -3
        assert rows(name, x=None) == -1 and rows(name, tok=None) == -1 and rows(name, chem=None) == -1 and rows(name, status=None) == -1
        assert rows(name, desc=None) == -1 and rows(name, key=None) == -1 and rows(name, ld=7) == -1 and rows(name, eos=29) == -1
        assert rows(name, eos=-1) == -1 and rows(name, V=65, mask=None) == -3

    def corpus(tokens=fake, offsets=fake, N=100, V=29, tok=fake, chem=fake, status=fake, mask=fake, desc=fake, key=fake):
        return lib.mvae_smiles_fragment_corpus(tokens, offsets, N, V, tok, chem, status, mask, desc, key, None)
    assert corpus(N=0) == -1 and corpus(N=-3) == -1 and corpus(V=0) == -1 and corpus(V=65) == -3
    assert corpus(tokens=None) == -1 and corpus(offsets=None) == -1 and corpus(tok=None) == -1 and corpus(chem=None) == -1
    assert corpus(status=None) == -1 and corpus(desc=None) == -1 and corpus(key=None) == -1

    def srows(name, B=4, T=8, V=29, x=fake, ld=8, tok=fake, chem=fake, emit=fake, bos=0, eos=1, pad=2, mc=127, T_out=129, out=fake,
              out_len=fake, status=fake, frag=0):
        tail = (None, frag, None, None) if name == SMILES_ENTRIES[0] else (frag, None)
        return getattr(lib, name)(B, T, V, x, ld, tok, chem, emit, bos, eos, pad, mc, T_out, out, out_len, status, *tail)
    for name in (SMILES_ENTRIES[0], SMILES_ENTRIES[2]):
        assert srows(name, B=0) == -1 and srows(name, T=0, ld=0) == -1 and srows(name, V=0, eos=0) == -1 and srows(name, V=65) == -3
        assert srows(name, x=None) == -1 and srows(name, tok=None) == -1 and srows(name, chem=None) == -1 and srows(name, status=None) == -1
        assert srows(name, emit=None) == -1 and srows(name, out=None) == -1 and srows(name, out_len=None) == -1 and srows(name, ld=7) == -1
        assert srows(name, eos=29) == -1 and srows(name, eos=-1) == -1 and srows(name, mc=0) == -1 and srows(name, mc=128) == -1
        assert srows(name, T_out=1) == -1 and srows(name, bos=-1) == -1 and srows(name, pad=65536) == -1 and srows(name, V=65, out=None) == -3
        assert srows(name, frag=-1) == -1 and srows(name, V=65, frag=-1) == -3

    def scorpus(tokens=fake, offsets=fake, N=100, rows=fake, B=4, V=29, tok=fake, chem=fake, emit=fake, mc=100, stride=100, tokens_out=fake,
                offsets_out=fake, status=fake, frag=0):
        return lib.mvae_smiles_fragment_smiles_corpus(tokens, offsets, N, rows, B, V, tok, chem, emit, mc, stride, tokens_out, offsets_out,
                                                      status, None, None, frag, None, None)
    assert scorpus(N=0) == -1 and scorpus(B=0) == -1 and scorpus(V=0) == -1 and scorpus(V=65) == -3 and scorpus(rows=None) == -1
    assert scorpus(tokens=None) == -1 and scorpus(offsets=None) == -1 and scorpus(tok=None) == -1 and scorpus(chem=None) == -1
    assert scorpus(emit=None) == -1 and scorpus(status=None) == -1 and scorpus(tokens_out=None) == -1 and scorpus(offsets_out=None) == -1
    assert scorpus(mc=0) == -1 and scorpus(mc=128, stride=128) == -1 and scorpus(stride=99) == -1 and scorpus(frag=-1) == -1
    with pytest.raises(ValueError, match=r"max_content must be in \[1, 127\]"):
        _host_smiles(["CCO"], 0, max_content=128)
    with pytest.raises(ValueError, match="frag must be >= 0"):
        _host_smiles(["CCO"], -1)


def test_python_surface_raises_before_device_work():
    torch.manual_seed(0)
    model = MV.VAE(VC.OneHotVocab(list("CNO(=)1")), dtype=torch.float32)
    big = MV.VAE(VC.OneHotVocab([chr(65 + i) for i in range(61)]), dtype=torch.float32)
    ds = D.MosesDeviceDataset(["CCO", "CC"], model.vocabulary, device="cpu")
    with pytest.raises(ValueError, match="fragments=True supports at most 64 ids"):
        mv.moses_generate(big, 4, max_len=8, fragments=True)
    with pytest.raises(ValueError, match="at most 64"):
        D.MosesDeviceDataset(["AB"], big.vocabulary, device="cpu").fragments()
    with pytest.raises(ValueError, match="at most 64"):
        D.MosesDeviceDataset(["AB"], big.vocabulary, device="cpu").rows_with_fragment(["AB"])
    with pytest.raises(ValueError, match="at most 64"):
        D.fragment_smiles(["AB"], big.vocabulary, device="cpu")
    with pytest.raises(ValueError, match="at least one string"):
        D.fragment_smiles([], model.vocabulary, device="cpu")
    with pytest.raises(L.MvaeError, match="MI355X only"):                            # a CPU model: no fallback
        mv.moses_generate(model, 4, max_len=8, fragments=True)
    for call in (lambda: model.fragments(["CCO"]), lambda: model.fragment_smiles(["CCO"]), ds.fragments, ds.fragment_histogram,
                 lambda: ds.rows_with_fragment(["CCO"])):
        with pytest.raises(L.MvaeError, match="MI355X only"):
            call()
