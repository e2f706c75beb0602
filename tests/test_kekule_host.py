"""CPU tests of the kekulisation surface (mvae_smiles_kekule_rows / _corpus / _host, VAE.kekule, VAE.chem_valid(kekule=),
MosesDeviceDataset.kekule, moses_generate(kekule=)): the host entry (the walk of csrc/smiles_graph.hpp with the recorder of
csrc/smiles_rounds.hpp and the matcher of csrc/kekule.hip, compiled for the CPU) against the reference of tests/kekule_ref.py -- which
takes its matching size from networkx -- on a hand-stated table, the mutation corpus and a corpus of random polycyclic aromatic systems
built to defeat bipartite and blossom-free matchers; the mate output, invariance under re-spelling, the edge rows, the argument checks of
the new entries (refused before anything is launched), the ABI, and the compiler's resource remarks for the new kernels."""
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
import kekule_ref as KR
import scaffold_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mvae_smiles_kekule_rows", "mvae_smiles_kekule_corpus", "mvae_smiles_kekule_host")

# (string, |N|, pairs), stated by hand; atoms are numbered in string order.  Status 0 <=> |N| == 2 * pairs.
PASS = [
    ("c1ccccc1", 6, 3),                         # benzene
    ("c1cc[nH]c1", 4, 2),                       # pyrrole: [nH] has U = v0 = 3 and takes no double bond
    ("c1ccoc1", 4, 2),                          # furan
    ("c1ccsc1", 4, 2),                          # thiophene
    ("c1cnc[nH]1", 4, 2),                       # imidazole: c=c and c=n
    ("c1cscn1", 4, 2),                          # thiazole
    ("c1ccncc1", 6, 3),                         # pyridine
    ("c1ccc2ccccc2c1", 10, 5),                  # naphthalene
    ("c1ccc2[nH]ccc2c1", 8, 4),                 # indole
    ("c1ccc2cccc2cc1", 10, 5),                  # azulene: an odd ring fused to an odd ring
    ("O=c1cccc[nH]1", 4, 2),                    # 2-pyridone: c(=O) has U = 4 and [nH] U = 3, the four CH pair up
    ("Cn1cnc2c1c(=O)n(C)c(=O)n2C", 4, 2),       # caffeine: c8=n9 in the five-ring, the two fusion carbons
    ("O=c1ccc(=O)cc1", 4, 2),                   # quinone written aromatic: two c=c
    ("[O-][n+]1ccccc1", 6, 3),                  # pyridine N-oxide: [n+] with three neighbours has U = 3, v0 = 4
    ("C[n+]1ccccc1", 6, 3),                     # N-methylpyridinium
    ("c1ccccc1c1ccccc1", 12, 6),                # biphenyl
    ("CC(=O)Oc1ccccc1C(=O)O", 6, 3),            # aspirin
    ("[O-][N+](=O)c1ccccc1", 6, 3),             # nitrobenzene
    ("[cH-]1cccc1", 4, 2),                      # cyclopentadienyl anion: [cH-] has U = v0 = 3
    ("c12ccc(n1)c2", 6, 3),                     # the blossom case: a three-ring and a five-ring sharing the bond 0-4 (|E| = 7)
    ("c1(C)(C)cccc1", 4, 2),                    # a FIVE-ring: atom 0 has four sigma bonds and is not in N, the other four pair up
    ("CCO", 0, 0),
]
FAIL = [
    ("c1cccn1", 5, 2),                          # pyrrole without its H
    ("c1cccc1", 5, 2),
    ("c1cncn1", 5, 2),
    ("c1(C)(C)ccccc1", 5, 2),                   # the six-ring with a quaternary aromatic carbon: five atoms left on a path
    ("c1ccc2cccc2c1", 9, 4),                    # indene-like: nine atoms
    ("c12cc1c3c2oc[nH]c3", 7, 3),
]


def _host(strings, T=None, **kw):
    v = CR.vocabulary()
    x = torch.from_numpy(CR.token_rows(strings, v, T))
    return tuple(None if t is None else t.numpy() for t in ops.smiles_kekule_host(x, VC.smiles_token_table(v), VC.smiles_chem_table(v), v.eos, **kw))


def _equal_rows(got, want_status, want_desc, strings):
    wrong = np.nonzero((got[0] != want_status) | (got[1] != want_desc).any(1))[0]
    assert wrong.size == 0, [(strings[i], int(got[0][i]), got[1][i].tolist(), int(want_status[i]), want_desc[i].tolist()) for i in wrong[:3]]


def test_entries_are_declared_bound_and_exported_at_abi_12():
    text = open(os.path.join(ROOT, "include", "mvae.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", header).group(1)) == 12 == L.ABI_VERSION
    lib = L.load()
    assert lib.mvae_abi_version() == 12
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert len(L.SIGNATURES[ENTRIES[0]][1]) == len(L.SIGNATURES[ENTRIES[2]][1]) + 1 == 12       # the host entry: no stream
    assert len(L.SIGNATURES[ENTRIES[1]][1]) == 10
    assert re.search(r"#define\s+MVAE_SMILES_KEKULE\s+7\b", header) and ops.SMILES_STATUS_KEKULE == 7 == KR.KEKULE
    assert ops.KEKULE_STATUS_NAMES == ops.SMILES_STATUS_NAMES + ("kekule",) and len(ops.SMILES_STATUS_NAMES) == 7
    assert "Kekulisation" in text and "not rdkit's Kekulize" in text and "errs towards passing" in text
    for fn in (ops.smiles_kekule_rows, ops.smiles_kekule_corpus, ops.smiles_kekule_host, MV.VAE.kekule, D.MosesDeviceDataset.kekule):
        assert callable(fn)
    assert inspect.signature(mv.moses_generate).parameters["kekule"].default is False
    assert inspect.signature(MV.VAE.chem_valid).parameters["kekule"].default is False
    build = open(os.path.join(ROOT, "molecular-vae_amd", "csrc", "build.sh")).read()
    assert build.count("kekule moses_decode scaffold fingerprint smiles_graph elementwise") == 2
    assert "build/kekule.o build/moses_decode.o" in build and "build/tune/kekule.o build/tune/moses_decode.o" in build
    assert "smiles_rounds.hpp -nt build/$f.o" in build
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        body = open(os.path.join(ROOT, doc)).read()
        assert "kekulisable" in body and "not rdkit's Kekulize" in body, doc
        assert "rdkit-valid" not in body, doc
    for doc in ("README.md", "INTEGRATION.md"):
        assert "valence-consistent" in open(os.path.join(ROOT, doc)).read(), doc


def test_new_kernels_use_no_scratch(tmp_path):
    """The compiler's resource remarks for the two kernels of kekule.hip: scratch 0, no spills (nothing indexed at run time is a private
    array), and the LDS per block include/mvae.h states, at most 80 KiB so that two blocks fit a CU.  The build leaves the remarks in
    csrc/build/kekule.usage.txt; on a tree whose library was built another way the test compiles the device code itself."""
    csrc = os.path.join(ROOT, "molecular-vae_amd", "csrc")
    usage = os.path.join(csrc, "build", "kekule.usage.txt")
    sources = ("kekule.hip", "smiles_rounds.hpp", "smiles_graph.hpp", "smiles_syntax.hpp")
    if os.path.exists(usage) and os.path.getmtime(usage) >= max(os.path.getmtime(os.path.join(csrc, f)) for f in sources):
        text = open(usage, errors="replace").read()
    else:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                              "-c", os.path.join(csrc, "kekule.hip"), "-o", str(tmp_path / "kekule.dev.o")],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert run.returncode == 0, run.stderr[-2000:]
        text = run.stderr
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 2 and all(any(k in n for n in names) for k in ("rows_kernelIN3kek6KekuleE", "corpus_kernelIN3kek6KekuleE")), names
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 2
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 2 and re.findall(r"SGPRs Spill: (\d+)", text) == ["0"] * 2
    header = open(os.path.join(ROOT, "include", "mvae.h")).read()
    stated = int(re.search(r"#define\s+MVAE_KEKULE_LDS_BYTES\s+(\d+)", header).group(1))
    assert list(map(int, re.findall(r"LDS Size \[bytes/block\]: (\d+)", text))) == [stated] * 2 and stated <= 80 * 1024
    assert f"{stated} B" in header
    assert all(int(v) <= 128 for v in re.findall(r" VGPRs: (\d+)", text))


def test_hand_stated_table():
    """|N| and the size of a maximum matching stated by hand for every row (PASS: status 0, FAIL: status 7); the reference agrees with
    the hand, the host entry with both.  The two rows a blossom-free matcher gets wrong are in it: naive_pairs finds 2 of 3 pairs."""
    strings = [s for s, _, _ in PASS + FAIL]
    status, desc, mate = _host(strings)
    for i, (s, nn, pairs) in enumerate(PASS + FAIL):
        want = 0 if i < len(PASS) else KR.KEKULE
        assert (want == 0) == (nn == 2 * pairs)
        ref = KR.kekule(s)
        assert ref[0] == want and ref[1][0] == nn and ref[1][2] == pairs, (s, ref[:2])
        assert status[i] == want and desc[i].tolist() == ref[1] and desc[i, 3] == nn - 2 * pairs, (s, int(status[i]), desc[i].tolist(), ref[1])
        KR.check_mate(mate[i], ref[2], ref[3], pairs)
    by = {s: desc[i].tolist() for i, s in enumerate(strings)}
    assert by["c12ccc(n1)c2"] == [6, 7, 3, 0] and by["c12cc1c3c2oc[nH]c3"][2:] == [3, 1] and by["c1ccc2cccc2c1"] == [9, 10, 4, 1]
    for s in ("c12ccc(n1)c2", "c12cc1c3c2oc[nH]c3"):
        N, E = KR.graph(s)
        assert KR.naive_pairs(N, E) == 2 and KR.max_pairs(N, E) == 3
    # the bond between the rings of biphenyl is not in E; a bond between aromatic atoms that closes a non-aromatic ring is
    assert by["c1ccccc1c1ccccc1"][1] == 12
    fluorene = _host(["c1ccc2c(c1)Cc1ccccc12"])
    assert fluorene[0][0] == 0 and fluorene[1][0].tolist() == [12, 13, 6, 0]
    # rows the walk refuses keep their status and get zeros and no mates
    rejected = [s for s, st, _ in CR.REJECTED if st != CR.OK] + ["C" * 128]
    out = _host(rejected)
    assert set(out[0].tolist()) == {1, 2, 3, 4, 5, 6} and not out[1].any() and (out[2] == 255).all()


def test_host_entry_equals_the_reference_on_the_mutation_corpus():
    """Status and desc, every one of the 4 250 rows.  The status differs from the graph entry's only where the reference says 7.  The
    input is not degenerate (asserted on the reference alone): of the 833 rows the walk calls 0, 606 kekulise and 227 do not."""
    strings, status, desc = KR.mutation_expected()
    walk = CR.corpus_and_expected()[1][0]
    n0, n7 = int((status == 0).sum()), int((status == KR.KEKULE).sum())
    print("rows:", len(strings), "walk status 0:", int((walk == 0).sum()), "kekulisable:", n0, "not:", n7)
    assert n0 >= 20 and n7 >= 20 and n0 + n7 == (walk == 0).sum() and ((status == walk) | (status == KR.KEKULE)).all()
    assert not desc[(status != 0) & (status != KR.KEKULE)].any()
    got = _host(strings)
    _equal_rows(got, status, desc, strings)
    v = CR.vocabulary()
    graph_status = ops.smiles_graph_host(torch.from_numpy(CR.token_rows(strings, v)), VC.smiles_token_table(v), VC.smiles_chem_table(v), v.eos)[0].numpy()
    differs = graph_status != got[0]
    assert (got[0][differs] == KR.KEKULE).all() and (graph_status[differs] == 0).all() and differs.sum() == n7
    other = (status != 0) & (status != KR.KEKULE)
    assert (got[2][other] == 255).all()


def test_host_entry_equals_the_reference_on_ring_systems():
    """3 000 random polycyclic aromatic systems (kekule_ref.ring_system_corpus, seed 7): status and desc equal networkx's on every row.
    Asserted on the reference alone, before the library is looked at: at least 500 rows that kekulise and 500 that do not, at least 1 000
    whose (N, E) is not bipartite, at least 20 on which the blossom-free naive_pairs is short of the maximum.  Seed 7 gives 1 441
    kekulisable, 1 559 not (71 with deficiency >= 2), 2 400 non-bipartite, naive_pairs short on 34.  The negative control: the same
    comparison with naive_pairs in place of the library's pairs column fails."""
    strings, status, desc, graphs = KR.ring_system_expected()
    n0, n7 = int((status == 0).sum()), int((status == KR.KEKULE).sum())
    odd = sum(not KR.bipartite(N, E) for N, E in graphs)
    naive = np.array([KR.naive_pairs(N, E) for N, E in graphs], np.int32)
    print("rows:", len(strings), "kekulisable:", n0, "not:", n7, "deficiency >= 2:", int((desc[:, 3] >= 2).sum()), "non-bipartite:", odd,
          "naive_pairs short:", int((naive < desc[:, 2]).sum()))
    assert len(strings) == 3000 and n0 + n7 == 3000 and n0 >= 500 and n7 >= 500 and odd >= 1000
    assert (naive <= desc[:, 2]).all() and (naive < desc[:, 2]).sum() >= 20
    got = _host(strings)
    _equal_rows(got, status, desc, strings)
    fake = got[1].copy()
    fake[:, 2] = naive
    with pytest.raises(AssertionError):
        _equal_rows((got[0], fake), status, desc, strings)
    for i, (N, E) in enumerate(graphs):
        KR.check_mate(got[2][i], N, E, int(desc[i, 2]))


def test_mate_is_a_maximum_matching_and_independent_of_the_other_outputs():
    """On the mutation corpus: for status 0 and 7 a valid matching of (N, E) with exactly `pairs` pairs, all 255 otherwise; identical with
    prefilled outputs; mate=False leaves status and desc unchanged."""
    strings, status, desc = KR.mutation_expected()
    got = _host(strings)
    seen = 0
    for i, s in enumerate(strings):
        if status[i] in (0, KR.KEKULE):
            N, E = KR.graph(s)
            KR.check_mate(got[2][i], N, E, int(desc[i, 2]))
            seen += bool(N)
        else:
            assert (got[2][i] == 255).all()
    assert seen >= 300
    n = len(strings)
    pre = (torch.full((n,), 0x7f7f7f7f, dtype=torch.int32), torch.full((n, 4), 0x7f7f7f7f, dtype=torch.int32),
           torch.full((n, 128), 0x7f, dtype=torch.uint8))
    again = _host(strings, status=pre[0], desc=pre[1], mate=pre[2])
    assert all((a == g).all() for a, g in zip(again, got))
    without = _host(strings, mate=False)
    assert without[2] is None and (without[0] == got[0]).all() and (without[1] == got[1]).all()


def test_result_does_not_depend_on_the_spelling():
    """Every FORMULAS string and the hand table, each in six rewrites: the rewriter is checked first (status 0 under the walk, the
    original's formula), then status and desc are equal."""
    rng = np.random.RandomState(13)
    originals = [s for s, _ in CR.FORMULAS] + [s for s, _, _ in PASS + FAIL]
    rewrites = [[SR.rewrite(s, rng)[0] for _ in range(6)] for s in originals]
    changed = 0
    for s, group in zip(originals, rewrites):
        a0 = CR.analyse(s)
        for t in group:
            a = CR.analyse(t)
            assert a[0] == CR.OK == a0[0] and CR.hill(a[3], a[2][6]) == CR.hill(a0[3], a0[2][6]), (s, t, a)
            changed += t != s
    assert changed >= 3 * len(originals)
    st0, desc0, _ = _host(originals)
    st1, desc1, _ = _host([t for group in rewrites for t in group])
    for i, group in enumerate(rewrites):
        for j, t in enumerate(group):
            assert st1[i * 6 + j] == st0[i] and desc1[i * 6 + j].tolist() == desc0[i].tolist(), (originals[i], t)


def test_host_entry_edge_rows_and_prefilled_outputs():
    """kekule_ref.edge_rows: the 125-atom aromatic ring (127 tokens, the whole graph one odd cycle): status 7 with 62 pairs; the 124-atom
    ring: status 0; 128 tokens: TOO_LONG; a ring whose closure joins atoms 3 and 69; 25 three-rings in a chain (25 searches that each
    end in a blossom and fail) and 25 fused ones; all ten ring digits open at once; two systems of more than 100 atoms on which the
    blossom-free matcher is one pair short.  The stated figures, the reference and the host entry agree.  Then rows without <eos>,
    ids -1 and V, a strided view; every element of 0x7f-prefilled outputs is written."""
    v = CR.vocabulary()
    tok, chem = VC.smiles_token_table(v), VC.smiles_chem_table(v)
    rows = KR.edge_rows()
    strings = [r[0] for r in rows]
    assert len(strings[0]) == 127 and max(len(s) for s in strings) == 128
    want_status, want_desc = KR.expected(strings)
    assert want_status.tolist() == [r[1] for r in rows] and want_desc.tolist() == [r[2] for r in rows]
    got = _host(strings, T=140)
    _equal_rows(got, want_status, want_desc, strings)
    for i, s in enumerate(strings):
        if want_status[i] in (0, KR.KEKULE):
            N, E = KR.graph(s)
            KR.check_mate(got[2][i], N, E, int(want_desc[i, 2]))
        else:
            assert (got[2][i] == 255).all()
    for s in KR.BIG_BLOSSOMS:
        N, E = KR.graph(s)
        assert max(N) > 100 and KR.naive_pairs(N, E) == KR.max_pairs(N, E) - 1
    x = torch.from_numpy(CR.token_rows(["c1cccn1", "c1ccccc1", "C=F", "c1ccncc1", "c1ccoc1"], v, T=12))
    x[0, 8] = v.pad                                                # no <eos>
    x[1, 3] = -1
    x[3, 2] = len(v)
    wide = torch.full((5, 40), v.eos, dtype=torch.long)
    wide[:, :12] = x
    status = torch.full((5,), 0x7f7f7f7f, dtype=torch.int32)
    desc = torch.full((5, 4), 0x7f7f7f7f, dtype=torch.int32)
    mate = torch.full((5, 128), 0x7f, dtype=torch.uint8)
    ops.smiles_kekule_host(wide[:, :12], tok, chem, v.eos, status, desc, mate)
    assert status.tolist() == [1, 1, 2, 1, 0] and not desc[:4].any() and (mate[:4] == 255).all()
    assert desc[4].tolist() == [4, 3, 2, 0] and sorted(mate[4, :5].tolist()) == [0, 1, 2, 4, 255] and (mate[4, 5:] == 255).all()
    without = ops.smiles_kekule_host(wide[:, :12], tok, chem, v.eos, mate=False)
    assert without[2] is None and torch.equal(without[0], status) and torch.equal(without[1], desc)


def test_entries_refuse_bad_arguments_before_launching():
    """Everything below returns before any HIP call (no device needed)."""
    lib = L.load()
    fake = ctypes.c_void_p(256)                                  # never dereferenced: every call below is refused first

    def rows(name, B=4, T=8, V=29, x=fake, ld=8, tok=fake, chem=fake, eos=1, status=fake, desc=fake, mate=fake):
        tail = (None,) if name == ENTRIES[0] else ()
        return getattr(lib, name)(B, T, V, x, ld, tok, chem, eos, status, desc, mate, *tail)
    for name in (ENTRIES[0], ENTRIES[2]):
        assert rows(name, B=0) == -1 and rows(name, T=0, ld=0) == -1 and rows(name, V=0, eos=0) == -1 and rows(name, V=65) == -3
        assert rows(name, x=None) == -1 and rows(name, tok=None) == -1 and rows(name, chem=None) == -1 and rows(name, status=None) == -1
        assert rows(name, desc=None) == -1 and rows(name, ld=7) == -1 and rows(name, eos=29) == -1
        assert rows(name, eos=-1) == -1 and rows(name, V=65, mate=None) == -3 and rows(name, B=0, mate=None) == -1

    def corpus(tokens=fake, offsets=fake, N=100, V=29, tok=fake, chem=fake, status=fake, desc=fake, mate=fake):
        return lib.mvae_smiles_kekule_corpus(tokens, offsets, N, V, tok, chem, status, desc, mate, None)
    assert corpus(N=0) == -1 and corpus(N=-3) == -1 and corpus(V=0) == -1 and corpus(V=65) == -3
    assert corpus(tokens=None) == -1 and corpus(offsets=None) == -1 and corpus(tok=None) == -1 and corpus(chem=None) == -1
    assert corpus(status=None) == -1 and corpus(desc=None) == -1 and corpus(N=0, mate=None) == -1


def test_python_surface_raises_before_device_work():
    torch.manual_seed(0)
    model = MV.VAE(VC.OneHotVocab(list("CNOc(=)1")), dtype=torch.float32)
    big = MV.VAE(VC.OneHotVocab([chr(65 + i) for i in range(61)]), dtype=torch.float32)
    ds = D.MosesDeviceDataset(["CCO", "c1ccccc1"], model.vocabulary, device="cpu")
    with pytest.raises(ValueError, match="kekule=True supports at most 64 ids"):
        mv.moses_generate(big, 4, max_len=8, kekule=True)
    with pytest.raises(ValueError, match="at most 64"):
        D.MosesDeviceDataset(["AB"], big.vocabulary, device="cpu").kekule()
    with pytest.raises(L.MvaeError, match="MI355X only"):                            # a CPU model: no fallback
        mv.moses_generate(model, 4, max_len=8, kekule=True)
    with pytest.raises(L.MvaeError, match="MI355X only"):
        model.kekule(["CCO"])
    with pytest.raises(L.MvaeError, match="MI355X only"):
        model.chem_valid(["CCO"], kekule=True)
    with pytest.raises(L.MvaeError, match="MI355X only"):
        ds.kekule()
