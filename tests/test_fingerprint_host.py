"""CPU tests of the fingerprint surface (mvae_smiles_fp_rows / _corpus / _host, mvae_tanimoto_knn, mvae_tanimoto_sum, VAE.fingerprints /
tanimoto, MosesDeviceDataset.fingerprints / nearest_fingerprints, moses_generate(int_div=, snn=)): the host entry (the walk of
csrc/smiles_graph.hpp with the recorder and the rounds of csrc/fingerprint.hip, compiled for the CPU) against the reference of
tests/fp_ref.py on the mutation corpus, hand-stated invariances, the argument checks of every new entry (refused before anything is
launched), the ABI, and the compiler's resource remarks for the new kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import molecular_vae_amd as mv
from molecular_vae_amd import _lib as L, data as D, mosesvae as MV, vocab as VC, ops
import chem_ref as CR
import fp_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP_ENTRIES = ("mvae_smiles_fp_rows", "mvae_smiles_fp_corpus", "mvae_smiles_fp_host")
ENTRIES = FP_ENTRIES + ("mvae_tanimoto_knn_workspace", "mvae_tanimoto_knn", "mvae_tanimoto_sum_workspace", "mvae_tanimoto_sum")


def _host(strings, T=None):
    v = CR.vocabulary()
    x = torch.from_numpy(CR.token_rows(strings, v, T))
    status, fp = ops.smiles_fp_host(x, VC.smiles_token_table(v), VC.smiles_chem_table(v), v.eos)
    return status.numpy(), fp.numpy()


def test_entries_are_declared_bound_and_exported_at_abi_12():
    text = open(os.path.join(ROOT, "include", "mvae.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", header).group(1)) == 12 == L.ABI_VERSION
    lib = L.load()
    assert lib.mvae_abi_version() == 12
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert len(L.SIGNATURES[FP_ENTRIES[0]][1]) == len(L.SIGNATURES[FP_ENTRIES[2]][1]) + 1 == 11        # the host entry: no stream
    assert len(L.SIGNATURES[FP_ENTRIES[1]][1]) == 9
    assert re.search(r"#define\s+MVAE_FP_WORDS\s+16\b", header) and ops.FP_WORDS == 16 == FR.WORDS
    assert "Circular fingerprint" in text and "NOT rdkit's Morgan fingerprint" in text and "not kekulised" in text
    for fn in (ops.smiles_fp_rows, ops.smiles_fp_corpus, ops.smiles_fp_host, ops.tanimoto_knn, ops.tanimoto_sum, MV.VAE.fingerprints,
               MV.VAE.tanimoto, D.MosesDeviceDataset.fingerprints, D.MosesDeviceDataset.nearest_fingerprints):
        assert callable(fn)
    build = open(os.path.join(ROOT, "molecular-vae_amd", "csrc", "build.sh")).read()
    assert build.count("fingerprint smiles_graph elementwise") == 2
    assert "build/fingerprint.o build/smiles_graph.o" in build and "build/tune/fingerprint.o build/tune/smiles_graph.o" in build
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        body = open(os.path.join(ROOT, doc)).read()
        assert "not rdkit's Morgan fingerprint" in body, doc


def test_new_kernels_use_no_scratch(tmp_path):
    """The compiler's resource remarks for the kernels of fingerprint.hip: scratch 0 and no spills in all six (nothing indexed at run
    time is a private array), 112 KiB of LDS in the two fingerprint kernels.  The build leaves the remarks in
    csrc/build/fingerprint.usage.txt; on a tree whose library was built another way the test compiles the device code itself."""
    csrc = os.path.join(ROOT, "molecular-vae_amd", "csrc")
    usage = os.path.join(csrc, "build", "fingerprint.usage.txt")
    if os.path.exists(usage) and os.path.getmtime(usage) >= max(os.path.getmtime(os.path.join(csrc, f))
                                                                for f in ("fingerprint.hip", "smiles_graph.hpp", "smiles_syntax.hpp")):
        text = open(usage, errors="replace").read()
    else:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                              "-c", os.path.join(csrc, "fingerprint.hip"), "-o", str(tmp_path / "fingerprint.dev.o")],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert run.returncode == 0, run.stderr[-2000:]
        text = run.stderr
    names = re.findall(r"Function Name: (\S+)", text)
    kernels = ("rows_kernelINS_2FpE", "corpus_kernelINS_2FpE", "tanimoto_knn_scan_kernel", "tanimoto_knn_merge_kernel", "tanimoto_sum_kernel",
               "tanimoto_sum_final_kernel")
    assert len(names) == 6 and all(any(k in n for n in names) for k in kernels), names
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 6
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 6 and re.findall(r"SGPRs Spill: (\d+)", text) == ["0"] * 6
    lds = dict(zip(names, map(int, re.findall(r"LDS Size \[bytes/block\]: (\d+)", text))))
    assert [v for n, v in lds.items() if "_kernelINS_2FpE" in n] == [112 * 1024] * 2
    assert all(int(v) <= 128 for v in re.findall(r" VGPRs: (\d+)", text))


def test_host_entry_equals_the_reference_on_the_mutation_corpus():
    """Word for word on the 4 250 rows; the status is the graph entry's.  The input is not degenerate: at least 800 rows with status 0,
    at least 600 distinct non-zero fingerprints (asserted on the reference alone)."""
    strings, status, want = FR.corpus_fingerprints()
    ok = status == 0
    distinct = {w.tobytes() for w in want if w.any()}
    pop = np.unpackbits(want[ok].view(np.uint8), axis=1).sum(1)
    print("rows:", len(strings), "status 0:", int(ok.sum()), "distinct fingerprints:", len(distinct), "popcounts:", pop.min(), "-", pop.max())
    assert ok.sum() >= 800 and len(distinct) >= 600 and pop.min() >= 1
    assert not want[~ok].any() and want[ok].any(1).all()
    got_status, got = _host(strings)
    assert (got_status == status).all()
    wrong = np.nonzero((got != want).any(1))[0]
    assert wrong.size == 0, [(strings[i], got[i].tolist(), want[i].tolist()) for i in wrong[:3]]
    v = CR.vocabulary()
    graph_status = ops.smiles_graph_host(torch.from_numpy(CR.token_rows(strings, v)), VC.smiles_token_table(v), VC.smiles_chem_table(v), v.eos)[0]
    assert (graph_status.numpy() == got_status).all()


def test_hand_stated_invariances():
    """Atom numbering does not matter; different atoms and aromatic against Kekule spelling do; every status but 0 gives zeros."""
    for same in (("CCO", "OCC", "C(O)C"), ("c1ccccc1C", "Cc1ccccc1", "c1(C)ccccc1")):
        status, fp = _host(list(same))
        assert (status == 0).all() and fp[0].any() and (fp == fp[0]).all(), same
        assert (FR.fingerprints(list(same)) == fp).all()
    status, fp = _host(["CCO", "CCN", "C1=CC=CC=C1", "c1ccccc1", "CC(C)=O", "CC(=O)C", "C[N+](C)(C)C", "[H]C", "C"])
    assert (status == 0).all()
    assert (fp[0] != fp[1]).any() and (fp[2] != fp[3]).any() and (fp[4] == fp[5]).all() and (fp[7] != fp[8]).any()
    bits = lambda row: int(np.unpackbits(row.view(np.uint8)).sum())
    assert bits(fp[8]) == 3 and 1 <= bits(fp[0]) <= 9                                  # one atom: three rounds; three atoms: at most nine bits
    rejected = [s for s, st, _ in CR.REJECTED if st != CR.OK] + ["C" * 128]
    status, fp = _host(rejected)
    assert set(status.tolist()) == {1, 2, 3, 4, 5, 6} and not fp.any()
    # bit b lives in word b >> 6, bit b & 63
    want = np.zeros(16, np.uint64)
    for b in FR.bits("CCO"):
        want[b >> 6] |= np.uint64(1) << np.uint64(b & 63)
    assert (_host(["CCO"])[1][0].view(np.uint64) == want).all()


def test_host_entry_edge_rows_and_prefilled_outputs():
    """The 127-token chain and the 128-token one, a ring between atom 3 and atom 69, 25 ring closures in one row, a cage, a 15-deep
    nest, a strided view, a row without <eos>, ids outside the vocabulary; every element of prefilled outputs is written."""
    v = CR.vocabulary()
    tok, chem = VC.smiles_token_table(v), VC.smiles_chem_table(v)
    many = "C1CC1" * 25 + "CC"
    fused = "C12C3C4C1C5C2C3C45" + "C" * 100                          # cubane: five closures on eight atoms, digits reused nowhere
    strings = ["C" * 127, "C" * 128, "CCC1" + "C" * 66 + "1", "C" + "(C" * 15 + ")" * 15, many, fused, "c1ccccc1" * 15 + "C" * 6 + "c"]
    status, fp = _host(strings, T=140)
    assert status.tolist() == [0, CR.TOO_LONG, 0, 0, 0, 0, CR.AROMATIC]
    assert status.tolist() == [CR.analyse(s)[0] for s in strings]
    assert (fp == FR.fingerprints(strings)).all() and not fp[1].any() and not fp[6].any()
    x = torch.from_numpy(CR.token_rows(["CCO", "CC(=O)O", "C=F", "CCN", "CCO"], v, T=12))
    x[0, 4] = v.pad                                                # no <eos>
    x[1, 3] = -1
    x[3, 2] = len(v)
    wide = torch.full((5, 40), v.eos, dtype=torch.long)
    wide[:, :12] = x
    status = torch.full((5,), 0x7f7f7f7f, dtype=torch.int32)
    fp = torch.full((5, 16), 0x7f7f7f7f7f7f7f7f, dtype=torch.int64)
    ops.smiles_fp_host(wide[:, :12], tok, chem, v.eos, status, fp)
    assert status.tolist() == [1, 1, 2, 1, 0] and not fp[:4].any() and (fp[4].numpy() == FR.fingerprint("CCO")).all()


def test_reference_similarity_and_knn_on_hand_cases():
    """The numpy side of fp_ref against hand-made bit rows: 2 / 3, an empty union, ties by the lower row, the excluded row, the tail."""
    rows = np.zeros((5, 16), np.int64)
    rows[0, 0] = 0b0111
    rows[1, 0] = 0b0011
    rows[2, 0] = 0b0011
    rows[3, 15] = 1
    sim = FR.similarity(rows[:1], rows)
    assert sim.dtype == np.float32 and sim[0].tolist() == [1.0, float(np.float32(2) / np.float32(3)), float(np.float32(2) / np.float32(3)), 0.0, 0.0]
    assert FR.similarity(rows[4:], rows[4:])[0, 0] == 0.0
    s, j = FR.knn(sim, 3)
    assert j.tolist() == [[0, 1, 2]] and FR.ties_at(sim, 2) == 1 and FR.ties_at(sim, 1) == 0
    s, j = FR.knn(sim, 5, exclude=np.array([1]))
    assert j.tolist() == [[0, 2, 3, 4, -1]] and s[0, 4] == -1.0
    assert FR.pair_sum(FR.similarity(rows, rows)) == pytest.approx(3 + 1 + 4 * (2 / 3) + 2, rel=1e-6)
    assert FR.pair_sum(FR.similarity(rows, rows), skip_diagonal=True) == pytest.approx(4 * (2 / 3) + 2, rel=1e-6)


def test_entries_refuse_bad_arguments_before_launching():
    """Everything below returns before any HIP call (no device needed)."""
    lib = L.load()
    fake = ctypes.c_void_p(256)                                  # never dereferenced: every call below is refused first

    def rows(name, B=4, T=8, V=29, x=fake, ld=8, tok=fake, chem=fake, eos=1, status=fake, fp=fake):
        tail = (None,) if name == FP_ENTRIES[0] else ()
        return getattr(lib, name)(B, T, V, x, ld, tok, chem, eos, status, fp, *tail)
    for name in (FP_ENTRIES[0], FP_ENTRIES[2]):
        assert rows(name, B=0) == -1 and rows(name, T=0, ld=0) == -1 and rows(name, V=0, eos=0) == -1 and rows(name, V=65) == -3
        assert rows(name, x=None) == -1 and rows(name, tok=None) == -1 and rows(name, chem=None) == -1 and rows(name, status=None) == -1
        assert rows(name, fp=None) == -1 and rows(name, ld=7) == -1 and rows(name, eos=29) == -1 and rows(name, eos=-1) == -1

    def corpus(tokens=fake, offsets=fake, N=100, V=29, tok=fake, chem=fake, status=fake, fp=fake):
        return lib.mvae_smiles_fp_corpus(tokens, offsets, N, V, tok, chem, status, fp, None)
    assert corpus(N=0) == -1 and corpus(N=-3) == -1 and corpus(V=0) == -1 and corpus(V=65) == -3
    assert corpus(tokens=None) == -1 and corpus(offsets=None) == -1 and corpus(tok=None) == -1 and corpus(chem=None) == -1
    assert corpus(status=None) == -1 and corpus(fp=None) == -1

    def knn(Q=4, N=100000, k=4, q=fake, table=fake, exclude=None, sim=fake, idx=fake, ws=fake, nb=1 << 30):
        return lib.mvae_tanimoto_knn(Q, N, k, q, table, exclude, sim, idx, ws, nb, None)
    assert knn(Q=0) == -1 and knn(N=0) == -1 and knn(k=0) == -1 and knn(q=None) == -1 and knn(table=None) == -1 and knn(sim=None) == -1
    assert knn(idx=None) == -1 and knn(q=ctypes.c_void_p(264)) == -1 and knn(table=ctypes.c_void_p(264)) == -1 and knn(k=33) == -3
    need = lib.mvae_tanimoto_knn_workspace(4, 100000, 4)
    assert need > 0 and need % (4 * 4 * 12) == 0 and knn(ws=None) == -2 and knn(nb=need - 1) == -2 and knn(ws=ctypes.c_void_p(257), nb=need) == -1
    assert lib.mvae_tanimoto_knn_workspace(4, 256, 4) == 0 == lib.mvae_tanimoto_knn_workspace(4, 100000, 33)
    assert lib.mvae_tanimoto_knn_workspace(0, 100, 4) == 0 == lib.mvae_tanimoto_knn_workspace(4, 0, 4)
    assert lib.mvae_tanimoto_knn_workspace(64, 100000, 4) == 16 * lib.mvae_tanimoto_knn_workspace(4, 100000, 4)     # (Q, N, k) alone

    def total(M=100, N=100, a=fake, b=fake, out=fake, ws=fake, nb=1 << 30):
        return lib.mvae_tanimoto_sum(M, N, a, b, 0, out, ws, nb, None)
    assert total(M=0) == -1 and total(N=0) == -1 and total(a=None) == -1 and total(b=None) == -1 and total(out=None) == -1
    assert total(a=ctypes.c_void_p(264)) == -1 and total(b=ctypes.c_void_p(264)) == -1
    need = lib.mvae_tanimoto_sum_workspace(100, 100)
    assert need >= 8 and need % 8 == 0 and total(ws=None) == -2 and total(nb=need - 1) == -2 and total(ws=ctypes.c_void_p(260), nb=need) == -1
    assert lib.mvae_tanimoto_sum_workspace(0, 5) == 0 == lib.mvae_tanimoto_sum_workspace(5, 0)


def test_python_surface_raises_before_device_work():
    torch.manual_seed(0)
    model = MV.VAE(VC.OneHotVocab(list("CNO(=)1")), dtype=torch.float32)
    big = MV.VAE(VC.OneHotVocab([chr(65 + i) for i in range(61)]), dtype=torch.float32)
    ds = D.MosesDeviceDataset(["CCO", "CC"], model.vocabulary, device="cpu")
    with pytest.raises(ValueError, match="int_div / snn support at most 64 ids"):
        mv.moses_generate(big, 4, max_len=8, int_div=True)
    with pytest.raises(ValueError, match="snn=True needs novel_against"):
        mv.moses_generate(model, 4, max_len=8, snn=True)
    with pytest.raises(ValueError, match="k must be an integer in \\[1, 32\\]"):
        ds.nearest_fingerprints(["CCO"], k=33)
    with pytest.raises(ValueError, match="at most 64"):
        D.MosesDeviceDataset(["AB"], big.vocabulary, device="cpu").nearest_fingerprints(["AB"])
    with pytest.raises(L.MvaeError, match="MI355X only"):                            # a CPU model: no fallback
        mv.moses_generate(model, 4, max_len=8, int_div=True)
    with pytest.raises(L.MvaeError, match="MI355X only"):
        model.fingerprints(["CCO"])
    with pytest.raises(L.MvaeError, match="MI355X only"):
        model.tanimoto(["CCO"], ["CCN"])
    with pytest.raises(L.MvaeError, match="MI355X only"):
        ds.fingerprints()
    with pytest.raises(L.MvaeError, match="MI355X only"):
        ds.nearest_fingerprints(["CCO"])
