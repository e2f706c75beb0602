"""CPU tests of the SMILES graph surface (vocab.smiles_chem_table, mvae_smiles_graph_rows / _corpus / _host, data.formula_strings,
VAE.chem_valid / descriptors, moses_generate(valence=)): the reference of tests/chem_ref.py against hand-stated formulas and rejected
strings, the host entry (the walk of csrc/smiles_graph.hpp compiled for the CPU) against that reference on the tables and on a mutation
corpus, the argument checks of the three entries (refused before anything is launched), and the ABI."""
import collections
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import molecular_vae_amd as mv
from molecular_vae_amd import _lib as L, data as D, mosesvae as MV, vocab as VC, ops
import chem_ref as CR
import syntax_ref as SY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mvae_smiles_graph_rows", "mvae_smiles_graph_corpus", "mvae_smiles_graph_host")


def _host(strings, vocab=None, T=None):
    v = vocab or CR.vocabulary()
    x = torch.from_numpy(CR.token_rows(strings, v, T))
    out = ops.smiles_graph_host(x, VC.smiles_token_table(v), VC.smiles_chem_table(v), v.eos)
    return tuple(t.numpy() for t in out)


def test_entries_are_declared_bound_and_exported_at_abi_12():
    text = open(os.path.join(ROOT, "include", "mvae.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", header).group(1)) == 12 == L.ABI_VERSION
    lib = L.load()
    assert lib.mvae_abi_version() == 12
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert len(L.SIGNATURES[ENTRIES[0]][1]) == len(L.SIGNATURES[ENTRIES[2]][1]) + 1 == 13         # the host entry: no stream
    assert len(L.SIGNATURES[ENTRIES[1]][1]) == 11
    for name, value in (("MVAE_SMILES_ELEMENTS", 11), ("MVAE_SMILES_DESC", 8), ("MVAE_SMILES_CONTENT_MAX", 127)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", header), name
    assert (ops.SMILES_ELEMENTS, ops.SMILES_DESC, ops.SMILES_CONTENT_MAX) == (11, 8, 127) and len(ops.SMILES_DESC_NAMES) == 8
    assert "SMILES graph" in text and "NECESSARY" in text and "valence-consistent" in text
    for fn in (ops.smiles_graph_rows, ops.smiles_graph_corpus, ops.smiles_graph_host, VC.smiles_chem_table, MV.VAE.chem_valid,
               MV.VAE.descriptors, D.MosesDeviceDataset.descriptors, D.formula_strings):
        assert callable(fn)
    build = open(os.path.join(ROOT, "molecular-vae_amd", "csrc", "build.sh")).read()
    assert build.count("smiles_graph elementwise") == 2 and "build/smiles_graph.o" in build and "build/tune/smiles_graph.o" in build
    for doc in ("README.md", "INTEGRATION.md"):
        body = open(os.path.join(ROOT, doc)).read()
        assert "valence-consistent" in body and "rdkit-valid" not in body, doc


def test_kernels_use_no_scratch_and_32_kib_of_lds(tmp_path):
    """The compiler's resource remarks for the two kernels: scratch 0 (the per-atom state is in LDS, not in a private array), no spills,
    32 KiB of LDS.  The build leaves the remarks in csrc/build/smiles_graph.usage.txt; on a tree whose library was built another way the
    test compiles the device code of smiles_graph.hip itself (a few seconds), so that it never passes without having looked."""
    import subprocess
    csrc = os.path.join(ROOT, "molecular-vae_amd", "csrc")
    usage = os.path.join(csrc, "build", "smiles_graph.usage.txt")
    sources = ("smiles_graph.hip", "smiles_rounds.hpp", "smiles_graph.hpp", "smiles_syntax.hpp")
    if os.path.exists(usage) and os.path.getmtime(usage) >= max(os.path.getmtime(os.path.join(csrc, f)) for f in sources):
        text = open(usage, errors="replace").read()
    else:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                              "-c", os.path.join(csrc, "smiles_graph.hip"), "-o", str(tmp_path / "smiles_graph.dev.o")],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert run.returncode == 0, run.stderr[-2000:]
        text = run.stderr
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 2 and any("rows_kernelIN3smg5CheckE" in n for n in names) and any("corpus_kernelIN3smg5CheckE" in n for n in names)
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0", "0"]
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0", "0"] and re.findall(r"LDS Size \[bytes/block\]: (\d+)", text) == ["32768", "32768"]
    assert all(int(v) <= 128 for v in re.findall(r" VGPRs: (\d+)", text))


def test_elements_weights_and_chem_table(golden_dir):
    assert VC.SMI_ELEMENTS == tuple(CR.ELEMENTS) and list(VC.ATOMIC_WEIGHTS) == CR.WEIGHTS
    g = np.load(os.path.join(golden_dir, "g5_vocab.npz"))
    g5 = VC.CharVocab(set(str(s) for s in g["symbols"] if len(str(s)) == 1))
    synth = VC.OneHotVocab.from_data(D.synthetic_smiles(2048, seed=0))
    for v in (g5, synth, CR.vocabulary()):
        t = VC.smiles_chem_table(v)
        assert t.dtype == torch.int32 and tuple(t.shape) == (len(v),)
        t, info = t.tolist(), VC.smiles_token_table(v).tolist()
        for ch, i in v.c2i.items():
            cls = info[i] & 0xFF if len(ch) == 1 else VC.SMI_OTHER
            if ch in "BCNOPSFI":
                assert t[i] == CR.ELEMENTS.index(ch), ch
            elif ch in "bcnops":
                assert t[i] == CR.ELEMENTS.index(ch.upper()) | 1 << 4, ch
            elif ch == "H":
                assert t[i] == 0 and cls == VC.SMI_H
            elif ch == "l":
                assert t[i] == CR.ELEMENTS.index("Cl")
            elif ch == "r":
                assert t[i] == CR.ELEMENTS.index("Br")
            elif ch in "=#:/\\-":
                assert t[i] == CR.BOND_ORDER[ch] << 8, ch
            else:
                assert t[i] == 0, ch
    assert "r" in g5.c2i and "[" in synth.c2i


@pytest.mark.parametrize("s,formula", CR.FORMULAS)
def test_reference_reproduces_the_hand_stated_formulas(s, formula):
    status, bad, desc, f = CR.analyse(s)
    assert (status, bad) == (CR.OK, -1) and CR.hill(f, desc[6]) == formula
    assert f[0] == desc[5] and sum(f[1:]) == desc[0] and desc[2] == desc[1] - (desc[0] + s.count("[H]")) + 1


def test_host_entry_on_the_tables():
    strings = [s for s, _ in CR.FORMULAS]
    status, bad, desc, formula = _host(strings)
    assert (status == 0).all() and (bad == -1).all()
    assert D.formula_strings(formula, desc[:, 6]) == [f for _, f in CR.FORMULAS]
    assert D.formula_strings(torch.from_numpy(formula)) == [re.sub(r"[+-]$", "", f) for _, f in CR.FORMULAS]
    want = CR.expected(strings)
    for got, ref in zip((status, bad, desc, formula), want):
        assert (got == ref).all()
    aspirin = dict(zip(ops.SMILES_DESC_NAMES, desc[0].tolist()))
    assert aspirin == {"heavy_atoms": 13, "bonds": 13, "rings": 1, "ring_atoms": 6, "aromatic_atoms": 6, "hydrogens": 8, "charge": 0,
                       "hetero_atoms": 4}
    strings = [s for s, _, _ in CR.REJECTED]
    status, bad, desc, formula = _host(strings)
    assert status.tolist() == [st for _, st, _ in CR.REJECTED]
    assert bad.tolist() == [p + 1 if p >= 0 else -1 for _, _, p in CR.REJECTED]
    assert (desc[status != 0] == 0).all() and (formula[status != 0] == 0).all()
    for got, ref in zip((status, bad, desc, formula), CR.expected(strings)):
        assert (got == ref).all()


def test_formula_strings():
    f = lambda **kw: [kw.get(e, 0) for e in CR.ELEMENTS]
    rows = [f(C=9, H=8, O=4), f(C=4, H=12, N=1), f(H=2, O=4, S=1), f(C=1, H=1, Cl=3), f(C=7, H=4, Br=1, N=1), f(), f(B=1, H=3, O=3), f(I=1, C=1, F=3)]
    assert D.formula_strings(rows) == ["C9H8O4", "C4H12N", "H2O4S", "CHCl3", "C7H4BrN", "", "BH3O3", "CF3I"]
    assert D.formula_strings(np.array(rows[:4]), [0, 1, -2, 3]) == ["C9H8O4", "C4H12N+", "H2O4S(2-)", "CHCl3(3+)"]
    assert D.formula_strings(torch.tensor(rows[1:2]), torch.tensor([1])) == ["C4H12N+"] == [CR.hill(rows[1], 1)]
    with pytest.raises(ValueError, match="charges"):
        D.formula_strings(rows, [0])


def test_mutation_corpus_against_the_reference():
    """Every output of the host entry equals the reference on the mutation corpus; the corpus holds each of the statuses 0-5 at least 20
    times (asserted on the reference alone); status is SYNTAX exactly where syntax_ref's validator refuses the string, with the syntax
    check's bad_pos; weight agrees with a float64 dot product within 2e-6 (22 float32 roundings of 2^-24 each: 11 products, 11 sums)."""
    strings, want = CR.corpus_and_expected()
    count = collections.Counter(want[0].tolist())
    print("statuses in the corpus:", sorted(count.items()), "rows:", len(strings))
    assert 3000 <= len(strings) <= 6000 and all(count[k] >= 20 for k in range(6)), count
    v = CR.vocabulary()
    got = _host(strings, v)
    for name, g, w in zip(("status", "bad_pos", "desc", "formula"), got, want):
        wrong = np.nonzero((g != w).reshape(len(strings), -1).any(1))[0]
        assert wrong.size == 0, (name, [(strings[i], g[i].tolist(), w[i].tolist()) for i in wrong[:5]])
    chars = SY.token_chars(v)
    x = CR.token_rows(strings, v)
    for b, s in enumerate(strings):
        assert (got[0][b] == CR.SYNTAX) == (not SY.valid_smiles(s)), s
        if got[0][b] == CR.SYNTAX:
            assert got[1][b] == SY.first_refusal(x[b], chars), s
    d = ops.graph_descriptors(*(torch.from_numpy(g) for g in got))
    assert set(d) == {"status", "bad_pos", "formula", "weight", *ops.SMILES_DESC_NAMES} and d["weight"].dtype == torch.float32
    ref = got[3].astype(np.float64) @ np.array(CR.WEIGHTS)
    assert (np.abs(d["weight"].numpy() - ref) <= 2e-6 * ref).all() and (ref[got[0] != 0] == 0).all() and (ref[got[0] == 0] > 0).all()
    assert abs(ref[strings.index("CC(=O)Oc1ccccc1C(=O)O")] - 180.159) < 1e-3
    for i, name in enumerate(ops.SMILES_DESC_NAMES):
        assert (d[name].numpy() == got[2][:, i]).all()


def test_host_entry_edge_rows():
    """T = 2 (bos + eos), the 127-token chain and the 128-token one, a ring closed between atom 3 and atom 69, a 15-deep nest, a row
    without <eos>, ids -1 and V, optional outputs, a strided view, prefilled buffers."""
    v = CR.vocabulary()
    tok, chem = VC.smiles_token_table(v), VC.smiles_chem_table(v)
    x = torch.tensor([[v.bos, v.eos]])
    assert [t.tolist() for t in ops.smiles_graph_host(x, tok, chem, v.eos)[:2]] == [[CR.SYNTAX], [1]]
    ring = "CCC1" + "C" * 66 + "1"
    nest = "C" + "(C" * 15 + ")" * 15
    strings = ["C" * 127, "C" * 128, ring, nest, "C" * 125 + "=O", "c1ccccc1" * 15 + "C" * 6 + "c"]
    status, bad, desc, formula = _host(strings, v, T=140)
    assert status.tolist() == [0, CR.TOO_LONG, 0, 0, 0, CR.AROMATIC] and bad.tolist() == [-1, 129, -1, -1, -1, 128]
    assert desc[0].tolist() == [127, 126, 0, 0, 0, 256, 0, 0] and formula[0].tolist() == [256, 0, 127] + [0] * 8
    assert desc[2].tolist() == [69, 69, 1, 67, 0, 138, 0, 0] and desc[3].tolist() == [16, 15, 0, 0, 0, 34, 0, 0]
    for got, ref in zip((status, bad, desc, formula), CR.expected(strings)):
        assert (got == ref).all()
    x = torch.from_numpy(CR.token_rows(["CCO", "CC(=O)O", "C=F", "CCN"], v, T=12))
    x[0, 4] = v.pad                                                # no <eos>: the pad is refused where it stands
    x[1, 3] = -1
    x[3, 2] = len(v)
    wide = torch.full((4, 40), v.eos, dtype=torch.long)
    wide[:, :12] = x
    out = [torch.full((4,), 0x7f7f7f7f, dtype=torch.int32), torch.full((4,), 0x7f7f7f7f, dtype=torch.int32),
           torch.full((4, 8), 0x7f7f7f7f, dtype=torch.int32), torch.full((4, 11), 0x7f7f7f7f, dtype=torch.int32)]
    ops.smiles_graph_host(wide[:, :12], tok, chem, v.eos, *out)
    assert out[0].tolist() == [1, 1, 2, 1] and out[1].tolist() == [4, 3, 3, 2] and not out[2].any() and not out[3].any()
    x = torch.tensor([[v.bos] + v.string2ids("CCO")])               # the row runs out: bad_pos = T
    lib = L.load()
    status = torch.full((1,), -5, dtype=torch.int32)
    assert lib.mvae_smiles_graph_host(1, 4, len(v), L.ptr(x), 4, L.ptr(tok), L.ptr(chem), v.eos, L.ptr(status), None, None, None) == 0
    assert status.tolist() == [CR.SYNTAX]
    assert [t.tolist() for t in ops.smiles_graph_host(x, tok, chem, v.eos)[:2]] == [[CR.SYNTAX], [4]]
    # another id that the table calls EOS is refused; eos_id ends the row whatever the table says of it
    tok2 = tok.clone()
    tok2[v.pad] = VC.SMI_EOS
    tok2[v.eos] = VC.SMI_OTHER
    x = torch.from_numpy(CR.token_rows(["CCO", "CC"], v, T=6))
    x[1, 3] = v.pad
    assert [t.tolist() for t in ops.smiles_graph_host(x, tok2, chem, v.eos)[:2]] == [[0, 1], [-1, 3]]


def test_entries_refuse_bad_arguments_before_launching():
    """Everything below returns before any HIP call (no device needed)."""
    lib = L.load()
    fake = ctypes.c_void_p(256)                                  # never dereferenced: every call below is refused first

    def rows(name, B=4, T=8, V=29, x=fake, ld=8, tok=fake, chem=fake, eos=1, status=fake):
        tail = (None,) if name == ENTRIES[0] else ()
        return getattr(lib, name)(B, T, V, x, ld, tok, chem, eos, status, None, None, None, *tail)
    for name in (ENTRIES[0], ENTRIES[2]):
        assert rows(name, B=0) == -1 and rows(name, T=0, ld=0) == -1 and rows(name, V=0, eos=0) == -1 and rows(name, V=65) == -3
        assert rows(name, x=None) == -1 and rows(name, tok=None) == -1 and rows(name, chem=None) == -1 and rows(name, status=None) == -1
        assert rows(name, ld=7) == -1 and rows(name, eos=29) == -1 and rows(name, eos=-1) == -1

    def corpus(tokens=fake, offsets=fake, N=100, V=29, tok=fake, chem=fake, status=fake):
        return lib.mvae_smiles_graph_corpus(tokens, offsets, N, V, tok, chem, status, None, None, None, None)
    assert corpus(N=0) == -1 and corpus(N=-3) == -1 and corpus(V=0) == -1 and corpus(V=65) == -3
    assert corpus(tokens=None) == -1 and corpus(offsets=None) == -1 and corpus(tok=None) == -1 and corpus(chem=None) == -1
    assert corpus(status=None) == -1


def test_python_surface_raises_before_device_work():
    torch.manual_seed(0)
    model = MV.VAE(VC.OneHotVocab(list("CNO(=)1")), dtype=torch.float32)
    big = MV.VAE(VC.OneHotVocab([chr(65 + i) for i in range(61)]), dtype=torch.float32)
    assert len(big.vocabulary) == 65
    with pytest.raises(ValueError, match="valence=True supports at most 64 ids"):
        mv.moses_generate(big, 4, max_len=8, valence=True)
    with pytest.raises(ValueError, match="n_samples, batch_size and max_len"):
        mv.moses_generate(model, 0, max_len=8, valence=True)
    with pytest.raises(ValueError, match="max_len >= 3"):
        mv.moses_generate(model, 4, max_len=2, syntax=True, valence=True)
    with pytest.raises(L.MvaeError, match="MI355X only"):                            # a CPU model: no fallback
        mv.moses_generate(model, 4, max_len=8, valence=True)
    with pytest.raises(L.MvaeError, match="MI355X only"):
        model.chem_valid(["CCO"])
    with pytest.raises(L.MvaeError, match="MI355X only"):
        model.descriptors(["CCO"])
    ds = D.MosesDeviceDataset(["CCO", "CC"], model.vocabulary, device="cpu")
    with pytest.raises(L.MvaeError, match="MI355X only"):
        ds.descriptors()
