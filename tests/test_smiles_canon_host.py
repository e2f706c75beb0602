"""CPU tests of the canonical SMILES (mvae_smiles_canon_rows / _corpus / _host): the host entry (csrc/smiles_canon.hip on the shared
writer of csrc/smiles_writer.hpp, compiled for the CPU) against the reference of tests/canon_ref.py, byte for byte in tokens, lengths,
statuses, info and rank; what the definition promises, on the corpus the reference is measured on -- invariance under eight respellings
of every row, the rank as a graph isomorphism, idempotence, one string whichever member is taken at every tie; the round trip through
the graph, fingerprint, scaffold and kekule entries, which know nothing of the new reference; two deliberately broken references that
the invariance check must catch; every refusal; the argument checks; the declarations and the compiler's resource remarks."""
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
from test_smiles_rewrite_host import round_trip_failures         # a pure function of its arguments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mvae_smiles_canon_rows", "mvae_smiles_canon_corpus", "mvae_smiles_canon_host")
SPELLINGS = 8
SEED = 5


def _host(strings, max_content=127, T=None, T_out=None, v=None, **kw):
    v = CR.vocabulary() if v is None else v
    x = torch.from_numpy(CR.token_rows(strings, v, T))
    out = ops.smiles_canon_host(x, VC.smiles_token_table(v), VC.smiles_chem_table(v), VC.smiles_emit_table(v), v.bos, v.eos, v.pad, max_content,
                                T_out, **kw)
    return tuple(t.numpy() for t in out)


def _decode(out, out_len, v):
    return ["".join(v.i2c[int(i)] for i in row[1:n - 1]) for row, n in zip(out, out_len)]


def _want(refs, v, T_out):
    """The reference's (status, string, info, rank) per row as the arrays the entries write."""
    B = len(refs)
    rows, lens = np.full((B, T_out), v.pad, np.int64), np.zeros(B, np.int32)
    status, info, rank = np.zeros(B, np.int32), np.zeros((B, 4), np.int32), np.full((B, 128), 0xFF, np.uint8)
    for b, (st, s, inf, rk) in enumerate(refs):
        ids = v.string2ids(s, add_bos=True, add_eos=True)
        rows[b, :len(ids)] = ids
        lens[b], status[b] = len(ids), st
        if inf is not None:
            info[b], rank[b, :len(rk)] = inf, rk
    return rows, lens, status, info, rank


def _equal(got, want):
    return [name for g, w, name in zip(got, want, ("out", "out_len", "status", "info", "rank")) if not np.array_equal(g, w)]


_CASES = {}


def cases():
    """(rows, the reference's result per row, the host entry's outputs) of canon_ref.corpus(): computed once per process and shared;
    callers leave it unchanged."""
    if "c" not in _CASES:
        rows = CN.corpus()
        _CASES["c"] = (rows, [CN.canon(s) for s in rows], _host(rows, T=131))
    return _CASES["c"]


def respellings():
    """(the row each came from, the spelling): SPELLINGS rewrite_ref.respell spellings of every corpus row, computed once."""
    if "r" not in _CASES:
        rows = cases()[0]
        res = [(i, RR.respell(s, SEED, 1000 * i + d)) for i, s in enumerate(rows) for d in range(SPELLINGS)]
        _CASES["r"] = ([i for i, r in res if r[0] == 0], [r[1] for _, r in res if r[0] == 0])
    return _CASES["r"]


def test_entries_are_declared_bound_and_exported_at_abi_12():
    text = open(os.path.join(ROOT, "include", "mvae.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", header).group(1)) == 12 == L.ABI_VERSION
    lib = L.load()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    # the rewrite entries' arguments without seed and draw, with info and rank
    for canon, rewrite in zip(ENTRIES, ("mvae_smiles_rewrite_rows", "mvae_smiles_rewrite_corpus", "mvae_smiles_rewrite_host")):
        assert len(L.SIGNATURES[canon][1]) == len(L.SIGNATURES[rewrite][1])
    assert len(ops.REWRITE_STATUS_NAMES) == 14
    assert "SMILES canon" in text and "no canonical SMILES" in text and "[CH4] and C stay different strings" in text
    assert int(re.search(r"#define\s+MVAE_CANON_INFO\s+(\d+)", header).group(1)) == len(ops.CANON_INFO) == 4
    build = open(os.path.join(ROOT, "molecular-vae_amd", "csrc", "build.sh")).read()
    assert build.count(" smiles_canon smiles_rewrite ") == 2 and "build/smiles_canon.o build/smiles_rewrite.o" in build
    assert "build/tune/smiles_canon.o build/tune/smiles_rewrite.o" in build and "smiles_writer.hpp -nt build/$f.o" in build
    # the writer is shared, not copied
    csrc = os.path.join(ROOT, "molecular-vae_amd", "csrc")
    for name in ("smiles_canon.hip", "smiles_rewrite.hip"):
        src = open(os.path.join(csrc, name)).read()
        assert '#include "smiles_writer.hpp"' in src and "EM_LPAR" not in src and "Writer<" not in src, name


def test_new_kernels_use_no_scratch(tmp_path):
    """The compiler's resource remarks for the two kernels of smiles_canon.hip: scratch 0, no spills, and the LDS per block that
    include/mvae.h states."""
    csrc = os.path.join(ROOT, "molecular-vae_amd", "csrc")
    usage = os.path.join(csrc, "build", "smiles_canon.usage.txt")
    sources = ("smiles_canon.hip", "smiles_writer.hpp", "smiles_rounds.hpp", "smiles_graph.hpp", "smiles_syntax.hpp", "common.hpp",
               "../../include/mvae.h")
    if os.path.exists(usage) and os.path.getmtime(usage) >= max(os.path.getmtime(os.path.join(csrc, f)) for f in sources):
        text = open(usage, errors="replace").read()
    else:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                              "-c", os.path.join(csrc, "smiles_canon.hip"), "-o", str(tmp_path / "smiles_canon.dev.o")],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert run.returncode == 0, run.stderr[-2000:]
        text = run.stderr
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 2 and all(any(k in n for n in names) for k in ("smiles_canon_rows_kernel", "smiles_canon_corpus_kernel")), names
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 2
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 2 and re.findall(r"SGPRs Spill: (\d+)", text) == ["0"] * 2
    header = open(os.path.join(ROOT, "include", "mvae.h")).read()
    stated = int(re.search(r"#define\s+MVAE_CANON_LDS_BYTES\s+(\d+)", header).group(1))
    assert list(map(int, re.findall(r"LDS Size \[bytes/block\]: (\d+)", text))) == [stated] * 2
    assert f"MVAE_CANON_LDS_BYTES = {stated} B" in header and stated <= 80 * 1024
    assert all(int(n) <= 128 for n in re.findall(r" VGPRs: (\d+)", text))


def test_host_entry_equals_the_reference_byte_for_byte():
    """Tokens, lengths, statuses, info and rank of every corpus row and of the ten cage and spiro rows.  The input is not degenerate
    (asserted on the reference alone)."""
    rows, refs, got = cases()
    v = CR.vocabulary()
    ties = sum(r[2][3] > 0 for r in refs)
    distinct = len({r[1] for r in refs})
    print("rows:", len(rows), "refused:", sum(r[0] != 0 for r in refs), "with a tie:", ties, "most ties:", max(r[2][3] for r in refs),
          "most rounds:", max(r[2][2] for r in refs), "distinct canonical strings:", distinct)
    assert sum(r[0] == 0 for r in refs) >= 1000 and ties >= 500 and distinct >= 800
    assert max(r[2][2] for r in refs) == 126 and all(r[2][2] <= 2 * r[2][0] and r[2][3] <= r[2][0] - 1 for r in refs)
    wrong = _equal(got, _want(refs, v, 131))
    assert not wrong, wrong
    cage = [CN.canon(s) for s in CN.CAGES]
    assert all(r[0] == 0 for r in cage)
    wrong = _equal(_host(CN.CAGES, T=131), _want(cage, v, 131))
    assert not wrong, wrong


def test_every_refusal_is_copied_through_unchanged():
    """Each walk status, STEREO, RING_MULTI on the cyclic allene, LONG through a small max_content, NO_TOKEN through a vocabulary
    without the digit the canonical spelling needs; info and rank are there exactly where the ranks were computed."""
    v = CR.vocabulary()
    rejected = [s for s, st, _ in CR.REJECTED if st != CR.OK and s] + ["C" * 128]
    stereo = ["C[C@H](N)O", "F/C=C/F", "F/C=C\\F", "C[C@@H](N)O"]
    # the cyclic allene, which the rewrite refuses on some draws, has a canonical spelling: its root is a CH2, never the allene's centre.
    # The ring with a methyl on an S that has two double bonds in it has none: the root is the methyl, so the S is entered by neither.
    rows = rejected + stereo + ["C1=S(C)=CCC1", "C1=C=CCCC1"]
    refs = [CN.canon(s) for s in rows]
    assert {r[0] for r in refs[:len(rejected)]} == {1, 2, 3, 4, 5, 6} and all(r[0] == RR.STEREO for r in refs[len(rejected):-2])
    assert [r[0] for r in refs[-2:]] == [RR.RING_MULTI, 0] and all(r[2] is None for r in refs[:-2]) and refs[-2][2] == [6, 4, 3, 1]
    got = _host(rows, T=140)
    wrong = _equal(got, _want(refs, v, 140))
    assert not wrong, wrong
    assert (got[0][:-1] == CR.token_rows(rows, v, 140)[:-1, :got[0].shape[1]]).all()
    # LONG: the canonical spelling of neopentane takes 8 tokens
    long_rows = ["CC(C)(C)C", "CCCCCC", "C(C)(C)(C)C", "CCCCCCC"]
    refs = [CN.canon(s, max_content=7) for s in long_rows]
    assert [r[0] for r in refs] == [RR.LONG, 0, RR.LONG, 0] and all(r[2] is not None for r in refs)
    got = _host(long_rows, max_content=7)
    wrong = _equal(got, _want(refs, v, got[0].shape[1]))
    assert not wrong, wrong
    # NO_TOKEN: the canonical spelling of a ring opens digit 1, which the vocabulary lacks
    small = VC.OneHotVocab(set(CR.ALPHABET) - {"1"})
    refs = [CN.canon(s, have=set(CR.ALPHABET) - {"1"}) for s in ("C2CC2", "CCC")]
    assert [r[0] for r in refs] == [RR.NO_TOKEN, 0] and refs[0][1] == "C2CC2"
    wrong = _equal(_host(["C2CC2", "CCC"], v=small, T_out=129), _want(refs, small, 129))
    assert not wrong, wrong


def test_respellings_canonicalise_to_one_row_and_rank_is_an_isomorphism():
    """Eight spellings of every row: the same canonical row as the original's, and the two rank vectors map one numbering onto the other
    as a graph isomorphism (atoms of equal rank have equal invariants and equal bonds)."""
    rows, refs, got = cases()
    origin, spelled = respellings()
    changed = sum(t != rows[i] for i, t in zip(origin, spelled))
    print("spellings:", len(spelled), "changed:", changed)
    assert changed >= 7000 and len(spelled) >= 8000             # a few 127-token rows grow beyond 127 tokens on every draw
    out, out_len, status, _, rank = _host(spelled, T=131)
    assert not status.any()
    same = (out == got[0][origin]).all(1) & (out_len == got[1][origin])
    assert same.all(), [(rows[origin[k]], spelled[k]) for k in np.nonzero(~same)[0][:3]]
    for k in range(0, len(spelled), 3):
        s, t = rows[origin[k]], spelled[k]
        n = int(got[3][origin[k], 0])
        assert CN.isomorphic(s, got[4][origin[k], :n].tolist(), t, rank[k, :n].tolist()), (s, t)
    # the check can fail: each broken reference gives two spellings of one row two canonical strings
    for broken in CN.BROKEN:
        caught = sum(CN.canon(t, broken=broken)[1] != CN.canon(rows[i], broken=broken)[1] for i, t in list(zip(origin, spelled))[::16])
        print(broken, "caught on", caught)
        assert caught >= 1, broken


def test_canonical_rows_are_fixed_points():
    rows, refs, got = cases()
    v = CR.vocabulary()
    canon = _decode(got[0], got[1], v)
    again = _host(canon, T=131)
    assert not again[2].any() and (again[0] == got[0]).all() and (again[1] == got[1]).all()
    n = got[3][:, 0]
    # a canonical row is written in search order, so its ranks need not be 0, 1, 2, ...; they are still a permutation
    assert all(sorted(again[4][b, :n[b]].tolist()) == list(range(n[b])) for b in range(len(rows)))
    assert (again[4][np.arange(128)[None, :] >= n[:, None]] == 0xFF).all()


def test_every_choice_at_every_tie_gives_one_string():
    """canon_ref.all_choices follows every member of the chosen class at every tie: on the corpus and on the cage and spiro rows one
    string comes out whichever is taken -- the condition under which equal graphs give equal rows -- and it is the host entry's."""
    rows, refs, got = cases()
    v = CR.vocabulary()
    canon = _decode(got[0], got[1], v)
    for s, c in list(zip(rows, canon)) + list(zip(CN.CAGES, _decode(*_host(CN.CAGES, T=131)[:2], v))):
        assert CN.all_choices(s) == {c}, s


def test_every_canonical_row_is_the_same_molecule():
    """The round trip through the entries that existed before the rewrite: independent of canon_ref."""
    rows, refs, got = cases()
    spelled = _decode(got[0], got[1], CR.vocabulary())
    bad = round_trip_failures(rows, spelled)
    assert bad.size == 0, [(rows[i], spelled[i]) for i in bad[:3]]
    assert sum(a != b for a, b in zip(rows, spelled)) >= 300


def test_hand_stated_spellings():
    v = CR.vocabulary()
    groups = (["OCC", "C(O)C", "CCO", "C(C)O"], ["c1ccccc1C", "Cc1ccccc1", "c1cc(C)ccc1", "c1(C)ccccc1"], ["C1=CC=CC=C1", "C1(=CC=CC=C1)", "C(=CC=C1)C=C1"],
              ["[CH4]"], ["C"], ["[NH4+]"], ["N#CC#N"], ["ClCCBr", "BrCCCl", "C(Cl)CBr"])
    seen = []
    for g in groups:
        out, out_len, status, _, _ = _host(g)
        spell = set(_decode(out, out_len, v))
        assert not status.any() and len(spell) == 1, (g, spell)
        seen.append(spell.pop())
    assert len(set(seen)) == len(groups) and seen[3] == "[CH4]" and seen[4] == "C"       # the bracket flag is kept
    assert _decode(*_host(["c1ccccc1"])[:2], v) != _decode(*_host(["C1=CC=CC=C1"])[:2], v)  # no aromaticity perception


def test_edge_rows_strided_input_and_prefilled_outputs():
    """A strided view (x_ld > T), rows without <eos> and with ids outside the vocabulary, T_out smaller than needed; every element of
    prefilled outputs is written and info / rank may be left out."""
    v = CR.vocabulary()
    tabs = (VC.smiles_token_table(v), VC.smiles_chem_table(v), VC.smiles_emit_table(v))
    x = torch.from_numpy(CR.token_rows(["c1cccn1", "c1ccccc1", "C=F", "c1ccncc1", "CC(C)CO"], v, T=12))
    x[0, 8] = v.pad                                                # no <eos>
    x[1, 3] = -1
    x[3, 2] = len(v)
    wide = torch.full((5, 40), v.eos, dtype=torch.long)
    wide[:, :12] = x
    pre = (torch.full((5, 20), 0x7f7f7f7f, dtype=torch.int64), torch.full((5,), 0x7f7f7f7f, dtype=torch.int32),
           torch.full((5,), 0x7f7f7f7f, dtype=torch.int32), torch.full((5, 4), 0x7f7f7f7f, dtype=torch.int32),
           torch.full((5, 128), 0x7f, dtype=torch.uint8))
    got = ops.smiles_canon_host(wide[:, :12], *tabs, v.bos, v.eos, v.pad, 127, 20, *pre)
    assert got[2].tolist() == [1, 1, 2, 1, 0] and got[1].tolist()[:4] == [12, 10, 5, 10]
    assert (got[0][:4, :12] == x[:4]).all() and (got[0][:, 12:] == v.pad).all()
    assert got[3].tolist() == [[0] * 4] * 4 + [CN.canon("CC(C)CO")[2]] and (got[4][:4] == 0xFF).all()
    fresh = ops.smiles_canon_host(wide[:, :12], *tabs, v.bos, v.eos, v.pad, 127, 20)
    assert all(torch.equal(a, b) for a, b in zip(fresh, got))
    cut = ops.smiles_canon_host(wide[:, :12], *tabs, v.bos, v.eos, v.pad, 127, 4, info=False, rank=False)
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

    def corpus(tokens=fake, offsets=fake, N=100, rows=fake, B=4, V=29, tok=fake, chem=fake, emit=fake, mc=100, stride=100, tokens_out=fake,
               offsets_out=fake, status=fake):
        return lib.mvae_smiles_canon_corpus(tokens, offsets, N, rows, B, V, tok, chem, emit, mc, stride, tokens_out, offsets_out, status,
                                            None, None, None, None, None)
    assert corpus(N=0) == -1 and corpus(B=0) == -1 and corpus(V=0) == -1 and corpus(V=65) == -3 and corpus(rows=None) == -1
    assert corpus(tokens=None) == -1 and corpus(offsets=None) == -1 and corpus(tok=None) == -1 and corpus(chem=None) == -1
    assert corpus(emit=None) == -1 and corpus(status=None) == -1 and corpus(tokens_out=None) == -1 and corpus(offsets_out=None) == -1
    assert corpus(mc=0) == -1 and corpus(mc=128, stride=128) == -1 and corpus(stride=99) == -1
    with pytest.raises(ValueError, match=r"max_content must be in \[1, 127\]"):
        _host(["CCO"], max_content=128)


def test_python_surface():
    """data.canonical_smiles through the host entry equals the reference; the device-only surfaces raise on a CPU model or corpus before
    any device work: no fallback; moses_generate refuses what canonical=True cannot take before any device work."""
    import inspect
    from molecular_vae_amd import data as D, mosesvae as MV, train as TR
    v = CR.vocabulary()
    strings = RR.fragment_corpus(12, seed=2) + ["OCC", "C(O)C", "C[C@H](N)O", "C("]
    got, status = D.canonical_smiles(strings, v, device="cpu", return_status=True)
    ref = [CN.canon(s) for s in strings]
    assert got == [r[1] for r in ref] and status.tolist() == [r[0] for r in ref]
    assert got[-4] == got[-3] and status[-2] == RR.STEREO and got[-1] == "C("
    with pytest.raises(ValueError, match="at least one string"):
        D.canonical_smiles([], v, device="cpu")
    torch.manual_seed(0)
    model = MV.VAE(VC.OneHotVocab(list("CNOc(=)1")), dtype=torch.float32)
    ds = D.MosesDeviceDataset(["CCO", "c1ccccc1"], model.vocabulary, device="cpu")
    with pytest.raises(L.MvaeError, match="MI355X only"):
        model.canonical(["CCO"])
    with pytest.raises(L.MvaeError, match="MI355X only"):
        ds.canonical()
    with pytest.raises(L.MvaeError, match="MI355X only"):
        ds.canonical_status
    assert inspect.signature(TR.moses_generate).parameters["canonical"].default is False
    with pytest.raises(ValueError, match="canonical=True supports max_len <= 129"):
        TR.moses_generate(model, 4, max_len=130, canonical=True)
    big = MV.VAE(VC.OneHotVocab([chr(0x100 + i) for i in range(70)]), dtype=torch.float32)
    with pytest.raises(ValueError, match="canonical=True supports at most 64 ids"):
        TR.moses_generate(big, 4, canonical=True)
