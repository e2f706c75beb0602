"""CPU tests of the SMILES rewrite (mvae_smiles_rewrite_rows / _corpus / _host, vocab.smiles_emit_table): the host entry (the walk of
csrc/smiles_graph.hpp with the recorder of csrc/smiles_rounds.hpp and the writer of csrc/smiles_rewrite.hip, compiled for the CPU)
against the reference of tests/rewrite_ref.py, byte for byte, on the mutation corpus and hand-picked rows at 16 draws each; the round
trip of every respelling through the existing graph, fingerprint, scaffold and kekule entries, which know nothing of the new reference,
with five deliberately broken writers that those checks must catch; hand-stated spellings; every refusal; the argument checks (refused
before anything is launched); prefilled outputs; the ABI and the compiler's resource remarks for the new kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from molecular_vae_amd import _lib as L, vocab as VC, ops
import chem_ref as CR
import rewrite_ref as RR
import syntax_ref as SY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mvae_smiles_rewrite_rows", "mvae_smiles_rewrite_corpus", "mvae_smiles_rewrite_host")
DRAWS = 16
SEED = 20171031
# chosen on the CPU with the reference alone: SEED_CCO reaches all four spellings of CCO within draws 0 .. 63
SEED_CCO = 0
# C1=C=CCCC1 under SEED: a draw the reference refuses with RING_MULTI and one it respells
ALLENE_MULTI_DRAW, ALLENE_OK_DRAW = 0, 2
# P ladders and combs (rails of double bonds, P takes valence 5): rows of at most 127 tokens that reach RING_DIGITS and DEPTH
LADDER = "P(=P1=P2=P3=P4=P5=P6)(P(=P1=P2=P3=P4=P5=P6)=P1=P2=P3=P4=P5)=P1=P2=P3=P4=P5"
COMB = "C" + "=P(C)" * 24 + "=C"
LADDER_DIGITS_DRAW, COMB_DEPTH_DRAW = 2, 0


def _tables(v):
    return VC.smiles_token_table(v), VC.smiles_chem_table(v), VC.smiles_emit_table(v)


def _host(strings, draws, seed=SEED, max_content=127, T=None, T_out=None, v=None, **kw):
    v = CR.vocabulary() if v is None else v
    x = torch.from_numpy(CR.token_rows(strings, v, T))
    tok, chem, emit = _tables(v)
    draw = None if draws is None else ops.draw_words(torch.as_tensor(np.asarray(draws, np.int64)))
    out = ops.smiles_rewrite_host(x, tok, chem, emit, v.bos, v.eos, v.pad, seed, draw, max_content, T_out, **kw)
    return tuple(t.numpy() for t in out)


def _rows_of(spellings, v, T_out):
    want = np.full((len(spellings), T_out), v.pad, np.int64)
    lens = np.zeros(len(spellings), np.int32)
    for b, s in enumerate(spellings):
        ids = v.string2ids(s, add_bos=True, add_eos=True)
        want[b, :len(ids)] = ids
        lens[b] = len(ids)
    return want, lens


def _decode(out, out_len, v):
    return ["".join(v.i2c[int(i)] for i in row[1:n - 1]) for row, n in zip(out, out_len)]


_CASES = {}


def cases():
    """(strings, draws, reference status, reference spellings) of the mutation corpus and rewrite_ref.HAND_ROWS at DRAWS draws each:
    computed once per process and shared; callers leave it unchanged."""
    if "c" not in _CASES:
        base = CR.mutation_corpus() + RR.HAND_ROWS
        strings = [s for s in base for _ in range(DRAWS)]
        draws = [1000 * k + d for k in range(len(base)) for d in range(DRAWS)]
        status, spell = RR.expected(strings, SEED, draws)
        _CASES["c"] = (strings, draws, status, spell)
    return _CASES["c"]


def round_trip_failures(originals, spellings):
    """The rows whose spelling is not the original's molecule, judged by the entries that existed before the rewrite and by syntax_ref: the
    graph entry's status, desc and formula, all 1024 fingerprint bits, both graph keys, the scaffold desc, the kekule status."""
    v = CR.vocabulary()
    tok, chem = VC.smiles_token_table(v), VC.smiles_chem_table(v)
    res = []
    for rows in (originals, spellings):
        ok = [s if 0 < len(s) <= 127 else "C" for s in rows]
        x = torch.from_numpy(CR.token_rows(ok, v))
        g = ops.smiles_graph_host(x, tok, chem, v.eos)
        f = ops.smiles_fp_host(x, tok, chem, v.eos)
        s = ops.smiles_scaffold_host(x, tok, chem, v.eos, mask=False)
        k = ops.smiles_kekule_host(x, tok, chem, v.eos, mate=False)
        res.append([t.numpy().reshape(len(rows), -1) for t in (g[0], g[2], g[3], f[1], s[2], s[3], k[0])])
    bad = np.zeros(len(originals), bool)
    for a, b in zip(*res):
        bad |= (a != b).any(1)
    bad |= np.array([not SY.valid_smiles(s) for s in spellings])
    return np.nonzero(bad)[0]


def test_entries_are_declared_bound_and_exported_at_abi_12():
    text = open(os.path.join(ROOT, "include", "mvae.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", header).group(1)) == 12 == L.ABI_VERSION
    lib = L.load()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert len(L.SIGNATURES[ENTRIES[0]][1]) == len(L.SIGNATURES[ENTRIES[2]][1]) + 2 == 20           # the host entry: no counts, no stream
    for i, name in enumerate(("STEREO", "RING_MULTI", "RING_DIGITS", "DEPTH", "LONG", "NO_TOKEN")):
        assert re.search(r"#define\s+MVAE_SMILES_" + name + r"\s+" + str(8 + i) + r"\b", header), name
        assert getattr(ops, "SMILES_STATUS_" + name) == 8 + i == getattr(RR, name)
    assert len(ops.REWRITE_STATUS_NAMES) == 14 and ops.REWRITE_STATUS_NAMES[:8] == ops.KEKULE_STATUS_NAMES
    assert "SMILES rewrite" in text and "no canonical SMILES" in text
    assert int(re.search(r"#define\s+MVAE_REWRITE_EMIT\s+(\d+)", header).group(1)) == VC.SMI_EMIT_WORDS == ops.REWRITE_EMIT
    build = open(os.path.join(ROOT, "molecular-vae_amd", "csrc", "build.sh")).read()
    assert build.count(" smiles_rewrite ") == 2 and "build/smiles_rewrite.o" in build and "build/tune/smiles_rewrite.o" in build


def test_emit_table():
    v = CR.vocabulary()
    emit = VC.smiles_emit_table(v).tolist()
    assert [v.i2c[i] for i in emit[:11]] == list("HBCNOFPSCBI")
    assert [v.i2c[i] if i >= 0 else None for i in emit[11:22]] == [None, "b", "c", "n", "o", None, "p", "s", None, None, None]
    assert "".join(v.i2c[i] for i in emit[22:43]) == "lr[]H+-=#()0123456789"
    mask = (emit[43] & 0xFFFFFFFF) | (emit[44] & 0xFFFFFFFF) << 32
    assert mask == sum(1 << v.c2i[c] for c in "@/\\") and emit[45:] == [0, 0, 0]
    small = VC.OneHotVocab(set("CNO=1)"))                         # ')' without '(': the token table calls it OTHER, so no role has it
    emit = VC.smiles_emit_table(small).tolist()
    assert emit[31] == emit[32] == -1 and emit[24] == -1 and emit[29] == small.c2i["="] and emit[43] == emit[44] == 0
    with pytest.raises(ValueError, match="at most 64"):
        VC.smiles_emit_table(VC.OneHotVocab([chr(65 + i) for i in range(61)]))


def test_new_kernels_use_no_scratch(tmp_path):
    """The compiler's resource remarks for the two kernels of smiles_rewrite.hip: scratch 0, no spills, and the LDS per block
    include/mvae.h states, at most 80 KiB so that two blocks fit a CU."""
    csrc = os.path.join(ROOT, "molecular-vae_amd", "csrc")
    usage = os.path.join(csrc, "build", "smiles_rewrite.usage.txt")
    sources = ("smiles_rewrite.hip", "smiles_writer.hpp", "smiles_rounds.hpp", "smiles_graph.hpp", "smiles_syntax.hpp", "common.hpp",
               "../../include/mvae.h")
    if os.path.exists(usage) and os.path.getmtime(usage) >= max(os.path.getmtime(os.path.join(csrc, f)) for f in sources):
        text = open(usage, errors="replace").read()
    else:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                              "-c", os.path.join(csrc, "smiles_rewrite.hip"), "-o", str(tmp_path / "smiles_rewrite.dev.o")],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert run.returncode == 0, run.stderr[-2000:]
        text = run.stderr
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 2 and all(any(k in n for n in names) for k in ("smiles_rewrite_rows_kernel", "smiles_rewrite_corpus_kernel")), names
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 2
    assert re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 2 and re.findall(r"SGPRs Spill: (\d+)", text) == ["0"] * 2
    header = open(os.path.join(ROOT, "include", "mvae.h")).read()
    stated = int(re.search(r"#define\s+MVAE_REWRITE_LDS_BYTES\s+(\d+)", header).group(1))
    assert list(map(int, re.findall(r"LDS Size \[bytes/block\]: (\d+)", text))) == [stated] * 2 and stated <= 80 * 1024
    assert f"{stated} B" in header
    assert all(int(n) <= 128 for n in re.findall(r" VGPRs: (\d+)", text))


def test_host_entry_equals_the_reference_byte_for_byte():
    """Tokens, lengths and statuses of every (row, draw).  The input is not degenerate (asserted on the reference alone): hundreds of
    status-0 rows, most of them respelled differently from the input, the walk statuses 1 - 5 and STEREO present (6 is in the refusal test)."""
    strings, draws, status, spell = cases()
    v = CR.vocabulary()
    changed = sum(a != b for a, b, st in zip(strings, spell, status) if st == 0)
    print("cases:", len(strings), "status 0:", int((status == 0).sum()), "changed:", changed, "statuses:", sorted(set(status.tolist())))
    assert (status == 0).sum() >= 5000 and changed >= 3000 and set(range(6)) | {RR.STEREO} <= set(status.tolist())
    out, out_len, got = _host(strings, draws, T=140)
    want, lens = _rows_of(spell, v, out.shape[1])
    wrong = np.nonzero((got != status) | (out_len != lens) | (out != want).any(1))[0]
    assert wrong.size == 0, [(strings[i], draws[i], int(got[i]), int(status[i]), _decode(out[i:i + 1], out_len[i:i + 1], v), spell[i])
                             for i in wrong[:3]]


def test_every_respelling_is_the_same_molecule_and_broken_writers_are_caught():
    """The round trip through the entries that existed before: independent of rewrite_ref.  Then the same check on the output of each
    broken reference writer must fail on at least one row."""
    strings, draws, status, _ = cases()
    v = CR.vocabulary()
    out, out_len, got = _host(strings, draws, T=140)
    keep = np.nonzero(got == 0)[0]
    originals = [strings[i] for i in keep]
    spellings = _decode(out[keep], out_len[keep], v)
    assert len(originals) >= 5000
    bad = round_trip_failures(originals, spellings)
    assert bad.size == 0, [(originals[i], spellings[i]) for i in bad[:3]]
    sub = keep[::4]
    for broken in RR.BROKEN:
        res = [RR.respell(strings[i], SEED, draws[i], broken=broken) for i in sub]
        pick = [k for k, r in enumerate(res) if r[0] == 0]
        bad = round_trip_failures([strings[sub[k]] for k in pick], [res[k][1] for k in pick])
        print(broken, "caught on", bad.size, "of", len(pick))
        assert bad.size >= 1, broken


def test_hand_stated_spellings():
    draws = list(range(64))
    for s, want in (("CCO", {"CCO", "OCC", "C(C)O", "C(O)C"}), ("c1ccccc1", {"c1ccccc1"}), ("C1=CC=CC=C1", {"C1=CC=CC=C1"})):
        ref = {RR.respell(s, SEED_CCO, d)[1] for d in draws}
        assert ref == want, (s, ref)
        out, out_len, status = _host([s] * 64, draws, seed=SEED_CCO)
        assert not status.any() and set(_decode(out, out_len, CR.vocabulary())) == want, s
    out, out_len, status = _host(["[N+1](C)(C)(C)C", "[C]", "[CH4]", "[H]C", "[NH4+]"], [0] * 5)
    got = _decode(out, out_len, CR.vocabulary())
    assert not status.any() and "[N+]" in got[0] and "+1" not in got[0] and got[1] == "[C]" and got[2] == "[CH4]" and got[4] == "[NH4+]"
    assert got[3] in ("[H]C", "C[H]")
    # draw NULL means the row number
    a = _host(["CC(C)(C)CCO"] * 8, None)
    b = _host(["CC(C)(C)CCO"] * 8, list(range(8)))
    assert all((p == q).all() for p, q in zip(a, b)) and len(set(_decode(a[0], a[1], CR.vocabulary()))) >= 3


def test_every_refusal_is_copied_through_unchanged():
    """Each walk status; STEREO; RING_MULTI on a stated draw of the cyclic allene and status 0 on another; LONG through a small
    max_content; NO_TOKEN through a vocabulary without '('; RING_DIGITS on a 12-rung ladder of P atoms written from one of its ends (11
    closures open at once) and DEPTH on a comb of 24 P atoms (16 branches open): both fit 127 tokens, so both are reached."""
    v = CR.vocabulary()
    rejected = [s for s, st, _ in CR.REJECTED if st != CR.OK and s] + ["C" * 128]
    stereo = ["C[C@H](N)O", "F/C=C/F", "F/C=C\\F", "C[C@@H](N)O"]
    rows = rejected + stereo + ["C1=C=CCCC1", "C1=C=CCCC1", LADDER, COMB]
    draws = [3] * (len(rejected) + len(stereo)) + [ALLENE_MULTI_DRAW, ALLENE_OK_DRAW, LADDER_DIGITS_DRAW, COMB_DEPTH_DRAW]
    ref_status, ref_spell = RR.expected(rows, SEED, draws)
    assert set(ref_status[:len(rejected)].tolist()) == {1, 2, 3, 4, 5, 6} and (ref_status[len(rejected):-4] == RR.STEREO).all()
    assert ref_status[-4:].tolist() == [RR.RING_MULTI, 0, RR.RING_DIGITS, RR.DEPTH] and len(LADDER) <= 127 and len(COMB) <= 127
    out, out_len, status = _host(rows, draws, T=140)
    want, lens = _rows_of(ref_spell, v, out.shape[1])
    assert (status == ref_status).all() and (out == want).all() and (out_len == lens).all()
    x = CR.token_rows(rows, v, 140)
    refused = status != 0
    assert (out[refused] == x[refused][:, :out.shape[1]]).all() and ref_spell[-3] != rows[-3]
    # LONG: CC(C)C respelt from an end needs two more tokens than CC(C)C has from the middle
    long_rows = ["C(C)(C)C"] * 32
    ref = RR.expected(long_rows, SEED, range(32), max_content=6)
    assert set(ref[0].tolist()) == {0, RR.LONG}
    out, out_len, status = _host(long_rows, list(range(32)), max_content=6)
    want, lens = _rows_of(ref[1], v, out.shape[1])
    assert (status == ref[0]).all() and (out == want).all() and (out_len == lens).all()
    assert all(s == "C(C)(C)C" for s, st in zip(ref[1], ref[0]) if st)
    # NO_TOKEN: CCC written from the middle needs a '(' the vocabulary lacks
    small = VC.OneHotVocab(set(CR.ALPHABET) - {"("})
    ref = RR.expected(["CCC"] * 16, SEED, range(16), have=set(CR.ALPHABET) - {"(", ")"})
    assert set(ref[0].tolist()) == {0, RR.NO_TOKEN}
    out, out_len, status = _host(["CCC"] * 16, list(range(16)), v=small)
    want, lens = _rows_of(ref[1], small, out.shape[1])
    assert (status == ref[0]).all() and (out == want).all() and (out_len == lens).all()


def test_edge_rows_strided_input_and_prefilled_outputs():
    """Rows without <eos>, ids -1 and V, a strided view (x_ld > T), T_out smaller than needed (the row is cut, out_len is not); every
    element of 0x7f-prefilled outputs is written and the result does not depend on what they held."""
    v = CR.vocabulary()
    tok, chem, emit = _tables(v)
    x = torch.from_numpy(CR.token_rows(["c1cccn1", "c1ccccc1", "C=F", "c1ccncc1", "CC(C)CO"], v, T=12))
    x[0, 8] = v.pad                                                # no <eos>
    x[1, 3] = -1
    x[3, 2] = len(v)
    wide = torch.full((5, 40), v.eos, dtype=torch.long)
    wide[:, :12] = x
    pre = (torch.full((5, 20), 0x7f7f7f7f, dtype=torch.int64), torch.full((5,), 0x7f7f7f7f, dtype=torch.int32),
           torch.full((5,), 0x7f7f7f7f, dtype=torch.int32))
    out, out_len, status = ops.smiles_rewrite_host(wide[:, :12], tok, chem, emit, v.bos, v.eos, v.pad, SEED, None, 127, 20, *pre)
    assert status.tolist() == [1, 1, 2, 1, 0] and out_len.tolist()[:4] == [12, 10, 5, 10] and out_len[4] == 9
    assert (out[:4, :12] == x[:4]).all() and (out[:, 12:] == v.pad).all() and out[2, 5:].eq(v.pad).all()
    fresh = ops.smiles_rewrite_host(wide[:, :12], tok, chem, emit, v.bos, v.eos, v.pad, SEED, None, 127, 20)
    assert all(torch.equal(a, b) for a, b in zip(fresh, (out, out_len, status)))
    cut = ops.smiles_rewrite_host(wide[:, :12], tok, chem, emit, v.bos, v.eos, v.pad, SEED, None, 127, 4)
    assert torch.equal(cut[0], out[:, :4]) and torch.equal(cut[1], out_len) and torch.equal(cut[2], status)


def test_entries_refuse_bad_arguments_before_launching():
    """Everything below returns before any HIP call (no device needed)."""
    lib = L.load()
    fake = ctypes.c_void_p(256)                                  # never dereferenced: every call below is refused first

    def rows(name, B=4, T=8, V=29, x=fake, ld=8, tok=fake, chem=fake, emit=fake, bos=0, eos=1, pad=2, mc=127, T_out=129, out=fake,
             out_len=fake, status=fake):
        tail = (fake, None) if name == ENTRIES[0] else ()
        return getattr(lib, name)(B, T, V, x, ld, tok, chem, emit, bos, eos, pad, 7, None, mc, T_out, out, out_len, status, *tail)
    for name in (ENTRIES[0], ENTRIES[2]):
        assert rows(name, B=0) == -1 and rows(name, T=0, ld=0) == -1 and rows(name, V=0, eos=0) == -1 and rows(name, V=65) == -3
        assert rows(name, x=None) == -1 and rows(name, tok=None) == -1 and rows(name, chem=None) == -1 and rows(name, status=None) == -1
        assert rows(name, emit=None) == -1 and rows(name, out=None) == -1 and rows(name, out_len=None) == -1 and rows(name, ld=7) == -1
        assert rows(name, eos=29) == -1 and rows(name, eos=-1) == -1 and rows(name, mc=0) == -1 and rows(name, mc=128) == -1
        assert rows(name, T_out=1) == -1 and rows(name, bos=-1) == -1 and rows(name, pad=65536) == -1 and rows(name, V=65, out=None) == -3

    def corpus(tokens=fake, offsets=fake, N=100, rows=fake, B=4, V=29, tok=fake, chem=fake, emit=fake, mc=100, stride=100, tokens_out=fake,
               offsets_out=fake, status=fake):
        return lib.mvae_smiles_rewrite_corpus(tokens, offsets, N, rows, B, V, tok, chem, emit, 7, None, mc, stride, tokens_out, offsets_out, status,
                                              None, None, None)
    assert corpus(N=0) == -1 and corpus(B=0) == -1 and corpus(V=0) == -1 and corpus(V=65) == -3 and corpus(rows=None) == -1
    assert corpus(tokens=None) == -1 and corpus(offsets=None) == -1 and corpus(tok=None) == -1 and corpus(chem=None) == -1
    assert corpus(emit=None) == -1 and corpus(status=None) == -1 and corpus(tokens_out=None) == -1 and corpus(offsets_out=None) == -1
    assert corpus(mc=0) == -1 and corpus(mc=128, stride=128) == -1 and corpus(stride=99) == -1
    with pytest.raises(ValueError, match=r"max_content must be in \[1, 127\]"):
        _host(["CCO"], [0], max_content=128)


def test_python_surface():
    """data.randomized_smiles through the host entry equals the reference (draw = i * n + j); the device-only surfaces raise on a CPU model
    or corpus before any device work: no fallback."""
    import inspect
    from molecular_vae_amd import data as D, mosesvae as MV
    v = CR.vocabulary()
    strings = RR.fragment_corpus(12, seed=2) + ["C[C@H](N)O", "C("]
    got, status = D.randomized_smiles(strings, v, 5, seed=9, device="cpu", return_status=True)
    for i, s in enumerate(strings):
        ref = [RR.respell(s, 9, i * 5 + j) for j in range(5)]
        assert got[i] == [r[1] for r in ref] and status[i].tolist() == [r[0] for r in ref], s
    assert status[-2].tolist() == [RR.STEREO] * 5 and got[-1] == ["C("] * 5
    with pytest.raises(ValueError, match="at least one string"):
        D.randomized_smiles([], v, 3, device="cpu")
    torch.manual_seed(0)
    model = MV.VAE(VC.OneHotVocab(list("CNOc(=)1")), dtype=torch.float32)
    ds = D.MosesDeviceDataset(["CCO", "c1ccccc1"], model.vocabulary, device="cpu")
    with pytest.raises(L.MvaeError, match="MI355X only"):
        model.respell(["CCO"])
    with pytest.raises(L.MvaeError, match="MI355X only"):
        ds.batches(2, augment=True)
    with pytest.raises(L.MvaeError, match="MI355X only"):
        ds.gather([0, 1], augment=True)
    for name in ("augment", "augment_seed", "augment_slack"):
        assert name in inspect.signature(D.MosesDeviceDataset.batches).parameters
    assert inspect.signature(D.MosesDeviceDataset.batches).parameters["augment"].default is False and ds.augment_counts is None
