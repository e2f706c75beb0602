"""GPU tests of the aromatic normal form: mvae_smiles_aromatize_rows / _corpus against the host entry (the same source compiled for the
CPU, which tests/test_smiles_aromatize_host.py holds against the reference), bit for bit in tokens, lengths, statuses, info and arom at
the block edges; invariance on the device (the device rewrite in front of the device aromatize); VAE.normal_form, data.normal_smiles and
MosesDeviceDataset.normal_form() against the host entry; moses_generate(normal=True) against values recomputed from its own samples."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from molecular_vae_amd import data as D, mosesvae as MV, train as TR, vocab as VC, ops   # noqa: E402
import arom_ref as AR                                                 # noqa: E402
import chem_ref as CR                                                 # noqa: E402
import rewrite_ref as RR                                              # noqa: E402
from test_smiles_aromatize_host import TABLE, STAY_KEKULE, NOT_AROMATIC, NOT_KEKULE, EIGHT_RING       # noqa: E402  (plain data)

DEV = torch.device("cuda")
FILL = 0x7f7f7f7f
NAMES = ("out", "out_len", "status", "info", "arom")


def _host_rows(strings, v, T=None, max_content=127, T_out=None):
    tabs = (VC.smiles_token_table(v), VC.smiles_chem_table(v), VC.smiles_emit_table(v))
    return ops.smiles_aromatize_host(torch.from_numpy(CR.token_rows(strings, v, T)), *tabs, v.bos, v.eos, v.pad, max_content, T_out)


def _spell(out, out_len, v):
    return ["".join(v.i2c[int(i)] for i in row[1:k - 1]) for row, k in zip(out.cpu().numpy(), out_len.cpu().numpy())]


@pytest.fixture(scope="module")
def env():
    """260 rows: the hand table in both spellings, the rows that stay Kekule, one refused row of every kind, the longest hand rows, 100
    molecules of MOSES' lengths and a slice of the mutation corpus; the host entry's outputs for them with T_out = 131, computed once
    and left unchanged."""
    v = CR.vocabulary()
    tok, chem, emit = VC.smiles_token_table(v), VC.smiles_chem_table(v), VC.smiles_emit_table(v)
    corpus = CR.mutation_corpus()
    strings = [s for _, ks, a, _ in TABLE for s in ks + [a]] + STAY_KEKULE + NOT_AROMATIC + NOT_KEKULE + [EIGHT_RING]
    strings += ["C[C@H](N)O", "F/C=C/F", "C" * 128, "C(", "C=F", "[N+2]C", "C1C1", "cc", "C1=S(C)=CCC1", "c1" + "c" * 123 + "1"] + RR.HAND_ROWS[-3:]
    strings += RR.fragment_corpus(100, seed=1)
    strings += corpus[1000:1000 + 260 - len(strings)]
    x = torch.from_numpy(CR.token_rows(strings, v, 134))
    host = ops.smiles_aromatize_host(x, tok, chem, emit, v.bos, v.eos, v.pad, 127, 131)
    st = host[2].tolist()
    assert len(strings) == 260 and set(st) >= {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 17} and (host[2] == 0).sum() >= 150 and (host[3][:, 2] > 0).sum() >= 20
    return {"v": v, "tabs": (tok.to(DEV), chem.to(DEV), emit.to(DEV)), "host_tabs": (tok, chem, emit), "strings": strings, "x": x, "host": host}


def _rows(env, x, max_content=127, T_out=131, counts=None, fill=True):
    v, B = env["v"], x.shape[0]
    pre = ((torch.full((B, T_out), FILL, dtype=torch.int64, device=DEV), torch.full((B,), FILL, dtype=torch.int32, device=DEV),
            torch.full((B,), FILL, dtype=torch.int32, device=DEV), torch.full((B, 4), FILL, dtype=torch.int32, device=DEV),
            torch.full((B, 128), 0x7f, dtype=torch.uint8, device=DEV)) if fill else (None,) * 5)
    return ops.smiles_aromatize_rows(x, *env["tabs"], v.bos, v.eos, v.pad, max_content, T_out, *pre, counts=counts)


def _differing(got, want):
    return [(name, torch.nonzero((g.cpu() != w).reshape(w.shape[0], -1).any(1)).flatten()[:5].tolist())
            for g, w, name in zip(got, want, NAMES) if not torch.equal(g.cpu(), w)]


@pytest.mark.parametrize("B", [1, 63, 65, 130, 260])
def test_rows_entry_equals_the_host_entry(env, B):
    """B around the block size of 64; a strided input (x_ld = 134 > T = 131); outputs garbage-filled beforehand, so every element must be
    written; a second run is bit-identical; counts is the histogram of status."""
    x = env["x"].to(DEV)[:B, :131]
    assert x.stride(0) == 134
    counts = torch.zeros(32, dtype=torch.int32, device=DEV)
    out = _rows(env, x, counts=counts)
    want = tuple(t[:B] for t in env["host"])
    assert not _differing(out, want), _differing(out, want)
    assert torch.equal(counts.cpu(), torch.bincount(want[2], minlength=32).int())
    again = _rows(env, x, fill=False)
    assert all(torch.equal(a, o) for a, o in zip(again, out))


def test_rows_entry_cuts_at_t_out_and_honours_max_content(env):
    """T_out smaller than needed: the rows are the first columns of the uncut ones and out_len stays; a small max_content turns long
    spellings into LONG; info and arom may be left out."""
    v = env["v"]
    x = env["x"].to(DEV)
    full = _rows(env, x)
    cut = _rows(env, x, T_out=9)
    assert torch.equal(cut[0], full[0][:, :9]) and all(torch.equal(c, f) for c, f in zip(cut[1:], full[1:]))
    assert (full[1] > 9).sum() > 50
    for mc in (1, 20):
        got = _rows(env, x, max_content=mc)
        want = ops.smiles_aromatize_host(env["x"], *env["host_tabs"], v.bos, v.eos, v.pad, mc, 131)
        assert not _differing(got, want) and (want[2] == RR.LONG).sum() >= 10
    bare = ops.smiles_aromatize_rows(x, *env["tabs"], v.bos, v.eos, v.pad, 127, 131, info=False, arom=False)
    assert bare[3] is None and bare[4] is None and all(torch.equal(b, f) for b, f in zip(bare[:3], full[:3]))


def _corpus_case(env, B):
    """A CSR corpus of the fixture's rows with an empty row in front, and B row ids with a repeat and two ids outside [0, N)."""
    v = env["v"]
    strings = [""] + [s for s in env["strings"] if len(s) <= 127]
    tokens, offsets = D.tokenize_corpus(strings, v)
    rs = np.random.RandomState(B)
    rows = rs.randint(0, len(strings), size=B)
    rows[0] = 0 if B > 1 else 2
    if B >= 4:
        rows[1], rows[2], rows[3] = rows[B - 1], -1, len(strings)
    return strings, tokens, offsets, rows


@pytest.mark.parametrize("B", [1, 63, 65, 130])
def test_corpus_entry_equals_the_host_entry(env, B):
    """One launch over selected CSR rows: tokens_out, offsets_out, status, info and arom equal what the host entry gives for the same
    strings; an id outside the corpus is an empty row with status 1, zeros / 0xFF in info / arom and err 2; counts is the histogram."""
    v = env["v"]
    strings, tokens, offsets, rows = _corpus_case(env, B)
    N, stride = len(strings), 127
    inside = (rows >= 0) & (rows < N)
    picked = [strings[r] if ok else "" for r, ok in zip(rows, inside)]
    want = ops.smiles_aromatize_host(torch.from_numpy(CR.token_rows(picked, v, 129)), *env["host_tabs"], v.bos, v.eos, v.pad, 127, 129)
    tokens_d = torch.from_numpy(np.concatenate([tokens, np.zeros(1, np.uint8)])).to(DEV)
    offsets_d, rows_d = torch.from_numpy(offsets).to(DEV), torch.from_numpy(rows).to(DEV)
    counts = torch.zeros(32, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    pre = (torch.full((B, stride), 0x7f, dtype=torch.uint8, device=DEV), torch.full((2 * B + 1,), FILL, dtype=torch.int64, device=DEV),
           torch.full((B,), FILL, dtype=torch.int32, device=DEV), torch.full((B, 4), FILL, dtype=torch.int32, device=DEV),
           torch.full((B, 128), 0x7f, dtype=torch.uint8, device=DEV))
    tokens_out, offsets_out, status, info, arom = ops.smiles_aromatize_corpus(tokens_d, offsets_d, N, rows_d, *env["tabs"], 127, stride, *pre,
                                                                              counts=counts, err=err)
    lens = want[1].numpy() - 2
    assert int(err.item()) == (2 if not inside.all() else 0)
    assert status.cpu().tolist() == [int(s) if ok else 1 for s, ok in zip(want[2], inside)]
    off = offsets_out.cpu().numpy()
    assert off[0::2].tolist() == [b * stride for b in range(B + 1)] and (off[1::2] - off[0:-1:2]).tolist() == lens.tolist()
    content = np.zeros((B, stride), np.int64)
    for b in range(B):
        content[b, :lens[b]] = want[0][b, 1:1 + lens[b]].numpy()
    assert (tokens_out.cpu().numpy() == content).all()
    assert torch.equal(info.cpu(), want[3]) and torch.equal(arom.cpu(), want[4])
    assert not info.cpu()[~inside].any() and (arom.cpu()[~inside] == 0xFF).all()
    assert torch.equal(counts.cpu(), torch.bincount(status.cpu(), minlength=32).int())
    again = ops.smiles_aromatize_corpus(tokens_d, offsets_d, N, rows_d, *env["tabs"], 127, stride)
    assert all(torch.equal(a, o) for a, o in zip(again, (tokens_out, offsets_out, status, info, arom)))


def test_device_respellings_give_the_originals_normal_form(env):
    """The device rewrite at 4 draws, then the device aromatize: every respelling of a status-0 row gives the row the original gives,
    with the same counts of atoms, aromatic atoms, raised atoms and lowered bonds."""
    v = env["v"]
    x = env["x"].to(DEV)[:, :131]
    base = _rows(env, x)
    fine = base[2] == 0
    changed = 0
    for d in range(4):
        draws = ops.draw_words(torch.arange(x.shape[0]) * 4 + d).to(DEV)
        spelled, _, st = ops.smiles_rewrite_rows(x, *env["tabs"], v.bos, v.eos, v.pad, 7, draws, 127, 131)
        got = _rows(env, spelled)
        both = fine & (st == 0)
        changed += int((both & (spelled != x).any(1)).sum())
        assert torch.equal(got[0][both], base[0][both]) and torch.equal(got[1][both], base[1][both]) and not got[2][both].any()
        assert torch.equal(got[3][both], base[3][both])
    assert changed >= 400


@pytest.fixture(scope="module")
def small():
    """A corpus that holds molecules under an aromatic and under a Kekule spelling: 100 molecules of MOSES' lengths, a Kekule spelling
    of the first 50 that have an aromatic atom, the hand table in both spellings, and 20 rows the entry refuses."""
    vocab = CR.vocabulary()
    base = RR.fragment_corpus(100, seed=5)
    arom = [s for s in base if "c" in s][:50]
    x = torch.from_numpy(CR.token_rows(arom, vocab))
    mate = ops.smiles_kekule_host(x, VC.smiles_token_table(vocab), VC.smiles_chem_table(vocab), vocab.eos)[2]
    kek = [AR.kekule_spelling(s, mate[k].tolist(), 3, k) for k, s in enumerate(arom)]
    assert len(arom) == 50 and all(t is not None and len(t) <= 127 and "c" not in t for t in kek)
    refused = ["C[C@H](N)O", "c1ccc1", "C(", "c1cccc1"] * 5
    smiles = base + kek + [s for _, ks, a, _ in TABLE for s in ks + [a]] + refused
    return smiles, vocab, D.MosesDeviceDataset(smiles, vocab, device=DEV)


def test_python_surface_equals_the_host_entry(small):
    smiles, vocab, ds = small
    host = _host_rows(smiles, vocab, T_out=129)
    want = _spell(host[0], host[1], vocab)
    nf = ds.normal_form()
    assert nf is ds.normal_form() and len(nf) == len(ds) == len(smiles) and nf.device == ds.device
    assert torch.equal(ds.normal_status().cpu(), host[2])
    assert ds.normal_counts().cpu().tolist() == np.bincount(host[2].numpy(), minlength=32).tolist()
    assert nf.smiles(list(range(len(smiles)))) == want
    fine = [i for i, st in enumerate(host[2].tolist()) if st == 0]
    # a Kekule and an aromatic spelling are one row here and two in the canonical corpus
    assert nf.n_distinct < ds.canonical().n_distinct and nf.n_distinct == len(set(want))
    model = MV.VAE(vocab, dtype=torch.float32).to(DEV)
    rows, status = model.normal_form(smiles)
    assert torch.equal(status.cpu(), host[2]) and torch.equal(rows.cpu()[:, :129], host[0]) and (rows[:, 129:] == vocab.pad).all()
    rows, status, extra = model.normal_form(smiles[:70], info=True)
    full = _host_rows(smiles[:70], vocab)
    assert all(torch.equal(extra[name].cpu(), full[3][:, i]) for i, name in enumerate(ops.AROMATIZE_INFO)) and torch.equal(extra["arom"].cpu(), full[4])
    # the Kekule spellings are found at the row of their aromatic spelling
    first = {}
    for r, c in enumerate(want):
        first.setdefault(c, r)
    look = nf.lookup(model.normal_form(smiles)[0]).cpu().tolist()
    assert [look[i] for i in fine] == [first[want[i]] for i in fine] and sum(look[i] != i for i in fine) >= 50
    got, st = D.normal_smiles(smiles[100:160] + ["C("], vocab, device=DEV, return_status=True)
    assert got == want[100:160] + ["C("] and st.tolist() == host[2][100:160].tolist() + [1]


def test_moses_generate_normal_equals_values_recomputed_from_its_samples():
    """Three batches, the last one short, of a small randomly initialised model sampling under the syntax automaton after prefixes that
    spell benzene and pyridine in aromatic and in Kekule form, over a vocabulary small enough that many continuations are molecules.  The corpus holds, for every other sample the entry accepts, the
    OTHER spelling than the sample's: its normal form for a Kekule sample, a Kekule spelling for an aromatic one (the samples depend on
    the seed alone, so a first run without a corpus shows them)."""
    vocab = VC.OneHotVocab(list("CcNnO1=()"))
    torch.manual_seed(0)
    model = MV.VAE(vocab, dtype=torch.float32).to(DEV)
    prefix = ["c1ccccc1", "C1=CC=CC=C1", "c1ccncc1", "C1=CC=NC=C1", "OCC", "C(O)C"]
    n, kw = 240, dict(batch_size=96, max_len=15, top_k=4, seed=2, syntax=True, prefix=prefix * 40)
    drawn = TR.moses_generate(model, n, **kw)["strings"]
    h = _host_rows(drawn, vocab)
    forms = _spell(h[0], h[1], vocab)
    mate = ops.smiles_kekule_host(torch.from_numpy(CR.token_rows(drawn, vocab)), VC.smiles_token_table(vocab), VC.smiles_chem_table(vocab), vocab.eos)[2]
    smiles = ["CCCCCCCCO", "C[C@H](N)O"]
    for i in [i for i, st in enumerate(h[2].tolist()) if st == 0][::2]:
        other = AR.kekule_spelling(drawn[i], mate[i].tolist(), 1, i) if "c" in drawn[i] or "n" in drawn[i] else forms[i]
        smiles.append(other if other is not None else forms[i])
    ds = D.MosesDeviceDataset(smiles, vocab, device=DEV)
    plain = TR.moses_generate(model, n, novel_against=ds, canonical=True, **kw)
    res = TR.moses_generate(model, n, novel_against=ds, canonical=True, normal=True, **kw)
    new = {"normal_status", "normal_status_counts", "normal_strings", "unique_normal"}
    new_novel = {"normal_corpus_row", "novel_normal"}
    assert set(res) == set(plain) | new | new_novel and {k: res[k] for k in plain} == plain and not (new | new_novel) & set(plain)
    bare = TR.moses_generate(model, n, normal=True, **kw)
    assert set(bare) == set(TR.moses_generate(model, n, **kw)) | new and all(bare[k] == res[k] for k in new)
    # the same figures from the returned samples, with the host entry.  syntax=True: every sample ends in <eos>, so a string's status is
    # its row's
    strings = res["strings"]
    assert strings == drawn
    status = h[2]
    fine = [i for i, st in enumerate(status.tolist()) if st == 0]
    hc = _host_rows(smiles, vocab)
    corpus = _spell(hc[0], hc[1], vocab)
    rows = [corpus.index(c) if c in corpus else -1 for c in forms]
    print("unique", len(strings), "status 0:", len(fine), "unique_normal", res["unique_normal"], "unique_canonical", res["unique_canonical"],
          "novel_normal", res["novel_normal"], "novel_canonical", res["novel_canonical"])
    # the input is not degenerate (asserted on the host entry's figures): corpus hits under the other aromaticity spelling, which the
    # canonical lookup misses, and novel molecules
    assert len(fine) >= 6 and sum(rows[i] >= 0 and res["canonical_corpus_row"][i] < 0 for i in fine) >= 1 and sum(rows[i] < 0 for i in fine) >= 1
    assert res["normal_status"] == status.tolist() and res["normal_strings"] == forms
    assert res["normal_status_counts"] == dict(enumerate(np.bincount(status.numpy(), minlength=18).tolist()))
    assert sum(res["normal_status_counts"].values()) == len(strings) == res["unique"]
    assert res["unique_normal"] == len({forms[i] for i in fine})
    assert res["normal_corpus_row"] == rows
    assert res["novel_normal"] == len({forms[i] for i in fine if rows[i] < 0}) <= res["novel_canonical"]
