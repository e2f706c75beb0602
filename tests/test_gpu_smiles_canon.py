"""GPU tests of the canonical SMILES: mvae_smiles_canon_rows / _corpus against the host entry (the same source compiled for the CPU,
which tests/test_smiles_canon_host.py holds against the reference), bit for bit in tokens, lengths, statuses, info and rank at the block
edges; invariance on the device (the device rewrite in front of the device canon); MosesDeviceDataset.canonical() and its graph-level
lookup; moses_generate(canonical=True) against values recomputed from its own samples."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from molecular_vae_amd import data as D, mosesvae as MV, train as TR, vocab as VC, ops   # noqa: E402
import canon_ref as CN                                                # noqa: E402
import chem_ref as CR                                                 # noqa: E402
import rewrite_ref as RR                                              # noqa: E402

DEV = torch.device("cuda")
FILL = 0x7f7f7f7f
NAMES = ("out", "out_len", "status", "info", "rank")


@pytest.fixture(scope="module")
def env():
    """260 rows: the hand rows (1 atom to 127 atoms, 127 tokens), one refused row of every kind, 100 molecules of MOSES' lengths and a
    slice of the mutation corpus; the host entry's outputs for them with T_out = 131, computed once and left unchanged."""
    v = CR.vocabulary()
    tok, chem, emit = VC.smiles_token_table(v), VC.smiles_chem_table(v), VC.smiles_emit_table(v)
    corpus = CR.mutation_corpus()
    strings = ["C"] + RR.HAND_ROWS + ["C[C@H](N)O", "F/C=C/F", "C" * 128, "C(", "C=F", "cc", "C1=S(C)=CCC1"]
    strings += RR.fragment_corpus(100, seed=1)
    strings += corpus[1000:1000 + 260 - len(strings)]
    x = torch.from_numpy(CR.token_rows(strings, v, 134))
    host = ops.smiles_canon_host(x, tok, chem, emit, v.bos, v.eos, v.pad, 127, 131)
    assert len(strings) == 260 and len(set(host[2].tolist())) >= 6 and (host[2] == 0).sum() >= 60 and int(host[3][:, 2].max()) == 126
    return {"v": v, "tabs": (tok.to(DEV), chem.to(DEV), emit.to(DEV)), "host_tabs": (tok, chem, emit), "strings": strings, "x": x, "host": host}


def _rows(env, x, max_content=127, T_out=131, counts=None, fill=True):
    v, B = env["v"], x.shape[0]
    pre = ((torch.full((B, T_out), FILL, dtype=torch.int64, device=DEV), torch.full((B,), FILL, dtype=torch.int32, device=DEV),
            torch.full((B,), FILL, dtype=torch.int32, device=DEV), torch.full((B, 4), FILL, dtype=torch.int32, device=DEV),
            torch.full((B, 128), 0x7f, dtype=torch.uint8, device=DEV)) if fill else (None,) * 5)
    return ops.smiles_canon_rows(x, *env["tabs"], v.bos, v.eos, v.pad, max_content, T_out, *pre, counts=counts)


def _differing(got, want):
    return [(name, torch.nonzero((g.cpu() != w).reshape(w.shape[0], -1).any(1)).flatten()[:5].tolist())
            for g, w, name in zip(got, want, NAMES) if not torch.equal(g.cpu(), w)]


@pytest.mark.parametrize("B", [1, 63, 65, 130, 260])
def test_rows_entry_equals_the_host_entry(env, B):
    """B around the block size of 64; a strided input (x_ld = 134 > T = 131); outputs garbage-filled beforehand, so every element must be
    written; a second run is bit-identical; counts is the histogram of status."""
    x = env["x"].to(DEV)[:B, :131]
    assert x.stride(0) == 134
    counts = torch.zeros(16, dtype=torch.int32, device=DEV)
    out = _rows(env, x, counts=counts)
    want = tuple(t[:B] for t in env["host"])
    assert not _differing(out, want), _differing(out, want)
    assert torch.equal(counts.cpu(), torch.bincount(want[2], minlength=16).int())
    again = _rows(env, x, fill=False)
    assert all(torch.equal(a, o) for a, o in zip(again, out))


def test_rows_entry_cuts_at_t_out_and_honours_max_content(env):
    """T_out smaller than needed: the rows are the first columns of the uncut ones and out_len stays; a small max_content turns long
    spellings into LONG; info and rank may be left out."""
    v = env["v"]
    x = env["x"].to(DEV)
    full = _rows(env, x)
    cut = _rows(env, x, T_out=9)
    assert torch.equal(cut[0], full[0][:, :9]) and all(torch.equal(c, f) for c, f in zip(cut[1:], full[1:]))
    assert (full[1] > 9).sum() > 50
    for mc in (1, 20):
        got = _rows(env, x, max_content=mc)
        want = ops.smiles_canon_host(env["x"], *env["host_tabs"], v.bos, v.eos, v.pad, mc, 131)
        assert not _differing(got, want) and (want[2] == RR.LONG).sum() >= 10
    bare = ops.smiles_canon_rows(x, *env["tabs"], v.bos, v.eos, v.pad, 127, 131, info=False, rank=False)
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
    """One launch over selected CSR rows: tokens_out, offsets_out, status, info and rank equal what the host entry gives for the same
    strings; an id outside the corpus is an empty row with status 1 and err 2; counts is the histogram."""
    v = env["v"]
    strings, tokens, offsets, rows = _corpus_case(env, B)
    N, stride = len(strings), 127
    inside = (rows >= 0) & (rows < N)
    picked = [strings[r] if ok else "" for r, ok in zip(rows, inside)]
    want = ops.smiles_canon_host(torch.from_numpy(CR.token_rows(picked, v, 129)), *env["host_tabs"], v.bos, v.eos, v.pad, 127, 129)
    tokens_d = torch.from_numpy(np.concatenate([tokens, np.zeros(1, np.uint8)])).to(DEV)
    offsets_d, rows_d = torch.from_numpy(offsets).to(DEV), torch.from_numpy(rows).to(DEV)
    counts = torch.zeros(16, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    pre = (torch.full((B, stride), 0x7f, dtype=torch.uint8, device=DEV), torch.full((2 * B + 1,), FILL, dtype=torch.int64, device=DEV),
           torch.full((B,), FILL, dtype=torch.int32, device=DEV), torch.full((B, 4), FILL, dtype=torch.int32, device=DEV),
           torch.full((B, 128), 0x7f, dtype=torch.uint8, device=DEV))
    tokens_out, offsets_out, status, info, rank = ops.smiles_canon_corpus(tokens_d, offsets_d, N, rows_d, *env["tabs"], 127, stride, *pre,
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
    assert torch.equal(info.cpu(), want[3]) and torch.equal(rank.cpu(), want[4])
    assert torch.equal(counts.cpu(), torch.bincount(status.cpu(), minlength=16).int())
    again = ops.smiles_canon_corpus(tokens_d, offsets_d, N, rows_d, *env["tabs"], 127, stride)
    assert all(torch.equal(a, o) for a, o in zip(again, (tokens_out, offsets_out, status, info, rank)))


def test_device_respellings_canonicalise_to_the_originals_rows(env):
    """The device rewrite at 4 draws, then the device canon: every respelling of a status-0 row gives the row the original gives."""
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
        assert torch.equal(got[3][both], base[3][both])          # atoms, classes, rounds and ties are the graph's, not the spelling's
    assert changed >= 400


@pytest.fixture(scope="module")
def small():
    """200 rows: 120 molecules of MOSES' lengths, 60 respellings of the first 60 (duplicates as graphs, mostly not as strings) and 20
    rows the canon refuses."""
    vocab = CR.vocabulary()
    base = RR.fragment_corpus(120, seed=5)
    dup = [RR.respell(s, 3, i)[1] for i, s in enumerate(base[:60])]
    refused = ["C[C@H](N)O", "F/C=C/F", "C(", "C=F"] * 5
    smiles = base + dup + refused
    return smiles, vocab, D.MosesDeviceDataset(smiles, vocab, device=DEV)


def test_dataset_canonical_answers_at_graph_level(small):
    smiles, vocab, ds = small
    ref = [CN.canon(s) for s in smiles]
    can = ds.canonical()
    assert can is ds.canonical() and len(can) == len(ds) == 200 and can.device == ds.device
    assert ds.canonical_status.cpu().tolist() == [r[0] for r in ref]
    assert ds.canonical_counts.cpu().tolist() == np.bincount([r[0] for r in ref], minlength=16).tolist()
    assert can.smiles(list(range(200))) == [r[1] for r in ref]
    assert can.n_distinct == len({r[1] for r in ref}) < ds.n_distinct
    # fresh spellings of corpus molecules: found at the lowest row that holds the graph, whatever the spelling
    model = MV.VAE(vocab, dtype=torch.float32).to(DEV)
    fresh = [RR.respell(s, 11, i)[1] for i, s in enumerate(smiles[:120])]
    assert sum(f not in smiles for f in fresh) >= 60
    rows, status = model.canonical(fresh)
    first = {}
    for r, c in enumerate(x[1] for x in ref):
        first.setdefault(c, r)
    assert not status.any() and can.lookup(rows).cpu().tolist() == [first[ref[i][1]] for i in range(120)]
    assert can.contains(rows).all() and (ds.lookup(fresh) >= 0).sum() < 120
    assert not can.contains(model.canonical(["CCCCCCCCCCCCO", "OCCCCCCCCCCCC"])[0]).any()
    got = D.canonical_smiles(fresh[:8] + ["C("], vocab, device=DEV)
    assert got == [ref[i][1] for i in range(8)] + ["C("]


def test_moses_generate_canonical_equals_values_recomputed_from_its_samples(small):
    """Three batches, the last one short, of a small randomly initialised model sampling under the syntax automaton after prefixes that
    spell ethanol four ways, so that some samples are one graph under several spellings and some are corpus molecules under another
    spelling than the corpus': the corpus is made of respellings of every other sample that the walk accepts (the samples depend on the
    seed alone, so a first run without a corpus shows them)."""
    vocab = small[1]
    torch.manual_seed(0)
    model = MV.VAE(vocab, dtype=torch.float32).to(DEV)
    n, kw = 240, dict(batch_size=96, max_len=10, top_k=4, seed=2, syntax=True, prefix=["OCC", "C(O)C", "CCO", "C(C)O", "c1ccccc1", "C"] * 40)
    drawn = [s for s in TR.moses_generate(model, n, **kw)["strings"] if CN.canon(s)[0] == 0]
    smiles = ["CCCCCCCCO", "C[C@H](N)O"] + [next((t for t in (RR.respell(s, 1, d)[1] for d in range(8)) if t != s), s) for s in drawn[::2]]
    ds = D.MosesDeviceDataset(smiles, vocab, device=DEV)
    plain = TR.moses_generate(model, n, novel_against=ds, **kw)
    res = TR.moses_generate(model, n, novel_against=ds, canonical=True, **kw)
    new = {"canonical_status", "canonical_status_counts", "canonical_strings", "unique_canonical"}
    new_novel = {"canonical_corpus_row", "novel_canonical"}
    assert set(res) == set(plain) | new | new_novel and {k: res[k] for k in plain} == plain and not (new | new_novel) & set(plain)
    bare = TR.moses_generate(model, n, canonical=True, **kw)
    assert set(bare) == set(TR.moses_generate(model, n, **kw)) | new and all(bare[k] == res[k] for k in new)
    # the same figures from the returned samples, with the host entry.  syntax=True: every sample ends in <eos>, so a string's status is
    # its row's
    strings = res["strings"]
    tabs = (VC.smiles_token_table(vocab), VC.smiles_chem_table(vocab), VC.smiles_emit_table(vocab))
    out, out_len, status, _, _ = ops.smiles_canon_host(torch.from_numpy(CR.token_rows(strings, vocab)), *tabs, vocab.bos, vocab.eos, vocab.pad)
    spell = ["".join(vocab.i2c[int(i)] for i in row[1:k - 1]) for row, k in zip(out.numpy(), out_len.numpy())]
    fine = [i for i, st in enumerate(status.tolist()) if st == 0]
    print("unique", len(strings), "status 0:", len(fine), "unique_canonical", res["unique_canonical"], "novel_canonical", res["novel_canonical"])
    corpus = [CN.canon(s)[1] for s in smiles]
    rows = [corpus.index(c) if c in corpus else -1 for c in spell]
    # the input is not degenerate (asserted on the host entry's figures): graphs drawn under two spellings, corpus hits under another
    # spelling than the corpus', novel graphs
    assert len(fine) >= 8 and len({spell[i] for i in fine}) < len(fine)
    assert sum(rows[i] >= 0 and strings[i] != smiles[rows[i]] for i in fine) >= 1 and sum(rows[i] < 0 for i in fine) >= 1
    assert res["canonical_status"] == status.tolist() and res["canonical_strings"] == spell
    assert res["canonical_status_counts"] == dict(enumerate(np.bincount(status.numpy(), minlength=14).tolist()))
    assert sum(res["canonical_status_counts"].values()) == len(strings) == res["unique"]
    assert res["unique_canonical"] == len({spell[i] for i in fine})
    assert res["canonical_corpus_row"] == rows
    assert res["novel_canonical"] == len({spell[i] for i in fine if rows[i] < 0})
