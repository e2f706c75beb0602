"""GPU tests of the substructure search: mvae_smiles_substruct_rows / _corpus against the host entry (the same source compiled for the
CPU, which tests/test_smiles_substruct_host.py holds against the reference), bit for bit in status, hit, undecided, map and steps at the
block edges and at 1, 22 and 64 queries; the step budget on the device; MosesDeviceDataset.substructure_counts /
rows_with_substructure, VAE.has_substructure and moses_generate(filters=) against the reference."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from molecular_vae_amd import data as D, mosesvae as MV, train as TR, vocab as VC, ops   # noqa: E402
import chem_ref as CR                                                 # noqa: E402
import rewrite_ref as RR                                              # noqa: E402
import substruct_ref as SR                                            # noqa: E402

DEV = torch.device("cuda")
FILL = 0x7f7f7f7f
NAMES = ("status", "hit", "undecided", "map", "steps")
# 64 queries: the 22 of the host test, then fragments of every size up to 32 atoms, an AROMATIC-status one and a refused one (no atoms)
QUERIES_64 = SR.QUERIES_22 + ["cC(=O)O", "C[C@H](N)O"] + ["C" * k for k in range(1, 33)] + ["N", "O", "c", "n", "Br", "CN(C)C", "C(C)(C)(C)C", "[nH]"]


@pytest.fixture(scope="module")
def env():
    """260 rows: the hand rows (1 atom to 127 atoms, 127 tokens), one refused row of every kind, 100 molecules of MOSES' lengths and a
    slice of the mutation corpus; the 64 compiled queries; the host entry's outputs per (Q, map query), computed once on first use and
    left unchanged."""
    v = CR.vocabulary()
    tok, chem, emit = VC.smiles_token_table(v), VC.smiles_chem_table(v), VC.smiles_emit_table(v)
    corpus = CR.mutation_corpus()
    strings = ["C"] + RR.HAND_ROWS + ["C[C@H](N)O", "F/C=C/F", "C" * 128, "C(", "C=F", "cc", "C1=S(C)=CCC1"]
    strings += RR.fragment_corpus(100, seed=1)
    strings += corpus[1000:1000 + 260 - len(strings)]
    x = torch.from_numpy(CR.token_rows(strings, v, 134))
    assert len(QUERIES_64) == 64
    table, qstatus = ops.smiles_substruct_compile(torch.from_numpy(CR.token_rows(QUERIES_64, v)), tok, chem, emit, v.eos)
    assert qstatus.tolist() == [0] * 23 + [RR.STEREO] + [0] * 40 and len(strings) == 260
    e = {"v": v, "tabs": (tok.to(DEV), chem.to(DEV)), "host_tabs": (tok, chem), "strings": strings, "x": x, "table": table,
         "table_dev": table.to(DEV), "host": {}}

    def host(Q, mq):
        if (Q, mq) not in e["host"]:
            e["host"][Q, mq] = ops.smiles_substruct_host(x[:, :131], tok, chem, v.eos, table[:Q].contiguous(), SR.STEPS, mq)
        return e["host"][Q, mq]
    e["host_of"] = host
    full = host(64, 63)
    assert len(set(full[0].tolist())) >= 6 and (full[0] == 0).sum() >= 60 and not full[2].any()
    per_query = ops.substruct_bits(full[1], 64).sum(0)
    assert (per_query > 0).sum() >= 40 and per_query[23] == 0 and (full[1] < 0).any()      # the refused query hits nothing; bit 63 is set somewhere
    return e


def _rows(env, x, Q, mq, max_steps=SR.STEPS, counts=None, fill=True):
    B = x.shape[0]
    pre = ((torch.full((B,), FILL, dtype=torch.int32, device=DEV), torch.full((B,), FILL, dtype=torch.int64, device=DEV),
            torch.full((B,), FILL, dtype=torch.int64, device=DEV), torch.full((B, 32), 0x7f, dtype=torch.uint8, device=DEV),
            torch.full((B, Q), FILL, dtype=torch.int32, device=DEV)) if fill else (None,) * 5)
    return ops.smiles_substruct_rows(x, *env["tabs"], env["v"].eos, env["table_dev"][:Q].contiguous(), max_steps, mq, *pre, counts=counts)


def _differing(got, want):
    return [(name, torch.nonzero((g.cpu() != w).reshape(w.shape[0], -1).any(1)).flatten()[:5].tolist())
            for g, w, name in zip(got, want, NAMES) if not torch.equal(g.cpu(), w)]


def _column_sums(hit, und, Q):
    return torch.stack([ops.substruct_bits(hit, Q).sum(0), ops.substruct_bits(und, Q).sum(0)], 1).int()


@pytest.mark.parametrize("Q", [1, 22, 64])
@pytest.mark.parametrize("B", [1, 63, 65, 130, 260])
def test_rows_entry_equals_the_host_entry(env, B, Q):
    """B around the block size of 64; a strided input (x_ld = 134 > T = 131); outputs garbage-filled beforehand, so every element must be
    written; the map for the first and the last query; a second run is bit-identical; counts is the column sums of the hit and the
    undecided bits."""
    x = env["x"].to(DEV)[:B, :131]
    assert x.stride(0) == 134 or B == 1
    for mq in sorted({0, Q - 1}):
        counts = torch.zeros(Q, 2, dtype=torch.int32, device=DEV)
        out = _rows(env, x, Q, mq, counts=counts)
        want = tuple(t[:B] for t in env["host_of"](Q, mq))
        assert not _differing(out, want), _differing(out, want)
        assert torch.equal(counts.cpu(), _column_sums(want[1], want[2], Q))
    again = _rows(env, x, Q, mq, fill=False)
    assert all(torch.equal(a, o) for a, o in zip(again, out))
    bare = ops.smiles_substruct_rows(x, *env["tabs"], env["v"].eos, env["table_dev"][:Q].contiguous(), steps=False)
    assert bare[3] is None and bare[4] is None and all(torch.equal(b, o) for b, o in zip(bare[:3], out[:3]))


@pytest.mark.parametrize("N", [1, 63, 65, 130])
def test_corpus_entry_equals_the_host_entry(env, N):
    """One launch over the first N rows of a CSR corpus of the fixture's strings with an empty row in front: every output equals what the
    host entry gives for the same strings as padded rows (the empty row: status 1, as the graph entry has it)."""
    v = env["v"]
    strings = ([""] + [s for s in env["strings"] if len(s) <= 127])[:N]
    tokens, offsets = D.tokenize_corpus(strings, v)
    tokens_d = torch.from_numpy(np.concatenate([tokens, np.zeros(1, np.uint8)])).to(DEV)
    offsets_d = torch.from_numpy(offsets).to(DEV)
    for Q, mq in ((22, 21), (64, 0)):
        table = env["table"][:Q].contiguous()
        want = ops.smiles_substruct_host(torch.from_numpy(CR.token_rows(strings, v, 129)), *env["host_tabs"], v.eos, table, SR.STEPS, mq)
        pre = (torch.full((N,), FILL, dtype=torch.int32, device=DEV), torch.full((N,), FILL, dtype=torch.int64, device=DEV),
               torch.full((N,), FILL, dtype=torch.int64, device=DEV), torch.full((N, 32), 0x7f, dtype=torch.uint8, device=DEV),
               torch.full((N, Q), FILL, dtype=torch.int32, device=DEV))
        counts = torch.zeros(Q, 2, dtype=torch.int32, device=DEV)
        got = ops.smiles_substruct_corpus(tokens_d, offsets_d, N, *env["tabs"], table.to(DEV), SR.STEPS, mq, *pre, counts=counts)
        assert not _differing(got, want), _differing(got, want)
        assert int(want[0][0]) == 1 and torch.equal(counts.cpu(), _column_sums(want[1], want[2], Q))
        graph = ops.smiles_graph_corpus(tokens_d, offsets_d, N, *env["tabs"])[0]
        assert torch.equal(got[0], graph)


def test_budget_on_the_device(env):
    """The 16-ring in 25 cyclopropanes at both budgets: undecided, hit and steps as the host gives them.  Bounded by construction: at most
    131,072 candidates on one lane."""
    v = env["v"]
    tok, chem = env["host_tabs"]
    table, _ = ops.smiles_substruct_compile(torch.from_numpy(CR.token_rows([SR.BUDGET_QUERY, "C1CC1"], v)), tok, chem, VC.smiles_emit_table(v), v.eos)
    x = torch.from_numpy(CR.token_rows([SR.BUDGET_ROW, "CCO", SR.BUDGET_ROW], v))
    for budget, undecided in ((65536, 1), (131072, 0)):
        want = ops.smiles_substruct_host(x, tok, chem, v.eos, table, budget, 0)
        assert want[2].tolist() == [undecided, 0, undecided] and want[4][0].tolist() == [min(budget, 92938), 4]
        counts = torch.zeros(2, 2, dtype=torch.int32, device=DEV)
        got = ops.smiles_substruct_rows(x.to(DEV), *env["tabs"], v.eos, table.to(DEV), budget, 0, counts=counts)
        assert not _differing(got, want), _differing(got, want)
        assert counts.cpu().tolist() == [[0, 2 * undecided], [2, 0]]


@pytest.fixture(scope="module")
def small():
    """200 rows: 120 molecules of MOSES' lengths, 60 respellings of the first 60 and 20 rows the walk or the rewrite refuses."""
    vocab = CR.vocabulary()
    base = RR.fragment_corpus(120, seed=5)
    dup = [RR.respell(s, 3, i)[1] for i, s in enumerate(base[:60])]
    refused = ["C[C@H](N)O", "F/C=C/F", "C(", "C=F"] * 5
    smiles = base + dup + refused
    return smiles, vocab, D.MosesDeviceDataset(smiles, vocab, device=DEV)


PATTERNS = ["C(=O)[O-]", "C#N", "S(=O)(=O)", "c1ccncc1", "C1CC1", "I", "cC(=O)O"]


def _reference(strings, patterns):
    """Per string the reference's result per pattern; a string the walk refuses contains nothing."""
    return [[SR.search(s, p)[0] if CR.analyse(s)[0] == 0 else SR.MISS for p in patterns] for s in strings]


def test_dataset_counts_and_rows_against_the_reference(small):
    smiles, vocab, ds = small
    ref = np.array(_reference(smiles, PATTERNS))
    counts = ds.substructure_counts(PATTERNS)
    assert counts.dtype == torch.int32 and counts.device.type == "cuda"
    assert counts.cpu().tolist() == [[int((ref[:, k] == SR.HIT).sum()), 0] for k in range(len(PATTERNS))]
    assert min(c[0] for c in counts.cpu().tolist()[:5]) >= 1 and counts[5, 0] == 0
    table = D.compile_substructures(PATTERNS, vocab)
    assert torch.equal(ds.substructure_counts(table), counts)
    for k in (0, 3, 5):
        rows, open_rows = ds.rows_with_substructure(PATTERNS[k], return_undecided=True)
        assert rows.dtype == torch.int64 and rows.cpu().tolist() == np.nonzero(ref[:, k] == SR.HIT)[0].tolist() and open_rows.numel() == 0
    one = [SR.search(s, "N", 1)[0] if CR.analyse(s)[0] == 0 else SR.MISS for s in smiles]         # one candidate: the first atom
    rows, open_rows = ds.rows_with_substructure("N", max_steps=1, return_undecided=True)
    assert rows.cpu().tolist() == [i for i, r in enumerate(one) if r == SR.HIT] and one.count(SR.UNDECIDED) >= 20
    assert open_rows.cpu().tolist() == [i for i, r in enumerate(one) if r == SR.UNDECIDED]
    # VAE.has_substructure on strings and on rows, with the map of one pattern
    model = MV.VAE(vocab, dtype=torch.float32).to(DEV)
    hit, und, emb = model.has_substructure(smiles, table, return_map=3)
    assert hit.dtype == torch.bool and tuple(hit.shape) == (200, 7) and not und.any()
    assert np.array_equal(hit.cpu().numpy(), ref == SR.HIT)
    want = [SR.search(s, PATTERNS[3])[1] if r == SR.HIT else None for s, r in zip(smiles, ref[:, 3])]
    assert all(e.tolist() == (w + [0xFF] * (32 - len(w)) if w else [0xFF] * 32) for e, w in zip(emb.cpu(), want))
    with pytest.raises(ValueError, match="'C\\('.*syntax"):
        model.has_substructure(smiles[:2], ["C("])
    with pytest.raises(ValueError, match=r"max_steps must be in \[1, 1048576\]"):
        model.has_substructure(smiles[:2], ["C"], max_steps=0)


def test_moses_generate_filters_equal_values_recomputed_from_its_samples(small):
    """Three batches, the last one short, of a small randomly initialised model sampling under the syntax automaton after prefixes that
    carry some of the filtered groups; the three figures recomputed from the returned strings and counts with the reference."""
    vocab = small[1]
    torch.manual_seed(0)
    model = MV.VAE(vocab, dtype=torch.float32).to(DEV)
    filters = ["C#N", "C(=O)O", "c1ccccc1", "I"]
    n, kw = 240, dict(batch_size=96, max_len=14, top_k=4, seed=2, syntax=True, prefix=["N#CC", "OC(=O)C", "c1ccccc1", "C", "CCO", "C(C#N)"] * 40)
    plain = TR.moses_generate(model, n, valence=True, **kw)
    res = TR.moses_generate(model, n, valence=True, filters=filters, **kw)
    new = {"filters", "filter_hits", "filter_undecided"}
    assert set(res) == set(plain) | new and {k: res[k] for k in plain} == plain
    bare = TR.moses_generate(model, n, filters=D.compile_substructures(filters, vocab), **kw)
    assert all(bare[k] == res[k] for k in new)
    # syntax=True: every sample ends in <eos>, so a string's status is its row's; duplicates count
    strings, counts = res["strings"], res["counts"]
    ref = _reference(strings, filters)
    fine = [i for i, s in enumerate(strings) if CR.analyse(s)[0] == 0]
    n_fine = sum(counts[i] for i in fine)
    print("samples", n, "unique", len(strings), "valence-consistent", n_fine, "filters", res["filters"], "hits", res["filter_hits"])
    assert n_fine == res["chem_valid"] >= 20
    assert res["filter_hits"] == [sum(counts[i] for i in fine if ref[i][k] == SR.HIT) for k in range(4)] and res["filter_undecided"] == [0] * 4
    assert res["filters"] == sum(counts[i] for i in fine if all(r == SR.MISS for r in ref[i])) / n_fine
    assert 0 < res["filters"] < 1 and min(res["filter_hits"][:3]) >= 1 and res["filter_hits"][3] == 0
