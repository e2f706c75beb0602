"""GPU tests of the scaffold SMILES: mvae_smiles_scaffold_smiles_rows / _corpus against the host entry (the same source compiled for the
CPU, which tests/test_scaffold_smiles_host.py holds against the reference), bit for bit in tokens, lengths, statuses and info at the
block edges; MosesDeviceDataset.scaffold_smiles(); VAE.scaffold_smiles in front of the substructure search; and
moses_generate(top_scaffolds=) against values recomputed from its own samples."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from molecular_vae_amd import data as D, mosesvae as MV, train as TR, vocab as VC, ops   # noqa: E402
import chem_ref as CR                                                 # noqa: E402
import rewrite_ref as RR                                              # noqa: E402
import scaffold_smiles_ref as SS                                      # noqa: E402
from test_scaffold_smiles_host import MULTI, DEEP, LADDER, WORKED    # noqa: E402  (constants)

DEV = torch.device("cuda")
FILL = 0x7f7f7f7f
NAMES = ("out", "out_len", "status", "info")
# 127 tokens and 125 atoms, every one of them in S: an atom takes a token and a ring two more, so no row with a ring has more atoms
RING125 = "C1" + "C" * 123 + "C1"


@pytest.fixture(scope="module")
def env():
    """260 rows: 1 atom to 127 atoms (the hand rows: a ring-free chain of 127 atoms, 25 rings in 127 tokens), the largest row that is
    all scaffold, one row of every refusal, the header's worked examples, 100 molecules of MOSES' lengths and a slice of the mutation
    corpus; the host entry's outputs for them with T_out = 131, computed once and left unchanged."""
    v = CR.vocabulary()
    tok, chem, emit = VC.smiles_token_table(v), VC.smiles_chem_table(v), VC.smiles_emit_table(v)
    corpus = CR.mutation_corpus()
    strings = ["C", "C1CC1", RING125] + RR.HAND_ROWS + ["C[C@H]1CC1", "F/C=C/C1CC1", "C" * 128, "C(", "C=F", "[N+2]C", "C1C1", "cc", MULTI,
                                                       LADDER, DEEP, "CCO"] + [w[0] for w in WORKED]
    strings += ["Cn1ccc2ccccc12", "Cn1cnc2ccccc12", "CCn1cccc1", "Cc1cc(C)n(C)c1"]                 # more atoms that gain a bracket
    strings += RR.fragment_corpus(100, seed=1)
    strings += corpus[1000:1000 + 260 - len(strings)]
    x = torch.from_numpy(CR.token_rows(strings, v, 134))
    host = ops.smiles_scaffold_smiles_host(x, tok, chem, emit, v.bos, v.eos, v.pad, 127, 131)
    assert len(strings) == 260 and set(host[2].tolist()) >= {0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 14} and (host[2] == 0).sum() >= 100
    assert int(host[3][:, 0].max()) == 125 and (host[3][:, 2] > 0).sum() >= 5 and (host[3][:, 3] > 0).sum() >= 80
    return {"v": v, "tabs": (tok.to(DEV), chem.to(DEV), emit.to(DEV)), "host_tabs": (tok, chem, emit), "strings": strings, "x": x, "host": host}


def _rows(env, x, max_content=127, T_out=131, counts=None, fill=True):
    v, B = env["v"], x.shape[0]
    pre = ((torch.full((B, T_out), FILL, dtype=torch.int64, device=DEV), torch.full((B,), FILL, dtype=torch.int32, device=DEV),
            torch.full((B,), FILL, dtype=torch.int32, device=DEV), torch.full((B, 4), FILL, dtype=torch.int32, device=DEV))
           if fill else (None,) * 4)
    return ops.smiles_scaffold_smiles_rows(x, *env["tabs"], v.bos, v.eos, v.pad, max_content, T_out, *pre, counts=counts)


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
    scaffolds into LONG, which are empty rows; info may be left out."""
    v = env["v"]
    x = env["x"].to(DEV)
    full = _rows(env, x)
    for T_out in (9, 2):
        cut = _rows(env, x, T_out=T_out)
        assert torch.equal(cut[0], full[0][:, :T_out]) and all(torch.equal(c, f) for c, f in zip(cut[1:], full[1:]))
    assert (full[1] > 9).sum() > 50
    for mc in (1, 20):
        got = _rows(env, x, max_content=mc)
        want = ops.smiles_scaffold_smiles_host(env["x"], *env["host_tabs"], v.bos, v.eos, v.pad, mc, 131)
        assert not _differing(got, want) and (want[2] == RR.LONG).sum() >= 10 and (want[1][want[2] != 0] == 2).all()
    bare = ops.smiles_scaffold_smiles_rows(x, *env["tabs"], v.bos, v.eos, v.pad, 127, 131, info=False)
    assert bare[3] is None and all(torch.equal(b, f) for b, f in zip(bare[:3], full[:3]))


def _corpus_case(env, B):
    """A CSR corpus of the fixture's rows with an empty row in front, and B shuffled row ids with a repeat and two ids outside [0, N)."""
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
    """One launch over selected CSR rows: tokens_out, offsets_out (the gapped CSR), status and info equal what the host entry gives for
    the same strings; an id outside the corpus is an empty row with status 1 and err 2; counts is the histogram."""
    v = env["v"]
    strings, tokens, offsets, rows = _corpus_case(env, B)
    N, stride = len(strings), 127
    inside = (rows >= 0) & (rows < N)
    picked = [strings[r] if ok else "" for r, ok in zip(rows, inside)]
    want = ops.smiles_scaffold_smiles_host(torch.from_numpy(CR.token_rows(picked, v, 129)), *env["host_tabs"], v.bos, v.eos, v.pad, 127, 129)
    tokens_d = torch.from_numpy(np.concatenate([tokens, np.zeros(1, np.uint8)])).to(DEV)
    offsets_d, rows_d = torch.from_numpy(offsets).to(DEV), torch.from_numpy(rows).to(DEV)
    counts = torch.zeros(16, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    pre = (torch.full((B, stride), 0x7f, dtype=torch.uint8, device=DEV), torch.full((2 * B + 1,), FILL, dtype=torch.int64, device=DEV),
           torch.full((B,), FILL, dtype=torch.int32, device=DEV), torch.full((B, 4), FILL, dtype=torch.int32, device=DEV))
    tokens_out, offsets_out, status, info = ops.smiles_scaffold_smiles_corpus(tokens_d, offsets_d, N, rows_d, *env["tabs"], 127, stride, *pre,
                                                                              counts=counts, err=err)
    lens = want[1].numpy() - 2
    assert int(err.item()) == (2 if not inside.all() else 0)
    assert status.cpu().tolist() == [int(s) if ok else 1 for s, ok in zip(want[2], inside)]
    off = offsets_out.cpu().numpy()
    assert off[0::2].tolist() == [b * stride for b in range(B + 1)] and (off[1::2] - off[0:-1:2]).tolist() == lens.tolist()
    assert (lens[status.cpu().numpy() != 0] == 0).all()
    content = np.zeros((B, stride), np.int64)
    for b in range(B):
        content[b, :lens[b]] = want[0][b, 1:1 + lens[b]].numpy()
    assert (tokens_out.cpu().numpy() == content).all()
    assert torch.equal(info.cpu(), want[3])
    assert torch.equal(counts.cpu(), torch.bincount(status.cpu(), minlength=16).int())
    again = ops.smiles_scaffold_smiles_corpus(tokens_d, offsets_d, N, rows_d, *env["tabs"], 127, stride)
    assert all(torch.equal(a, o) for a, o in zip(again, (tokens_out, offsets_out, status, info)))


@pytest.fixture(scope="module")
def small():
    """200 rows: 120 molecules of MOSES' lengths, 60 respellings of the first 60 (the same scaffolds under other spellings), the worked
    examples, and rows without a scaffold."""
    vocab = CR.vocabulary()
    base = RR.fragment_corpus(120, seed=5)
    dup = [RR.respell(s, 3, i)[1] for i, s in enumerate(base[:60])]
    rest = [w[0] for w in WORKED] + ["C[C@H]1CC1", "F/C=C/F", "C(", "C=F", "CCO", "CC(C)C", "C"] + ["OCC"] * 6
    smiles = base + dup + rest
    assert len(smiles) == 200
    return smiles, vocab, D.MosesDeviceDataset(smiles, vocab, device=DEV)


def test_dataset_scaffold_smiles(small):
    smiles, vocab, ds = small
    want, status = D.scaffold_smiles(smiles, vocab, device="cpu", return_status=True)
    ds_scaf, rows = ds.scaffold_smiles()
    again = ds.scaffold_smiles()
    assert again[0] is ds_scaf and again[1] is rows and ds_scaf.device == ds.device and rows.dtype == torch.int64
    have = [i for i, st in enumerate(status.tolist()) if st == 0]
    assert 100 <= len(have) < 200 and rows.cpu().tolist() == have and len(ds_scaf) == len(have)
    assert ds.scaffold_smiles_status.cpu().tolist() == status.tolist()
    assert ds.scaffold_smiles_counts.cpu().tolist() == np.bincount(status, minlength=16).tolist()
    got = ds_scaf.smiles(list(range(len(have))))
    assert got == [want[i] for i in have] and all(got) and int(ds_scaf.lengths.min()) >= 3
    assert got[-7:] == [w[1] for w in WORKED]
    assert ds_scaf.n_distinct == len({want[i] for i in have}) == len({SS.scaffold(smiles[i])[1] for i in have}) < len(have)
    assert D.scaffold_smiles(smiles[:8] + ["CCO"], vocab, device=DEV) == want[:8] + [""]


def test_model_scaffolds_are_substructures_of_their_rows(small):
    """VAE.scaffold_smiles, decoded, compiled and searched for in its own inputs: row b contains scaffold b."""
    smiles, vocab, _ = small
    model = MV.VAE(vocab, dtype=torch.float32).to(DEV)
    ringed = [s for s, t in zip(smiles[:120], D.scaffold_smiles(smiles[:120], vocab, device="cpu")) if t]
    rows = ringed[:56] + [w[0] for w in WORKED] + ["CCO"]
    out, out_len, status = model.scaffold_smiles(rows)
    want, want_status = D.scaffold_smiles(rows, vocab, device="cpu", return_status=True)
    assert status.cpu().tolist() == want_status.tolist() == [0] * 63 + [SS.NO_RING] and out.shape[1] == 129
    assert out_len.cpu().tolist() == [len(s) + 2 for s in want] and out[-1].cpu().tolist() == [vocab.bos, vocab.eos] + [vocab.pad] * 127
    got = [vocab.ids2string(r[:k], rem_bos=True, rem_eos=True) for r, k in zip(out.cpu().tolist(), out_len.cpu().tolist())]
    assert got == want
    table = D.compile_substructures(got[:63], vocab)
    hit, undecided = model.has_substructure(rows[:63], table)
    q = torch.arange(63)
    assert hit[q, q].all() and not undecided.any()
    assert not hit.all()                                            # and not because everything hits everything


def test_moses_generate_top_scaffolds_equals_values_recomputed_from_its_samples(small):
    """Three batches, the last one short, of a small randomly initialised model sampling under the syntax automaton after prefixes that
    hold rings, so that scaffolds repeat: the counts are recomputed from the returned samples with the host entry."""
    vocab = small[1]
    torch.manual_seed(0)
    model = MV.VAE(vocab, dtype=torch.float32).to(DEV)
    n, kw = 240, dict(batch_size=96, max_len=14, top_k=4, seed=2, syntax=True, scaffolds=True,
                      prefix=["c1ccccc1", "C1CC1", "c1ccncc1", "O=C1CCCC1", "C", "c1ccccc1C"] * 40)
    plain = TR.moses_generate(model, n, **kw)
    res = TR.moses_generate(model, n, top_scaffolds=3, **kw)
    assert set(res) == set(plain) | {"top_scaffolds"} and {k: res[k] for k in plain} == plain
    assert TR.moses_generate(model, n, top_scaffolds=0, **kw) == plain
    strings, counts = res["strings"], res["counts"]
    tabs = (VC.smiles_token_table(vocab), VC.smiles_chem_table(vocab), VC.smiles_emit_table(vocab))
    out, out_len, status, _ = ops.smiles_scaffold_smiles_host(torch.from_numpy(CR.token_rows(strings, vocab)), *tabs, vocab.bos, vocab.eos,
                                                              vocab.pad, T_out=129)
    drawn = {}
    for row, k, st, c in zip(out.tolist(), out_len.tolist(), status.tolist(), counts):
        if st == 0:
            drawn[tuple(row)] = drawn.get(tuple(row), 0) + c
    order = sorted(drawn, key=lambda r: (-drawn[r], r))
    want = [(vocab.ids2string(list(r[:r.index(vocab.eos) + 1]), rem_bos=True, rem_eos=True), drawn[r]) for r in order]
    print("scaffolds:", len(want), "top:", want[:4])
    assert len(want) >= 4 and want[0][1] >= 2 and len({c for _, c in want}) < len(want)      # repeats, and a tie for the rows to break
    assert res["top_scaffolds"] == want[:3]
    assert TR.moses_generate(model, n, top_scaffolds=1000, **kw)["top_scaffolds"] == want
