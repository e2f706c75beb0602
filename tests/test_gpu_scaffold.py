"""GPU tests of the scaffold feature: mvae_smiles_scaffold_rows / _corpus against the host entry (the same source compiled for the CPU)
and the reference of tests/scaffold_ref.py, bit for bit; VAE.scaffolds, MosesDeviceDataset.scaffolds / scaffold_histogram /
rows_with_scaffold / scaffold_split and moses_generate(scaffolds=True) against the reference on the strings."""
import collections
import inspect
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import molecular_vae_amd as mv                                        # noqa: E402
from molecular_vae_amd import data as D, mosesvae as MV, vocab as VC, ops   # noqa: E402
import chem_ref as CR                                                 # noqa: E402
import scaffold_ref as SR                                             # noqa: E402

DEV = torch.device("cuda")
KEYS = {"total", "unique", "strings", "counts", "logq"}
KEYS_NOVEL = {"corpus_row", "is_novel", "novel"}
NEW = {"mol_key", "scaffold_key", "scaffold_atoms", "unique_graphs", "n_scaffolds"}
NEW_NOVEL = {"scaf", "scaffold_novel", "graph_novel"}


@pytest.fixture(scope="module")
def env():
    v = CR.vocabulary()
    tok, chem = VC.smiles_token_table(v), VC.smiles_chem_table(v)
    strings, want = SR.corpus_expected()
    x = torch.from_numpy(CR.token_rows(strings, v))
    host = tuple(t.numpy() for t in ops.smiles_scaffold_host(x, tok, chem, v.eos))
    for h, w in zip(host, want):
        assert (h == w).all()
    return {"v": v, "tok": tok, "chem": chem, "tok_d": tok.to(DEV), "chem_d": chem.to(DEV), "strings": strings, "x": x, "host": host}


def _filled(n):
    return (torch.full((n,), 0x7f7f7f7f, dtype=torch.int32, device=DEV), torch.full((n, 2), 0x7f7f7f7f7f7f7f7f, dtype=torch.int64, device=DEV),
            torch.full((n, 4), 0x7f7f7f7f, dtype=torch.int32, device=DEV), torch.full((n, 2), 0x7f7f7f7f7f7f7f7f, dtype=torch.int64, device=DEV))


def _same(got, want):
    for g, w, name in zip(got, want, ("status", "mask", "desc", "key")):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        w = w.cpu().numpy() if torch.is_tensor(w) else w
        wrong = np.nonzero((g != w).reshape(g.shape[0], -1).any(1))[0]
        assert g.shape == w.shape and wrong.size == 0, (name, wrong[:5].tolist(), g[wrong[:3]].tolist(), w[wrong[:3]].tolist())


@pytest.mark.parametrize("B", [1, 63, 64, 65, 4250])
def test_rows_entry_equals_the_host_entry(env, B):
    """B around the block size of 64, and the whole corpus; the outputs are garbage-filled beforehand, so every element must be written
    and a row that is not ok must come back zeroed; a second run is bit-identical; the mask may be left out."""
    lo = 0 if B == 4250 else 1000                                    # a stretch of the sorted corpus with several statuses
    x = env["x"][lo:lo + B].to(DEV)
    want = tuple(w[lo:lo + B] for w in env["host"])
    assert B < 60 or len(set(want[0].tolist())) >= 3
    out = _filled(B)
    ops.smiles_scaffold_rows(x, env["tok_d"], env["chem_d"], env["v"].eos, *out)
    _same(out, want)
    bad = out[0] != 0
    assert not out[1][bad].any() and not out[2][bad].any() and not out[3][bad].any()
    again = ops.smiles_scaffold_rows(x, env["tok_d"], env["chem_d"], env["v"].eos)
    assert all(torch.equal(a, o) for a, o in zip(again, out))
    status, _, desc, key = _filled(B)
    got = ops.smiles_scaffold_rows(x, env["tok_d"], env["chem_d"], env["v"].eos, status, False, desc, key)
    assert got[1] is None and torch.equal(status, out[0]) and torch.equal(desc, out[2]) and torch.equal(key, out[3])


@pytest.mark.parametrize("N", [1, 63, 64, 65, 4250])
def test_corpus_entry_equals_the_host_entry(env, N):
    """The CSR entry in one launch, with an empty row, a 127-token row and a 128-token row in front (3 < N < 4250)."""
    v = env["v"]
    first = ["", "C1CC1" + "C" * 117 + "C1CC1", "C" * 128]
    strings = [first[1]] if N == 1 else first + env["strings"][1000:1000 + N - 3] if N < 4250 else env["strings"]
    assert len(strings) == N
    tokens, offsets = D.tokenize_corpus(strings, v)
    tokens = torch.from_numpy(np.concatenate([tokens, np.zeros(1, np.uint8)])).to(DEV)
    offsets = torch.from_numpy(offsets).to(DEV)
    out = _filled(N)
    ops.smiles_scaffold_corpus(tokens, offsets, N, env["tok_d"], env["chem_d"], *out)
    if N == 4250:
        want = env["host"]
    else:
        want = tuple(t.numpy() for t in ops.smiles_scaffold_host(torch.from_numpy(CR.token_rows(strings, v)), env["tok"], env["chem"], v.eos))
    _same(out, want)
    again = ops.smiles_scaffold_corpus(tokens, offsets, N, env["tok_d"], env["chem_d"])
    assert all(torch.equal(a, o) for a, o in zip(again, out))
    without = ops.smiles_scaffold_corpus(tokens, offsets, N, env["tok_d"], env["chem_d"], mask=False)
    assert without[1] is None and torch.equal(without[3], out[3])
    if 3 < N < 4250:
        assert out[0][:3].tolist() == [CR.SYNTAX, 0, CR.TOO_LONG] and out[2][1].tolist() == [123, 124, 117, 0]


def test_rows_entry_edge_rows(env):
    """127 tokens in ring-bearing rows (two rings and a 117-atom linker; one ring of 125 atoms -- a ring takes two digit tokens, so 125 is
    the most atoms such a row has), 128 content tokens (TOO_LONG, zeros), a ring and a linker that each straddle atom 64, 25 rings in one
    row, a cage, and a strided view with x_ld > T: against the reference and the host entry."""
    v = env["v"]
    strings = ["C1CC1" + "C" * 117 + "C1CC1", "C1" + "C" * 124 + "1", "C" * 128, "C" * 60 + "C1CCCCCCC1", "c1ccccc1" + "C" * 62 + "c1ccccc1",
               "C1CC1" * 25 + "CC", "C12C3C4C1C5C2C3C45" + "C" * 100, "CCC1" + "C" * 66 + "1", "C" * 122 + "c1ccc1"]
    x_h = torch.from_numpy(CR.token_rows(strings, v))
    out = _filled(len(strings))
    ops.smiles_scaffold_rows(x_h.to(DEV), env["tok_d"], env["chem_d"], v.eos, *out)
    assert out[0].tolist() == [0, 0, CR.TOO_LONG, 0, 0, 0, 0, 0, CR.TOO_LONG]
    _same(out, SR.expected(strings))
    _same(out, ops.smiles_scaffold_host(x_h, env["tok"], env["chem"], v.eos))
    assert out[2][:2].tolist() == [[123, 124, 117, 0], [125, 125, 0, 0]] and out[2][4].tolist() == [74, 75, 62, 0]
    assert (out[1][3] != 0).all() and (out[1][4] != 0).all()          # both mask words in use
    wide = torch.full((len(strings), 200), v.eos, dtype=torch.long)
    wide[:, :x_h.shape[1]] = x_h
    view = wide.to(DEV)[:, :x_h.shape[1]]
    assert view.stride(0) == 200
    got = ops.smiles_scaffold_rows(view, env["tok_d"], env["chem_d"], v.eos)
    assert all(torch.equal(g, o) for g, o in zip(got, out))


# ---------------------------------------------------------------------------------------------------------------- the Python surface
@pytest.fixture(scope="module")
def setup(env):
    vocab = env["v"]
    pick = np.random.RandomState(9).choice(len(env["strings"]), size=300, replace=False)
    smiles = [env["strings"][i] for i in pick] + [s for s, _ in CR.FORMULAS]
    torch.manual_seed(5)
    model = MV.VAE(vocab, dtype=torch.float32).to(DEV).eval()
    return smiles, D.MosesDeviceDataset(smiles, vocab, device=DEV), model, SR.expected(smiles)


def _check_dict(d, want, n):
    assert set(d) == {"status", "mask", "atoms", "bonds", "linker_atoms", "exo_atoms", "mol_key", "scaffold_key"}
    assert all(t.is_cuda and t.shape[0] == n for t in d.values())
    assert d["status"].cpu().tolist() == want[0][:n].tolist() and (d["mask"].cpu().numpy() == want[1][:n]).all()
    for i, name in enumerate(("atoms", "bonds", "linker_atoms", "exo_atoms")):
        assert d[name].dtype == torch.int32 and d[name].cpu().tolist() == want[2][:n, i].tolist(), name
    for i, name in enumerate(("mol_key", "scaffold_key")):
        assert d[name].dtype == torch.int64 and d[name].cpu().tolist() == want[3][:n, i].tolist(), name


def test_vae_and_dataset_methods(setup):
    smiles, ds, model, want = setup
    _check_dict(model.scaffolds(smiles[:70]), want, 70)
    seqs = [model.string2tensor(s, device="cpu") for s in smiles[:70]]
    assert torch.equal(model.scaffolds(seqs)["scaffold_key"], model.scaffolds(smiles[:70])["scaffold_key"])
    d = ds.scaffolds()
    assert ds.scaffolds() is d
    _check_dict(d, want, len(smiles))
    counter = collections.Counter(k for k in want[3][:, 1].tolist() if k)
    keys, counts = ds.scaffold_histogram()
    assert ds.scaffold_histogram()[0] is keys and keys.is_cuda and keys.tolist() == sorted(counter)
    assert counts.tolist() == [counter[k] for k in sorted(counter)] and len(counter) >= 20
    assert ds.mol_keys_sorted().tolist() == sorted(want[3][:, 0].tolist())
    # the corpus rows of a query's scaffold: benzene's (toluene is no corpus row but has the same scaffold), none for a chain, a bad row
    queries = ["Cc1ccccc1", "CCCC", "C(", smiles[0], "c1ccccc1", "C1CCC1CCC1CC1"]
    qk = SR.expected(queries)[3][:, 1]
    offsets, rows = ds.rows_with_scaffold(queries)
    assert offsets.is_cuda and rows.is_cuda and offsets.dtype == rows.dtype == torch.int64 and offsets[0] == 0 and offsets.numel() == 7
    offsets, rows = offsets.tolist(), rows.tolist()
    for i, k in enumerate(qk.tolist()):
        assert rows[offsets[i]:offsets[i + 1]] == ([j for j, c in enumerate(want[3][:, 1].tolist()) if c == k] if k else []), queries[i]
    assert offsets[1] - offsets[0] >= 5 and offsets[2] == offsets[1] == offsets[3]
    assert rows[offsets[0]:offsets[1]] == rows[offsets[4]:offsets[5]]
    got = ds.smiles(rows[offsets[0]:offsets[1]])
    assert all(SR.scaffold(s)[3][1] == qk[0] for s in got)


@pytest.mark.parametrize("fraction", [0.0, 0.25, 1.0])
def test_scaffold_split(setup, fraction):
    """The two sides are disjoint, cover every row and share no non-zero scaffold key; rows without a scaffold stay in train; at least
    the asked fraction of the ring-bearing rows is held out; the same seed gives the same split, and the split equals the one
    ops.scaffold_split_rows makes of the same keys on the CPU."""
    smiles, ds, model, want = setup
    keys = want[3][:, 1]
    train, test = ds.scaffold_split(fraction, seed=7)
    assert train.is_cuda and test.is_cuda and train.dtype == test.dtype == torch.int64
    tr, te = train.tolist(), test.tolist()
    assert sorted(tr + te) == list(range(len(smiles))) and tr == sorted(tr) and te == sorted(te)
    assert not (set(keys[tr].tolist()) - {0}) & set(keys[te].tolist()) and 0 not in set(keys[te].tolist())
    ringed = int((keys != 0).sum())
    assert len(te) >= fraction * ringed and (fraction > 0 or not te) and (fraction < 1 or len(te) == ringed)
    again = ds.scaffold_split(fraction, seed=7)
    assert torch.equal(again[0], train) and torch.equal(again[1], test)
    cpu = ops.scaffold_split_rows(torch.from_numpy(keys.copy()), fraction, seed=7)
    assert cpu[0].tolist() == tr and cpu[1].tolist() == te
    if fraction == 0.25:
        assert ds.scaffold_split(fraction, seed=8)[1].tolist() != te


def test_moses_generate_scaffolds(setup):
    """Three batches, the last one short.  Every new key of the result equals the reference computed from the returned strings, "scaf" is
    within 8 x 2^-53 relative of the Counter cosine; without the flag the result has the keys it had, and the values the run with the
    flag reports for them; the ValueErrors come before device work.  A second run with a benzene prefix, whose scaffolds the corpus
    has, gives the cosine a value strictly between 0 and 1."""
    smiles, ds, model, want = setup
    assert inspect.signature(mv.moses_generate).parameters["scaffolds"].default is False
    n, kw = 200, dict(batch_size=96, max_len=20, top_k=4, seed=2, syntax=True)
    z = torch.from_numpy(np.random.RandomState(4).standard_normal((n, model.d_z)).astype(np.float32)).to(DEV)
    plain = mv.moses_generate(model, n, z=z, novel_against=ds, **kw)
    assert set(plain) == KEYS | KEYS_NOVEL
    res = mv.moses_generate(model, n, z=z, novel_against=ds, scaffolds=True, **kw)
    assert set(res) == set(plain) | NEW | NEW_NOVEL
    assert {key: res[key] for key in plain} == plain
    assert set(mv.moses_generate(model, n, z=z, **kw)) == KEYS
    only = mv.moses_generate(model, n, z=z, scaffolds=True, **kw)
    assert set(only) == KEYS | NEW and all(only[key] == res[key] for key in NEW)
    big = MV.VAE(VC.OneHotVocab([chr(65 + i) for i in range(61)]), dtype=torch.float32)
    with pytest.raises(ValueError, match="scaffolds=True supports at most 64 ids"):
        mv.moses_generate(big, 4, max_len=8, scaffolds=True)
    # syntax=True: every sample ends in <eos>, so a string's status is its row's
    strings = res["strings"]
    ref = SR.expected(strings)
    assert res["mol_key"] == ref[3][:, 0].tolist() and res["scaffold_key"] == ref[3][:, 1].tolist()
    assert res["scaffold_atoms"] == ref[2][:, 0].tolist()
    graphs, scafs = set(ref[3][:, 0].tolist()) - {0}, set(ref[3][:, 1].tolist()) - {0}
    print("unique", len(strings), "status 0:", int((ref[0] == 0).sum()), "unique graphs", len(graphs), "scaffolds", len(scafs), "scaf", res["scaf"],
          "scaffold_novel", res["scaffold_novel"], "graph_novel", res["graph_novel"])
    assert res["unique_graphs"] == len(graphs) >= 2 and res["n_scaffolds"] == len(scafs)
    assert sum(res["counts"]) == n
    gen = collections.Counter()
    for k, c in zip(res["scaffold_key"], res["counts"]):
        if k:
            gen[k] += c
    corpus = collections.Counter(k for k in want[3][:, 1].tolist() if k)
    cos = SR.cosine(gen, corpus)
    if math.isnan(cos):
        assert math.isnan(res["scaf"]) and not gen
    else:
        assert abs(res["scaf"] - cos) <= 8 * 2.0 ** -53 * cos
    assert res["scaffold_novel"] == len(scafs - set(corpus)) and res["graph_novel"] == len(graphs - set(want[3][:, 0].tolist()))
    assert res["graph_novel"] <= res["novel"]                         # a graph that is new is spelled by strings that are new
    # every sample starting with a benzene ring: scaffolds the corpus has, so the cosine is not trivially 0
    res = mv.moses_generate(model, n, z=z, novel_against=ds, scaffolds=True, prefix="c1ccccc1", **kw)
    ref = SR.expected(res["strings"])
    assert res["mol_key"] == ref[3][:, 0].tolist() and res["scaffold_key"] == ref[3][:, 1].tolist()
    gen = collections.Counter()
    for k, c in zip(res["scaffold_key"], res["counts"]):
        if k:
            gen[k] += c
    cos = SR.cosine(gen, corpus)
    print("with the prefix: unique", res["unique"], "scaffolds", len(gen), "samples with one", sum(gen.values()), "scaf", res["scaf"], "Counter", cos)
    assert len(gen) >= 2 and set(gen) & set(corpus) and 0 < cos < 1 and abs(res["scaf"] - cos) <= 8 * 2.0 ** -53 * cos
    assert res["n_scaffolds"] == len(gen) and res["scaffold_novel"] == len(set(gen) - set(corpus))
