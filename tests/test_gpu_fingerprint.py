"""GPU tests of the fingerprint feature: mvae_smiles_fp_rows / _corpus against the host entry (the same source compiled for the CPU) and
the reference of tests/fp_ref.py; mvae_tanimoto_knn against numpy for exact equality of (similarity bits, row); mvae_tanimoto_sum against
the numpy float64 sum; VAE.fingerprints / tanimoto, MosesDeviceDataset.fingerprints / nearest_fingerprints and
moses_generate(int_div=, snn=) against the reference on the strings."""
import inspect

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import molecular_vae_amd as mv                                        # noqa: E402
from molecular_vae_amd import _lib as L, data as D, mosesvae as MV, vocab as VC, ops   # noqa: E402
import chem_ref as CR                                                 # noqa: E402
import fp_ref as FR                                                   # noqa: E402

DEV = torch.device("cuda")
R = 256                                                               # table rows per block step of the search
KEYS = {"total", "unique", "strings", "counts", "logq"}
KEYS_NOVEL = {"corpus_row", "is_novel", "novel"}


@pytest.fixture(scope="module")
def env():
    v = CR.vocabulary()
    tok, chem = VC.smiles_token_table(v), VC.smiles_chem_table(v)
    strings, status, fp = FR.corpus_fingerprints()
    x = torch.from_numpy(CR.token_rows(strings, v))
    host = tuple(t.numpy() for t in ops.smiles_fp_host(x, tok, chem, v.eos))
    assert (host[0] == status).all() and (host[1] == fp).all()
    table = np.ascontiguousarray(fp[status == 0])                   # the 833 status-0 fingerprints
    queries = np.concatenate([table[:64], np.zeros((2, 16), np.int64)])
    return {"v": v, "tok": tok, "chem": chem, "tok_d": tok.to(DEV), "chem_d": chem.to(DEV), "strings": strings, "x": x, "host": host,
            "table": table, "queries": queries, "sim": FR.similarity(queries, table)}


def _filled(n):
    return torch.full((n,), 0x7f7f7f7f, dtype=torch.int32, device=DEV), torch.full((n, 16), 0x7f7f7f7f7f7f7f7f, dtype=torch.int64, device=DEV)


def _knn(q, table, k, exclude=None):
    """One launch into NaN / garbage-filled outputs, and a second one: bit-equal."""
    q, table = torch.from_numpy(q).to(DEV), torch.from_numpy(table).to(DEV)
    ex = None if exclude is None else torch.from_numpy(exclude).to(DEV)
    sim = torch.full((q.shape[0], k), float("nan"), device=DEV)
    idx = torch.full((q.shape[0], k), 0x7f7f7f7f7f7f7f7f, dtype=torch.int64, device=DEV)
    ops.tanimoto_knn(q, table, k, exclude=ex, sim=sim, idx=idx)
    again = ops.tanimoto_knn(q, table, k, exclude=ex)
    assert torch.equal(sim.view(torch.int32), again[0].view(torch.int32)) and torch.equal(idx, again[1])
    return sim.cpu().numpy(), idx.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- fingerprints
@pytest.mark.parametrize("B", [1, 63, 64, 65, 4250])
def test_rows_entry_equals_the_host_entry(env, B):
    """B around the block size of 64, and the whole corpus; the outputs are garbage-filled beforehand, so every element must be written
    and a row that is not ok must come back zeroed; a second run is bit-identical."""
    lo = 0 if B == 4250 else 1000                                    # a stretch of the sorted corpus with several statuses
    x = env["x"][lo:lo + B].to(DEV)
    want = tuple(w[lo:lo + B] for w in env["host"])
    assert B < 60 or len(set(want[0].tolist())) >= 3
    status, fp = _filled(B)
    ops.smiles_fp_rows(x, env["tok_d"], env["chem_d"], env["v"].eos, status, fp)
    assert (status.cpu().numpy() == want[0]).all() and (fp.cpu().numpy() == want[1]).all()
    assert not fp[status != 0].any()
    again = ops.smiles_fp_rows(x, env["tok_d"], env["chem_d"], env["v"].eos)
    assert torch.equal(again[0], status) and torch.equal(again[1], fp)


def test_rows_entry_edge_rows(env):
    """127 content tokens and 128 (TOO_LONG), a ring across both mask words, 25 closures in one row, a strided view with x_ld > T."""
    v = env["v"]
    strings = ["C" * 127, "C" * 128, "CCC1" + "C" * 66 + "1", "C1CC1" * 25 + "CC", "c1ccccc1" * 15 + "C" * 6 + "c", "C" * 122 + "c1ccc1"]
    x_h = torch.from_numpy(CR.token_rows(strings, v))
    status, fp = _filled(len(strings))
    ops.smiles_fp_rows(x_h.to(DEV), env["tok_d"], env["chem_d"], v.eos, status, fp)
    assert status.tolist() == [0, CR.TOO_LONG, 0, 0, CR.AROMATIC, CR.TOO_LONG]
    assert (fp.cpu().numpy() == FR.fingerprints(strings)).all() and not fp[1].any()
    host = ops.smiles_fp_host(x_h, env["tok"], env["chem"], v.eos)
    assert torch.equal(host[0], status.cpu()) and torch.equal(host[1], fp.cpu())
    wide = torch.full((len(strings), 200), v.eos, dtype=torch.long)
    wide[:, :x_h.shape[1]] = x_h
    view = wide.to(DEV)[:, :x_h.shape[1]]
    assert view.stride(0) == 200
    got = ops.smiles_fp_rows(view, env["tok_d"], env["chem_d"], v.eos)
    assert torch.equal(got[0], status) and torch.equal(got[1], fp)


@pytest.mark.parametrize("N", [1, 63, 65, 4250])
def test_corpus_entry_equals_the_host_entry(env, N):
    """The CSR entry in one launch, with an empty row, a 127-token row and a 128-token row in front (N > 3)."""
    v = env["v"]
    strings = ["C" * 127] if N == 1 else ["", "C" * 127, "C" * 128] + env["strings"][1000:1000 + N - 3] if N < 4250 else env["strings"]
    assert len(strings) == N
    tokens, offsets = D.tokenize_corpus(strings, v)
    tokens = torch.from_numpy(np.concatenate([tokens, np.zeros(1, np.uint8)])).to(DEV)
    offsets = torch.from_numpy(offsets).to(DEV)
    status, fp = _filled(N)
    ops.smiles_fp_corpus(tokens, offsets, N, env["tok_d"], env["chem_d"], status, fp)
    if N == 4250:
        want = env["host"]
    else:
        want = tuple(t.numpy() for t in ops.smiles_fp_host(torch.from_numpy(CR.token_rows(strings, v)), env["tok"], env["chem"], v.eos))
    assert (status.cpu().numpy() == want[0]).all() and (fp.cpu().numpy() == want[1]).all()
    again = ops.smiles_fp_corpus(tokens, offsets, N, env["tok_d"], env["chem_d"])
    assert torch.equal(again[0], status) and torch.equal(again[1], fp)
    if 3 < N < 4250:
        assert status[:3].tolist() == [CR.SYNTAX, 0, CR.TOO_LONG]


# ---------------------------------------------------------------------------------------------------------------- the search
@pytest.mark.parametrize("k", [1, 4, 32])
def test_ties_are_abundant(env, k):
    """At least 10 of the 64 queries have equal similarity at ranks k and k + 1 (asserted on the reference alone)."""
    ties = FR.ties_at(env["sim"][:64], k)
    print("k", k, "queries with a tie at ranks k, k + 1:", ties)
    assert ties >= 10


@pytest.mark.parametrize("Q", [1, 3, 64, 65])
@pytest.mark.parametrize("k", [1, 4, 32])
def test_knn_equals_numpy(env, k, Q):
    """The 833-row table (four 256-row steps: four slots and the merge launch for these Q) and queries that include an all-zero
    fingerprint (similarity 0 to everything: the lowest rows)."""
    pick = {1: [0], 3: [0, 64, 7], 64: list(range(64)), 65: list(range(65))}[Q]
    assert L.load().mvae_tanimoto_knn_workspace(Q, 833, k) > 0
    got = _knn(env["queries"][pick], env["table"], k)
    FR.check_knn(*got, *FR.knn(env["sim"][pick], k))
    if Q == 65:
        assert got[1][64].tolist() == list(range(k)) and (got[0][64] == 0).all()
    if Q >= 64:                                                      # a query's answer is unchanged when it runs alone
        for i in (5, 63):
            alone = _knn(env["queries"][i:i + 1], env["table"], k)
            assert (alone[0].view(np.int32) == got[0][i:i + 1].view(np.int32)).all() and (alone[1] == got[1][i:i + 1]).all()


@pytest.mark.parametrize("N", [1, 3, R - 1, R, R + 1, 2 * R + 3])
def test_knn_table_sizes_around_the_block_step(env, N):
    """N = 1 and 3 < k give the (-1.0, -1) tail; R + 1 and 2 R + 3 leave one and three rows to the last step."""
    k, pick = 4, [0, 65, 9]
    got = _knn(env["queries"][pick], env["table"][:N], k)
    FR.check_knn(*got, *FR.knn(env["sim"][pick][:, :N], k))
    if N < k:
        assert (got[0][:, N:] == -1.0).all() and (got[1][:, N:] == -1).all()
    assert (L.load().mvae_tanimoto_knn_workspace(3, N, k) > 0) == (N > R)


def test_knn_large_table_with_duplicates(env):
    """The table tiled 100 times (83 300 rows, 10 MB): 163 slots of two 256-row steps each and the merge launch; every row has 100
    copies, so every rank is a tie that must resolve to the lower row."""
    reps, k, pick = 100, 32, [0, 65, 9]
    table = np.tile(env["table"], (reps, 1))
    lib = L.load()
    assert lib.mvae_tanimoto_knn_workspace(3, table.shape[0], k) == 163 * 3 * k * 12
    got = _knn(env["queries"][pick], table, k)
    FR.check_knn(*got, *FR.knn(np.tile(env["sim"][pick], (1, reps)), k))
    assert (np.diff(got[1][0]) > 0).sum() >= 16                      # runs of equal similarity in ascending rows


def test_knn_every_row_duplicated(env):
    """Each row twice, side by side: ties resolve to the lower row at every rank."""
    table = np.repeat(env["table"], 2, axis=0)
    got = _knn(env["queries"][:64], table, 32)
    FR.check_knn(*got, *FR.knn(np.repeat(env["sim"][:64], 2, axis=1), 32))
    assert (got[1][:, 0] % 2 == 0).all() and (got[1][:, 1] == got[1][:, 0] + 1).all() and (got[0][:, :2] == 1.0).all()


def test_knn_exclude(env):
    """Queries 0 .. 63 are table rows 0 .. 63: excluding the own row moves everything up one rank; -1 excludes nothing; with N - 1 < k
    the tail is (-1.0, -1)."""
    exclude = np.arange(66, dtype=np.int64)
    exclude[[3, 64, 65]] = -1
    got = _knn(env["queries"], env["table"], 4, exclude)
    FR.check_knn(*got, *FR.knn(env["sim"], 4, exclude))
    assert (got[1] != np.where(exclude >= 0, exclude, -2)[:, None]).all() and (got[1][3] == FR.knn(env["sim"][3:4], 4)[1][0]).all()
    got = _knn(env["queries"][:5], env["table"][:4], 4, exclude[:5])
    FR.check_knn(*got, *FR.knn(env["sim"][:5, :4], 4, exclude[:5]))
    assert (got[1][[0, 1, 2], 3] == -1).all() and (got[0][[0, 1, 2], 3] == -1.0).all() and (got[1][3] >= 0).all()


# ---------------------------------------------------------------------------------------------------------------- the pairwise sum
@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("N", [1, 65, 833])
@pytest.mark.parametrize("M", [1, 65, 833])
def test_sum_equals_numpy(env, M, N, skip):
    """Against the numpy float64 sum of the f32 similarities, within 2 n 2^-53 relative (n the pair count: the bound for any summation
    order of non-negative terms); two runs are bitwise equal."""
    a, b = env["table"][-M:], env["table"][:N]
    want = FR.pair_sum(FR.similarity(a, b), skip)
    a_d, b_d = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    out = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
    ops.tanimoto_sum(a_d, b_d, skip, out)
    got = float(out)
    print("M", M, "N", N, "skip", skip, "sum", got, "reference", want, "difference", got - want)
    assert abs(got - want) <= 2 * M * N * 2.0 ** -53 * want
    assert torch.equal(ops.tanimoto_sum(a_d, b_d, skip).view(torch.int64), out.view(torch.int64))
    if M == N == 833 and not skip:
        same = float(ops.tanimoto_sum(b_d, b_d))
        assert abs(same - float(ops.tanimoto_sum(b_d, b_d, True)) - 833.0) <= 1e-9 * same       # the diagonal is 833 ones


# ---------------------------------------------------------------------------------------------------------------- the Python surface
@pytest.fixture(scope="module")
def setup(env):
    vocab = env["v"]
    pick = np.random.RandomState(9).choice(len(env["strings"]), size=300, replace=False)
    smiles = [env["strings"][i] for i in pick] + [s for s, _ in CR.FORMULAS]
    torch.manual_seed(5)
    model = MV.VAE(vocab, dtype=torch.float32).to(DEV).eval()
    return smiles, D.MosesDeviceDataset(smiles, vocab, device=DEV), model


def test_vae_and_dataset_methods(env, setup):
    smiles, ds, model = setup
    want = FR.fingerprints(smiles)
    status = CR.expected(smiles)[0]
    f = model.fingerprints(smiles[:70])
    assert set(f) == {"status", "fp"} and f["fp"].is_cuda and f["fp"].dtype == torch.int64 and tuple(f["fp"].shape) == (70, 16)
    assert f["status"].cpu().tolist() == status[:70].tolist() and (f["fp"].cpu().numpy() == want[:70]).all()
    seqs = [model.string2tensor(s, device="cpu") for s in smiles[:70]]
    assert torch.equal(model.fingerprints(seqs)["fp"], f["fp"])
    d = ds.fingerprints()
    assert ds.fingerprints() is d and d["status"].cpu().tolist() == status.tolist() and (d["fp"].cpu().numpy() == want).all()
    sim = FR.similarity(want, want)
    t = model.tanimoto(smiles[:70], smiles[70:140])
    assert t.dtype == torch.float32 and (np.abs(t.cpu().numpy() - sim[np.arange(70), np.arange(70, 140)]) <= 2.0 ** -24).all()
    with pytest.raises(ValueError, match="rows against"):
        model.tanimoto(smiles[:3], smiles[:4])
    queries = smiles[:40] + ["CCOCC", "c1ccncc1C", "C(", "C=F"]
    qsim = FR.similarity(FR.fingerprints(queries), want)
    got = ds.nearest_fingerprints(queries, k=5)
    FR.check_knn(got[0].cpu().numpy(), got[1].cpu().numpy(), *FR.knn(qsim, 5))
    own = ds.lookup(queries).cpu().numpy()
    assert (own[:40] >= 0).all()
    got = ds.nearest_fingerprints(queries, k=5, exclude_self=True)
    FR.check_knn(got[0].cpu().numpy(), got[1].cpu().numpy(), *FR.knn(qsim, 5, own))
    assert (got[1].cpu().numpy() != own[:, None]).all()


def test_moses_generate_int_div_and_snn(setup):
    """Three batches, the last one short.  int_div and snn equal the reference computed from the returned strings (within the bound of
    the float64 sums; snn_sim and snn_row exactly); without the flags the result has the keys it had, and the values the run with the
    flags reports for them -- asking for the figures changes nothing under the old keys."""
    smiles, ds, model = setup
    sig = inspect.signature(mv.moses_generate).parameters
    assert sig["int_div"].default is False and sig["snn"].default is False
    n, kw = 200, dict(batch_size=96, max_len=14, top_k=4, seed=2, syntax=True)
    z = torch.from_numpy(np.random.RandomState(4).standard_normal((n, model.d_z)).astype(np.float32)).to(DEV)
    plain = mv.moses_generate(model, n, z=z, novel_against=ds, **kw)
    assert set(plain) == KEYS | KEYS_NOVEL
    res = mv.moses_generate(model, n, z=z, novel_against=ds, int_div=True, snn=True, **kw)
    assert set(res) == set(plain) | {"int_div", "n_fingerprinted", "snn", "snn_sim", "snn_row"}
    assert {key: res[key] for key in plain} == plain
    assert set(mv.moses_generate(model, n, z=z, **kw)) == KEYS
    only = mv.moses_generate(model, n, z=z, int_div=True, **kw)
    assert set(only) == KEYS | {"int_div", "n_fingerprinted"} and only["int_div"] == res["int_div"]
    with pytest.raises(ValueError, match="snn=True needs novel_against"):
        mv.moses_generate(model, n, z=z, snn=True, **kw)
    # syntax=True: every sample ends in <eos>, so a string's status is its row's
    strings = res["strings"]
    fp = FR.fingerprints(strings)
    ok = CR.expected(strings)[0] == 0
    m = int(ok.sum())
    print("unique", len(strings), "status 0:", m, "int_div", res["int_div"], "snn", res["snn"])
    assert res["n_fingerprinted"] == m >= 2 and len(res["snn_sim"]) == len(res["snn_row"]) == len(strings)
    total = FR.pair_sum(FR.similarity(fp[ok], fp[ok]))
    assert abs((1.0 - res["int_div"]) - total / (m * m)) <= 2 * m * m * 2.0 ** -53 * total / (m * m) + 2.0 ** -52
    corpus = ds.fingerprints()["fp"].cpu().numpy()
    want_s, want_j = FR.knn(FR.similarity(fp, corpus), 1)
    want_s, want_j = np.where(ok, want_s[:, 0], np.float32(-1.0)), np.where(ok, want_j[:, 0], -1)
    assert (np.array(res["snn_sim"], np.float32).view(np.int32) == want_s.view(np.int32)).all() and res["snn_row"] == want_j.tolist()
    mean = want_s[ok].astype(np.float64).sum() / m
    assert abs(res["snn"] - mean) <= 2 * m * 2.0 ** -53 * mean + 2.0 ** -52
    hit = np.array(res["corpus_row"]) >= 0
    assert (np.array(res["snn_sim"])[hit & ok] == 1.0).all()                    # a sample that is a corpus row is its own nearest
