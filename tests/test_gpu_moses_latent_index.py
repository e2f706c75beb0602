"""GPU tests of the latent table of a device corpus: mosesvae.VAE.encode, MosesDeviceDataset.encode_latents / smiles and
data.MosesLatentIndex.search / neighbors, on a randomly initialised model over a 300-row synthetic corpus."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import molecular_vae_amd as mv                                    # noqa: E402
from molecular_vae_amd import data as D, mosesvae as MV, ops, vocab as VC   # noqa: E402
import knn_ref as KR                                              # noqa: E402

DEV = torch.device("cuda")
ALPHABET = "CNOSFcnos()=#123[]@H+-lBrIPe%4"                       # 30 characters
N, BS = 300, 64


@pytest.fixture(scope="module")
def setup():
    """(model, corpus strings, dataset, latent index): lengths from {0, 1, 7, 57}, every fourth row a repeat of an earlier one."""
    rs = np.random.RandomState(5)
    strings = []
    for r in range(N):
        if r % 4 == 3:
            strings.append(strings[int(rs.randint(0, r))])
        else:
            strings.append("".join(rs.choice(list(ALPHABET), size=int(rs.choice([0, 1, 7, 57])))))
    torch.manual_seed(3)
    model = MV.VAE(VC.OneHotVocab(set(ALPHABET)), dtype=torch.bfloat16).to(DEV).eval()
    ds = D.MosesDeviceDataset(strings, model.vocabulary, device=DEV)
    index = ds.encode_latents(model, batch_size=BS)
    ds.check_errors()
    return model, strings, ds, index


def test_encode_latents_is_the_encoder_mean_of_every_row_chunk_by_chunk(setup):
    model, strings, ds, index = setup
    assert isinstance(index, mv.MosesLatentIndex) and index.dataset is ds and len(index) == N
    assert index.mu.shape == (N, model.d_z) and index.mu.dtype == torch.float32 and index.mu.is_cuda
    want = torch.full((N, model.d_z), float("nan"), device=DEV)
    chunks = 0
    with torch.no_grad():
        for lo in range(0, N, BS):                                 # five chunks: 64, 64, 64, 64, 44
            hi = min(lo + BS, N)
            batch = ds.gather(torch.arange(lo, hi, device=DEV), T=int(ds.lengths[lo:hi].max()) + 2)
            z, _, _ = model.forward_encoder(batch, eps=torch.zeros(hi - lo, model.d_z, device=DEV))
            want[batch.rows] = z.float()
            chunks += 1
    assert chunks == 5 and torch.equal(index.mu, want) and torch.isfinite(index.mu).all()
    same = [r for r in range(N) if strings[r] in strings[:r]]      # equal strings: equal content, so a neighbour at distance ~0
    assert len(same) > 50


def test_encode_keeps_the_order_of_its_input_and_restores_the_mode(setup):
    model, strings, ds, index = setup
    rows = [5, 200, 17, 42, 299, 0, 121]
    seqs = sorted((model.string2tensor(strings[r]) for r in rows), key=lambda t: -t.numel())
    mu, logvar = model.encode(seqs)
    assert mu.shape == logvar.shape == (len(rows), model.d_z) and mu.dtype == logvar.dtype == torch.float32
    z, _, lv = model.forward_encoder(seqs, eps=torch.zeros(len(rows), model.d_z, device=DEV))
    assert torch.equal(mu, z.float()) and torch.equal(logvar, lv.float()) and not mu.requires_grad
    batch = ds.gather(rows)                                         # a PaddedBatch: rows in the collate's order
    mu_b, _ = model.encode(batch)
    by_row = {int(r): mu_b[i] for i, r in enumerate(batch.rows.tolist())}
    for i, s in enumerate(seqs):                                    # the same molecule gives the same row wherever it stands
        r = next(r for r in rows if model.string2tensor(strings[r]).equal(s))
        assert torch.allclose(by_row[r], mu[i], rtol=1e-2, atol=1e-2)
    model.train()
    try:
        mu_t, _ = model.encode(seqs)
        assert model.training and torch.equal(mu_t, mu)             # eval mode for the call, the flag restored
    finally:
        model.eval()


def test_search_is_latent_knn_on_the_table(setup):
    model, strings, ds, index = setup
    z = torch.from_numpy(np.random.RandomState(1).standard_normal((70, model.d_z)).astype(np.float32)).to(DEV) * 0.1
    dist, rows = index.search(z, 8)
    d2, r2 = ops.latent_knn(z, index.mu, 8)
    assert torch.equal(dist, d2) and torch.equal(rows, r2)
    KR.check(dist.cpu().numpy(), rows.cpu().numpy(), z.cpu().numpy(), index.mu.cpu().numpy(), 8)
    ex = rows[:, 0].clone()
    dist_e, rows_e = index.search(z, 8, exclude=ex)
    assert not (rows_e == ex[:, None]).any() and torch.equal(rows_e[:, :7], rows[:, 1:])


def test_neighbors_encodes_then_searches(setup):
    model, strings, ds, index = setup
    queries = sorted(set(strings[::7]) | {"CCO", "c1ccccc1", "N" * 20}, key=lambda s: -len(s))     # corpus rows and strangers
    k = 5
    dist, rows = index.neighbors(queries, k, model)
    mu = model.encode([model.string2tensor(s) for s in queries])[0]
    d2, r2 = index.search(mu, k)
    assert torch.equal(dist, d2) and torch.equal(rows, r2)
    shuffled = queries[::-1]                                        # any order goes in; the answers follow it
    dist_s, rows_s = index.neighbors(shuffled, k, model)
    assert torch.equal(rows_s, rows.flip(0)) and torch.allclose(dist_s, dist.flip(0), rtol=1e-3, atol=1e-6)
    batch = ds.gather([3, 9, 250])
    dist_b, rows_b = index.neighbors(batch, k, model)
    d3, r3 = index.search(model.encode(batch)[0], k)
    assert torch.equal(dist_b, d3) and torch.equal(rows_b, r3)


def test_exclude_self_keeps_a_corpus_query_from_answering_with_itself(setup):
    model, strings, ds, index = setup
    queries = sorted(set(strings[::5]) | {"CCOCC", "S" * 9}, key=lambda s: -len(s))
    found = ds.lookup(queries)
    assert (found >= 0).sum() >= 30 and (found < 0).sum() == 2
    k = 4
    dist, rows = index.neighbors(queries, k, model, exclude_self=True)
    assert not (rows == found[:, None])[found >= 0].any()
    plain_d, plain_r = index.neighbors(queries, k, model)
    stranger = (found < 0).nonzero().view(-1)
    assert torch.equal(rows[stranger], plain_r[stranger]) and torch.equal(dist[stranger], plain_d[stranger])
    ids = [model.string2tensor(s) for s in queries]                 # id tensors are looked up as the strings are
    dist_i, rows_i = index.neighbors(ids, k, model, exclude_self=True)
    assert torch.equal(rows_i, rows) and torch.equal(dist_i, dist)


def test_smiles_returns_the_corpus_strings(setup):
    model, strings, ds, index = setup
    rows = [0, 299, 7, 7, 150, 3]
    assert ds.smiles(rows) == [strings[r] for r in rows]
    assert ds.smiles(torch.tensor(rows, device=DEV).view(2, 3)) == [strings[r] for r in rows]
    _, near = index.search(index.mu[:4], 3)
    assert ds.smiles(near) == [strings[r] for r in near.view(-1).tolist()]
    assert ds.smiles(torch.tensor([-1, 2], device=DEV)) == [None, strings[2]]
    with pytest.raises(ValueError, match="outside"):
        ds.smiles([N])


def test_value_errors_come_before_any_device_work(setup):
    model, strings, ds, index = setup
    torch.manual_seed(0)
    cpu_model = MV.VAE(model.vocabulary, dtype=torch.float32)
    foreign = MV.VAE(VC.OneHotVocab(set(ALPHABET[:-1])), dtype=torch.bfloat16).to(DEV)
    for bad, what in ((cpu_model, "lives on"), (foreign, "another vocabulary")):
        with pytest.raises(ValueError, match=what):
            ds.encode_latents(bad)
        with pytest.raises(ValueError, match=what):
            index.neighbors(["CCO"], 2, bad)
    with pytest.raises(ValueError, match="z must be"):
        index.search(torch.zeros(3, model.d_z + 1, device=DEV), 2)
