"""GPU tests of the Levenshtein surface of the MOSES pipeline -- MosesDeviceDataset.nearest_strings, mosesvae.VAE.edit_distance,
moses_reconstruction(edit_distance=True) and moses_generate(nearest=True) -- against tests/edit_ref.py on a synthetic SMILES corpus of about
300 rows and a small random model."""
import inspect

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import molecular_vae_amd as mv                                     # noqa: E402
from molecular_vae_amd import data as D, mosesvae as MV, ops, vocab as VC    # noqa: E402
import edit_ref as ER                                              # noqa: E402

DEV = torch.device("cuda")


@pytest.fixture(scope="module")
def setup():
    smiles = D.synthetic_smiles(300, seed=3, lo=8, hi=40)
    smiles[7] = smiles[2]                                           # an exact duplicate: the lower row answers
    vocab = VC.OneHotVocab.from_data(smiles)
    torch.manual_seed(5)
    model = MV.VAE(vocab, dtype=torch.float32).to(DEV).eval()
    return smiles, vocab, D.MosesDeviceDataset(smiles, vocab, device=DEV), model


def _ids(vocab, s):
    return np.array(vocab.string2ids(s), np.int64)


def _ref(vocab, queries, corpus, k, exclude=None):
    return ER.knn([_ids(vocab, s) for s in queries], [_ids(vocab, s) for s in corpus], k, exclude, V=len(vocab))


def test_nearest_strings_takes_strings_id_tensors_and_padded_ids(setup):
    smiles, vocab, ds, model = setup
    rs = np.random.RandomState(1)
    chars = sorted(set("".join(smiles)))
    queries = []
    for i in range(40):                                             # corpus strings with 0 to 3 character edits
        s = list(smiles[rs.randint(len(smiles))])
        for _ in range(i % 4):
            op, pos = rs.randint(3), rs.randint(len(s))
            if op == 0:
                s[pos] = chars[rs.randint(len(chars))]
            elif op == 1 and len(s) > 1:
                del s[pos]
            else:
                s.insert(pos, chars[rs.randint(len(chars))])
        queries.append("".join(s))
    queries += ["", "C"]
    k = 4
    ref_d, ref_j = _ref(vocab, queries, smiles, k)
    dist, rows = ds.nearest_strings(queries, k=k)
    assert dist.dtype == torch.int32 and rows.dtype == torch.long and dist.is_cuda and tuple(dist.shape) == (len(queries), k)
    assert np.array_equal(dist.cpu().numpy(), ref_d) and np.array_equal(rows.cpu().numpy(), ref_j)
    tensors = [torch.tensor(vocab.string2ids(s, add_bos=True, add_eos=True)) for s in queries]
    d2, r2 = ds.nearest_strings(tensors, k=k)
    padded = torch.nn.utils.rnn.pad_sequence(tensors, batch_first=True, padding_value=vocab.pad)
    d3, r3 = ds.nearest_strings(padded.to(DEV), k=k)
    assert torch.equal(dist, d2) and torch.equal(rows, r2) and torch.equal(dist, d3) and torch.equal(rows, r3)
    assert ds.smiles(rows[:3, 0]) == [smiles[j] for j in ref_j[:3, 0]]
    # the corpus against itself: distance 0 at lookup's row; without itself, the next one
    d0, r0 = ds.nearest_strings(smiles)
    look = ds.lookup(smiles)
    assert tuple(d0.shape) == (300, 1) and (d0 == 0).all() and torch.equal(r0[:, 0], look) and look[7] == 2
    d1, r1 = ds.nearest_strings(smiles, k=2, exclude_self=True)
    want = _ref(vocab, smiles, smiles, 2, exclude=look.cpu().numpy())
    assert np.array_equal(d1.cpu().numpy(), want[0]) and np.array_equal(r1.cpu().numpy(), want[1])
    assert not (r1 == look[:, None]).any() and d1[2, 0] == 0 and r1[2, 0] == 7
    for bad in (0, 33):
        with pytest.raises(ValueError, match="k must be"):
            ds.nearest_strings(queries, k=bad)
    with pytest.raises(ValueError, match="columns"):
        ds.nearest_strings(["C" * 128])


def test_vae_edit_distance_matches_the_reference(setup):
    smiles, vocab, ds, model = setup
    xs, ys = smiles[:60], smiles[30:90]
    ref = np.array([ER.lev(_ids(vocab, a), _ids(vocab, b), len(vocab)) for a, b in zip(xs, ys)], np.int32)
    got = model.edit_distance(xs, ys)
    assert got.dtype == torch.int32 and got.is_cuda and np.array_equal(got.cpu().numpy(), ref) and (ref[30:] > 0).any() and ref.max() > 5
    tx = [model.string2tensor(s) for s in xs]
    ty = torch.nn.utils.rnn.pad_sequence([model.string2tensor(s) for s in ys], batch_first=True, padding_value=vocab.pad)
    assert torch.equal(model.edit_distance(tx, ty), got) and torch.equal(model.edit_distance(ty, xs), got)
    assert (model.edit_distance(xs, xs) == 0).all()
    with pytest.raises(ValueError, match="rows against"):
        model.edit_distance(xs, ys[:5])


def test_moses_reconstruction_reports_the_mean_edit_distance(setup):
    smiles, vocab, ds, model = setup
    assert inspect.signature(mv.moses_reconstruction).parameters["edit_distance"].default is False
    order = sorted(range(64), key=lambda i: -len(smiles[i]))
    batches = [[model.string2tensor(smiles[i]) for i in order[:40]], [model.string2tensor(smiles[i]) for i in order[40:]]]
    plain = mv.moses_reconstruction(model, batches, max_len=50)
    full = mv.moses_reconstruction(model, batches, max_len=50, edit_distance=True)
    assert len(plain) == 2 and len(full) == 3 and full[:2] == plain
    dists = []
    for batch in batches:
        mu = model.encode(batch)[0]
        hyps = model.decode(mu, max_len=50, return_tokens=True)[0]
        for x, h in zip(batch, hyps):
            best = h[0] if isinstance(h, (list, tuple)) else h
            dists.append(ER.lev(ER.content(best.cpu().numpy(), vocab.eos), ER.content(x.cpu().numpy(), vocab.eos), len(vocab)))
    assert full[2] == sum(dists) / len(dists) and full[2] > 0
    assert plain[0] == sum(d == 0 for d in dists) / len(dists)
    padded = [ds.gather(order[:40]), ds.gather(order[40:])]                              # PaddedBatches: the same figures
    assert mv.moses_reconstruction(model, padded, max_len=50, edit_distance=True) == pytest.approx(full, rel=1e-5)


def test_moses_generate_reports_the_nearest_corpus_row(setup):
    smiles, vocab, ds, model = setup
    assert inspect.signature(mv.moses_generate).parameters["nearest"].default is False
    n, kw = 200, dict(batch_size=96, max_len=24, top_k=3, seed=2, syntax=True)             # batches of 96, 96 and 8
    z = torch.from_numpy(np.random.RandomState(4).standard_normal((n, model.d_z)).astype(np.float32)).to(DEV)
    first = mv.moses_generate(model, n, z=z, **kw)
    corpus = smiles[:100] + first["strings"][::3] + first["strings"][::6]                  # some samples are corpus rows, some of them twice
    d = D.MosesDeviceDataset(corpus, vocab, device=DEV)
    base = mv.moses_generate(model, n, z=z, novel_against=d, **kw)
    res = mv.moses_generate(model, n, z=z, novel_against=d, nearest=True, **kw)
    assert set(res) - set(base) == {"nearest_row", "nearest_dist"} and {k_: res[k_] for k_ in base} == base
    S = res["strings"]
    assert len(res["nearest_row"]) == len(res["nearest_dist"]) == len(S) > 10
    ref_d, ref_j = _ref(vocab, S, corpus, 1)
    assert res["nearest_dist"] == ref_d[:, 0].tolist() and res["nearest_row"] == ref_j[:, 0].tolist()
    zero = [dd == 0 for dd in res["nearest_dist"]]
    assert zero == [r >= 0 for r in res["corpus_row"]] and any(zero) and not all(zero)
    assert all(nr == cr for nr, cr, z0 in zip(res["nearest_row"], res["corpus_row"], zero) if z0)
    with pytest.raises(ValueError, match="needs novel_against"):
        mv.moses_generate(model, n, z=z, nearest=True, **kw)
