"""GPU tests of the device-resident MOSES feed: mvae_moses_collate against the integer reference tests/collate_ref.py (torch.equal
everywhere) at the wave and block edges of its rank count and row writes, its in-kernel guards, and data.MosesDeviceDataset against the
DataLoader + ShardedSampler + get_padded_collate_fn feed it replaces."""
import numpy as np
import pytest
import torch

import molecular_vae_amd as mv
from molecular_vae_amd import data as D, mosesvae as MV, vocab as VC, ops
import collate_ref as CR

pytestmark = pytest.mark.gpu
BOS, EOS, PAD, CANARY = 250, 251, 252, -77
DEV = "cuda"

# one corpus for every kernel case: 40 rows with lengths from {0, 1, 7, 57} (many ties), ids 0 .. 199
_rs = np.random.RandomState(7)
SEQS = [_rs.randint(0, 200, size=int(n)).tolist() for n in _rs.choice([0, 1, 7, 57], size=40)]
SEQS[3], SEQS[4] = [5] * 57, [6] * 57                              # two longest rows that differ only in content
N = len(SEQS)


@pytest.fixture(scope="module")
def corpus():
    tokens, offsets = CR.corpus(SEQS)
    return torch.from_numpy(np.concatenate([tokens, np.zeros(1, np.uint8)])).to(DEV), torch.from_numpy(offsets).to(DEV)


def run(corpus, rows, T, x_ld=None, n=N, fill=CANARY, extra_rows=0):
    """-> (backing buffer [B + extra_rows, x_ld] int64 pre-filled with `fill`, lengths, rows_sorted, err) on the host."""
    B, x_ld = len(rows), T if x_ld is None else x_ld
    backing = torch.full((B + extra_rows, x_ld), fill, dtype=torch.long, device=DEV)
    lengths = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    rows_sorted = torch.full((B,), -1, dtype=torch.long, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.moses_collate(corpus[0], corpus[1], torch.tensor(rows, dtype=torch.long, device=DEV), backing, lengths, T, n, BOS, EOS, PAD, rows_sorted, err)
    torch.cuda.synchronize()
    return backing.cpu(), lengths.cpu(), rows_sorted.cpu(), int(err.item())


def rows_for(B):
    if B == 1:
        return [3]
    if B == 2:
        return [4, 3]                                               # equal lengths, different content: the tie keeps batch order
    return np.random.RandomState(B).randint(0, N, size=B).tolist()   # permuted, with repeats (B > N)


@pytest.mark.parametrize("B", [1, 2, 64, 65, 130])
@pytest.mark.parametrize("slack", [0, 5])
def test_collate_equals_the_reference(corpus, B, slack):
    rows = rows_for(B)
    T = max(len(SEQS[r]) for r in rows) + 2 + slack
    x, lengths, order = CR.collate([SEQS[r] for r in rows], BOS, EOS, PAD, T=T)
    got_x, got_len, got_rows, err = run(corpus, rows, T, x_ld=T + 3)
    assert err == 0
    assert torch.equal(got_x[:, :T], torch.from_numpy(x))
    assert torch.equal(got_len, torch.from_numpy(lengths))
    assert got_rows.tolist() == [rows[i] for i in order]
    assert bool((got_x[:, T:] == CANARY).all())                       # x_ld > T: the columns beyond T are not touched
    if B == 2:
        assert got_rows.tolist() == [4, 3] and got_x[0, 1] == 6 and got_x[1, 1] == 5
    if B >= 64:
        assert len(set(rows)) < B                                      # repeats
        # rows_sorted maps back: collating it again reproduces the batch (already sorted: the stable order is the identity)
        again_x, again_len, again_rows, _ = run(corpus, got_rows.tolist(), T)
        assert torch.equal(again_x, got_x[:, :T]) and torch.equal(again_len, got_len) and torch.equal(again_rows, got_rows)


def test_a_row_that_does_not_fit_is_cut_and_flagged(corpus):
    rows = [7, 3, 9, 4, 11]                                            # rows 3 and 4 hold 57 tokens
    T = 57 + 2 - 1
    x, lengths, order = CR.collate([SEQS[r] for r in rows], BOS, EOS, PAD, T=T)
    got_x, got_len, got_rows, err = run(corpus, rows, T, x_ld=T + 8, extra_rows=3)
    assert err == 1
    assert torch.equal(got_x[:5, :T], torch.from_numpy(x)) and torch.equal(got_len, torch.from_numpy(lengths)) and int(got_len.max()) == T
    assert got_rows.tolist() == [rows[i] for i in order]
    assert bool((got_x[:5, T:] == CANARY).all()) and bool((got_x[5:] == CANARY).all())    # nothing outside [:B, :T] of the backing buffer


def test_a_row_id_outside_the_corpus_is_an_empty_row_and_flagged(corpus):
    rows = [7, N, 3]
    T = 59
    seqs = [SEQS[7], [], SEQS[3]]
    x, lengths, order = CR.collate(seqs, BOS, EOS, PAD, T=T)
    got_x, got_len, got_rows, err = run(corpus, rows, T, x_ld=T + 8, extra_rows=3)
    assert err == 2
    assert torch.equal(got_x[:3, :T], torch.from_numpy(x)) and torch.equal(got_len, torch.from_numpy(lengths))
    assert got_rows.tolist() == [rows[i] for i in order]
    assert bool((got_x[:3, T:] == CANARY).all()) and bool((got_x[3:] == CANARY).all())


# ------------------------------------------------------------------------------------------------ MosesDeviceDataset
@pytest.fixture(scope="module")
def small_corpus():
    rs = np.random.RandomState(5)
    smiles = ["".join(rs.choice(list("abc"), size=int(n))) for n in rs.choice([0, 1, 2, 5, 9, 9, 14], size=300)]
    vocab = VC.OneHotVocab(list("abc"))
    return smiles, vocab, D.MosesDeviceDataset(smiles, vocab, device=DEV)


def test_dataset_epoch_equals_the_dataloader_feed(small_corpus):
    smiles, vocab, ds = small_corpus
    assert len(ds) == 300 and ds.lengths.dtype == np.int32 and ds.lengths.tolist() == list(map(len, smiles))
    for epoch in (0, 1):
        sampler = mv.ShardedSampler(300, rank=0, world=1, seed=2)
        sampler.set_epoch(epoch)
        loader = torch.utils.data.DataLoader(list(range(300)), batch_size=32, sampler=sampler, drop_last=True, collate_fn=list)
        collate = VC.get_padded_collate_fn(vocab)
        got = list(ds.batches(32, epoch=epoch, seed=2))
        want_rows = list(loader)
        assert len(got) == len(want_rows) == 9
        for b, rows in zip(got, want_rows):
            want = collate([smiles[i] for i in rows])
            assert b.x_pad.is_cuda and b.lengths.dtype == torch.int32
            assert torch.equal(b.x_pad.cpu(), want.x_pad) and torch.equal(b.lengths.cpu(), want.lengths)
            assert b.rows.tolist() == sorted(rows, key=lambda i: len(smiles[i]), reverse=True)      # the stable order, row by row
    ds.check_errors()


def test_dataset_gather_and_bucketed_epoch(small_corpus):
    smiles, vocab, ds = small_corpus
    b = ds.gather([5, 200, 5, 17])
    want = VC.get_padded_collate_fn(vocab)([smiles[i] for i in (5, 200, 5, 17)])
    assert torch.equal(b.x_pad.cpu(), want.x_pad) and torch.equal(b.lengths.cpu(), want.lengths)
    again = ds.gather(b.rows, T=b.x_pad.shape[1])                       # device rows: rows_sorted reproduces the batch
    assert torch.equal(again.x_pad, b.x_pad) and torch.equal(again.lengths, b.lengths) and torch.equal(again.rows, b.rows)
    wide = ds.gather(torch.tensor([5, 200]), T=30)
    assert wide.x_pad.shape == (2, 30) and bool((wide.x_pad[:, 16:] == vocab.pad).all())
    with pytest.raises(ValueError):
        ds.gather([300])
    with pytest.raises(ValueError):
        ds.gather([])
    with pytest.raises(ValueError):
        ds.gather([1], T=1)
    with pytest.raises(ValueError):
        next(ds.batches(0))
    with pytest.raises(ValueError):
        next(ds.batches(8, world=2, drop_last=False))
    ds.check_errors()
    seen = []
    for epoch in (0, 1):
        batches = list(ds.batches(16, epoch=epoch, seed=1, bucket=8))
        rows = torch.cat([b.rows for b in batches]).tolist()
        assert len(batches) == 300 // 16 and len(rows) == len(set(rows)) and all(0 <= r < 300 for r in rows)
        for b in batches:
            lens = b.lengths.tolist()
            assert lens == sorted(lens, reverse=True) and b.x_pad.shape[1] == lens[0]
            assert lens == [len(smiles[r]) + 2 for r in b.rows.tolist()]
        seen.append(rows)
    assert seen[0] != seen[1]
    ds.check_errors()
    ds.gather(torch.tensor([5, int(np.argmax(ds.lengths))], device=DEV), T=3)     # a T too small from device rows: flagged, not a fault
    with pytest.raises(RuntimeError, match="cut"):
        ds.check_errors()
    ds.check_errors()                                                  # the flag was cleared


def test_two_epochs_of_training_from_the_device_feed(small_corpus):
    smiles, vocab, ds = small_corpus
    torch.manual_seed(0)
    model = MV.VAE(vocab, dtype=torch.float32).to(DEV)
    opt = mv.FusedAdam(model.parameters(), lr=3e-4, max_grad_norm=50.0)
    for epoch in range(2):
        post = mv.moses_train_epoch(model, epoch, ds.batches(32, epoch=epoch, bucket=4 * epoch), 0.1, opt)
        assert post["mode"] == "Train"
        for k in ("loss", "kl_loss", "recon_loss"):
            assert np.isfinite(post[k]), (k, post)
    ds.check_errors()
