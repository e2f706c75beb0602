"""CPU tests of the device-resident MOSES feed (data.MosesDeviceDataset): mvae_moses_collate is declared, bound and exported at ABI 12 and
refuses bad arguments before anything is launched; tokenize_corpus equals vocab.string2ids; the epoch plan (data.moses_epoch_plan, host
only) equals the DataLoader + ShardedSampler feed with bucket=0 and is a balanced, reproducible, shorter-T cover with bucket=8; and the
integer reference tests/collate_ref.py is itself pinned to vocab.get_padded_collate_fn."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import molecular_vae_amd as mv
from molecular_vae_amd import _lib as L, data as D, vocab as VC, ops
import collate_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvae.h")).read(), flags=re.S)
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", header).group(1)) == 12 == L.ABI_VERSION
    lib = L.load()
    assert lib.mvae_abi_version() == 12
    assert re.search(r"\bmvae_moses_collate\s*\(", header)
    assert "mvae_moses_collate" in L.SIGNATURES and hasattr(lib, "mvae_moses_collate")
    assert len(L.SIGNATURES["mvae_moses_collate"][1]) == 15
    assert callable(ops.moses_collate)
    for name in ("MosesDeviceDataset", "tokenize_corpus", "moses_epoch_plan"):
        assert name in mv.__all__ and getattr(mv, name) is getattr(D, name)


def test_entry_point_refuses_bad_arguments_before_launching():
    """Everything below returns before any HIP call (no device needed)."""
    lib = L.load()
    fake = ctypes.c_void_p(256)                                  # never dereferenced: every call below is refused first

    def call(tokens=fake, offsets=fake, rows=fake, B=4, T=9, N=10, bos=3, eos=4, pad=5, x_pad=fake, x_ld=9, lengths=fake, rows_sorted=None,
             err=None):
        return lib.mvae_moses_collate(tokens, offsets, rows, B, T, N, bos, eos, pad, x_pad, x_ld, lengths, rows_sorted, err, None)
    for bad in (dict(tokens=None), dict(offsets=None), dict(rows=None), dict(x_pad=None), dict(lengths=None), dict(B=0), dict(B=-1), dict(T=1),
                dict(T=0), dict(N=0), dict(x_ld=8), dict(bos=-1), dict(bos=65536), dict(eos=-1), dict(eos=65536), dict(pad=-1), dict(pad=65536),
                dict(rows_sorted=fake, err=fake, B=0)):
        assert call(**bad) == -1, bad


def test_padded_batch_carries_rows():
    b = VC.PaddedBatch(torch.zeros(2, 3, dtype=torch.long), torch.tensor([3, 2], dtype=torch.int32))
    assert b.rows is None and b.to("cpu").rows is None
    b = VC.PaddedBatch(b.x_pad, b.lengths, rows=torch.tensor([7, 5]))
    assert b.to("cpu").rows.tolist() == [7, 5]


# ------------------------------------------------------------------------------------------------ tokenize_corpus
def test_tokenize_corpus_equals_string2ids():
    smiles = ["CCO", "", "c1ccccc1", "C?l", "N", "", "CC(=O)Oc1ccccc1C(=O)O"]                 # empty strings, an unknown '?', longest last
    vocab = VC.OneHotVocab.from_data([s.replace("?", "") for s in smiles])
    assert "?" not in vocab.c2i
    tokens, offsets = D.tokenize_corpus(smiles, vocab)
    assert tokens.dtype == np.uint8 and offsets.dtype == np.int64 and offsets.shape == (len(smiles) + 1,) and offsets[0] == 0
    assert offsets[-1] == tokens.shape[0] == sum(map(len, smiles))
    for i, s in enumerate(smiles):
        assert tokens[offsets[i]:offsets[i + 1]].tolist() == vocab.string2ids(s), s
    assert tokens[offsets[3] + 1] == vocab.unk
    t0, o0 = D.tokenize_corpus([], vocab)
    assert t0.shape == (0,) and o0.tolist() == [0]
    t1, o1 = D.tokenize_corpus(["", ""], vocab)
    assert t1.shape == (0,) and o1.tolist() == [0, 0, 0]
    many = D.synthetic_smiles(200, seed=5, lo=0, hi=40, structured=False)
    v2 = VC.CharVocab.from_data(many)
    tk, of = D.tokenize_corpus(many, v2)
    assert all(tk[of[i]:of[i + 1]].tolist() == v2.string2ids(many[i]) for i in range(200))


def test_tokenize_corpus_value_errors():
    big = VC.CharVocab([chr(0x100 + i) for i in range(253)])                                   # 253 + 4 specials = 257 ids
    assert len(big) == 257
    with pytest.raises(ValueError, match="uint8"):
        D.tokenize_corpus(["a"], big)
    with pytest.raises(ValueError, match="vocabulary character"):
        D.tokenize_corpus(["a"], VC.CharVocab(["a", "€"]))
    with pytest.raises(ValueError, match="corpus character"):
        D.tokenize_corpus(["a", "b€"], VC.CharVocab(["a", "b"]))
    D.tokenize_corpus(["a\xe9"], VC.CharVocab(["a", "\xe9"]))                                  # latin-1 beyond ASCII is one byte: legal


# ------------------------------------------------------------------------------------------------ the epoch plan
def _loader_batches(n, B, rank, world, seed, epoch):
    sampler = mv.ShardedSampler(n, rank=rank, world=world, seed=seed)
    sampler.set_epoch(epoch)
    loader = torch.utils.data.DataLoader(list(range(n)), batch_size=B, sampler=sampler, drop_last=True, collate_fn=list)
    return [list(b) for b in loader]


def _plan_batches(lengths, B, **kw):
    order, cuts = D.moses_epoch_plan(lengths, B, **kw)
    assert order.dtype == np.int64
    for lo, hi, T in cuts:
        assert T == int(lengths[order[lo:hi]].max()) + 2                                        # every batch's planned T is its own maximum + 2
    return [order[lo:hi].tolist() for lo, hi, _ in cuts], [T for _, _, T in cuts]


@pytest.mark.parametrize("world", [1, 4])
def test_plan_without_bucketing_equals_the_dataloader_feed(world):
    n, B, seed = 1000, 32, 3
    lengths = CR.example_lengths(n, seed=1)
    for epoch in (0, 1):
        for rank in range(world):
            got, _ = _plan_batches(lengths, B, epoch=epoch, seed=seed, rank=rank, world=world)
            want = _loader_batches(n, B, rank, world, seed, epoch)
            assert got == want and len(got) == (n // world) // B
    got, _ = _plan_batches(lengths, B, shuffle=False, rank=world - 1, world=world)
    per = n // world
    assert got[0] == list(range((world - 1) * per, (world - 1) * per + B))
    if world == 1:
        got, Ts = _plan_batches(lengths, B, shuffle=False, drop_last=False)
        assert len(got) == 32 and len(got[-1]) == 1000 - 31 * 32 and sum(got, []) == list(range(n))


@pytest.mark.parametrize("world", [1, 4])
def test_bucketed_plan_is_a_balanced_reproducible_cover_with_smaller_T(world):
    n, B, k = 2048, 64, 8
    lengths = CR.example_lengths(n, seed=0)
    per_rank = [_plan_batches(lengths, B, epoch=2, seed=5, rank=r, world=world, bucket=k) for r in range(world)]
    counts = {len(b) for b, _ in per_rank}
    assert counts == {n // (B * world)}                                                       # every rank: the same batch count
    rows = [i for b, _ in per_rank for batch in b for i in batch]
    assert len(rows) == len(set(rows)) and all(0 <= i < n for i in rows)                       # ranks disjoint, no row twice
    assert n - len(rows) < B * world                                                          # at most one global step dropped
    assert all(len(batch) == B for b, _ in per_rank for batch in b)
    again = [_plan_batches(lengths, B, epoch=2, seed=5, rank=r, world=world, bucket=k) for r in range(world)]
    assert again == per_rank
    other = _plan_batches(lengths, B, epoch=3, seed=5, rank=0, world=world, bucket=k)
    assert other[0] != per_rank[0][0]
    flat = [_plan_batches(lengths, B, epoch=2, seed=5, rank=r, world=world) for r in range(world)]
    sum_bucket, sum_flat = sum(sum(T) for _, T in per_rank), sum(sum(T) for _, T in flat)
    assert sum_bucket < sum_flat, (sum_bucket, sum_flat)
    # the ranks' batches of one step hold neighbouring lengths: their T differ by less than the spread of T over the epoch
    if world > 1:
        Ts = np.array([T for _, T in per_rank])
        assert (Ts.max(0) - Ts.min(0)).max() < Ts.max() - Ts.min()
    # not monotone in time: the steps were shuffled
    T0 = per_rank[0][1]
    assert T0 != sorted(T0) and T0 != sorted(T0, reverse=True)


def test_bucketed_plan_keeps_a_short_last_batch_on_one_rank_and_drops_a_partial_step():
    lengths = CR.example_lengths(1000, seed=2)
    b, _ = _plan_batches(lengths, 64, bucket=4, drop_last=False)
    assert sorted(sum(b, [])) == list(range(1000)) and sorted(map(len, b))[0] == 1000 % 64
    b, _ = _plan_batches(lengths, 64, bucket=4)
    assert len(b) == 15 and len(set(sum(b, []))) == 15 * 64
    b, _ = _plan_batches(lengths[:10], 64, bucket=4)                                           # fewer rows than one batch: an empty epoch
    assert b == []


def test_plan_refuses_bad_arguments():
    lengths = CR.example_lengths(100)
    for bad in (dict(batch_size=0), dict(batch_size=-3), dict(batch_size=2.5), dict(world=0), dict(rank=1), dict(rank=-1), dict(rank=4, world=4),
                dict(bucket=-1), dict(bucket=1.5), dict(epoch=-1), dict(seed=-1), dict(drop_last=False, world=2)):
        kw = dict(batch_size=8)
        kw.update(bad)
        with pytest.raises(ValueError):
            D.moses_epoch_plan(lengths, **kw)


# ------------------------------------------------------------------------------------------------ the reference itself
def test_collate_ref_equals_get_padded_collate_fn():
    rs = np.random.RandomState(11)
    alphabet = list("CNO()=c1")
    vocab = VC.OneHotVocab(alphabet)
    collate = VC.get_padded_collate_fn(vocab)
    for B in (1, 2, 7, 33):
        strings = ["".join(rs.choice(alphabet, size=int(n))) for n in rs.choice([0, 1, 3, 3, 9], size=B)]
        want = collate(strings)
        x, lengths, order = CR.collate([vocab.string2ids(s) for s in strings], vocab.bos, vocab.eos, vocab.pad)
        assert torch.equal(torch.from_numpy(x), want.x_pad) and torch.equal(torch.from_numpy(lengths), want.lengths)
        assert [strings[i] for i in order] == sorted(strings, key=len, reverse=True)
    x, lengths, _ = CR.collate([[0, 1, 2], [3]], 9, 8, 7, T=6)                                   # a wider T: extra pad columns
    assert x.tolist() == [[9, 0, 1, 2, 8, 7], [9, 3, 8, 7, 7, 7]] and lengths.tolist() == [5, 3]
    x, lengths, _ = CR.collate([[0, 1, 2], [3]], 9, 8, 7, T=4)                                   # too small a T: the row is cut
    assert x.tolist() == [[9, 0, 1, 2], [9, 3, 8, 7]] and lengths.tolist() == [4, 3]
    tokens, offsets = CR.corpus([[1, 2], [], [3]])
    assert tokens.tolist() == [1, 2, 3] and offsets.tolist() == [0, 2, 2, 3]
