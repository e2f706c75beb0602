"""Integer reference of the MOSES collate (moses_train_distrib.py:127-135 + pad_sequence): batch members sorted by length, longest first,
stable (``sorted(data, key=len, reverse=True)``), each as <bos> + ids + <eos>, padded to T.  No floats anywhere: every comparison against
it is exact.  tests/test_moses_device_data_host.py pins it to ``vocab.get_padded_collate_fn``."""
import numpy as np


def stable_order(lengths):
    """order[r] = the batch member that lands in output row r."""
    return sorted(range(len(lengths)), key=lambda i: lengths[i], reverse=True)


def collate(seqs, bos, eos, pad, T=None):
    """seqs: the batch members' ids (without specials) in batch order -> (x_pad int64 [B, T], lengths int32 [B], order [B]).  T=None: the
    longest + 2.  A member with len + 2 > T is cut at T columns and reports length T (what mvae_moses_collate documents)."""
    seqs = [list(map(int, s)) for s in seqs]
    order = stable_order([len(s) for s in seqs])
    if T is None:
        T = max(len(s) for s in seqs) + 2
    x = np.full((len(seqs), T), pad, dtype=np.int64)
    lengths = np.zeros(len(seqs), dtype=np.int32)
    for r, i in enumerate(order):
        row = ([bos] + seqs[i] + [eos])[:T]
        x[r, :len(row)] = row
        lengths[r] = len(row)
    return x, lengths, np.asarray(order, dtype=np.int64)


def corpus(seqs):
    """ids per row -> the CSR pair (tokens uint8, offsets int64 [N + 1])."""
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=offsets[1:])
    tokens = np.array([t for s in seqs for t in s], dtype=np.uint8)
    return tokens, offsets


def example_lengths(n, seed=0):
    """The length distribution of examples/train_moses.py's synthetic corpus: N(38, 8) clipped to [10, 57], truncated to int."""
    return np.clip(np.random.RandomState(seed).normal(38, 8, size=n), 10, 57).astype(int)
