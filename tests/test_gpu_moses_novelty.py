"""GPU tests of the corpus index (mvae_corpus_index_build / mvae_corpus_index_probe, MosesDeviceDataset.lookup / contains / n_distinct,
moses_generate(novel_against=)) against tests/novelty_ref.py, a Python dict from a row's content to the lowest row that holds it.  The
index is integer logic and exact, so every comparison is torch.equal / ==: ties, duplicates inside one wave and across waves and blocks,
prefixes, the cut at <eos>, ids that are no uint8, tables that are all but full, and the generation pipeline end to end."""
import inspect

import numpy as np
import pytest
import torch

import molecular_vae_amd as mv
from molecular_vae_amd import data as D, mosesvae as MV, vocab as VC, ops
import novelty_ref as NR

pytestmark = pytest.mark.gpu
DEV = "cuda"
VOCAB = VC.CharVocab([chr(c) for c in range(10, 256)])                 # 246 characters = ids 0 .. 245, then bos, eos, pad, unk: 250 ids
BOS, EOS, PAD = VOCAB.bos, VOCAB.eos, VOCAB.pad
CANARY = 7                                                             # behind column T: a legal token, so reading it would change a content


def _edge_corpus():
    """140 rows over ids 0 .. 199 with lengths from {0, 1, 2, 7, 57}: empty rows, one 7-token content at every odd row (70 copies: the
    equal-content race inside a wave and across the block's waves), two 57-token rows that differ in the last token only, a 1-token row
    that is a prefix of a 2-token row that is a prefix of a 7-token row that is a prefix of a 57-token row, and ties of every length."""
    rs = np.random.RandomState(7)
    seqs = [rs.randint(0, 200, size=int(n)).tolist() for n in rs.choice([0, 1, 2, 7, 57], size=140)]
    often = rs.randint(0, 200, size=7).tolist()
    for r in range(1, 140, 2):
        seqs[r] = list(often)
    long = rs.randint(0, 200, size=57).tolist()
    seqs[10], seqs[96] = list(long), long[:56] + [(long[56] + 1) % 200]
    seqs[20], seqs[22], seqs[24] = long[:7], long[:2], long[:1]
    seqs[4], seqs[70], seqs[138] = [], [], []
    seqs[8] = rs.randint(0, 200, size=2).tolist()
    seqs[44] = rs.randint(0, 200, size=7).tolist()
    seqs[30], seqs[6], seqs[100] = list(seqs[8]), list(seqs[44]), list(seqs[44])      # more repeats
    return seqs


SEQS = _edge_corpus()
N = len(SEQS)
TABLE = NR.index(SEQS)


def _csr(seqs):
    offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in seqs], out=offsets[1:])
    return np.array([t for s in seqs for t in s], dtype=np.uint8), offsets


@pytest.fixture(scope="module")
def ds():
    return D.MosesDeviceDataset(_csr(SEQS), VOCAB, device=DEV)


def _padded(rows, T=None, fill=None):
    T = max(len(r) for r in rows) if T is None else T
    return torch.tensor([list(r) + [PAD if fill is None else fill] * (T - len(r)) for r in rows], dtype=torch.long)


def test_the_edge_corpus_is_what_it_says():
    lens = [len(s) for s in SEQS]
    assert set(lens) == {0, 1, 2, 7, 57} and lens.count(0) >= 3
    assert sum(s == SEQS[1] for s in SEQS) == 70 > 64
    assert SEQS[10][:56] == SEQS[96][:56] and SEQS[10][56] != SEQS[96][56]
    assert NR.n_distinct(TABLE) < N - 69 and TABLE[tuple(SEQS[30])] == 8 and TABLE[tuple(SEQS[100])] == TABLE[tuple(SEQS[44])] == 6


def test_n_distinct_and_every_corpus_row(ds):
    assert ds._slots is None                                               # the constructor builds nothing
    assert ds.build_index() is ds and ds._slots.numel() == 512 and ds._slots.dtype == torch.long      # the smallest power of two >= 2 N
    table = ds._slots
    assert ds.build_index()._slots is table                                # idempotent
    assert ds.n_distinct == NR.n_distinct(TABLE) and ds.n_distinct == NR.n_distinct(TABLE)
    batch = ds.gather(list(range(N)))
    got = ds.lookup(batch.x_pad)
    want = [TABLE[tuple(SEQS[r])] for r in batch.rows.tolist()]
    assert got.dtype == torch.long and got.device.type == "cuda" and got.tolist() == want
    assert torch.equal(ds.contains(batch.x_pad), torch.ones(N, dtype=torch.bool, device=DEV))
    assert any(w != r for w, r in zip(want, batch.rows.tolist()))           # repeats answer with the LOWEST row, not with themselves


@pytest.mark.parametrize("B", [1, 2, 64, 65, 130])
def test_lookup_at_the_wave_and_block_edges_with_a_wider_row_stride(ds, B):
    rows = ((np.arange(B) * 37 + B) % N).tolist()
    batch = ds.gather(rows)
    T = batch.x_pad.shape[1]
    backing = torch.full((B + 2, T + 3), CANARY, dtype=torch.long, device=DEV)
    backing[:B, :T] = batch.x_pad
    got = ds.lookup(backing[:B, :T])                                       # x_ld = T + 3
    assert got.shape == (B,) and got.tolist() == [TABLE[tuple(SEQS[r])] for r in batch.rows.tolist()]
    assert got.tolist() == NR.lookup(TABLE, batch.x_pad.tolist(), EOS)


def test_misses_the_cut_and_ids_that_are_no_uint8(ds):
    base, long = SEQS[20], SEQS[10]                                         # 7 and 57 tokens, both in the corpus
    other = next(t for t in range(200) if t != base[3])
    rows = [
        [BOS] + base + [EOS],                                               # 0: the row itself
        [BOS] + base[:3] + [other] + base[4:] + [EOS],                      # 1: one token changed
        [BOS] + base[:6] + [EOS],                                           # 2: one token shorter
        [BOS] + base + [base[0], EOS],                                      # 3: one token longer
        [BOS] + base,                                                       # 4: no <eos>, padded below: the pads are content
        [BOS] + base[:3] + [base[3] + 256] + base[4:] + [EOS],              # 5: an id whose low byte is the corpus token
        [BOS] + base[:3] + [70000] + base[4:] + [EOS],                      # 6
        [BOS] + base[:3] + [-1] + base[4:] + [EOS],                         # 7
        [BOS, 256, EOS],                                                    # 8
        [BOS, EOS] + long,                                                  # 9: <eos> in column 1, a corpus row behind it: the empty content
        [BOS, EOS, 300, 70000, -5],                                         # 10: ... and ids that are no uint8 behind it
        [BOS] + base + [EOS] + long[:40],                                   # 11: a copy of corpus tokens behind the <eos>
        [BOS] + base + [EOS] + [256, 1 << 40, -1, 999],                     # 12
        [BOS] + long + [EOS],                                               # 13
        [BOS] + long[:56] + [EOS],                                          # 14: a strict prefix of a corpus row, itself absent
        [BOS] + long[:2] + [EOS],                                           # 15: a prefix that IS a corpus row
        [BOS] + long[:56] + [(long[56] + 2) % 200, EOS],                    # 16: differs from two corpus rows in the last token only
    ]
    x = _padded(rows)
    want = NR.lookup(TABLE, x.tolist(), EOS)
    empty = TABLE[()]
    assert want == [20, -1, -1, -1, -1, -1, -1, -1, -1, empty, empty, 20, 20, 10, -1, 22, -1] and empty == min(r for r in range(N) if not SEQS[r])
    got = ds.lookup(x.to(DEV))
    assert got.tolist() == want
    assert ds.contains(x.to(DEV)).tolist() == [w >= 0 for w in want]
    # garbage behind the <eos> changes nothing: the same rows padded with ids >= 256 instead of <pad>
    assert ds.lookup(_padded(rows, fill=300).to(DEV)).tolist() == want
    # T = 1: the empty content
    assert ds.lookup(torch.full((3, 1), BOS, dtype=torch.long, device=DEV)).tolist() == [empty] * 3
    # a sample cut at T, compared by the tokens it has: no <eos>, and behind column T a token and an <eos> that must not be reached
    backing = torch.tensor([[BOS] + base + [base[0], EOS, EOS, EOS], [BOS] + base[:6] + [EOS] + [base[0], EOS, EOS, EOS]], device=DEV)
    assert ds.lookup(backing[:, :8]).tolist() == [20, -1]
    assert ds.lookup(backing[:, :3]).tolist() == [22, 22]                   # cut to two tokens
    assert ds.lookup(backing[:, :2]).tolist() == [24, 24]


def _raw(seqs, n_slots, queries, slots=None):
    """The raw entries on a table of n_slots -> (match list, n_distinct, slots).  A fresh table starts as garbage: build must clear it."""
    tokens, offsets = _csr(seqs)
    tokens = torch.from_numpy(np.concatenate([tokens, np.zeros(1, np.uint8)])).to(DEV)
    offsets = torch.from_numpy(offsets).to(DEV)
    if slots is None:
        slots = torch.randint(-(1 << 62), 1 << 62, (n_slots,), dtype=torch.long, device=DEV)
    nd = torch.full((1,), -5, dtype=torch.long, device=DEV)
    ops.corpus_index_build(tokens, offsets, len(seqs), slots, nd)
    x = queries.to(DEV)
    match = torch.full((x.shape[0],), -9, dtype=torch.long, device=DEV)
    ops.corpus_index_probe(tokens, offsets, len(seqs), slots, x, EOS, match)
    torch.cuda.synchronize()
    return match.tolist(), int(nd.item()), slots


def _distinct_rows(n, seed):
    rs = np.random.RandomState(seed)
    seen, out = {()}, [[]]
    while len(out) < n:
        s = tuple(rs.randint(0, 200, size=int(rs.randint(1, 4))).tolist())
        if s not in seen:
            seen.add(s); out.append(list(s))
    order = rs.permutation(n)
    return [out[i] for i in order]


@pytest.mark.parametrize("n", [1, 3, 255])
def test_crowded_tables(n):
    """n distinct rows in the smallest legal table, n + 1 slots for these n: one empty slot, chains that run the length of the table and
    wrap past its last slot."""
    seqs = _distinct_rows(n, seed=n)
    n_slots = n + 1
    assert n_slots & (n_slots - 1) == 0
    misses = [[199, 199, 199, 199], [0], [1, 2, 3, 4, 5]] + [s + [s[0]] for s in seqs if s][:20]
    queries = _padded([[BOS] + s + [EOS] for s in seqs + misses])
    table = NR.index(seqs)
    want = NR.lookup(table, queries.tolist(), EOS)
    assert want[:n] == list(range(n)) and -1 in want
    got, nd, slots = _raw(seqs, n_slots, queries)
    assert got == want and nd == n
    again, nd2, _ = _raw(seqs, n_slots, queries, slots=slots)               # once more into the table as it stands
    assert again == want and nd2 == n


def test_two_builds_agree_with_duplicates_across_blocks():
    rs = np.random.RandomState(3)
    pool = [rs.randint(0, 200, size=int(k)).tolist() for k in rs.choice([0, 1, 2, 7, 57], size=40)]
    seqs = [pool[i] for i in rs.randint(0, 40, size=1000)]                  # four blocks of 256 rows, every content ~25 times
    table = NR.index(seqs)
    absent = [[BOS] + s + [7, EOS] for s in pool[:10]]
    queries = _padded([[BOS] + s + [EOS] for s in seqs[::3]] + absent)
    want = NR.lookup(table, queries.tolist(), EOS)
    a, nd_a, _ = _raw(seqs, 2048, queries)
    b, nd_b, _ = _raw(seqs, 1024, queries)                                   # another table size: other homes, other chains, the same answers
    assert a == want and b == want and nd_a == nd_b == NR.n_distinct(table)
    assert want[:len(seqs[::3])] != list(range(0, 1000, 3)) and -1 in want    # a hit names the lowest of a content's ~25 rows, not the row asked


def test_lookup_of_strings_and_of_id_tensors():
    strings = ["CCO", "", "c1ccccc1", "C?l", "N", "", "CC(=O)Oc1ccccc1C(=O)O", "CCO", "N"]
    vocab = VC.OneHotVocab.from_data([s.replace("?", "") for s in strings])   # '?' is unknown: <unk> in the corpus and in the query
    d = D.MosesDeviceDataset(strings, vocab, device=DEV)
    table = NR.index([vocab.string2ids(s) for s in strings])
    assert d.n_distinct == len(set(strings)) == 6
    batch = d.gather(list(range(len(strings))))
    by_string = d.lookup(strings)
    assert by_string.tolist() == [0, 1, 2, 3, 4, 1, 6, 0, 4]
    assert torch.equal(by_string[batch.rows], d.lookup(batch.x_pad))
    queries = ["CCO", "CC", "CCOC", "C!l", "C?", "", "c1ccccc1", "N", "O", "€"]          # '!' is <unk> too; the last one is no latin-1
    want = [table.get(tuple(vocab.string2ids(s)), -1) for s in queries]
    assert want == [0, -1, -1, 3, -1, 1, 2, 4, -1, -1]
    assert d.lookup(queries).tolist() == want and d.lookup(queries[:-1]).tolist() == want[:-1]
    tensors = [torch.tensor(vocab.string2ids(s, add_bos=True, add_eos=True)) for s in queries]
    assert d.lookup(tensors).tolist() == want
    assert d.contains(queries).tolist() == [w >= 0 for w in want]


# ---------------------------------------------------------------------------------------------- moses_generate
ALPHABET = "CNOSFcnos()=#123[]@H+-lBr"


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(11)
    return MV.VAE(VC.OneHotVocab(set(ALPHABET)), dtype=torch.bfloat16).to(DEV).eval()


def _latents(n, dz, seed):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal((n, dz)).astype(np.float32)).to(DEV)


def test_moses_generate_counts_novel_samples(model):
    v = model.vocabulary
    n, kw = 300, dict(batch_size=128, max_len=10, top_k=2, seed=5, syntax=True)            # batches of 128, 128 and 44
    z = _latents(n, model.d_z, seed=2)
    plain = mv.moses_generate(model, n, z=z, **kw)
    S = plain["strings"]
    assert 4 < plain["unique"] < n and len(set(S)) == len(S)                                # duplicates occurred; constrained rows end in <eos>
    never = ["C" * 30, "N" * 31, "c1ccccc1" * 4]
    corpus = never + S[::2] + S[::4]                                                        # every second sample, some of them twice
    assert not set(never) & set(S)
    d = D.MosesDeviceDataset(corpus, v, device=DEV)
    table = NR.index([v.string2ids(s) for s in corpus])
    res = mv.moses_generate(model, n, z=z, novel_against=d, **kw)
    assert {k: res[k] for k in plain} == plain                                              # strings, counts, unique, logq, total: unchanged
    assert set(res) - set(plain) == {"novel", "is_novel", "corpus_row"}
    assert res["is_novel"] == [s not in set(corpus) for s in S]
    assert res["corpus_row"] == [table.get(tuple(v.string2ids(s)), -1) for s in S]
    assert all(3 <= r < 3 + len(S[::2]) for r in res["corpus_row"] if r >= 0)               # the lowest row, not the repeat further on
    assert res["novel"] == sum(res["is_novel"]) == len(S) - len(S[::2]) > 0
    both = mv.moses_generate(model, n, z=z, novel_against=d, count_valid=True, **kw)
    assert {k: both[k] for k in res} == res
    assert set(both) - set(res) == {"valid", "valid_unique", "valid_unique_novel"}
    assert both["valid_unique_novel"] == both["novel"] and both["valid"] == n and both["valid_unique"] == both["unique"]


def test_moses_generate_without_novel_against_is_what_it_was(model):
    assert inspect.signature(mv.moses_generate).parameters["novel_against"].default is None
    z = _latents(150, model.d_z, seed=4)
    plain = mv.moses_generate(model, 150, batch_size=64, max_len=10, top_k=3, seed=1, z=z)
    assert set(plain) == {"total", "unique", "strings", "counts", "logq"}
    valid = mv.moses_generate(model, 150, batch_size=64, max_len=10, top_k=3, seed=1, z=z, count_valid=True, novel_against=None)
    assert set(valid) == set(plain) | {"valid", "valid_unique"} and {k: valid[k] for k in plain} == plain
    # unconstrained samples: rows cut at max_len and specials inside a content are looked up like any other row
    d = D.MosesDeviceDataset(plain["strings"][::2] + ["C"], model.vocabulary, device=DEV)
    res = mv.moses_generate(model, 150, batch_size=64, max_len=10, top_k=3, seed=1, z=z, novel_against=d)
    assert {k: res[k] for k in plain} == plain and res["novel"] == sum(res["is_novel"]) == sum(r < 0 for r in res["corpus_row"])
