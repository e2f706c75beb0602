"""Input side of the training path: the ``(LongTensor[L], FloatTensor[L, C])`` contract of ``data_loader.MoleLoader``
(data_loader.py:26-31) without its per-item sklearn ``OneHotEncoder.fit_transform``, plus a device-resident variant.

  * ``build_vocab``     -- train.py:45-60 with a *sorted* character order (the reference iterates a ``set``, so its ids are not
                           reproducible across runs); ``' '`` is the padding character (``ljust``), as in the reference.
  * ``MoleLoader``      -- same constructor / ``__getitem__`` contract as the reference class (drop-in for ``DataLoader``).
  * ``encode_smiles``   -- whole-corpus vectorised encoding to uint8 ``[N, L]`` (120 B / molecule; 250k ZINC = 30 MB).
  * ``DeviceDataset``   -- the encoded corpus resident in HBM; per-epoch shuffled, rank-sharded batches expanded on device
                           (``mvae_expand_indices``) to the same ``(idx, ohe)`` pair -- no host work in the step.
  * ``tokenize_corpus`` -- the MOSES corpus as CSR (uint8 tokens without specials + int64 offsets) through a 256-entry byte table.
  * ``moses_epoch_plan`` / ``MosesDeviceDataset`` -- that corpus resident in HBM; every batch is ONE launch (``mvae_moses_collate``) that
                           yields the ``PaddedBatch`` ``mosesvae.VAE.forward`` takes: the stable length-descending collate of
                           ``vocab.get_padded_collate_fn`` without its per-string host work.  Opt-in length bucketing.
                           ``lookup`` / ``contains`` / ``n_distinct``: an exact hash index of the corpus rows on the device
                           (``mvae_corpus_index_build`` / ``_probe``), which ``train.moses_generate(novel_against=)`` counts novelty with.
                           ``encode_latents`` -> ``MosesLatentIndex``: the encoder mean of every corpus row in HBM and an exact k-NN
                           search over it (``mvae_latent_knn``); ``smiles`` reads corpus rows back as strings; ``nearest_strings``
                           is the exact k-NN by token-level Levenshtein distance over the same corpus (``mvae_edit_knn``).
                           ``batches(augment=True)`` respells every row on the device first (SMILES enumeration:
                           ``mvae_smiles_rewrite_corpus`` in front of the unchanged collate); ``randomized_smiles`` does it for strings.
                           ``canonical()`` is the corpus in canonical spelling (one ``mvae_smiles_canon_corpus`` launch), whose
                           ``lookup`` / ``n_distinct`` answer per graph; ``canonical_smiles`` does it for strings.
  * ``load_smiles`` / ``save_encoded`` / ``load_encoded`` -- ``.smi``/CSV in, ``.npz`` (indices + charset + max_len) out.
"""
import numpy as np
import torch


def build_vocab(smiles, max_len=None):
    """char -> id over every string shorter than max_len (train.py:47-54), plus ' '; sorted for reproducibility."""
    chars = set(" ")
    for s in smiles:
        if max_len is None or len(s) < max_len:
            chars.update(s)
    return {ch: i for i, ch in enumerate(sorted(chars))}


def encode_smiles(smiles, vocab, max_len):
    """uint8 [N, max_len]; strings are right-padded with ' ' (str.ljust, data_loader.py:27); unknown chars raise KeyError
    (as the reference's dict lookup does); longer strings raise ValueError."""
    if len(vocab) > 256:
        raise ValueError("vocabulary does not fit uint8")
    out = np.full((len(smiles), max_len), vocab[" "], dtype=np.uint8)
    for n, s in enumerate(smiles):
        if len(s) > max_len:
            raise ValueError(f"SMILES longer than max_len={max_len}: {s!r}")
        out[n, :len(s)] = [vocab[ch] for ch in s]
    return out


class MoleLoader(torch.utils.data.Dataset):
    """data_loader.py:7-31: ``df`` is anything indexable whose rows' first column is the SMILES string (a pandas DataFrame, as
    in the reference, or a plain list of strings)."""

    def __init__(self, df, vocab, max_len=70, num=None):
        super().__init__()
        self.df, self.vocab, self.max_len = df, vocab, max_len
        self._eye = np.eye(len(vocab), dtype=np.float32)

    def __len__(self):
        return self.df.shape[0] if hasattr(self.df, "shape") else len(self.df)

    def _smile(self, item):
        return str(self.df.iloc[item, 0]) if hasattr(self.df, "iloc") else str(self.df[item])

    def __getitem__(self, item):
        smile = self._smile(item).ljust(self.max_len, " ")
        embedding = np.array([self.vocab[ch] for ch in smile])
        return torch.LongTensor(embedding), torch.from_numpy(self._eye[embedding])


class DeviceDataset:
    """uint8 indices [N, L] in HBM; ``batches()`` yields (LongTensor[B,L], FloatTensor[B,L,C]) device tensors."""

    def __init__(self, indices_u8, n_classes, device="cuda"):
        self.store = torch.as_tensor(np.ascontiguousarray(indices_u8), dtype=torch.uint8).to(device)
        self.n, self.L = self.store.shape
        self.C = int(n_classes)
        self.device = self.store.device

    def __len__(self):
        return self.n

    def epoch_order(self, epoch=0, seed=0, shuffle=True, rank=0, world=1):
        """This rank's contiguous shard of the (optionally shuffled) epoch permutation, on device."""
        if shuffle:
            g = torch.Generator(); g.manual_seed(seed + epoch)
            perm = torch.randperm(self.n, generator=g)
        else:
            perm = torch.arange(self.n)
        per = self.n // world
        return perm[rank * per:(rank + 1) * per].to(self.device)

    def batches(self, batch_size, epoch=0, seed=0, shuffle=True, rank=0, world=1, drop_last=True, want_onehot=True):
        from . import ops
        order = self.epoch_order(epoch, seed, shuffle, rank, world)
        n = order.numel()
        stop = n - n % batch_size if drop_last else n
        for lo in range(0, stop, batch_size):
            rows = order[lo:lo + batch_size].contiguous()
            B = rows.numel()
            idx = torch.empty(B, self.L, dtype=torch.long, device=self.device)
            ohe = torch.empty(B, self.L, self.C, dtype=torch.float32, device=self.device) if want_onehot else None
            ops.expand_indices(self.store, rows, idx, ohe, B, self.L, self.C)
            yield idx, ohe


def tokenize_corpus(smiles, vocab):
    """A list of strings -> (tokens uint8 [total], offsets int64 [N + 1]): ``vocab.string2ids`` of every string, without specials, back to
    back.  Vectorised: the joined strings go through a 256-entry table built from ``vocab.c2i`` (a character the vocabulary lacks gets what
    ``CharVocab.char2id`` gives it, <unk>).  Empty strings are legal.  ValueError: more than 256 ids, or a character of the vocabulary or of
    the corpus that is not one byte in latin-1."""
    if len(vocab) > 256:
        raise ValueError(f"tokenize_corpus: {len(vocab)} ids do not fit uint8")
    table = np.full(256, vocab.unk, dtype=np.uint8)
    for ch, i in vocab.c2i.items():
        if len(ch) != 1:
            continue                                          # the specials: never part of a string
        if ord(ch) > 255:
            raise ValueError(f"tokenize_corpus: vocabulary character {ch!r} is not a single latin-1 byte")
        table[ord(ch)] = i
    smiles = list(smiles)
    offsets = np.zeros(len(smiles) + 1, dtype=np.int64)
    if smiles:
        np.cumsum(np.fromiter(map(len, smiles), dtype=np.int64, count=len(smiles)), out=offsets[1:])
    try:
        raw = "".join(smiles).encode("latin-1")
    except UnicodeEncodeError as e:
        raise ValueError(f"tokenize_corpus: corpus character {e.object[e.start]!r} is not a single latin-1 byte") from None
    return table[np.frombuffer(raw, dtype=np.uint8)], offsets


def moses_epoch_plan(lengths, batch_size, epoch=0, seed=0, shuffle=True, rank=0, world=1, drop_last=True, bucket=0):
    """One epoch of ``MosesDeviceDataset.batches`` for one rank, on the host: (order, cuts) -- ``order`` int64 ndarray, the corpus rows
    of this rank's batches back to back, and ``cuts`` a list of (lo, hi, T): batch i is ``order[lo:hi]`` and T its longest row + 2.
    `lengths`: the corpus' row lengths without specials.

    bucket = 0: the batches of ``DataLoader(sampler=ShardedSampler(n, rank, world, seed), batch_size, drop_last)`` at that epoch -- this
      rank's contiguous shard of ``torch.randperm(n, generator=manual_seed(seed + epoch))`` (``arange`` without shuffle) in chunks.
    bucket = k > 0: the global order is cut into windows of k * world batches; each window's rows are sorted by length (stable, descending)
      and cut into batches; the `world` consecutive batches of a window form one step (rank r takes the r-th: neighbouring lengths, so the
      ranks' T are balanced); the steps are then shuffled with the same generator, so length is not monotone in time.  Every rank has the
      same number of batches; the rows that do not fill a last global step are dropped (world == 1 and drop_last=False: kept as a short
      batch)."""
    lengths = np.asarray(lengths)
    n = int(lengths.shape[0])
    for name, v in (("batch_size", batch_size), ("world", world)):
        if int(v) != v or v < 1:
            raise ValueError(f"{name} must be a positive integer, got {v!r}")
    for name, v in (("bucket", bucket), ("epoch", epoch), ("seed", seed)):
        if int(v) != v or v < 0:
            raise ValueError(f"{name} must be a non-negative integer, got {v!r}")
    if int(rank) != rank or not 0 <= rank < world:
        raise ValueError(f"rank {rank!r} outside [0, {world})")
    if not drop_last and world != 1:
        raise ValueError("drop_last=False would give the ranks different batch counts: world == 1 only")
    B, world, rank, bucket = int(batch_size), int(world), int(rank), int(bucket)
    g = torch.Generator(); g.manual_seed(int(seed) + int(epoch))
    perm = (torch.randperm(n, generator=g) if shuffle else torch.arange(n)).numpy()
    if bucket == 0:
        per = n // world
        stop = per - per % B if drop_last else per
        order = perm[rank * per:rank * per + stop]
        bounds = [(lo, min(lo + B, stop)) for lo in range(0, stop, B)]
    else:
        G = B * world                                         # rows of one global step
        steps = n // G if drop_last else -(-n // G)
        perm = perm[:min(n, steps * G)]
        win = bucket * G
        mine = []
        for w0 in range(0, perm.shape[0], win):
            rows = perm[w0:w0 + win]
            rows = rows[np.argsort(-lengths[rows].astype(np.int64), kind="stable")]
            for s0 in range(0, rows.shape[0], G):
                mine.append(rows[s0 + rank * B:s0 + (rank + 1) * B])
        if shuffle:
            mine = [mine[i] for i in torch.randperm(len(mine), generator=g).tolist()]
        order = np.concatenate(mine) if mine else perm[:0]
        ends = np.cumsum([m.shape[0] for m in mine]).tolist()
        bounds = list(zip([0] + ends[:-1], ends))
    order = np.ascontiguousarray(order, dtype=np.int64)
    if bounds:
        starts = np.array([lo for lo, _ in bounds])
        tmax = np.maximum.reduceat(lengths[order].astype(np.int64), starts)
    else:
        tmax = []
    return order, [(lo, hi, int(t) + 2) for (lo, hi), t in zip(bounds, tmax)]


class MosesDeviceDataset:
    """The tokenised MOSES corpus in HBM (CSR: uint8 tokens, int64 offsets) and its batches as device ``PaddedBatch``es, one
    ``mvae_moses_collate`` launch each: what ``DataLoader(smiles, sampler=ShardedSampler, collate_fn=get_padded_collate_fn(vocab))``
    feeds ``mosesvae.VAE``, without host work in the step.  The row lengths stay on the host as well (``lengths``, int32, without
    specials), so a batch's T is known without asking the device.

    ``gather`` / ``batches`` never wait for the device; ``err`` (int32 [1], device) is raised by a launch whose T was too small (1) or
    that met a row id outside the corpus (2) -- ``check_errors()`` reads it.  The batches of ``batches()`` cannot raise it."""

    def __init__(self, smiles_or_encoded, vocab, device="cuda"):
        enc = smiles_or_encoded
        if isinstance(enc, tuple) and len(enc) == 2 and not isinstance(enc[0], str):
            tokens, offsets = np.asarray(enc[0]), np.asarray(enc[1])
            if tokens.dtype != np.uint8 or tokens.ndim != 1 or offsets.ndim != 1 or offsets.shape[0] < 1:
                raise ValueError("MosesDeviceDataset: (tokens uint8 [total], offsets int64 [N + 1]) expected")
            offsets = offsets.astype(np.int64)
            if offsets[0] != 0 or offsets[-1] != tokens.shape[0] or (np.diff(offsets) < 0).any():
                raise ValueError("MosesDeviceDataset: offsets must rise from 0 to len(tokens)")
            if tokens.size and int(tokens.max()) >= len(vocab):
                raise ValueError("MosesDeviceDataset: token id outside the vocabulary")
        else:
            tokens, offsets = tokenize_corpus(enc, vocab)
        if offsets.shape[0] < 2:
            raise ValueError("MosesDeviceDataset: empty corpus")
        for name in ("bos", "eos", "pad"):
            if not 0 <= getattr(vocab, name) <= 65535:
                raise ValueError(f"MosesDeviceDataset: vocab.{name} outside [0, 65535]")
        self.vocab, self.n = vocab, int(offsets.shape[0] - 1)
        self.lengths = np.diff(offsets).astype(np.int32)
        self.max_len = int(self.lengths.max())
        self.device = torch.device(device)
        # one spare byte, so that a corpus of empty strings still has a tokens pointer
        self.tokens = torch.from_numpy(np.concatenate([tokens, np.zeros(1, np.uint8)])).to(self.device)
        self.offsets = torch.from_numpy(np.ascontiguousarray(offsets)).to(self.device)
        self.err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._no_caches()

    def _no_caches(self):
        self._slots = self._n_distinct_d = self._n_distinct = None     # the corpus index: built on first use
        self._descriptors = None                                       # descriptors(): computed on first use
        self._fingerprints = None                                      # fingerprints(): computed on first use
        self._scaffolds = self._scaffold_hist = self._scaffold_order = self._mol_keys = None     # scaffolds() and what is derived from it
        self._kekule = None
        self._canonical = None                                         # canonical(): (dataset, status, counts), computed on first use
        self._normal = None                                            # normal_form(): (dataset, status, counts), likewise
        self._fragments = self._fragment_hist = self._fragment_order = None      # fragments() and what is derived from it
        self._scaffold_smiles = None                                   # scaffold_smiles(): (dataset, rows, status, counts), likewise
        self._selfies = None                                           # selfies(): (dataset, status, counts), likewise

    def __len__(self):
        return self.n

    def build_index(self):
        """The exact corpus index behind ``lookup`` / ``contains`` / ``n_distinct``: an open-addressing hash table over the CSR rows (int64
        slots, the smallest power of two >= 2 N of them, so at most half full), filled by one ``mvae_corpus_index_build`` launch.  Does
        nothing when the index is there; never waits for the device.  Returns self."""
        if self._slots is None:
            from . import ops
            from .models import _require_cuda
            _require_cuda(self.device, "MosesDeviceDataset's corpus index")
            n_slots = 1 << (2 * self.n - 1).bit_length()
            slots = torch.empty(n_slots, dtype=torch.long, device=self.device)
            self._n_distinct_d = torch.empty(1, dtype=torch.long, device=self.device)
            ops.corpus_index_build(self.tokens, self.offsets, self.n, slots, self._n_distinct_d)
            self._slots = slots
        return self

    @property
    def n_distinct(self):
        """The number of distinct corpus rows, a Python int (waits for the device once, then cached)."""
        if self._n_distinct is None:
            self.build_index()
            self._n_distinct = int(self._n_distinct_d.item())
        return self._n_distinct

    def _probe(self, x):
        """lookup() of a device int64 [B, T] with unit column stride: one launch, no wait."""
        from . import ops
        self.build_index()
        match = torch.empty(x.shape[0], dtype=torch.long, device=self.device)
        ops.corpus_index_probe(self.tokens, self.offsets, self.n, self._slots, x, self.vocab.eos, match)
        return match

    def _token_rows(self, x, who):
        """What ``lookup`` and ``nearest_strings`` take -- padded ids [B, T] (bos first), or a list of id tensors (bos first) or strings --
        as a device int64 [B, T] with unit column stride.  Strings go through ``tokenize_corpus``' byte table, as the corpus did."""
        from .vocab import token_rows
        v = self.vocab
        if not torch.is_tensor(x):
            x = list(x)
            csr = None
            if x and all(isinstance(s, str) for s in x):
                try:
                    csr = tokenize_corpus(x, v)
                except ValueError:                                # a character beyond latin-1: <unk> by the slow route below
                    pass
            if csr is not None:
                tokens, offsets = csr
                lens = np.diff(offsets)
                cols = int(lens.max()) + 2
                host = np.full((len(x), cols), v.pad, dtype=np.int64)
                host[:, 0] = v.bos
                host[:, 1:-1][np.arange(cols - 2)[None, :] < lens[:, None]] = tokens      # the mask's row-major order is the CSR's order
                host[np.arange(len(x)), lens + 1] = v.eos
                x = torch.from_numpy(host)
        return token_rows(x, lambda s: v.string2ids(s, add_bos=True, add_eos=True), v.pad, who, self.device)

    def lookup(self, x):
        """Which corpus row each token row equals: int64 [B] on the device, the LOWEST corpus row with exactly those tokens, -1 for none
        (``mvae_corpus_index_probe``; builds the index on first use).  x: padded ids [B, T] (bos first) on the device, or a list of id
        tensors (bos first) or strings.  A row's content is what stands between <bos> and its first <eos> (or its last column); a special
        token inside it matches nothing.  Strings go through ``tokenize_corpus``' byte table, as the corpus did, so an unknown character
        is <unk> on both sides.  Exact: token rows are compared, not hashes."""
        return self._probe(self._token_rows(x, "lookup"))

    def nearest_strings(self, x, k=1, exclude_self=False):
        """The k corpus rows at the smallest token-level Levenshtein distance (unit costs, no transposition) from each row of x, which is
        whatever ``lookup`` takes: (dist int32 [Q, k], rows int64 [Q, k]) on the device, ascending in (distance, row) -- equal distances
        rank by the lower row, so a query that IS a corpus row gets (0, ``lookup``'s row) first; a tail that cannot be filled is
        (``ops.EDIT_NONE``, -1).  The model-free counterpart of ``MosesLatentIndex.neighbors``: one ``mvae_edit_knn`` launch (two when the
        corpus is split over workgroups), no host wait.  A special token inside a query's content equals no corpus token.
        ``exclude_self``: a query that is itself a corpus row (``lookup``) does not answer with that row.  ValueError, before any device
        work: a vocabulary of more than 64 ids, k outside [1, 32], a query wider than 129 columns."""
        from . import ops
        if len(self.vocab) > ops.EDIT_V_MAX:
            raise ValueError(f"nearest_strings: the vocabulary has {len(self.vocab)} ids, at most {ops.EDIT_V_MAX} are supported")
        if int(k) != k or not 1 <= k <= ops.EDIT_K_MAX:
            raise ValueError(f"nearest_strings: k must be an integer in [1, {ops.EDIT_K_MAX}], got {k!r}")
        if torch.is_tensor(x):
            width = x.shape[1] if x.dim() == 2 else 0
        else:
            x = list(x)
            width = max((len(s) + 2 if isinstance(s, str) else int(torch.as_tensor(s).numel()) for s in x), default=0)
        if width - 1 > ops.EDIT_PATTERN_MAX:
            raise ValueError(f"nearest_strings: a query has {width} columns, at most {ops.EDIT_PATTERN_MAX + 1} are supported")
        x = self._token_rows(x, "nearest_strings")
        from .models import _require_cuda
        _require_cuda(self.device, "MosesDeviceDataset.nearest_strings")
        exclude = self._probe(x) if exclude_self else None
        return ops.edit_knn(x, self.tokens, self.offsets, self.n, int(k), self.vocab.eos, len(self.vocab), exclude=exclude)

    def descriptors(self):
        """``VAE.descriptors`` of every corpus row, in corpus order: the same dict (status, bad_pos, heavy_atoms, ..., formula, weight), from
        ONE ``mvae_smiles_graph_corpus`` launch over the CSR rows (and the matrix-vector product of the weight).  bad_pos is 0-based in the row's string.  Cached; never waits for the
        device.  ValueError for a vocabulary of more than 64 ids."""
        if self._descriptors is None:
            from . import ops
            from .models import _require_cuda
            from .vocab import smiles_token_table, smiles_chem_table
            if len(self.vocab) > 64:
                raise ValueError(f"descriptors: the vocabulary has {len(self.vocab)} ids, at most 64 are supported")
            _require_cuda(self.device, "MosesDeviceDataset.descriptors")
            tok, chem = smiles_token_table(self.vocab).to(self.device), smiles_chem_table(self.vocab).to(self.device)
            self._descriptors = ops.graph_descriptors(*ops.smiles_graph_corpus(self.tokens, self.offsets, self.n, tok, chem))
        return self._descriptors

    def _fp_tables(self, who):
        from .models import _require_cuda
        from .vocab import smiles_token_table, smiles_chem_table
        if len(self.vocab) > 64:
            raise ValueError(f"{who}: the vocabulary has {len(self.vocab)} ids, at most 64 are supported")
        _require_cuda(self.device, "MosesDeviceDataset." + who)
        if self.__dict__.get("_smi_tables") is None:
            self._smi_tables = (smiles_token_table(self.vocab).to(self.device), smiles_chem_table(self.vocab).to(self.device))
        return self._smi_tables

    def fingerprints(self):
        """The circular fingerprint of every corpus row, in corpus order: {"status": int32 [N], "fp": int64 [N, 16]} on the device
        (``VAE.fingerprints``: 1024 bits, built like ECFP4 but not rdkit's Morgan fingerprint; zeros where status is not 0), from ONE
        ``mvae_smiles_fp_corpus`` launch over the CSR rows.  Cached; never waits for the device.  ValueError for a vocabulary of more
        than 64 ids."""
        if self._fingerprints is None:
            from . import ops
            tok, chem = self._fp_tables("fingerprints")
            status, fp = ops.smiles_fp_corpus(self.tokens, self.offsets, self.n, tok, chem)
            self._fingerprints = {"status": status, "fp": fp}
        return self._fingerprints

    def nearest_fingerprints(self, x, k=1, exclude_self=False):
        """The k corpus rows whose fingerprints are most similar (Tanimoto) to that of each row of x, which is whatever ``lookup``
        takes: (sim float32 [Q, k], rows int64 [Q, k]) on the device, ordered by (similarity descending, row ascending); a tail that
        cannot be filled is (-1.0, -1).  The structure-aware counterpart of ``nearest_strings``: one fingerprint launch for x and one
        ``mvae_tanimoto_knn`` launch (two when the corpus is split over workgroups) against ``fingerprints()``, no host wait.  Every
        corpus row is eligible, a row that is not ok with its all-zero fingerprint (similarity 0); a query that is not ok is similar
        to nothing (0 everywhere, so it answers with the lowest rows).  ``exclude_self``: a query that is itself a corpus row
        (``lookup``) does not answer with that row.  ValueError, before any device work: a vocabulary of more than 64 ids, k outside
        [1, 32]."""
        from . import ops
        if len(self.vocab) > 64:
            raise ValueError(f"nearest_fingerprints: the vocabulary has {len(self.vocab)} ids, at most 64 are supported")
        if int(k) != k or not 1 <= k <= ops.TANIMOTO_K_MAX:
            raise ValueError(f"nearest_fingerprints: k must be an integer in [1, {ops.TANIMOTO_K_MAX}], got {k!r}")
        x = self._token_rows(x, "nearest_fingerprints")
        tok, chem = self._fp_tables("nearest_fingerprints")
        _, fp = ops.smiles_fp_rows(x, tok, chem, self.vocab.eos)
        exclude = self._probe(x) if exclude_self else None
        return ops.tanimoto_knn(fp, self.fingerprints()["fp"], int(k), exclude=exclude)

    def scaffolds(self):
        """The Murcko scaffold and the graph keys of every corpus row, in corpus order: ``VAE.scaffolds``' dict (status, mask, atoms,
        bonds, linker_atoms, exo_atoms, mol_key, scaffold_key) on the device, from ONE ``mvae_smiles_scaffold_corpus`` launch over the
        CSR rows.  Not rdkit's MurckoScaffold, and the keys ignore stereochemistry (include/mvae.h, "Murcko scaffold", "Graph key").
        Cached; never waits for the device.  ValueError for a vocabulary of more than 64 ids."""
        if self._scaffolds is None:
            from . import ops
            tok, chem = self._fp_tables("scaffolds")
            self._scaffolds = ops.scaffold_dict(*ops.smiles_scaffold_corpus(self.tokens, self.offsets, self.n, tok, chem))
        return self._scaffolds

    def fragments(self):
        """The fragments of every corpus row and their graph keys, in corpus order: ``VAE.fragments``' dict (status, mask, fragments,
        cuts, acyl_cuts, largest, keys) on the device, from ONE ``mvae_smiles_fragment_corpus`` launch over the CSR rows.  This
        library's own rule, not BRICS and not RECAP (include/mvae.h, "Fragments").  Cached; never waits for the device.  ValueError for
        a vocabulary of more than 64 ids."""
        if self._fragments is None:
            from . import ops
            tok, chem = self._fp_tables("fragments")
            self._fragments = ops.fragment_dict(*ops.smiles_fragment_corpus(self.tokens, self.offsets, self.n, tok, chem))
        return self._fragments

    def fragment_histogram(self):
        """(keys int64 [n], counts int64 [n]) on the device: the distinct fragment keys of the corpus, ascending, and how many fragments
        have each, a fragment that occurs twice in a row counting twice (``ops.key_histogram`` over all 16 slots; the unused slots, the
        rows that are not ok and the rows of more than 16 fragments hold 0 and are not counted).  Cached."""
        if self._fragment_hist is None:
            from . import ops
            self._fragment_hist = ops.key_histogram(self.fragments()["keys"])
        return self._fragment_hist

    def rows_with_fragment(self, x):
        """For each row of x (whatever ``lookup`` takes; ask with a fragment, such as a decoded ``VAE.fragment_smiles`` row), the corpus
        rows that have a fragment with the key of its FIRST fragment: CSR ``(offsets int64 [Q + 1], rows int64 [offsets[-1]])`` on the
        device, the rows of query i at ``rows[offsets[i] : offsets[i + 1]]``, ascending, a row that has the fragment twice listed once.
        A query that is not ok gets none.  One fragment launch for x against the cached, sorted corpus keys; the one host wait is the
        size of the answer."""
        from . import ops
        if len(self.vocab) > 64:
            raise ValueError(f"rows_with_fragment: the vocabulary has {len(self.vocab)} ids, at most 64 are supported")
        x = self._token_rows(x, "rows_with_fragment")
        tok, chem = self._fp_tables("rows_with_fragment")
        if self._fragment_order is None:
            # (key, row) pairs of all slots, sorted by key then row, the repeats of a pair within a row dropped
            keys = self.fragments()["keys"]
            row = torch.arange(self.n, device=self.device).repeat_interleave(keys.shape[1])
            ks, order = torch.sort(keys.reshape(-1), stable=True)
            rs = row[order]
            first = torch.ones_like(ks, dtype=torch.bool)
            first[1:] = (ks[1:] != ks[:-1]) | (rs[1:] != rs[:-1])
            self._fragment_order = (ks[first].contiguous(), rs[first].contiguous())
        keys, order = self._fragment_order
        q = ops.smiles_fragment_rows(x, tok, chem, self.vocab.eos, mask=False)[3][:, 0].contiguous()
        lo = torch.searchsorted(keys, q)
        n = torch.where(q != 0, torch.searchsorted(keys, q, right=True) - lo, torch.zeros_like(lo))
        offsets = torch.zeros(q.shape[0] + 1, dtype=torch.long, device=self.device)
        offsets[1:] = torch.cumsum(n, 0)
        owner = torch.repeat_interleave(torch.arange(q.shape[0], device=self.device), n)
        rows = order[lo[owner] + torch.arange(owner.shape[0], device=self.device) - offsets[owner]]
        return offsets, rows

    def kekule(self):
        """The kekulisation test of every corpus row, in corpus order: {"status", "n_atoms", "n_bonds", "pairs", "deficiency": int32
        [N]} on the device (``VAE.kekule`` without the mates), from ONE ``mvae_smiles_kekule_corpus`` launch over the CSR rows.  Status
        0 means "kekulisable", 7 that the aromatic atoms cannot all take their ring double bond; not rdkit's Kekulize (include/mvae.h,
        "Kekulisation").  The tool to audit a training file: every row of a sanitised corpus should pass.  Cached; never waits for
        the device.  ValueError for a vocabulary of more than 64 ids."""
        if self._kekule is None:
            from . import ops
            tok, chem = self._fp_tables("kekule")
            out = ops.kekule_dict(*ops.smiles_kekule_corpus(self.tokens, self.offsets, self.n, tok, chem, mate=False))
            del out["mate"]
            self._kekule = out
        return self._kekule

    def _compacted(self, tokens_out, offsets_out, rows):
        """The gapped CSR of a writer _corpus launch (ops.smiles_rewrite_corpus) as a ``MosesDeviceDataset`` on the same device, compacted
        there: batch members `rows` (int64, ascending), all of them for None.  The host waits once, for the row lengths."""
        dev, stride = self.device, tokens_out.shape[1]
        lens = offsets_out[1::2] - offsets_out[0:-1:2]
        if rows is not None:
            lens, tokens_out = lens[rows], tokens_out[rows]
        n = lens.numel()
        offsets = torch.zeros(n + 1, dtype=torch.long, device=dev)
        offsets[1:] = torch.cumsum(lens, 0)
        keep = torch.arange(stride, device=dev)[None, :] < lens[:, None]
        ds = object.__new__(MosesDeviceDataset)
        ds.vocab, ds.n, ds.device = self.vocab, n, dev
        ds.lengths = lens.to(torch.int32).cpu().numpy()
        ds.max_len = int(ds.lengths.max()) if n else 0
        ds.tokens = torch.cat([tokens_out[keep], torch.zeros(1, dtype=torch.uint8, device=dev)])      # the spare byte of __init__
        ds.offsets = offsets
        ds.err = torch.zeros(1, dtype=torch.int32, device=dev)
        ds._no_caches()
        return ds

    def canonical(self):
        """The corpus in canonical spelling: a ``MosesDeviceDataset`` on the same device whose row r is the canonical spelling of this
        one's row r (include/mvae.h, "SMILES canon"; a row that cannot be written -- ``canonical_status`` != 0 -- keeps its own
        spelling), from ONE ``mvae_smiles_canon_corpus`` launch over all rows, its gapped CSR compacted on the device.  Its ``lookup`` /
        ``contains`` / ``n_distinct`` answer at the level of graphs when they are asked with canonical rows (``VAE.canonical``): two
        spellings of one graph are one row there, exactly -- token rows are compared, no hash decides.  Not rdkit's canonical SMILES: no
        aromaticity perception, no stereo.  Cached; the host waits once, for the row lengths.  ValueError for a vocabulary of more than
        64 ids."""
        if self._canonical is None:
            from . import ops
            from .vocab import smiles_emit_table
            tok, chem = self._fp_tables("canonical")
            dev, n, stride = self.device, self.n, max(127, self.max_len)          # a row that is copied through fits
            counts = torch.zeros(ops.REWRITE_COUNTS, dtype=torch.int32, device=dev)
            tokens_out, offsets_out, status, _, _ = ops.smiles_canon_corpus(
                self.tokens, self.offsets, n, torch.arange(n, dtype=torch.long, device=dev), tok, chem, smiles_emit_table(self.vocab).to(dev),
                127, stride, info=False, rank=False, counts=counts)
            ds = self._compacted(tokens_out, offsets_out, None)
            self._canonical = (ds, status, counts)
        return self._canonical[0]

    @property
    def canonical_status(self):
        """The status of every corpus row under ``canonical()``: int32 [N] on the device, the codes of ``ops.REWRITE_STATUS_NAMES`` (0: row
        r of ``canonical()`` is the canonical spelling; anything else: it is this corpus' own row r)."""
        self.canonical()
        return self._canonical[1]

    @property
    def canonical_counts(self):
        """How many corpus rows have each ``canonical_status``: int32 [16] on the device, kept by the kernel's integer atomic adds."""
        self.canonical()
        return self._canonical[2]

    def normal_form(self):
        """The corpus in aromatic normal form: a ``MosesDeviceDataset`` on the same device whose row r is the normal form of this one's
        row r (include/mvae.h, "Aromatic normal form": aromaticity perceived by this library's own rule, then the canonical spelling; a
        row that cannot be written -- ``normal_status()`` != 0 -- keeps its own spelling), from ONE ``mvae_smiles_aromatize_corpus``
        launch over all rows, its gapped CSR compacted on the device.  Asked with ``VAE.normal_form`` rows, its ``lookup`` / ``contains`` /
        ``n_distinct`` count a Kekule and an aromatic spelling of one molecule once, which ``canonical()`` does not.  NOT rdkit's
        aromaticity model or canonical SMILES; no stereo.  Cached; the host waits once, for the row lengths.  ValueError for a
        vocabulary of more than 64 ids."""
        if self._normal is None:
            from . import ops
            from .vocab import smiles_emit_table
            tok, chem = self._fp_tables("normal_form")
            dev, n, stride = self.device, self.n, max(127, self.max_len)          # a row that is copied through fits
            counts = torch.zeros(ops.AROMATIZE_COUNTS, dtype=torch.int32, device=dev)
            tokens_out, offsets_out, status, _, _ = ops.smiles_aromatize_corpus(
                self.tokens, self.offsets, n, torch.arange(n, dtype=torch.long, device=dev), tok, chem, smiles_emit_table(self.vocab).to(dev),
                127, stride, info=False, arom=False, counts=counts)
            ds = self._compacted(tokens_out, offsets_out, None)
            self._normal = (ds, status, counts)
        return self._normal[0]

    def normal_status(self):
        """The status of every corpus row under ``normal_form()``: int32 [N] on the device, the codes of ``ops.AROMATIZE_STATUS_NAMES``
        (0: row r of ``normal_form()`` is the normal form; anything else: it is this corpus' own row r)."""
        self.normal_form()
        return self._normal[1]

    def normal_counts(self):
        """How many corpus rows have each ``normal_status()``: int32 [32] on the device, kept by the kernel's integer atomic adds."""
        self.normal_form()
        return self._normal[2]

    def selfies(self, svocab=None):
        """The encodable rows of the corpus as a SELFIES training corpus: a ``MosesDeviceDataset`` in the tokens of `svocab` (a
        ``vocab.SelfiesVocab``; None: ``SelfiesVocab.default()``) on the same device, from ONE ``mvae_selfies_encode_corpus`` launch over
        all rows, its gapped CSR compacted on the device.  Row i of the result encodes corpus row ``source_rows[i]`` (int64 on the
        device, ascending): the rows whose ``selfies_status()`` is 0.  The encoding keeps the atoms in their string order (include/mvae.h,
        "SELFIES": Encode) and is this library's own, NOT the selfies package's encoder.  Cached per call with the same vocabulary
        object; the host waits once, for the row lengths.  ValueError for a vocabulary of more than 64 ids."""
        from .vocab import SelfiesVocab
        if self._selfies is None or (svocab is not None and svocab is not self._selfies[0].vocab):
            from . import ops
            from .vocab import smiles_emit_table, selfies_emit_table
            svocab = SelfiesVocab.default() if svocab is None else svocab
            tok, chem = self._fp_tables("selfies")
            dev, n = self.device, self.n
            counts = torch.zeros(ops.SELFIES_COUNTS, dtype=torch.int32, device=dev)
            tokens_out, offsets_out, status, _ = ops.selfies_encode_corpus(
                self.tokens, self.offsets, n, torch.arange(n, dtype=torch.long, device=dev), tok, chem, smiles_emit_table(self.vocab).to(dev),
                selfies_emit_table(svocab).to(dev), 127, 127, info=False, counts=counts)
            rows = torch.nonzero(status == 0).view(-1)
            ds = self._compacted(tokens_out, offsets_out, rows)
            ds.vocab, ds.source_rows = svocab, rows
            self._selfies = (ds, status, counts)
        return self._selfies[0]

    def selfies_status(self):
        """The status of every corpus row under ``selfies()``: int32 [N] on the device, the codes of ``ops.SELFIES_STATUS_NAMES`` (0: the
        row is in ``selfies()``; 13: a symbol the vocabulary lacks; 18: an atom over the capacity of its symbol)."""
        self.selfies()
        return self._selfies[1]

    def scaffold_smiles(self):
        """The Murcko scaffolds of the corpus as token rows (include/mvae.h, "Scaffold SMILES"): (ds_scaf, rows) -- a
        ``MosesDeviceDataset`` on the same device holding the scaffold, in canonical spelling, of every corpus row that has one
        (``scaffold_smiles_status`` 0), in corpus order and without empty rows, and rows int64 [M], the corpus row of each.  From ONE
        ``mvae_smiles_scaffold_smiles_corpus`` launch over all rows, its gapped CSR compacted on the device.  ``ds_scaf.n_distinct`` is
        the exact number of distinct scaffold structures -- token rows are compared, no hash decides -- where ``scaffold_histogram()``
        counts keys; ``ds_scaf.smiles(i)`` shows one, ``ds_scaf.lookup`` finds one (ask with ``VAE.scaffold_smiles`` rows).  NOT rdkit's
        MurckoScaffoldSmiles: nothing is sanitised, no aromaticity perception, and a row with a stereo token has no scaffold.  Cached;
        the host waits for M and for the row lengths.  ValueError for a vocabulary of more than 64 ids."""
        if self._scaffold_smiles is None:
            from . import ops
            from .vocab import smiles_emit_table
            tok, chem = self._fp_tables("scaffold_smiles")
            dev, n = self.device, self.n
            counts = torch.zeros(ops.REWRITE_COUNTS, dtype=torch.int32, device=dev)
            tokens_out, offsets_out, status, _ = ops.smiles_scaffold_smiles_corpus(
                self.tokens, self.offsets, n, torch.arange(n, dtype=torch.long, device=dev), tok, chem, smiles_emit_table(self.vocab).to(dev),
                127, 127, info=False, counts=counts)
            rows = torch.nonzero(status == 0).flatten()
            self._scaffold_smiles = (self._compacted(tokens_out, offsets_out, rows), rows, status, counts)
        return self._scaffold_smiles[:2]

    @property
    def scaffold_smiles_status(self):
        """The status of every corpus row under ``scaffold_smiles()``: int32 [N] on the device, the codes of
        ``ops.SCAFFOLD_SMILES_STATUS_NAMES`` (0: the row has a scaffold there; 14: it has no ring)."""
        self.scaffold_smiles()
        return self._scaffold_smiles[2]

    @property
    def scaffold_smiles_counts(self):
        """How many corpus rows have each ``scaffold_smiles_status``: int32 [16] on the device, kept by the kernel's integer atomic adds."""
        self.scaffold_smiles()
        return self._scaffold_smiles[3]

    def _substructures(self, who, patterns, max_steps, counts=None):
        from . import ops
        tok, chem = self._fp_tables(who)
        table = compile_substructures(patterns, self.vocab)
        out = ops.smiles_substruct_corpus(self.tokens, self.offsets, self.n, tok, chem, table.on(self.device), max_steps, steps=False, counts=counts)
        return table, out

    def substructure_counts(self, patterns, max_steps=65536):
        """How many corpus rows contain each pattern (``compile_substructures``: SMILES fragments or a ``SubstructureTable``), and on how
        many the search ran out of its ``max_steps`` candidates and says neither: int32 [Q, 2] on the device, columns (hits,
        undecided), from ONE ``mvae_smiles_substruct_corpus`` launch over the CSR rows -- each row's graph built once for all patterns,
        the counts kept by the kernel's integer atomic adds; never waits for the device.  Rows the walk refuses contain nothing.  Graph
        containment on (element, aromatic, charge) and bond classes (include/mvae.h, "SMILES substructure"): not SMARTS, not rdkit's
        HasSubstructMatch.  ValueError for a refused pattern or a vocabulary of more than 64 ids."""
        from .models import _require_cuda
        _require_cuda(self.device, "MosesDeviceDataset.substructure_counts")
        table = compile_substructures(patterns, self.vocab)
        counts = torch.zeros(len(table), 2, dtype=torch.int32, device=self.device)
        self._substructures("substructure_counts", table, max_steps, counts)
        return counts

    def rows_with_substructure(self, pattern, max_steps=65536, return_undecided=False):
        """The corpus rows that contain one pattern: int64 row ids on the device, ascending (one ``mvae_smiles_substruct_corpus`` launch;
        the host waits once, for their number).  ``return_undecided=True`` also returns the rows on which the search ran out of
        ``max_steps``."""
        from .models import _require_cuda
        _require_cuda(self.device, "MosesDeviceDataset.rows_with_substructure")
        if not isinstance(pattern, str):
            raise ValueError("rows_with_substructure: one pattern, a string")
        _, (_, hit, undecided, _, _) = self._substructures("rows_with_substructure", [pattern], max_steps)
        rows = torch.nonzero(hit & 1).flatten()
        return (rows, torch.nonzero(undecided & 1).flatten()) if return_undecided else rows

    def scaffold_histogram(self):
        """(keys int64 [n], counts int64 [n]) on the device: the distinct scaffold keys of the corpus rows whose status is 0, ascending,
        and how many rows have each (``ops.key_histogram``; rows without a ring have no scaffold and are not counted).  Cached."""
        if self._scaffold_hist is None:
            from . import ops
            self._scaffold_hist = ops.key_histogram(self.scaffolds()["scaffold_key"])       # a row that is not ok has key 0
        return self._scaffold_hist

    def mol_keys_sorted(self):
        """The molecule keys of the corpus rows, ascending (zeros, the rows that are not ok, included): what ``ops.keys_in`` searches to
        tell whether a generated graph is in the corpus.  Cached; never waits."""
        if self._mol_keys is None:
            self._mol_keys = torch.sort(self.scaffolds()["mol_key"])[0]
        return self._mol_keys

    def rows_with_scaffold(self, x):
        """For each row of x (whatever ``lookup`` takes), the corpus rows that have its scaffold key: CSR ``(offsets int64 [Q + 1], rows
        int64 [offsets[-1]])`` on the device, the rows of query i at ``rows[offsets[i] : offsets[i + 1]]``, ascending.  A query without a
        scaffold (no ring, or not ok) gets none.  One scaffold launch for x against the cached, sorted corpus keys; the one host wait is
        the size of the answer."""
        from . import ops
        if len(self.vocab) > 64:
            raise ValueError(f"rows_with_scaffold: the vocabulary has {len(self.vocab)} ids, at most 64 are supported")
        x = self._token_rows(x, "rows_with_scaffold")
        tok, chem = self._fp_tables("rows_with_scaffold")
        if self._scaffold_order is None:
            self._scaffold_order = torch.sort(self.scaffolds()["scaffold_key"], stable=True)       # equal keys: ascending rows
        keys, order = self._scaffold_order
        q = ops.smiles_scaffold_rows(x, tok, chem, self.vocab.eos, mask=False)[3][:, 1].contiguous()
        lo = torch.searchsorted(keys, q)
        n = torch.where(q != 0, torch.searchsorted(keys, q, right=True) - lo, torch.zeros_like(lo))
        offsets = torch.zeros(q.shape[0] + 1, dtype=torch.long, device=self.device)
        offsets[1:] = torch.cumsum(n, 0)
        owner = torch.repeat_interleave(torch.arange(q.shape[0], device=self.device), n)
        rows = order[lo[owner] + torch.arange(owner.shape[0], device=self.device) - offsets[owner]]
        return offsets, rows

    def scaffold_split(self, test_fraction, seed=0):
        """A scaffold-held-out split: ``(train_rows, test_rows)``, int64 on the device, ascending, disjoint, covering every row.  Whole
        scaffolds go to the test side, in an order drawn from ``seed``, until at least ``test_fraction`` of the ring-bearing rows are
        there, so no non-zero scaffold key occurs on both sides; acyclic rows and rows that are not ok stay in train.  Deterministic
        (``ops.scaffold_split_rows``).  ValueError for a fraction outside [0, 1]."""
        from . import ops
        if not 0.0 <= float(test_fraction) <= 1.0:
            raise ValueError(f"scaffold_split: test_fraction must be in [0, 1], got {test_fraction!r}")
        return ops.scaffold_split_rows(self.scaffolds()["scaffold_key"].contiguous(), test_fraction, seed)

    def contains(self, x):
        """``lookup(x) >= 0``: bool [B] on the device."""
        return self.lookup(x) >= 0

    def _check_model(self, model, who):
        """The checks ``moses_generate(novel_against=)`` makes, before any device work: the model's vocabulary gives every character and
        special the id this corpus was tokenised with, and the model lives on this corpus' device."""
        if self.vocab.c2i != model.vocabulary.c2i:
            raise ValueError(f"{who}: the corpus was tokenised with another vocabulary than the model's")
        d, dev = self.device, model.device
        if d.type != dev.type or (d.type == "cuda" and (torch.cuda.current_device() if d.index is None else d.index)
                                  != (torch.cuda.current_device() if dev.index is None else dev.index)):
            raise ValueError(f"{who}: the corpus lives on {d}, the model on {dev}")

    @torch.no_grad()
    def encode_latents(self, model, batch_size=4096):
        """The latent table of the corpus: a ``MosesLatentIndex`` whose ``mu`` (float32 [N, d_z], on the device) holds in row r the
        encoder mean of corpus row r under ``model`` (``VAE.encode``: eps = 0, eval mode, no gradients).  The rows are visited in
        ascending order in chunks of ``batch_size`` (the last one shorter); each chunk is collated by ``gather`` (T = the chunk's longest
        row + 2, known on the host), encoded and scattered to ``mu[batch.rows]``.  Never waits for the device.  ValueError, before any
        device work: another vocabulary than the model's, or a model on another device."""
        self._check_model(model, "encode_latents")
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError(f"encode_latents: batch_size must be >= 1, got {batch_size}")
        mu = torch.empty(self.n, model.d_z, dtype=torch.float32, device=self.device)
        rows = torch.arange(self.n, device=self.device)
        for lo in range(0, self.n, batch_size):
            hi = min(lo + batch_size, self.n)
            batch = self.gather(rows[lo:hi], T=int(self.lengths[lo:hi].max()) + 2)
            mu[batch.rows] = model.encode(batch)[0]
        return MosesLatentIndex(mu, self)

    def smiles(self, rows):
        """The strings of corpus rows (a list, an ndarray or a tensor on either side, any shape; the result is flat): the rows' CSR slices
        are gathered on the device and come back in ONE device-to-host copy.  A row id of -1 (the tail of a short k-NN answer) gives
        None; any other id outside the corpus raises ValueError."""
        r = torch.as_tensor(rows).to(self.device, torch.long).reshape(-1)
        if r.numel() < 1:
            return []
        L = max(self.max_len, 1)
        safe = r.clamp(0, self.n - 1)
        start = self.offsets[safe]
        lens = self.offsets[safe + 1] - start
        pos = (start[:, None] + torch.arange(L, device=self.device)[None, :]).clamp_(max=self.tokens.numel() - 1)
        host = torch.cat([r[:, None], lens[:, None], self.tokens[pos].long()], dim=1).cpu().numpy()
        table = np.array([self.vocab.i2c[i] for i in range(len(self.vocab))], dtype=object)
        out = []
        for row in host:
            if row[0] == -1:
                out.append(None)
                continue
            if not 0 <= row[0] < self.n:
                raise ValueError(f"smiles: row id {int(row[0])} outside [0, {self.n})")
            out.append("".join(table[row[2:2 + row[1]]]))
        return out

    def _collate(self, rows, T):
        from . import ops
        from .vocab import PaddedBatch
        B, v = rows.numel(), self.vocab
        x_pad = torch.empty(B, T, dtype=torch.long, device=self.device)
        lengths = torch.empty(B, dtype=torch.int32, device=self.device)
        rows_sorted = torch.empty(B, dtype=torch.long, device=self.device)
        ops.moses_collate(self.tokens, self.offsets, rows, x_pad, lengths, T, self.n, v.bos, v.eos, v.pad, rows_sorted, self.err)
        return PaddedBatch(x_pad, lengths, rows=rows_sorted)

    def _collate_augmented(self, rows, T, seed, epoch, slack):
        """_collate with every row respelled first: one mvae_smiles_rewrite_corpus launch into a gapped CSR (batch member b at byte
        b * stride), which the unchanged collate reads with rows = 0, 2, 4, ...; T + slack columns."""
        from . import ops
        from .vocab import PaddedBatch, smiles_emit_table
        tok, chem = self._fp_tables("augment")
        if self.__dict__.get("_emit") is None:
            self._emit = smiles_emit_table(self.vocab).to(self.device)
            self._augment_counts = torch.zeros(ops.REWRITE_COUNTS, dtype=torch.int32, device=self.device)
            self._even = {}
        slack = int(slack)
        if slack < 0:
            raise ValueError(f"augment_slack must be >= 0, got {slack}")
        B, v, T = rows.numel(), self.vocab, T + slack
        stride = max(T - 2, 1)                                   # a row that is copied through fits: the plan's T covers the longest
        draw = ops.draw_words(rows + ((int(epoch) * 0x9E3779B1) & 0xFFFFFFFF))
        tokens_out, offsets_out, _ = ops.smiles_rewrite_corpus(self.tokens, self.offsets, self.n, rows, tok, chem, self._emit, seed, draw,
                                                               min(stride, 127), stride, counts=self._augment_counts, err=self.err)
        if B not in self._even:
            self._even[B] = torch.arange(0, 2 * B, 2, dtype=torch.long, device=self.device)
        x_pad = torch.empty(B, T, dtype=torch.long, device=self.device)
        lengths = torch.empty(B, dtype=torch.int32, device=self.device)
        member = torch.empty(B, dtype=torch.long, device=self.device)
        ops.moses_collate(tokens_out.view(-1), offsets_out, self._even[B], x_pad, lengths, T, 2 * B, v.bos, v.eos, v.pad, member, self.err)
        return PaddedBatch(x_pad, lengths, rows=rows[member // 2])

    @property
    def augment_counts(self):
        """The per-status histogram of every row respelled so far by ``batches(augment=True)`` / ``gather(augment=True)``: int32 [16] on the
        device, indexed by the codes of ``ops.REWRITE_STATUS_NAMES`` (0: respelled; anything else: that row went in unchanged); kept by the
        kernel's integer atomic adds.  None before the first augmented batch."""
        return self.__dict__.get("_augment_counts")

    def gather(self, rows, T=None, augment=False, augment_seed=0, augment_epoch=0, augment_slack=0):
        """Corpus rows (a list, an ndarray or a tensor; any order, repeats allowed) -> PaddedBatch of T columns, its rows in the collate's
        stable length-descending order and ``.rows`` the corpus row behind each.  T=None: the longest of the rows + 2 when `rows` is on the
        host, else the corpus' longest + 2 (no device round trip).  ``augment=True``: every row is respelled first (``batches``), the
        batch has T + augment_slack columns and its order follows the new lengths."""
        if torch.is_tensor(rows) and rows.is_cuda:
            rows_d = rows.to(self.device, torch.long).contiguous().view(-1)
            T = self.max_len + 2 if T is None else T
        else:
            host = np.asarray(rows.cpu() if torch.is_tensor(rows) else rows)
            if host.size and not np.issubdtype(host.dtype, np.integer):
                raise ValueError("gather: integer row ids expected")
            host = host.astype(np.int64).reshape(-1)
            if host.size and (host.min() < 0 or host.max() >= self.n):
                raise ValueError(f"gather: row id outside [0, {self.n})")
            if T is None and host.size:
                T = int(self.lengths[host].max()) + 2
            rows_d = torch.from_numpy(host).to(self.device)
        if rows_d.numel() < 1:
            raise ValueError("gather: no rows")
        if int(T) != T or T < 2:
            raise ValueError(f"gather: T must be an integer >= 2, got {T!r}")
        if augment:
            return self._collate_augmented(rows_d, int(T), augment_seed, augment_epoch, augment_slack)
        return self._collate(rows_d, int(T))

    def check_errors(self):
        """Waits for the device; raises when a launch since the last call cut a row (T too small) or met a row id outside the corpus."""
        e = int(self.err.item())
        self.err.zero_()
        if e:
            raise RuntimeError("mvae_moses_collate: " + ("a row id outside the corpus" if e == 2 else "a row longer than T - 2 was cut"))

    def batches(self, batch_size, epoch=0, seed=0, shuffle=True, rank=0, world=1, drop_last=True, bucket=0, augment=False, augment_seed=0,
                augment_slack=0):
        """Generator of this rank's device PaddedBatches of one epoch (``moses_epoch_plan``): one host plan and one upload of the order per
        epoch, then a slice and one launch per batch.  bucket=0 gives exactly the batches of the DataLoader + ShardedSampler +
        get_padded_collate_fn feed; bucket=k groups rows of similar length within windows of k batches per rank (other batches, smaller T).
        ``augment=True`` (SMILES enumeration; ValueError for a vocabulary of more than 64 ids): every row goes in under a randomised
        spelling of the same graph (include/mvae.h, "SMILES rewrite"), one ``mvae_smiles_rewrite_corpus`` launch in front of the
        collate and a few elementwise ones for the draws, no host wait.  The spelling of corpus row r is a pure function of (augment_seed,
        epoch, r) -- draw = epoch * 0x9E3779B1 + r -- whatever the batch size, the rank count or its place in the batch.  A batch keeps
        its planned width plus ``augment_slack`` columns: a spelling that does not fit (about half are two or more tokens longer than the
        original, but only one longer than the batch's longest row does not fit) and a row that cannot be respelled go in unchanged, and ``augment_counts`` says how many of each.  The batch order
        within a batch follows the new lengths.  ``augment=False`` launches exactly what it always did."""
        order, cuts = moses_epoch_plan(self.lengths, batch_size, epoch, seed, shuffle, rank, world, drop_last, bucket)
        if augment:
            self._fp_tables("augment")                           # raises before the generator is handed out
            if int(augment_slack) < 0:
                raise ValueError(f"augment_slack must be >= 0, got {augment_slack}")
        return self._run_plan(order, cuts, (augment_seed, epoch, augment_slack) if augment else None)

    def _run_plan(self, order, cuts, augment=None):
        order_d = torch.from_numpy(order).to(self.device)
        for lo, hi, T in cuts:
            yield self._collate(order_d[lo:hi], T) if augment is None else self._collate_augmented(order_d[lo:hi], T, *augment)


class MosesLatentIndex:
    """The latent table of a ``MosesDeviceDataset`` (``encode_latents``): ``mu`` float32 [N, d_z] on the device, row r the encoder mean of
    corpus row r, and ``dataset``.  ``search`` is the exact k-nearest-neighbour search over it (``mvae_latent_knn``: squared Euclidean
    distance as a direct f32 difference, ties by the lower row, no Q x N buffer)."""

    def __init__(self, mu, dataset):
        if mu.dim() != 2 or mu.dtype != torch.float32 or mu.shape[0] != dataset.n:
            raise ValueError(f"MosesLatentIndex: mu must be float32 [{dataset.n}, d_z], got {mu.dtype} {tuple(mu.shape)}")
        self.mu, self.dataset = mu, dataset

    def __len__(self):
        return self.mu.shape[0]

    def search(self, z, k, exclude=None):
        """(dist2 float32 [Q, k], rows int64 [Q, k]) on the device: the k corpus rows nearest to each latent point of z [Q, d_z], ascending
        in (distance, row); ``exclude`` (int64 [Q], -1 = none) names a row each query skips; a tail that cannot be filled is (+inf, -1).
        One launch (two when the table is split over workgroups), no host wait."""
        from . import ops
        z = z.to(self.mu.device, torch.float32)
        if z.dim() != 2 or z.shape[1] != self.mu.shape[1] or z.shape[0] < 1:
            raise ValueError(f"search: z must be [Q, {self.mu.shape[1]}], got {tuple(z.shape)}")
        if exclude is not None:
            exclude = exclude.to(self.mu.device, torch.long)
        return ops.latent_knn(z, self.mu, k, exclude=exclude)

    def neighbors(self, x, k, model, exclude_self=False):
        """``search`` around the encoder means of x under ``model``: x is a list of strings or of id tensors (bos first; any order), or a
        PaddedBatch; the answers are in the order of x.  ``exclude_self``: a query that is itself a corpus row (``dataset.lookup``: its
        lowest row with those tokens) does not answer with that row."""
        from .vocab import PaddedBatch, length_order
        self.dataset._check_model(model, "neighbors")
        if isinstance(x, PaddedBatch):
            mu, keys = model.encode(x)[0], x.x_pad
        else:
            keys = list(x)
            if not keys:
                raise ValueError("neighbors: needs at least one query")
            seqs = [model.string2tensor(s) if isinstance(s, str) else torch.as_tensor(s, dtype=torch.long).view(-1) for s in keys]
            order, perm = length_order(seqs, model.device)
            mu_sorted = model.encode([seqs[i] for i in order])[0]
            mu = torch.empty_like(mu_sorted)
            mu[perm] = mu_sorted
        exclude = self.dataset.lookup(keys) if exclude_self else None
        return self.search(mu, k, exclude=exclude)


def synthetic_smiles(n, seed=0, lo=20, hi=60, structured=True):
    """A stand-in corpus over the ZINC alphabet (no data set ships with the reference: .MISSING_LARGE_BLOBS).  structured: every string is
    a short random motif repeated to its length, so that a model can learn something in a few hundred steps (tests / examples);
    otherwise i.i.d. characters."""
    rs = np.random.RandomState(seed)
    alphabet = list("CNOSFcnos()=#123[]@H+-lBr")
    out = []
    for _ in range(n):
        ln = int(rs.randint(lo, hi))
        if structured:
            m = rs.choice(alphabet, size=int(rs.randint(3, 8)))
            out.append("".join(np.resize(m, ln)))
        else:
            out.append("".join(rs.choice(alphabet, size=ln)))
    return out


def formula_strings(formula, charge=None):
    """Molecular formulas in Hill notation from ``formula`` rows ([B, 11] counts per element of ``vocab.SMI_ELEMENTS``, hydrogens first; a
    tensor on either side, an ndarray or lists): carbon, hydrogen, then the other elements alphabetically -- all alphabetically when
    there is no carbon --, a count of 1 left out: ``C9H8O4``.  ``charge`` ([B], optional) appends the net charge: ``C4H12N+``,
    ``C2H3O2-``, beyond one ``(2+)`` / ``(2-)``.  An all-zero row (a row that is not ok) gives the empty string.  Waits for the device
    when given device tensors."""
    from .vocab import SMI_ELEMENTS
    f = np.asarray(formula.cpu() if torch.is_tensor(formula) else formula).reshape(-1, len(SMI_ELEMENTS))
    q = np.zeros(f.shape[0], np.int64) if charge is None else np.asarray(charge.cpu() if torch.is_tensor(charge) else charge).reshape(-1)
    if q.shape[0] != f.shape[0]:
        raise ValueError(f"formula_strings: {f.shape[0]} formulas, {q.shape[0]} charges")
    with_c = ["C", "H"] + sorted(e for e in SMI_ELEMENTS if e not in ("C", "H"))
    without_c = sorted(SMI_ELEMENTS)
    col = {e: i for i, e in enumerate(SMI_ELEMENTS)}
    out = []
    for row, c in zip(f.tolist(), q.tolist()):
        s = "".join(e + (str(row[col[e]]) if row[col[e]] > 1 else "") for e in (with_c if row[col["C"]] else without_c) if row[col[e]] > 0)
        if c:
            sign = "+" if c > 0 else "-"
            s += sign if abs(c) == 1 else f"({abs(c)}{sign})"
        out.append(s)
    return out


def randomized_smiles(strings, vocab, n, seed=0, device="cuda", return_status=False):
    """n randomised spellings of every string (SMILES enumeration): a list of n-lists, spelling j of string i drawn with draw = i * n + j
    (include/mvae.h, "SMILES rewrite"): the same graph under this library's walk, NOT canonical and not rdkit's doRandom.  A string that
    cannot be respelled comes back as it is, n times; ``return_status=True`` also returns the int32 [len(strings), n] statuses
    (ops.REWRITE_STATUS_NAMES).  One mvae_smiles_rewrite_rows launch on ``device``; ``device="cpu"`` asks for the host entry instead
    (the same source compiled for the CPU).  ValueError for a vocabulary of more than 64 ids, n < 1 or no strings."""
    from . import ops
    from .vocab import smiles_token_table, smiles_chem_table, smiles_emit_table
    strings, n = list(strings), int(n)
    if n < 1 or not strings:
        raise ValueError("randomized_smiles: needs at least one string and n >= 1")
    if len(vocab) > 64:
        raise ValueError(f"randomized_smiles: the vocabulary has {len(vocab)} ids, at most 64 are supported")
    dev = torch.device(device)
    ids = [vocab.string2ids(s, add_bos=True, add_eos=True) for s in strings for _ in range(n)]
    x = torch.full((len(ids), max(map(len, ids))), vocab.pad, dtype=torch.long)
    for b, row in enumerate(ids):
        x[b, :len(row)] = torch.as_tensor(row)
    tables = (smiles_token_table(vocab), smiles_chem_table(vocab), smiles_emit_table(vocab))
    if dev.type == "cpu":
        out, out_len, status = ops.smiles_rewrite_host(x, *tables, vocab.bos, vocab.eos, vocab.pad, seed)
    else:
        from .models import _require_cuda
        _require_cuda(dev, "data.randomized_smiles")
        out, out_len, status = ops.smiles_rewrite_rows(x.to(dev), *(t.to(dev) for t in tables), vocab.bos, vocab.eos, vocab.pad, seed)
    out, out_len, status = out.cpu().numpy(), out_len.cpu().numpy(), status.cpu().numpy()
    table = np.array([vocab.i2c[i] for i in range(len(vocab))], dtype=object)
    flat = [s if st else "".join(table[row[1:k - 1]]) for s, row, k, st in zip((s for s in strings for _ in range(n)), out, out_len, status)]
    res = [flat[i * n:(i + 1) * n] for i in range(len(strings))]
    return (res, status.reshape(len(strings), n)) if return_status else res


def canonical_smiles(strings, vocab, device="cuda", return_status=False):
    """The canonical spelling of every string (include/mvae.h, "SMILES canon"): a list of strings, equal for two spellings of one graph
    under this library's walk -- NOT rdkit's canonical SMILES: no aromaticity perception, no stereo.  A string that cannot be written
    comes back as it is; ``return_status=True`` also returns the int32 [len(strings)] statuses (ops.REWRITE_STATUS_NAMES).  One
    mvae_smiles_canon_rows launch on ``device``; ``device="cpu"`` asks for the host entry instead (the same source compiled for the
    CPU).  ValueError for a vocabulary of more than 64 ids or no strings."""
    from . import ops
    from .vocab import smiles_token_table, smiles_chem_table, smiles_emit_table
    strings = list(strings)
    if not strings:
        raise ValueError("canonical_smiles: needs at least one string")
    if len(vocab) > 64:
        raise ValueError(f"canonical_smiles: the vocabulary has {len(vocab)} ids, at most 64 are supported")
    dev = torch.device(device)
    ids = [vocab.string2ids(s, add_bos=True, add_eos=True) for s in strings]
    x = torch.full((len(ids), max(map(len, ids))), vocab.pad, dtype=torch.long)
    for b, row in enumerate(ids):
        x[b, :len(row)] = torch.as_tensor(row)
    tables = (smiles_token_table(vocab), smiles_chem_table(vocab), smiles_emit_table(vocab))
    if dev.type == "cpu":
        out, out_len, status, _, _ = ops.smiles_canon_host(x, *tables, vocab.bos, vocab.eos, vocab.pad, info=False, rank=False)
    else:
        from .models import _require_cuda
        _require_cuda(dev, "data.canonical_smiles")
        out, out_len, status, _, _ = ops.smiles_canon_rows(x.to(dev), *(t.to(dev) for t in tables), vocab.bos, vocab.eos, vocab.pad, info=False,
                                                           rank=False)
    out, out_len, status = out.cpu().numpy(), out_len.cpu().numpy(), status.cpu().numpy()
    table = np.array([vocab.i2c[i] for i in range(len(vocab))], dtype=object)
    res = [s if st else "".join(table[row[1:k - 1]]) for s, row, k, st in zip(strings, out, out_len, status)]
    return (res, status) if return_status else res


def normal_smiles(strings, vocab, device="cuda", return_status=False):
    """The aromatic normal form of every string (include/mvae.h, "Aromatic normal form"): a list of strings, equal for a Kekule spelling,
    an aromatic spelling and every respelling of one molecule -- aromaticity perceived by this library's own rule, then the spelling of
    ``canonical_smiles``; NOT rdkit's aromaticity model or canonical SMILES, no stereo.  A string that cannot be written comes back as it
    is; ``return_status=True`` also returns the int32 [len(strings)] statuses (ops.AROMATIZE_STATUS_NAMES: 7 = does not kekulise, 17 = a
    lower-case atom the rule does not find aromatic).  One mvae_smiles_aromatize_rows launch on ``device``; ``device="cpu"`` asks for the
    host entry instead (the same source compiled for the CPU).  ValueError for a vocabulary of more than 64 ids or no strings."""
    from . import ops
    from .vocab import smiles_token_table, smiles_chem_table, smiles_emit_table
    strings = list(strings)
    if not strings:
        raise ValueError("normal_smiles: needs at least one string")
    if len(vocab) > 64:
        raise ValueError(f"normal_smiles: the vocabulary has {len(vocab)} ids, at most 64 are supported")
    dev = torch.device(device)
    ids = [vocab.string2ids(s, add_bos=True, add_eos=True) for s in strings]
    x = torch.full((len(ids), max(map(len, ids))), vocab.pad, dtype=torch.long)
    for b, row in enumerate(ids):
        x[b, :len(row)] = torch.as_tensor(row)
    tables = (smiles_token_table(vocab), smiles_chem_table(vocab), smiles_emit_table(vocab))
    if dev.type == "cpu":
        out, out_len, status, _, _ = ops.smiles_aromatize_host(x, *tables, vocab.bos, vocab.eos, vocab.pad, info=False, arom=False)
    else:
        from .models import _require_cuda
        _require_cuda(dev, "data.normal_smiles")
        out, out_len, status, _, _ = ops.smiles_aromatize_rows(x.to(dev), *(t.to(dev) for t in tables), vocab.bos, vocab.eos, vocab.pad, info=False,
                                                           arom=False)
    out, out_len, status = out.cpu().numpy(), out_len.cpu().numpy(), status.cpu().numpy()
    table = np.array([vocab.i2c[i] for i in range(len(vocab))], dtype=object)
    res = [s if st else "".join(table[row[1:k - 1]]) for s, row, k, st in zip(strings, out, out_len, status)]
    return (res, status) if return_status else res


def selfies_from_smiles(strings, vocab, svocab, return_status=False):
    """Every SMILES string as SELFIES text in the symbols of `svocab` (a ``vocab.SelfiesVocab``), by the host entry
    mvae_selfies_encode_host (include/mvae.h, "SELFIES": Encode): "" for a string that cannot be encoded; ``return_status=True`` also
    returns the int32 statuses (ops.SELFIES_STATUS_NAMES).  This library's own encoding, NOT the selfies package's.  ValueError for a
    vocabulary of more than 64 ids or no strings."""
    from . import ops
    from .vocab import smiles_token_table, smiles_chem_table, smiles_emit_table, selfies_emit_table, token_rows
    strings = list(strings)
    if len(vocab) > 64 or len(svocab) > 64:
        raise ValueError("selfies_from_smiles: at most 64 ids are supported")
    x = token_rows(strings, lambda s: vocab.string2ids(s, add_bos=True, add_eos=True), vocab.pad, "selfies_from_smiles")
    out, out_len, status, _ = ops.selfies_encode_host(x, smiles_token_table(vocab), smiles_chem_table(vocab), smiles_emit_table(vocab), vocab.eos,
                                                      selfies_emit_table(svocab), svocab.bos, svocab.eos, svocab.pad, info=False)
    res = [svocab.ids2string(row[:k].tolist()) for row, k in zip(out, out_len.tolist())]
    return (res, status.numpy()) if return_status else res


def smiles_from_selfies(strings, svocab, vocab, return_status=False):
    """Every SELFIES text (symbols of `svocab`) as the canonical Kekule SMILES string of the molecule it denotes, by the host entry
    mvae_selfies_decode_host (include/mvae.h, "SELFIES"): "" for a row that cannot be written; ``return_status=True`` also returns the
    int32 statuses (ops.SELFIES_STATUS_NAMES).  This library's own derivation, NOT the selfies package's decoder.  ValueError for a
    vocabulary of more than 64 ids or no strings."""
    from . import ops
    from .vocab import smiles_emit_table, selfies_info_table, token_rows
    strings = list(strings)
    if len(vocab) > 64 or len(svocab) > 64:
        raise ValueError("smiles_from_selfies: at most 64 ids are supported")
    x = token_rows(strings, lambda s: svocab.string2ids(s, add_bos=True, add_eos=True), svocab.pad, "smiles_from_selfies")
    out, out_len, status, _ = ops.selfies_decode_host(x, selfies_info_table(svocab), smiles_emit_table(vocab), vocab.bos, vocab.eos, vocab.pad,
                                                      info=False)
    res = [vocab.ids2string(row[:k].tolist()) for row, k in zip(out, out_len.tolist())]
    return (res, status.numpy()) if return_status else res


def scaffold_smiles(strings, vocab, device="cuda", return_status=False):
    """The Murcko scaffold of every string as a string (include/mvae.h, "Scaffold SMILES"): the scaffold atoms of ``scaffolds``, every
    lost bond turned into hydrogens, in the spelling of ``canonical_smiles`` -- "" where there is no scaffold (no ring, a stereo token,
    a string the walk refuses).  NOT rdkit's MurckoScaffoldSmiles: nothing is sanitised, no aromaticity perception, no stereo.
    ``return_status=True`` also returns the int32 [len(strings)] statuses (ops.SCAFFOLD_SMILES_STATUS_NAMES).  One
    mvae_smiles_scaffold_smiles_rows launch on ``device``; ``device="cpu"`` asks for the host entry instead (the same source compiled
    for the CPU).  ValueError for a vocabulary of more than 64 ids or no strings."""
    from . import ops
    from .vocab import smiles_token_table, smiles_chem_table, smiles_emit_table
    strings = list(strings)
    if not strings:
        raise ValueError("scaffold_smiles: needs at least one string")
    if len(vocab) > 64:
        raise ValueError(f"scaffold_smiles: the vocabulary has {len(vocab)} ids, at most 64 are supported")
    dev = torch.device(device)
    ids = [vocab.string2ids(s, add_bos=True, add_eos=True) for s in strings]
    x = torch.full((len(ids), max(map(len, ids))), vocab.pad, dtype=torch.long)
    for b, row in enumerate(ids):
        x[b, :len(row)] = torch.as_tensor(row)
    tables = (smiles_token_table(vocab), smiles_chem_table(vocab), smiles_emit_table(vocab))
    if dev.type == "cpu":
        out, out_len, status, _ = ops.smiles_scaffold_smiles_host(x, *tables, vocab.bos, vocab.eos, vocab.pad, info=False)
    else:
        from .models import _require_cuda
        _require_cuda(dev, "data.scaffold_smiles")
        out, out_len, status, _ = ops.smiles_scaffold_smiles_rows(x.to(dev), *(t.to(dev) for t in tables), vocab.bos, vocab.eos, vocab.pad,
                                                                  info=False)
    out, out_len, status = out.cpu().numpy(), out_len.cpu().numpy(), status.cpu().numpy()
    table = np.array([vocab.i2c[i] for i in range(len(vocab))], dtype=object)
    res = ["".join(table[row[1:k - 1]]) for row, k in zip(out, out_len)]
    return (res, status) if return_status else res


def fragment_smiles(strings, vocab, device="cuda", return_status=False):
    """The fragments of every string as strings (include/mvae.h, "Fragments"): a list, per string, of its fragments in the order of their
    lowest atom, every lost bond turned into hydrogens, in the spelling of ``canonical_smiles`` -- [] for a string the walk refuses or
    one with a stereo token.  This library's own rule: NOT BRICS, not RECAP.  ``return_status=True`` also returns the int32
    [len(strings)] statuses of fragment 0 (ops.FRAGMENT_SMILES_STATUS_NAMES).  One mvae_smiles_fragment_rows launch for the counts and
    one mvae_smiles_fragment_smiles_rows launch per fragment number up to the largest count among the strings, on ``device``;
    ``device="cpu"`` asks for the host entries instead (the same source compiled for the CPU).  ValueError for a vocabulary of more
    than 64 ids or no strings."""
    from . import ops
    from .vocab import smiles_token_table, smiles_chem_table, smiles_emit_table
    strings = list(strings)
    if not strings:
        raise ValueError("fragment_smiles: needs at least one string")
    if len(vocab) > 64:
        raise ValueError(f"fragment_smiles: the vocabulary has {len(vocab)} ids, at most 64 are supported")
    dev = torch.device(device)
    ids = [vocab.string2ids(s, add_bos=True, add_eos=True) for s in strings]
    x = torch.full((len(ids), max(map(len, ids))), vocab.pad, dtype=torch.long)
    for b, row in enumerate(ids):
        x[b, :len(row)] = torch.as_tensor(row)
    tables = [smiles_token_table(vocab), smiles_chem_table(vocab), smiles_emit_table(vocab)]
    if dev.type == "cpu":
        count, write = ops.smiles_fragment_host, ops.smiles_fragment_smiles_host
    else:
        from .models import _require_cuda
        _require_cuda(dev, "data.fragment_smiles")
        count, write = ops.smiles_fragment_rows, ops.smiles_fragment_smiles_rows
        x, tables = x.to(dev), [t.to(dev) for t in tables]
    most = int(count(x, tables[0], tables[1], vocab.eos, mask=False)[2][:, 0].max())
    table = np.array([vocab.i2c[i] for i in range(len(vocab))], dtype=object)
    res, first = [[] for _ in strings], None
    for f in range(max(most, 1)):
        out, out_len, status, _ = write(x, *tables, vocab.bos, vocab.eos, vocab.pad, f, info=False)
        out, out_len, status = out.cpu().numpy(), out_len.cpu().numpy(), status.cpu().numpy()
        first = status if first is None else first
        for b in np.nonzero(status == 0)[0]:
            res[b].append("".join(table[out[b, 1:out_len[b] - 1]]))
    return (res, first) if return_status else res


class SubstructureTable:
    """Compiled substructure queries (``compile_substructures``): ``patterns`` (a tuple of strings), ``table`` (int32 [Q, 100], what the
    mvae_smiles_substruct entries take) and ``qstatus`` (int32 [Q], all 0), both on the host; ``on(device)`` is the table there,
    uploaded once per device."""

    def __init__(self, patterns, table, qstatus):
        self.patterns, self.table, self.qstatus = tuple(patterns), table, qstatus
        self._on = {}

    def __len__(self):
        return len(self.patterns)

    def on(self, device):
        device = torch.device(device)
        if device.type == "cpu":
            return self.table
        if device not in self._on:
            self._on[device] = self.table.to(device)
        return self._on[device]


def compile_substructures(patterns, vocab):
    """SMILES fragments compiled into a ``SubstructureTable`` for ``VAE.has_substructure``, ``MosesDeviceDataset.substructure_counts`` /
    ``rows_with_substructure`` and ``moses_generate(filters=)`` (include/mvae.h, "SMILES substructure"): 1 to 64 patterns in the model's
    vocabulary, each of at most 32 atoms, each a string the SMILES walk accepts -- or refuses only because an aromatic atom stands
    outside a ring, so that ``cC(=O)O`` is a pattern.  They are matched as graphs on (element, aromatic, charge) and bond classes: NOT
    SMARTS -- no wildcards, no recursive queries, no hydrogen counts -- and not rdkit's HasSubstructMatch.  Host only (one
    mvae_smiles_substruct_compile_host call).  ValueError naming the pattern and the reason for one that is refused (a character outside
    the vocabulary, ``ops.SUBSTRUCT_QSTATUS_NAMES``: syntax, valence, charge, ring_bond, too_long, stereo, query_atoms), for no patterns
    or more than 64, and for a vocabulary of more than 64 ids.  A ``SubstructureTable`` is returned as it is."""
    from . import ops
    from .vocab import smiles_token_table, smiles_chem_table, smiles_emit_table
    if isinstance(patterns, SubstructureTable):
        return patterns
    patterns = [patterns] if isinstance(patterns, str) else list(patterns)
    if not 1 <= len(patterns) <= ops.SUBSTRUCT_QUERIES:
        raise ValueError(f"compile_substructures: 1 to {ops.SUBSTRUCT_QUERIES} patterns, got {len(patterns)}")
    if len(vocab) > 64:
        raise ValueError(f"compile_substructures: the vocabulary has {len(vocab)} ids, at most 64 are supported")
    for p in patterns:
        missing = sorted({ch for ch in p if ch not in vocab.c2i})
        if missing:
            raise ValueError(f"compile_substructures: pattern {p!r}: {''.join(missing)!r} is not in the vocabulary")
    ids = [vocab.string2ids(p, add_bos=True, add_eos=True) for p in patterns]
    x = torch.full((len(ids), max(map(len, ids))), vocab.pad, dtype=torch.long)
    for b, row in enumerate(ids):
        x[b, :len(row)] = torch.as_tensor(row)
    table, qstatus = ops.smiles_substruct_compile(x, smiles_token_table(vocab), smiles_chem_table(vocab), smiles_emit_table(vocab), vocab.eos)
    for p, st in zip(patterns, qstatus.tolist()):
        if st:
            raise ValueError(f"compile_substructures: pattern {p!r} is refused: {ops.SUBSTRUCT_QSTATUS_NAMES[st]}")
    return SubstructureTable(patterns, table, qstatus)


def indices_to_smiles(idx, charset):
    """Rows of class indices -> strings, right-stripped of the padding character (train_sample.py:36: "".join(charset[i]).rstrip()).
    `charset`: id -> char (dict or list), the ``charset`` entry of the reference's checkpoints (train.py:174)."""
    arr = np.asarray(idx.detach().cpu() if hasattr(idx, "detach") else idx)
    if isinstance(charset, dict):
        table = np.array([charset[i] for i in range(len(charset))])
    else:
        table = np.array(list(charset))
    return ["".join(table[row]).rstrip() for row in arr]


def load_smiles(path, column=0):
    """.smi / headerless CSV: one molecule per line, SMILES in `column` (train.py:41 pd.read_csv(..., header=None))."""
    out = []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line:
                out.append(line.replace("\t", ",").split(",")[column].split()[0])
    return out


def save_encoded(path, indices_u8, vocab, max_len):
    chars = sorted(vocab, key=vocab.get)
    np.savez_compressed(path, indices=indices_u8, charset=np.array(chars), max_len=np.int64(max_len))


def load_encoded(path):
    z = np.load(path)
    chars = [str(c) for c in z["charset"]]
    return z["indices"], {ch: i for i, ch in enumerate(chars)}, int(z["max_len"])
