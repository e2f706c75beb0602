"""Character vocabulary of the MOSES path (behaviour of vocab.py:10-87 / mosesvocab.py:26-103).

Symbols are the sorted characters of the corpus followed by the four specials <bos>, <eos>, <pad>, <unk> (in that
order), so ids are reproducible.  ``OneHotVocab.vectors`` is the identity that initialises ``VAE.x_emb`` (mosesvae.py:48-50).
"""
import re

import torch


class SS:
    bos, eos, pad, unk = "<bos>", "<eos>", "<pad>", "<unk>"


class CharVocab:
    def __init__(self, chars, ss=SS):
        specials = [ss.bos, ss.eos, ss.pad, ss.unk]
        if any(sp in chars for sp in specials):
            raise ValueError("SS in chars")
        self.ss = ss
        symbols = sorted(chars) + specials
        self.c2i = dict(zip(symbols, range(len(symbols))))
        self.i2c = dict(enumerate(symbols))

    @classmethod
    def from_data(cls, data, *args, **kwargs):
        return cls(set().union(*map(set, data)) if data else set(), *args, **kwargs)

    def __len__(self):
        return len(self.c2i)

    bos = property(lambda self: self.c2i[self.ss.bos])
    eos = property(lambda self: self.c2i[self.ss.eos])
    pad = property(lambda self: self.c2i[self.ss.pad])
    unk = property(lambda self: self.c2i[self.ss.unk])

    def char2id(self, char):
        return self.c2i.get(char, self.unk)

    def id2char(self, id):
        return self.i2c.get(id, self.ss.unk)

    def string2ids(self, string, add_bos=False, add_eos=False):
        ids = [self.char2id(ch) for ch in string]
        return ([self.bos] if add_bos else []) + ids + ([self.eos] if add_eos else [])

    def ids2string(self, ids, rem_bos=True, rem_eos=True):
        ids = list(ids)
        if ids and rem_bos and ids[0] == self.bos:
            ids = ids[1:]
        if ids and rem_eos and ids[-1] == self.eos:
            ids = ids[:-1]
        return "".join(self.id2char(i) for i in ids)


class OneHotVocab(CharVocab):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.vectors = torch.eye(len(self.c2i))


def string2tensor(vocab, string):
    """moses_train_distrib.py:91-97: <bos> + ids + <eos>, int64."""
    return torch.tensor(vocab.string2ids(string, add_bos=True, add_eos=True), dtype=torch.long)


def get_collate_fn(vocab):
    """moses_train_distrib.py:127-135: sort the strings by length, longest first (stable), then tokenise."""
    def collate(data):
        data = sorted(data, key=len, reverse=True)
        return [string2tensor(vocab, s) for s in data]
    return collate


class PaddedBatch:
    """A collated batch already in the layout the kernels read: ``x_pad`` int64 [B, T] (pad-filled, rows sorted by length descending)
    and ``lengths`` int32 [B], both on the target device.  ``mosesvae.VAE.forward`` takes it in place of the list of per-sequence
    tensors: ONE host->device transfer per batch instead of the reference's one ``.cuda()`` per sequence (moses_train_distrib.py:271).
    ``rows`` (optional, int64 [B]): the corpus row behind each batch row, where the batch came from a corpus (data.MosesDeviceDataset)."""

    def __init__(self, x_pad, lengths, rows=None):
        self.x_pad, self.lengths, self.rows = x_pad, lengths, rows

    def __len__(self):
        return self.x_pad.shape[0]

    def to(self, device, non_blocking=True):
        return PaddedBatch(self.x_pad.to(device, non_blocking=non_blocking), self.lengths.to(device, non_blocking=non_blocking),
                           rows=None if self.rows is None else self.rows.to(device, non_blocking=non_blocking))

    def tensors(self):
        """The reference's representation (list of LongTensors) -- for code that still wants it."""
        return [self.x_pad[b, :int(n)] for b, n in enumerate(self.lengths.tolist())]


def pad_batch(tensors, pad):
    """list of LongTensors sorted by length descending -> PaddedBatch (on the tensors' device)."""
    lengths = [int(t.numel()) for t in tensors]
    if any(lengths[i] < lengths[i + 1] for i in range(len(lengths) - 1)):
        raise RuntimeError("sequences must be sorted by length in decreasing order (pack_sequence, mosesvae.py:151)")
    x_pad = torch.nn.utils.rnn.pad_sequence(list(tensors), batch_first=True, padding_value=pad)
    return PaddedBatch(x_pad, torch.tensor(lengths, dtype=torch.int32, device=x_pad.device))


def token_rows(x, to_ids, pad, who, device=None):
    """Token rows in, for every entry point that takes them: padded ids [B, T] (bos first), or a list of strings (to_ids(s): one string's
    ids, <bos> and <eos> included) and id tensors (bos first; flattened), padded with `pad` -> int64 [B, T] with unit column stride, on
    `device` (None: where it is).  ValueError with the caller's name `who` in front for an empty list and for anything but two
    dimensions."""
    if not torch.is_tensor(x):
        seqs = [torch.as_tensor(to_ids(s) if isinstance(s, str) else s, dtype=torch.long).view(-1) for s in x]
        if not seqs:
            raise ValueError(f"{who}: needs at least one row")
        x = torch.nn.utils.rnn.pad_sequence(seqs, batch_first=True, padding_value=pad)
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{who}: x must be [B, T], got {tuple(x.shape)}")
    x = x.to(device=device, dtype=torch.long)
    return x if x.stride(1) == 1 else x.contiguous()


def length_order(seqs, device):
    """The stable length-descending order the GRUs' packed layout wants (sequences of equal length keep their input order):
    (order as a list of indices into seqs, the same as an int64 tensor on `device`, to scatter the results back with)."""
    order = sorted(range(len(seqs)), key=lambda b: -int(seqs[b].numel()))
    return order, torch.tensor(order, dtype=torch.long, device=device)


def get_padded_collate_fn(vocab, pin_memory=False):
    """Like ``get_collate_fn`` but returns a PaddedBatch (host tensors, optionally pinned) ready for one asynchronous ``.to(device)``."""
    inner = get_collate_fn(vocab)

    def collate(data):
        b = pad_batch(inner(data), vocab.pad)
        if pin_memory:
            b = PaddedBatch(b.x_pad.pin_memory(), b.lengths.pin_memory())
        return b
    return collate


# token classes of the SMILES syntax automaton (include/mvae.h, "SMILES syntax"; csrc/smiles_syntax.hpp)
(SMI_OTHER, SMI_ATOM, SMI_TAIL, SMI_H, SMI_BOND, SMI_MINUS, SMI_PLUS, SMI_AT, SMI_DIGIT, SMI_LPAR, SMI_RPAR, SMI_LBRK, SMI_RBRK,
 SMI_EOS) = range(14)
_SMI_TAIL_HEAD = {"l": "C", "r": "B"}
_SMI_CLASS = {**{ch: SMI_ATOM for ch in "BCNOPSFIbcnops"}, **{ch: SMI_BOND for ch in "=#:/\\"}, **{ch: SMI_DIGIT for ch in "0123456789"},
              "l": SMI_TAIL, "r": SMI_TAIL, "H": SMI_H, "-": SMI_MINUS, "+": SMI_PLUS, "@": SMI_AT, "(": SMI_LPAR, ")": SMI_RPAR,
              "[": SMI_LBRK, "]": SMI_RBRK}


def smiles_token_table(vocab):
    """The per-token table of the SMILES syntax automaton for a CharVocab: int32 [V], one word per id -- bits 0-7 the class (SMI_*), bits
    8-15 for a tail ('l' of Cl, 'r' of Br) the id of its head character plus 1, bits 16-19 for a digit its value.  A tail whose head
    character the vocabulary lacks is OTHER (never allowed), and so are '(' / ')' and '[' / ']' unless both of the pair exist; <eos> is
    EOS, every other special and every unknown character OTHER.  ValueError when no atom token exists (nothing could be generated)."""
    c2i = vocab.c2i
    table = [SMI_OTHER] * len(vocab)
    for ch, i in c2i.items():
        cls = _SMI_CLASS.get(ch, SMI_OTHER)
        word = cls
        if cls == SMI_TAIL:
            head = c2i.get(_SMI_TAIL_HEAD[ch])
            word = SMI_OTHER if head is None else cls | (head + 1) << 8
        elif cls == SMI_DIGIT:
            word = cls | int(ch) << 16
        elif cls in (SMI_LPAR, SMI_RPAR) and not ("(" in c2i and ")" in c2i):
            word = SMI_OTHER
        elif cls in (SMI_LBRK, SMI_RBRK) and not ("[" in c2i and "]" in c2i):
            word = SMI_OTHER
        table[i] = word
    table[vocab.eos] = SMI_EOS
    if not any(w & 0xFF == SMI_ATOM for w in table):
        raise ValueError("smiles_token_table: the vocabulary has no atom token (one of B C N O P S F I b c n o p s)")
    return torch.tensor(table, dtype=torch.int32)


# the SMILES graph walk (include/mvae.h, "SMILES graph"; csrc/smiles_graph.hpp): the elements in formula order and their standard atomic weights
SMI_ELEMENTS = ("H", "B", "C", "N", "O", "F", "P", "S", "Cl", "Br", "I")
ATOMIC_WEIGHTS = (1.008, 10.81, 12.011, 14.007, 15.999, 18.998, 30.974, 32.06, 35.45, 79.904, 126.904)
SMI_AROMATIC = 1 << 4
_SMI_BOND_ORDER = {"=": 2, "#": 3, ":": 1, "/": 1, "\\": 1, "-": 1}
_SMI_TAIL_ELEMENT = {"l": "Cl", "r": "Br"}


def smiles_chem_table(vocab):
    """The per-token chemistry table of the SMILES graph walk for a CharVocab, beside ``smiles_token_table``: int32 [V], one word per id --
    bits 0-3 the element as an index into SMI_ELEMENTS (an atom token and 'H': the token's element; a tail: the element the pair spells,
    'l' Cl and 'r' Br), bit 4 set for a lower-case (aromatic) atom, bits 8-9 the bond order of a bond token and of '-' (= 2, # 3, every
    other 1).  Every other token has 0."""
    table = [0] * len(vocab)
    for ch, i in vocab.c2i.items():
        cls = _SMI_CLASS.get(ch, SMI_OTHER)
        if cls == SMI_ATOM:
            table[i] = SMI_ELEMENTS.index(ch.upper()) | (SMI_AROMATIC if ch.islower() else 0)
        elif cls == SMI_H:
            table[i] = SMI_ELEMENTS.index("H")
        elif cls == SMI_TAIL:
            table[i] = SMI_ELEMENTS.index(_SMI_TAIL_ELEMENT[ch])
        elif cls in (SMI_BOND, SMI_MINUS):
            table[i] = _SMI_BOND_ORDER[ch] << 8
    return torch.tensor(table, dtype=torch.int32)


# the SMILES rewrite (include/mvae.h, "SMILES rewrite"; csrc/smiles_rewrite.hip): the roles of the emit table
SMI_EMIT_WORDS = 48
SMI_EMIT_ALIPHATIC, SMI_EMIT_AROMATIC = 0, 11                      # + the element's index into SMI_ELEMENTS
_SMI_EMIT_ROLES = {22: "l", 23: "r", 24: "[", 25: "]", 26: "H", 27: "+", 28: "-", 29: "=", 30: "#", 31: "(", 32: ")",
                   **{33 + d: str(d) for d in range(10)}}
SMI_EMIT_STEREO = 43                                               # words 43 / 44: the low / high half of the stereo mask
_SMI_STEREO_CHARS = "@/\\"


def smiles_emit_table(vocab):
    """The table the SMILES rewrite writes its output from, beside ``smiles_token_table`` / ``smiles_chem_table``: int32 [48], one id per
    role -- [0 .. 10] the first character of element e in upper case (H B C N O F P S C B I: Cl and Br are written head plus tail),
    [11 .. 21] in lower case (b c n o p s; -1 for the rest), then 'l' 'r' '[' ']' 'H' '+' '-' '=' '#' '(' ')' and the digits 0 .. 9;
    -1 where the vocabulary lacks the character or ``smiles_token_table`` calls it OTHER (a lone parenthesis, a tail without its head).
    Words 43 / 44: the low / high 32 bits of the mask of the stereo tokens '@' '/' '\\' (bit i: id i).  ValueError for more than 64 ids."""
    if len(vocab) > 64:
        raise ValueError(f"smiles_emit_table: the vocabulary has {len(vocab)} ids, at most 64 are supported")
    usable = smiles_token_table(vocab)

    def role(ch):
        i = vocab.c2i.get(ch)
        return -1 if i is None or (int(usable[i]) & 0xFF) == SMI_OTHER else i
    table = [0] * SMI_EMIT_WORDS
    for e, sym in enumerate(SMI_ELEMENTS):
        table[SMI_EMIT_ALIPHATIC + e] = role(sym[0])
        table[SMI_EMIT_AROMATIC + e] = role(sym.lower()) if sym in ("B", "C", "N", "O", "P", "S") else -1
    for k, ch in _SMI_EMIT_ROLES.items():
        table[k] = role(ch)
    mask = sum(1 << vocab.c2i[ch] for ch in _SMI_STEREO_CHARS if ch in vocab.c2i)
    for k in range(2):
        half = (mask >> (32 * k)) & 0xFFFFFFFF
        table[SMI_EMIT_STEREO + k] = half - (1 << 32) if half >= 1 << 31 else half
    return torch.tensor(table, dtype=torch.int32)


# SELFIES (include/mvae.h, "SELFIES"; csrc/selfies.hpp): the symbol kinds of the info table and the roles of the emit table
(SELFIES_OTHER, SELFIES_ATOM, SELFIES_BRANCH, SELFIES_RING, SELFIES_NOP, SELFIES_EOS) = range(6)
SELFIES_EMIT_WORDS = 529
SELFIES_EMIT_BRANCH, SELFIES_EMIT_RING, SELFIES_EMIT_INDEX = 495, 504, 513
SELFIES_MAX_SYMBOLS = 60                                          # + the four specials = the 64 ids the sampling launches take
SELFIES_INDEX_SYMBOLS = ("[C]", "[Ring1]", "[Ring2]", "[Branch1]", "[=Branch1]", "[#Branch1]", "[Branch2]", "[=Branch2]", "[#Branch2]",
                         "[O]", "[N]", "[=N]", "[=C]", "[#C]", "[S]", "[P]")
_SELFIES_DEFAULT = SELFIES_INDEX_SYMBOLS + (
    "[=Ring1]", "[=Ring2]", "[nop]", "[F]", "[Cl]", "[Br]", "[I]", "[B]", "[=O]", "[=S]", "[#N]", "[=P]", "[=B]",
    "[N+1]", "[=N+1]", "[#N+1]", "[NH1+1]", "[=NH1+1]", "[NH2+1]", "[=NH2+1]", "[NH3+1]", "[N-1]", "[=N-1]", "[NH1-1]", "[NH1]", "[O-1]",
    "[O+1]", "[=O+1]", "[OH1+1]", "[S-1]", "[S+1]", "[=S+1]", "[SH1]", "[C-1]", "[#C-1]", "[CH1-1]", "[CH1]", "[=CH1]", "[CH2]", "[B-1]",
    "[PH1]", "[P+1]", "[=P+1]", "[H]")
_SELFIES_ATOM = re.compile(r"\[(=|#)?(Cl|Br|[HBCNOFPSI])(?:H([1-4]))?(?:([+-])1)?\]")
_SELFIES_STRUCT = re.compile(r"\[(=|#)?(Branch|Ring)([1-3])\]")
_SELFIES_SYMBOL = re.compile(r"\[[^\[\]]*\]")
# the largest valence by charge -1 / 0 / +1 (csrc/smiles_graph.hpp: VMAX_NEG, VMAX_0, VMAX_POS; None: no entry)
_SELFIES_VMAX = {"H": (0, 1, 0), "B": (4, 3, None), "C": (3, 4, 3), "N": (2, 3, 4), "O": (1, 2, 3), "F": (0, 1, None), "P": (2, 5, 4),
                 "S": (1, 6, 5), "Cl": (0, 1, None), "Br": (0, 1, None), "I": (0, 5, None)}


def selfies_symbol(symbol):
    """One SELFIES symbol as the definition reads it: a dict with kind and beta, for an atom element / charge / h / bracket / cap, for a
    branch or ring symbol L.  ValueError for a symbol that does not parse, whose (element, charge) has no valence entry, or whose
    capacity is below 1 (include/mvae.h, "SELFIES": Symbols, Capacity)."""
    if symbol == "[nop]":
        return {"kind": SELFIES_NOP, "beta": 1}
    m = _SELFIES_STRUCT.fullmatch(symbol)
    if m:
        return {"kind": SELFIES_BRANCH if m.group(2) == "Branch" else SELFIES_RING, "beta": {None: 1, "=": 2, "#": 3}[m.group(1)],
                "L": int(m.group(3))}
    m = _SELFIES_ATOM.fullmatch(symbol)
    if not m:
        raise ValueError(f"SelfiesVocab: {symbol!r} is no SELFIES symbol this library reads")
    el, h, chg = m.group(2), int(m.group(3) or 0), {None: 0, "+": 1, "-": -1}[m.group(4)]
    vmax = _SELFIES_VMAX[el][chg + 1]
    if vmax is None:
        raise ValueError(f"SelfiesVocab: {symbol!r}: no valence entry for {el} with charge {chg:+d}")
    cap = (1 if el == "I" and chg == 0 else vmax) - h
    if cap < 1:
        raise ValueError(f"SelfiesVocab: {symbol!r} has capacity {cap}: it could not be bonded to anything")
    return {"kind": SELFIES_ATOM, "beta": {None: 1, "=": 2, "#": 3}[m.group(1)], "element": SMI_ELEMENTS.index(el), "charge": chg, "h": h,
            "bracket": int(h > 0 or chg != 0 or el == "H"), "cap": cap}


class SelfiesVocab(OneHotVocab):
    """A vocabulary of SELFIES symbols: a CharVocab whose characters are private characters, one per symbol (U+00A1 onwards, in the sorted
    order of the symbols: single latin-1 bytes that no SMILES uses, so that ``tokenize_corpus`` takes ``encode_chars`` text), so that
    everything written for a CharVocab -- the models, the collate, the device corpus -- takes it as it is.
    ``string2ids`` takes SELFIES text and splits it at the brackets, ``ids2string`` returns SELFIES text; ``symbols`` is the sorted list.
    At most 60 symbols.  The reading of the symbols is this library's (include/mvae.h, "SELFIES"), NOT the selfies package's."""

    def __init__(self, symbols, ss=SS):
        symbols = sorted(set(symbols))
        if len(symbols) > SELFIES_MAX_SYMBOLS:
            raise ValueError(f"SelfiesVocab: {len(symbols)} symbols, at most {SELFIES_MAX_SYMBOLS} are supported")
        self.parsed = {s: selfies_symbol(s) for s in symbols}
        self.symbols = symbols
        self.sym2char = {s: chr(0xA1 + k) for k, s in enumerate(symbols)}
        self.char2sym = {c: s for s, c in self.sym2char.items()}
        super().__init__(set(self.sym2char.values()), ss)

    @classmethod
    def from_data(cls, data, *args, **kwargs):
        return cls({s for row in data for s in split_selfies(row)}, *args, **kwargs)

    @classmethod
    def default(cls):
        """A fixed alphabet: the 16 index symbols, [=Ring1], [=Ring2], [nop], and C N O F S P Cl Br I B with the common charged and
        hydrogen forms."""
        return cls(_SELFIES_DEFAULT)

    @staticmethod
    def split(string):
        return split_selfies(string)

    def symbol2id(self, symbol):
        return self.c2i.get(self.sym2char.get(symbol), self.unk)

    def id2symbol(self, id):
        ch = self.i2c.get(id, self.ss.unk)
        return self.char2sym.get(ch, ch)

    def encode_chars(self, string):
        """SELFIES text as the string of private characters a CharVocab-based corpus holds."""
        return "".join(self.sym2char.get(s, "\xa0") for s in split_selfies(string))

    def string2ids(self, string, add_bos=False, add_eos=False):
        ids = [self.symbol2id(s) for s in split_selfies(string)]
        return ([self.bos] if add_bos else []) + ids + ([self.eos] if add_eos else [])

    def ids2string(self, ids, rem_bos=True, rem_eos=True):
        ids = list(ids)
        if ids and rem_bos and ids[0] == self.bos:
            ids = ids[1:]
        if ids and rem_eos and ids[-1] == self.eos:
            ids = ids[:-1]
        return "".join(self.id2symbol(int(i)) for i in ids)


def split_selfies(string):
    """The symbols of SELFIES text.  ValueError for text outside brackets."""
    symbols = _SELFIES_SYMBOL.findall(string)
    if sum(map(len, symbols)) != len(string):
        raise ValueError(f"split_selfies: {string!r} has text outside [...]")
    return symbols


def selfies_info_table(vocab):
    """The decode table of a SelfiesVocab: int32 [V], one word per id -- bits 0-2 the kind (SELFIES_*), 3-4 beta; an atom: 5-8 the element
    (index into SMI_ELEMENTS), 9-10 the charge + 1, 11 bracket atom, 12-14 the stated hydrogens; a branch or ring symbol: 16-17 L; bits
    20-23 the index value of the symbol.  <eos> is SELFIES_EOS, the other specials SELFIES_OTHER."""
    table = [SELFIES_OTHER] * len(vocab)
    for sym, p in vocab.parsed.items():
        word = p["kind"] | p["beta"] << 3
        if p["kind"] == SELFIES_ATOM:
            word |= p["element"] << 5 | (p["charge"] + 1) << 9 | p["bracket"] << 11 | p["h"] << 12
        elif p["kind"] in (SELFIES_BRANCH, SELFIES_RING):
            word |= p["L"] << 16
        if sym in SELFIES_INDEX_SYMBOLS:
            word |= SELFIES_INDEX_SYMBOLS.index(sym) << 20
        table[vocab.symbol2id(sym)] = word
    table[vocab.eos] = SELFIES_EOS
    return torch.tensor(table, dtype=torch.int32)


def selfies_emit_table(vocab):
    """The encode table of a SelfiesVocab: int32 [529], role -> id, -1 where the vocabulary lacks the symbol -- the atom symbol of (beta,
    element, charge, hydrogens) at (((beta - 1) * 11 + element) * 3 + charge + 1) * 5 + hydrogens, [bBranchL] at 495 + (beta - 1) * 3 +
    L - 1, [bRingL] at 504 + the same, the symbol of index value v at 513 + v."""
    table = [-1] * SELFIES_EMIT_WORDS
    for sym, p in vocab.parsed.items():
        i = vocab.symbol2id(sym)
        if p["kind"] == SELFIES_ATOM:
            table[(((p["beta"] - 1) * 11 + p["element"]) * 3 + p["charge"] + 1) * 5 + p["h"]] = i
        elif p["kind"] in (SELFIES_BRANCH, SELFIES_RING):
            table[(SELFIES_EMIT_BRANCH if p["kind"] == SELFIES_BRANCH else SELFIES_EMIT_RING) + (p["beta"] - 1) * 3 + p["L"] - 1] = i
        if sym in SELFIES_INDEX_SYMBOLS:
            table[SELFIES_EMIT_INDEX + SELFIES_INDEX_SYMBOLS.index(sym)] = i
    return torch.tensor(table, dtype=torch.int32)
