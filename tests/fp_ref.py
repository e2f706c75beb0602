"""Reference for the fingerprint feature (mvae_smiles_fp_rows / _corpus / _host, mvae_tanimoto_knn, mvae_tanimoto_sum): pure Python on
strings, written from the definition in include/mvae.h ("Circular fingerprint", "Tanimoto similarity") and NOT from the kernel's method --

  the molecule is an adjacency structure of its own (a dict of neighbour -> bond order per atom), built with chem_ref's token and
  bracket expressions and bond orders; every atom sums over its neighbours, where the kernel walks an edge list;
  ring membership is chem_ref._ring_atoms (non-bridge edges, a low-link search), never a walk along predecessors;
  the status is chem_ref.analyse's.

`fingerprint(s)` returns the 16 int64 words of one string (zeros unless the status is 0).  The numpy side: `similarity` (the f32 matrix,
one division per pair), `knn` (ordered by similarity descending, row ascending), `pair_sum` (float64), and `check_knn`."""
import numpy as np

import chem_ref as CR

WORDS = 16
MASK = 0xFFFFFFFF


def mix(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & MASK
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & MASK
    h ^= h >> 16
    return h


def molecule(s):
    """The atoms of a string chem_ref.analyse calls OK, each {"el", "arom", "chg", "h", "nb": {neighbour: order}}."""
    atoms, stack, ring_open = [], [], {}
    cur, order = None, 1

    def add(el, arom, chg, h):
        atoms.append({"el": el, "arom": arom, "chg": chg, "h": h, "nb": {}})
        k = len(atoms) - 1
        if cur is not None:
            atoms[k]["nb"][cur] = atoms[cur]["nb"][k] = order
        return k

    for m in CR._TOKEN.finditer(s):
        kind, text = m.lastgroup, m.group()
        if kind == "atom":
            cur, order = add(text if len(text) == 2 else text.upper(), text.islower(), 0, 0), 1
        elif kind == "bracket":
            b = CR._BRACKET.fullmatch(text)
            sym, h, chg = b.group("sym"), b.group("h"), b.group("chg")
            h = 0 if not h else (1 if len(h) == 1 else int(h[1]))
            chg = 0 if not chg else (1 if chg[0] == "+" else -1) * (int(chg[1]) if len(chg) == 2 else 1)
            cur, order = add(sym if sym in ("Cl", "Br", "H") else sym.upper(), sym.islower(), chg, h), 1
        elif kind == "bond":
            order = CR.BOND_ORDER[text]
        elif kind == "open":
            stack.append(cur)
        elif kind == "close":
            cur = stack.pop()
        elif kind == "digit":
            if text not in ring_open:
                ring_open[text] = cur
            else:
                i = ring_open.pop(text)
                atoms[cur]["nb"][i] = atoms[i]["nb"][cur] = 1          # ring-closure bonds are order 1
    return atoms


def bits(s):
    """The set of bit numbers of a string (empty unless its status is 0)."""
    if CR.analyse(s)[0] != CR.OK:
        return set()
    atoms = molecule(s)
    members = CR._ring_atoms(atoms)
    ids = []
    for k, a in enumerate(atoms):
        used = a["h"] + sum(a["nb"].values())
        w = CR.ELEMENTS.index(a["el"]) | int(a["arom"]) << 4 | (a["chg"] + 1) << 5 | int(k in members) << 7 | len(a["nb"]) << 8 | used << 12
        ids.append(mix(w))
    out = {i & 1023 for i in ids}
    for r in (1, 2):
        nxt = []
        for k, a in enumerate(atoms):
            total = 0
            for j, order in a["nb"].items():
                bt = 4 if order == 1 and a["arom"] and atoms[j]["arom"] else order
                total += mix(ids[j] ^ ((bt * 0x7FEB352D) & MASK))
            nxt.append(mix((ids[k] * 0x9E3779B1 + r + total) & MASK))
        ids = nxt
        out.update(i & 1023 for i in ids)
    return out


def fingerprint(s):
    words = np.zeros(WORDS, np.uint64)
    for b in bits(s):
        words[b >> 6] |= np.uint64(1) << np.uint64(b & 63)
    return words.view(np.int64)


def fingerprints(strings):
    return np.stack([fingerprint(s) for s in strings]) if len(strings) else np.zeros((0, WORDS), np.int64)


_CACHE = {}


def corpus_fingerprints():
    """(strings, status, fp [n, 16] int64) of chem_ref's mutation corpus, computed once per process and shared: callers leave it unchanged."""
    if "c" not in _CACHE:
        strings, want = CR.corpus_and_expected()
        _CACHE["c"] = (strings, want[0], fingerprints(strings))
    return _CACHE["c"]


# ------------------------------------------------------------------------------------------------ Tanimoto, in numpy
def _unpacked(fp):
    fp = np.ascontiguousarray(fp, dtype=np.int64)
    return np.unpackbits(fp.view(np.uint8).reshape(fp.shape[0], -1), axis=1).astype(np.float32)      # counts <= 1024 are exact in f32


def similarity(a, b):
    """float32 [M, N]: |a & b| / |a | b| as ONE f32 division of the two integers, 0 where the union is empty."""
    ua, ub = _unpacked(a), _unpacked(b)
    c = ua @ ub.T
    u = ua.sum(1)[:, None] + ub.sum(1)[None, :] - c
    assert c.dtype == u.dtype == np.float32
    out = np.zeros_like(c)
    np.divide(c, u, out=out, where=u > 0)
    return out


def knn(sim, k, exclude=None):
    """(sim [Q, k] f32, rows [Q, k] i64) of a similarity matrix: ordered by (similarity descending, row ascending), the row exclude[i]
    skipped (-1: none), a short tail (-1.0, -1)."""
    Q, N = sim.shape
    out_s, out_j = np.full((Q, k), -1.0, np.float32), np.full((Q, k), -1, np.int64)
    for i in range(Q):
        order = np.argsort(-sim[i], kind="stable")                     # stable: equal similarities keep ascending rows
        if exclude is not None and exclude[i] >= 0:
            order = order[order != exclude[i]]
        order = order[:k]
        out_s[i, :order.size], out_j[i, :order.size] = sim[i, order], order
    return out_s, out_j


def check_knn(got_sim, got_idx, want_sim, want_idx):
    """Exact equality of (similarity bits, row)."""
    got_sim, got_idx = np.asarray(got_sim), np.asarray(got_idx)
    assert got_sim.dtype == np.float32 and got_idx.dtype == np.int64 and got_sim.shape == want_sim.shape == got_idx.shape == want_idx.shape
    bad = np.nonzero((got_sim.view(np.int32) != want_sim.view(np.int32)) | (got_idx != want_idx))
    assert bad[0].size == 0, [(int(i), int(r), float(got_sim[i, r]), int(got_idx[i, r]), float(want_sim[i, r]), int(want_idx[i, r]))
                              for i, r in zip(bad[0][:5], bad[1][:5])]


def ties_at(sim, k, exclude=None):
    """How many queries have equal similarity at ranks k and k + 1 (1-based) of their eligible rows."""
    s, _ = knn(sim, k + 1, exclude)
    return int(((s[:, k - 1] == s[:, k]) & (s[:, k] >= 0)).sum())


def pair_sum(sim, skip_diagonal=False):
    """The float64 sum of the f32 similarities, the pairs i == j left out on request."""
    s = sim.astype(np.float64)
    if skip_diagonal:
        n = min(s.shape)
        s[np.arange(n), np.arange(n)] = 0.0
    return float(s.sum())
