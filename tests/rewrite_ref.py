"""Reference for the SMILES rewrite (mvae_smiles_rewrite_rows / _corpus / _host): pure Python on strings, written from the rules of
include/mvae.h ("SMILES rewrite") and NOT from the kernel's method --

  the string is cut into tokens by chem_ref's regular expressions and the molecule is chem_ref's adjacency structure (a dict of
  neighbour -> bond order per atom); whether the walk accepts the row at all is chem_ref.analyse's business;
  the traversal and the emission are two plain recursions over that structure: no stacks, no half-edge list, no packed words;
  the open ring digits are a dict, the refusals are exceptions raised where the rules name them.

`respell(s, seed, draw)` returns (status, string): the new spelling for status 0, the input for every refusal.  `broken=` selects one of
the deliberately wrong writers the tests use to show that their round-trip checks can fail."""
import numpy as np

import chem_ref as CR

STEREO, RING_MULTI, RING_DIGITS, DEPTH, LONG, NO_TOKEN = range(8, 14)
BROKEN = ("dropped_double", "digit_reused", "lost_h", "no_parentheses", "wrong_ancestor")
M32 = 0xFFFFFFFF


def mix(h):
    h ^= h >> 16
    h = h * 0x85EBCA6B & M32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M32
    h ^= h >> 16
    return h


def prio(seed, draw, a):
    return mix(mix((seed * 0x9E3779B1 + draw) & M32) ^ (a * 0x85EBCA6B & M32))


def atoms_of(s):
    """chem_ref's adjacency structure of a string analyse() calls OK: a list of {"el", "arom", "bracket", "chg", "h", "nb": {atom: order}}."""
    atoms, stack, ring_open = [], [], {}
    cur, order = None, 1
    for m in CR._TOKEN.finditer(s):
        kind, text = m.lastgroup, m.group()
        if kind in ("atom", "bracket"):
            if kind == "atom":
                a = {"el": text if len(text) == 2 else text.upper(), "arom": text.islower(), "bracket": False, "chg": 0, "h": 0, "nb": {}}
            else:
                b = CR._BRACKET.fullmatch(text)
                sym, h, chg = b.group("sym"), b.group("h"), b.group("chg")
                a = {"el": sym if sym in ("Cl", "Br", "H") else sym.upper(), "arom": sym.islower(), "bracket": True,
                     "chg": 0 if not chg else (1 if chg[0] == "+" else -1) * (int(chg[1]) if len(chg) == 2 else 1),
                     "h": 0 if not h else (1 if len(h) == 1 else int(h[1])), "nb": {}}
            atoms.append(a)
            k = len(atoms) - 1
            if cur is not None:
                a["nb"][cur] = atoms[cur]["nb"][k] = order
            cur, order = k, 1
        elif kind == "bond":
            order = CR.BOND_ORDER[text]
        elif kind == "open":
            stack.append(cur)
        elif kind == "close":
            cur = stack.pop()
        elif text not in ring_open:
            ring_open[text] = cur
        else:
            i = ring_open.pop(text)
            atoms[cur]["nb"][i] = atoms[i]["nb"][cur] = 1
    return atoms


class Refused(Exception):
    pass


def respell(s, seed=0, draw=0, max_content=127, have=None, broken=None):
    """(status, spelling) of string s under (seed, draw).  have: the characters the vocabulary can write (None: all)."""
    status = CR.analyse(s)[0]
    if status != CR.OK:
        return status, s
    if any(ch in s for ch in "@/\\"):
        return STEREO, s
    atoms = atoms_of(s)
    key = lambda a: (prio(seed, draw, a), a)
    root = min(range(len(atoms)), key=key)
    index, parent, children, closures = {}, {root: None}, {}, []          # closures: (ancestor, descendant)
    multi = []

    def search(a):
        index[a] = len(index)
        children[a] = []
        nb = atoms[a]["nb"]
        for b in sorted((b for b in nb if b != parent[a]), key=lambda b: (nb[b] < 2, key(b))):
            if b not in index:
                parent[b] = a
                children[a].append(b)
                search(b)
            elif index[b] < index[a]:
                closures.append((b, a))
                if nb[b] != 1:
                    multi.append((b, a))
    search(root)
    if multi:
        return RING_MULTI, s
    if broken == "wrong_ancestor":
        closures = [(parent[i] if parent[i] is not None and parent[i] not in atoms[j]["nb"] else i, j) for i, j in closures]
    out, digit_of, depth = [], {}, [0]

    def put(ch):
        for c in ch:
            if have is not None and c not in have:
                raise Refused(NO_TOKEN)
            if len(out) >= max_content:
                raise Refused(LONG)
            out.append(c)

    def write(a):
        at = atoms[a]
        if parent[a] is not None and at["nb"][parent[a]] >= 2 and broken != "dropped_double":
            put("=" if at["nb"][parent[a]] == 2 else "#")
        sym = at["el"].lower() if at["arom"] else at["el"]
        if at["bracket"]:
            h = 0 if broken == "lost_h" else at["h"]
            put("[" + sym + ("H" if h >= 1 else "") + (str(h) if h >= 2 else "") + {0: "", 1: "+", -1: "-"}[at["chg"]] + "]")
        else:
            put(sym)
        here = set()
        for d in sorted(d for d, c in digit_of.items() if c[1] == a):
            put(str(d))
            here.add(d)
            del digit_of[d]
        for c in sorted((c for c in closures if c[0] == a), key=lambda c: index[c[1]]):
            free = [d for d in (1, 2, 3, 4, 5, 6, 7, 8, 9, 0) if d not in digit_of and (d not in here or broken == "digit_reused")]
            if not free:
                raise Refused(RING_DIGITS)
            digit_of[free[0]] = c
            here.add(free[0])
            put(str(free[0]))
        for k, b in enumerate(children[a]):
            if k + 1 < len(children[a]) and broken != "no_parentheses":
                if depth[0] >= 15:
                    raise Refused(DEPTH)
                depth[0] += 1
                put("(")
                write(b)
                put(")")
                depth[0] -= 1
            else:
                write(b)
    try:
        write(root)
    except Refused as r:
        return r.args[0], s
    return CR.OK, "".join(out)


def expected(strings, seed, draws, max_content=127, have=None):
    """respell() of every string with its draw: (status int32 [B], list of spellings)."""
    res = [respell(s, seed, int(d), max_content, have) for s, d in zip(strings, draws)]
    return np.array([r[0] for r in res], np.int32), [r[1] for r in res]


HAND_ROWS = [
    "C1CCC2CCCCC2C1", "c1ccc2ccccc2c1", "C1CCC2(CC1)CCCC2", "C1CC2(C1)CC2", "c1ccc2c(c1)Cc1ccccc12",      # fused and spiro rings
    "C12C3C4C1C5C2C3C45",                                                                              # cubane: every atom on three rings
    "c1cc[nH]c1", "[NH4+]", "[CH4]", "[N+1](C)(C)(C)C", "[H]C", "[C]", "[O-]C(=O)C", "C[S+](C)C", "[Cl-]", "[nH]1cccc1",
    "ClCCBr", "Clc1ccc(Br)cc1", "BrC(Cl)(Cl)I",
    "C1=C=CCCC1", "O=S1(=O)CCCC1", "C1=CC=CC=C1", "N#CC#N", "C=C=C",
    "C" * 127,                                                                                          # 127 atoms
    "C(C)" * 31 + "CCC",                                                                                # 127 tokens, 65 atoms
    "C1CC1" * 25 + "CC",                                                                                # 127 tokens, 25 rings
]
assert len(HAND_ROWS[-1]) == len(HAND_ROWS[-2]) == len(HAND_ROWS[-3]) == 127

# fragments any concatenation of which the walk accepts: each starts at an atom with a free valence and leaves one on its last atom
FRAGMENTS = ("C", "CC", "C(C)", "C(=O)", "N", "O", "C(F)", "C(Cl)", "S(=O)(=O)", "c1ccc(cc1)", "C1CCN(CC1)", "C(C#N)", "N(C)", "C=C",
             "c1ccc2ccccc2c1", "c1cc[nH]c1C", "C(Br)", "c1ccncc1C", "C1CC1C", "C[N+](C)(C)C", "C(C(=O)[O-])")


def fragment_corpus(n, seed=0, lo=30, hi=52):
    """n strings the walk gives status 0 (checked with chem_ref.analyse), lengths in [lo, hi) like MOSES': random concatenations of
    FRAGMENTS, each ending in a carbon.  Chemistry is not the point -- only valence matters to the walk."""
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        want, s = int(rs.randint(lo, hi)), ""
        while len(s) < want - 1:
            f = FRAGMENTS[int(rs.randint(len(FRAGMENTS)))]
            if len(s) + len(f) < hi - 1:
                s += f
            elif len(s) >= lo - 1:
                break
        s += "C"
        if CR.analyse(s)[0] == CR.OK:
            out.append(s)
    return out
