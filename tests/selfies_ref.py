"""Reference for the SELFIES feature (mvae_selfies_decode_* / mvae_selfies_encode_*, vocab.SelfiesVocab): pure Python on strings, written
from the rules of include/mvae.h ("SELFIES") and NOT from the kernel's method --

  a symbol is read by a regular expression of this file's own, its capacity comes from chem_ref's valence SETS;
  the derivation is a plain recursion over lists of symbols (a branch is a slice of the list it stands in), with the molecule as
  chem_ref's adjacency structure (a dict of neighbour -> bond order per atom): no stack, no packed words, no predecessor array, and
  NO re-parenting -- a multiple ring bond is simply a bond of the dict;
  `spell(atoms)` is a naive SMILES writer of that structure (a depth-first search, multiple bonds first, from the first root that
  leaves no ring closure in need of an order); the tests compare graphs by sending its string through ops.smiles_canon_host;
  the encoder is a plain recursion over the tree the SMILES string spells, with the Kekule bonds from a matching the caller supplies
  (the definition says "the matching of Kekulisation": the tests take the kekule entry's, which test_kekule_host checks).

`derive(symbols)` returns (status, atoms, notes); notes counts what the round-trip test wants to know: branches and rings skipped,
chains that ended with symbols left, and the ring bonds that stayed bonds of their own with their final orders."""
import re

import chem_ref as CR

SYNTAX, KEKULE, STEREO, RING_MULTI, LONG, NO_TOKEN, CAPACITY = 1, 7, 8, 9, 12, 13, 18
INDEX = ["[C]", "[Ring1]", "[Ring2]", "[Branch1]", "[=Branch1]", "[#Branch1]", "[Branch2]", "[=Branch2]", "[#Branch2]", "[O]", "[N]", "[=N]",
         "[=C]", "[#C]", "[S]", "[P]"]
_ATOM = re.compile(r"\[(?P<b>[=#]?)(?P<el>Cl|Br|[HBCNOFPSI])(?:H(?P<h>[1-4]))?(?:(?P<sign>[+-])1)?\]")
_STRUCT = re.compile(r"\[(?P<b>[=#]?)(?P<what>Branch|Ring)(?P<L>[1-3])\]")
_BETA = {"": 1, "=": 2, "#": 3}


def split(text):
    return re.findall(r"\[[^\[\]]*\]|<[a-z]+>", text)


def capacity(el, chg, h):
    allowed = CR.VALENCES[el][chg + 1]
    if allowed is None:
        return None
    return (1 if el == "I" and chg == 0 else max(allowed)) - h


def read(symbol):
    """("atom", beta, el, chg, h, cap) / ("branch" | "ring", beta, L) / ("nop",) / None for anything that is no symbol."""
    if symbol == "[nop]":
        return ("nop",)
    m = _STRUCT.fullmatch(symbol)
    if m:
        return (m.group("what").lower(), _BETA[m.group("b")], int(m.group("L")))
    m = _ATOM.fullmatch(symbol)
    if not m:
        return None
    el, h, chg = m.group("el"), int(m.group("h") or 0), {None: 0, "+": 1, "-": -1}[m.group("sign")]
    cap = capacity(el, chg, h)
    return None if cap is None or cap < 1 else ("atom", _BETA[m.group("b")], el, chg, h, cap)


def index_of(symbols, L):
    q = 0
    for i in range(L):
        q = 16 * q + (INDEX.index(symbols[i]) if i < len(symbols) and symbols[i] in INDEX else 0)
    return q


def derive(symbols):
    """The derivation of a list of symbols (the content of a row: no <bos>, nothing behind <eos>)."""
    notes = {"skipped": 0, "early": 0, "ring_orders": []}
    if len(symbols) > 127:
        return SYNTAX, [], notes
    if any(read(s) is None for s in symbols):
        return SYNTAX, [], notes
    atoms, caps, rings = [], [], []

    def chain(syms, s, prev):
        i = 0
        while i < len(syms):
            r = read(syms[i])
            i += 1
            if r[0] == "atom":
                _, beta, el, chg, h, cap = r
                o = 0 if s == 0 else min(beta, s, cap)
                atoms.append({"el": el, "arom": False, "bracket": h > 0 or chg != 0 or el == "H", "chg": chg, "h": h, "nb": {}})
                caps.append(cap)
                k = len(atoms) - 1
                if prev is not None:
                    atoms[k]["nb"][prev] = atoms[prev]["nb"][k] = o
                prev, s = k, cap - o
                if s == 0:
                    notes["early"] += i < len(syms)
                    return
            elif r[0] == "branch":
                _, beta, L = r
                if s <= 1:
                    notes["skipped"] += 1
                    continue
                b = min(s - 1, beta)
                q = index_of(syms[i:], L)
                i = min(i + L, len(syms))
                chain(syms[i:i + q + 1], b, prev)
                i = min(i + q + 1, len(syms))
                s -= b
            elif r[0] == "ring":
                _, beta, L = r
                if s == 0:
                    notes["skipped"] += 1
                    continue
                o = min(beta, s)
                q = index_of(syms[i:], L)
                i = min(i + L, len(syms))
                rings.append((max(0, prev - (q + 1)), prev, o))
                s -= o
                if s == 0:
                    notes["early"] += i < len(syms)
                    return

    chain(list(symbols), 0, None)
    if not atoms:
        return SYNTAX, [], notes
    own = {}
    for l, r, o in rings:
        if l == r:
            continue
        o = min(o, caps[l] - sum(atoms[l]["nb"].values()), caps[r] - sum(atoms[r]["nb"].values()))
        if o <= 0:
            continue
        have = atoms[l]["nb"].get(r, 0)
        add = min(o, 3 - have) if have else o
        atoms[l]["nb"][r] = atoms[r]["nb"][l] = have + add
        if not have or (l, r) in own:
            own[l, r] = have + add
    notes["ring_orders"] = list(own.values())
    return 0, atoms, notes


def atom_text(a):
    if not a["bracket"]:
        return a["el"]
    return "[" + a["el"] + ("H" + (str(a["h"]) if a["h"] > 1 else "") if a["h"] else "") + {0: "", 1: "+", -1: "-"}[a["chg"]] + "]"


def spell(atoms):
    """A SMILES string of the adjacency structure: the first root, in atom order, from which the depth-first search (multiple bonds
    first) leaves no multiple bond as a ring closure and never needs more than ten ring digits at once; None if no root does."""
    for root in range(len(atoms)):
        s = spell_from(atoms, root)
        if s is not None:
            return s
    return None


def spell_from(atoms, root):
    n = len(atoms)
    parent, kids, back, seen = {root: None}, {a: [] for a in range(n)}, {a: [] for a in range(n)}, set()

    def visit(u):
        seen.add(u)
        for v in sorted(atoms[u]["nb"], key=lambda v: (-(atoms[u]["nb"][v] >= 2), v)):
            if v == parent[u]:
                continue
            if v not in seen:
                parent[v] = u
                kids[u].append(v)
                visit(v)
            elif u not in back[v]:
                back[u].append(v)
                back[v].append(u)
    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 2000))
    visit(root)
    if len(seen) != n or any(atoms[u]["nb"][v] >= 2 for u in back for v in back[u]):
        return None
    out, free, digit, written = [], list("1234567890"), {}, set()

    def write(u):
        p = parent[u]
        if p is not None and atoms[u]["nb"][p] >= 2:
            out.append("=" if atoms[u]["nb"][p] == 2 else "#")
        out.append(atom_text(atoms[u]))
        written.add(u)
        closed = [digit.pop(frozenset((u, v))) for v in back[u] if v in written]
        out.extend(closed)
        for v in back[u]:
            if v not in written:
                if not free:
                    return False
                digit[frozenset((u, v))] = free.pop(0)
                out.append(digit[frozenset((u, v))])
        free.extend(closed)
        for i, v in enumerate(kids[u]):
            last = i == len(kids[u]) - 1
            out.append("" if last else "(")
            if not write(v):
                return False
            out.append("" if last else ")")
        return True
    return "".join(out) if write(root) else None


# ------------------------------------------------------------------------------------------------------------------------ encode
def tree(s):
    """A string chem_ref.analyse calls OK as (atoms, pred, closures): chem_ref's adjacency structure in string order, the atom every
    atom was bonded to when it was written, and the ring-closure pairs (earlier, later)."""
    atoms, pred, closures, stack, ring_open = [], [], [], [], {}
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
            pred.append(cur)
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
            closures.append((i, cur))
    return atoms, pred, closures


def index_symbols(q):
    return ([INDEX[q >> 4]] if q >= 16 else []) + [INDEX[q & 15]]


def encode(s, mate=None, have=None, max_content=127):
    """(status, SELFIES text) of a SMILES string.  mate: the mates of the atoms of the set N of "Kekulisation" (atom -> atom), needed for a
    string with lower-case atoms; have: the symbols the vocabulary holds (None: every one)."""
    status = CR.analyse(s)[0]
    if status != CR.OK:
        return status, ""
    if any(ch in s for ch in "@/\\"):
        return STEREO, ""
    atoms, pred, closures = tree(s)
    if any(a["arom"] for a in atoms):
        if mate is None:
            return KEKULE, ""
        for a, b in mate.items():
            atoms[a]["nb"][b] = 2
        for a in atoms:
            a["arom"] = False
    symbol_h = []
    for k, a in enumerate(atoms):
        total = sum(a["nb"].values())
        h = a["h"]
        writable = not a["bracket"] or a["el"] == "H" or ((h > 0 or a["chg"] != 0) and h <= 4)
        symbol_h.append(h if writable else None)
        if writable and total > capacity(a["el"], a["chg"], h):
            status = CAPACITY
    if status:
        return status, ""
    kids = [[] for _ in atoms]
    for k, p in enumerate(pred):
        if p is not None:
            kids[p].append(k)

    def sub(k, beta):
        a, b = atoms[k], {1: "", 2: "=", 3: "#"}[beta]
        h = symbol_h[k]
        out = [None if h is None else "[" + b + a["el"] + (f"H{h}" if h else "") + {0: "", 1: "+1", -1: "-1"}[a["chg"]] + "]"]
        for l, r in sorted(c for c in closures if c[1] == k):
            q = k - l - 1
            out += ["[" + ("=" if a["nb"][l] == 2 else "") + f"Ring{1 if q < 16 else 2}]"] + index_symbols(q)
        for c in kids[k][:-1]:
            body = sub(c, a["nb"][c])
            q = len(body) - 1
            out += ["[" + {1: "", 2: "=", 3: "#"}[a["nb"][c]] + f"Branch{1 if q < 16 else 2}]"] + index_symbols(q) + body
        if kids[k]:
            out += sub(kids[k][-1], a["nb"][kids[k][-1]])
        return out
    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 2000))
    symbols = sub(0, 1)
    for i, sym in enumerate(symbols):
        if sym is None or (have is not None and sym not in have):
            return NO_TOKEN, ""
        if i >= max_content:
            return LONG, ""
    return 0, "".join(symbols)
