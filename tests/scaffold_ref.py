"""Reference for the scaffold feature (mvae_smiles_scaffold_rows / _corpus / _host, ops.key_histogram / histogram_cosine): pure Python on
strings, written from the definitions in include/mvae.h ("Murcko scaffold", "Graph key") and NOT from the kernel's method --

  the molecule is fp_ref.molecule's adjacency structure (a dict of neighbour -> bond order per atom), the status chem_ref.analyse's;
  Core by the component criterion, not by pruning and not along tree predecessors: a non-ring atom is a linker iff at least two of the
  components left when it is removed contain a ring atom (a flood fill per atom);
  ring bonds are the non-bridge edges (a low-link search of its own, on edges), ring atoms chem_ref._ring_atoms;
  the keys are computed per atom over its neighbour dict, where the kernel walks an edge list.

`scaffold(s)` returns (status, S as a set of atom numbers, desc [4], (molecule key, scaffold key)) with the keys as signed 64-bit integers.
`rewrite(s, rng)` re-spells a status-0 string from a random root with random neighbour order and returns the new string and, for every
new atom number, the old one: what the invariance tests are made of.  `cosine` is the Counter side of histogram_cosine."""
import math
import sys

import numpy as np

import chem_ref as CR
import fp_ref as FR
from fp_ref import mix, MASK

ROUNDS = 8
sys.setrecursionlimit(max(sys.getrecursionlimit(), 4000))


def _signed(v):
    return v - (1 << 64) if v >= 1 << 63 else v


def ring_bonds(atoms):
    """The bonds that lie on a cycle, as frozensets {a, b}: the edges that are no bridges (low-link search; the graph is simple)."""
    n = len(atoms)
    disc, low, counter, bridges = [-1] * n, [0] * n, [0], set()

    def visit(u, parent):
        disc[u] = low[u] = counter[0]
        counter[0] += 1
        for v in atoms[u]["nb"]:
            if v == parent:
                continue
            if disc[v] < 0:
                visit(v, u)
                low[u] = min(low[u], low[v])
                if low[v] > disc[u]:
                    bridges.add(frozenset((u, v)))
            else:
                low[u] = min(low[u], disc[v])
    for a in range(n):
        if disc[a] < 0:
            visit(a, -1)
    return {frozenset((u, v)) for u in range(n) for v in atoms[u]["nb"]} - bridges


def _components_with_ring(atoms, removed, members):
    """How many connected components of the graph without atom `removed` contain a ring atom."""
    seen, count = {removed}, 0
    for start in range(len(atoms)):
        if start in seen:
            continue
        todo, has = [start], False
        seen.add(start)
        while todo:
            u = todo.pop()
            has = has or u in members
            for v in atoms[u]["nb"]:
                if v not in seen:
                    seen.add(v)
                    todo.append(v)
        count += has
    return count


def sets(atoms):
    """(ring atoms, Core, Exo) of a molecule."""
    members = CR._ring_atoms(atoms)
    core = set(members)
    if members:
        core.update(a for a in range(len(atoms)) if a not in members and _components_with_ring(atoms, a, members) >= 2)
    exo = {a for a in range(len(atoms)) if a not in core and any(b in core and order == 2 for b, order in atoms[a]["nb"].items())}
    return members, core, exo


def graph_key(atoms, U, members, rbonds, with_used):
    """The key of the atom subset U (a set) with its induced bonds; 0 for the empty set."""
    if not U:
        return 0
    nb = {a: {b: o for b, o in atoms[a]["nb"].items() if b in U} for a in U}
    ids = {}
    for a in U:
        at = atoms[a]
        w = CR.ELEMENTS.index(at["el"]) | int(at["arom"]) << 4 | (at["chg"] + 1) << 5 | int(a in members) << 7 | len(nb[a]) << 8
        if with_used:
            w |= (at["h"] + sum(at["nb"].values())) << 12
        ids[a] = mix(w)
    for r in range(1, ROUNDS + 1):
        nxt = {}
        for a in U:
            total = 0
            for b, order in nb[a].items():
                bt = 4 if order == 1 and atoms[a]["arom"] and atoms[b]["arom"] else order
                bt += 8 * (frozenset((a, b)) in rbonds)
                total += mix(ids[b] ^ ((bt * 0x7FEB352D) & MASK))
            nxt[a] = mix((ids[a] * 0x9E3779B1 + r + total) & MASK)
        ids = nxt
    bonds = sum(len(v) for v in nb.values()) // 2
    lo = mix((len(U) * 0x9E3779B1 + sum(mix(i) for i in ids.values())) & MASK)
    hi = mix((bonds * 0x85EBCA6B + sum(mix(i ^ 0x5BD1E995) for i in ids.values())) & MASK)
    key = lo | hi << 32
    return _signed(key if key else 1)


def scaffold(s):
    status = CR.analyse(s)[0]
    if status != CR.OK:
        return status, set(), [0, 0, 0, 0], (0, 0)
    atoms = FR.molecule(s)
    members, core, exo = sets(atoms)
    S = core | exo
    rb = ring_bonds(atoms)
    bonds = sum(1 for a in S for b in atoms[a]["nb"] if b in S) // 2
    keys = (graph_key(atoms, set(range(len(atoms))), members, rb, True), graph_key(atoms, S, members, rb, False))
    return status, S, [len(S), bonds, len(core) - len(members), len(exo)], keys


def mask_words(S):
    """The two int64 words of an atom set."""
    lo = sum(1 << a for a in S if a < 64)
    hi = sum(1 << (a - 64) for a in S if a >= 64)
    return [_signed(lo), _signed(hi)]


def expected(strings):
    """scaffold() of every string as the arrays the entries write: status int32 [B], mask int64 [B, 2], desc int32 [B, 4], key int64 [B, 2]."""
    res = [scaffold(s) for s in strings]
    return (np.array([r[0] for r in res], np.int32), np.array([mask_words(r[1]) for r in res], np.int64).reshape(-1, 2),
            np.array([r[2] for r in res], np.int32).reshape(-1, 4), np.array([r[3] for r in res], np.int64).reshape(-1, 2))


_CACHE = {}


def corpus_expected():
    """(strings, expected(strings)) of chem_ref's mutation corpus, computed once per process and shared: callers leave it unchanged."""
    if "c" not in _CACHE:
        strings = CR.mutation_corpus()
        _CACHE["c"] = (strings, expected(strings))
    return _CACHE["c"]


# ------------------------------------------------------------------------------------------------ re-spelling
def _parse(s):
    """The atoms of a status-0 string as (token text, {neighbour: bond symbol}) -- the symbol '=' or '#', '' for every bond of order 1."""
    atoms, stack, ring_open = [], [], {}
    cur, sym = None, ""
    for m in CR._TOKEN.finditer(s):
        kind, text = m.lastgroup, m.group()
        if kind in ("atom", "bracket"):
            atoms.append((text, {}))
            k = len(atoms) - 1
            if cur is not None:
                atoms[k][1][cur] = atoms[cur][1][k] = sym
            cur, sym = k, ""
        elif kind == "bond":
            sym = text if text in "=#" else ""
        elif kind == "open":
            stack.append(cur)
        elif kind == "close":
            cur = stack.pop()
        elif kind == "digit":
            if text not in ring_open:
                ring_open[text] = cur
            else:
                i = ring_open.pop(text)
                atoms[cur][1][i] = atoms[i][1][cur] = ""
    return atoms


def rewrite(s, rng, tries=200):
    """Another spelling of the status-0 string s: a depth-first spelling from a random root with the neighbours in random order.  Bracket
    atoms are copied verbatim, explicit '=' and '#' are kept, the ring digits 0-9 are reused.  A ring closure cannot carry a bond symbol in
    this grammar, so an order whose closures would fall on a double or triple bond, or that needs more than ten digits at once, is drawn
    again.  Returns (string, old) with old[k] the number atom k of the new string has in s."""
    atoms = _parse(s)
    n = len(atoms)
    for _ in range(tries):
        root = int(rng.randint(n))
        order, parent, children, back = [], {root: None}, {a: [] for a in range(n)}, {a: [] for a in range(n)}
        state = {}

        def visit(u):
            state[u] = 1
            order.append(u)
            nbrs = list(atoms[u][1])
            rng.shuffle(nbrs)
            for v in nbrs:
                if v == parent[u]:
                    continue
                if v not in state:
                    parent[v] = u
                    children[u].append(v)
                    visit(v)
                elif state[v] == 1:                         # v is an ancestor: (u, v) closes a ring
                    back[u].append(v)
                    back[v].append(u)
            state[u] = 2
        visit(root)
        if any(atoms[u][1][v] for u in range(n) for v in back[u]):
            continue
        out, free, digit, written, failed = [], list("0123456789"), {}, set(), [False]

        def write(u):
            out.append(atoms[u][0])
            written.add(u)
            closed = []
            for v in back[u]:
                e = frozenset((u, v))
                if v in written:
                    out.append(digit[e])
                    closed.append(digit.pop(e))
            for v in back[u]:
                e = frozenset((u, v))
                if v not in written:
                    if not free:
                        failed[0] = True
                        return
                    digit[e] = free.pop(0)
                    out.append(digit[e])
            free.extend(closed)                              # a digit closed at this atom is not opened again at it
            free.sort()
            for i, v in enumerate(children[u]):
                last = i == len(children[u]) - 1
                if not last:
                    out.append("(")
                out.append(atoms[u][1][v])
                write(v)
                if not last:
                    out.append(")")
        write(root)
        if not failed[0]:
            return "".join(out), order
    raise AssertionError(f"no spelling of {s!r} in {tries} tries")


def renumbered(S, old):
    """The atom set S of the original string in the numbering of a rewrite (old[k]: the old number of new atom k)."""
    return {k for k, o in enumerate(old) if o in S}


# ------------------------------------------------------------------------------------------------ histograms
def cosine(a, b):
    """The cosine similarity of two collections.Counter histograms: exact integer dot product and squared norms, one sqrt, one division;
    NaN if either is empty."""
    if not a or not b:
        return float("nan")
    dot = sum(c * b.get(k, 0) for k, c in a.items())
    na, nb = sum(c * c for c in a.values()), sum(c * c for c in b.values())
    return dot / math.sqrt(float(na) * float(nb))
