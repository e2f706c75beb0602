"""Reference for the kekulisation feature (mvae_smiles_kekule_rows / _corpus / _host): pure Python on strings, written from the definition
in include/mvae.h ("Kekulisation") and NOT from the kernel's method --

  the molecule is fp_ref.molecule's adjacency structure (a dict of neighbour -> bond order per atom), the walk status chem_ref.analyse's;
  ring bonds are the non-bridge edges (scaffold_ref.ring_bonds, a low-link search), never a walk along predecessors;
  N comes from chem_ref's valence SETS (the smallest member >= the used valence), where the kernel steps through nibble tables;
  the size of a maximum matching of (N, E) is networkx.max_weight_matching(G, maxcardinality=True), where the kernel runs its own
  blossom search from a greedy start.

`kekule(s)` returns (status, [|N|, |E|, pairs, deficiency], N, E) with E a set of frozensets.  `naive_pairs(N, E)` is a deliberately
INCOMPLETE matcher -- greedy, then augmenting searches that never contract a blossom -- which the tests use as their negative control: a
comparison that it passes proves nothing about odd rings.  `ring_system_corpus(seed)` makes the polycyclic aromatic systems the
comparison runs over."""
import networkx as nx
import numpy as np

import chem_ref as CR
import fp_ref as FR
import scaffold_ref as SR

KEKULE = 7


def graph(s):
    """(N, E) of a string whose walk status is 0: N a set of atom numbers, E a set of frozensets {a, b}."""
    atoms = FR.molecule(s)
    N = set()
    for k, a in enumerate(atoms):
        if not a["arom"]:
            continue
        used = a["h"] + sum(a["nb"].values())
        v0 = min(v for v in CR.VALENCES[a["el"]][a["chg"] + 1] if v >= used)
        if v0 - used >= 1:
            N.add(k)
    rings = SR.ring_bonds(atoms)
    E = {frozenset((a, b)) for a in N for b, order in atoms[a]["nb"].items()
         if b in N and order == 1 and atoms[a]["arom"] and atoms[b]["arom"] and frozenset((a, b)) in rings}
    return N, E


def nx_graph(N, E):
    G = nx.Graph()
    G.add_nodes_from(N)
    G.add_edges_from(tuple(e) for e in E)
    return G


def max_pairs(N, E):
    return len(nx.max_weight_matching(nx_graph(N, E), maxcardinality=True))


def kekule(s):
    status = CR.analyse(s)[0]
    if status != CR.OK:
        return status, [0, 0, 0, 0], set(), set()
    N, E = graph(s)
    pairs = max_pairs(N, E)
    return (CR.OK if 2 * pairs == len(N) else KEKULE), [len(N), len(E), pairs, len(N) - 2 * pairs], N, E


def expected(strings):
    """kekule() of every string as the arrays the entries write: status int32 [B], desc int32 [B, 4]."""
    res = [kekule(s) for s in strings]
    return np.array([r[0] for r in res], np.int32), np.array([r[1] for r in res], np.int32).reshape(-1, 4)


def bipartite(N, E):
    return nx.is_bipartite(nx_graph(N, E))


def naive_pairs(N, E, greedy=True):
    """The size of the matching a blossom-free method finds: greedy in atom order (every free atom takes its lowest free neighbour), then
    from every free atom a breadth-first alternating search that labels each vertex once and never contracts an odd cycle.  Always a
    valid matching, not always a maximum one."""
    nb = {a: sorted(b for e in E if a in e for b in e if b != a) for a in N}
    mate = {}
    if greedy:
        for a in sorted(N):
            if a not in mate:
                for b in nb[a]:
                    if b not in mate:
                        mate[a], mate[b] = b, a
                        break
    for root in sorted(N):
        if root in mate:
            continue
        parent, label, queue, end = {}, {root: 0}, [root], None
        while queue and end is None:
            v = queue.pop(0)
            for to in nb[v]:
                if to in label:
                    continue                                   # labelled once: an edge between two even vertices is ignored
                label[to], parent[to] = 1, v
                if to not in mate:
                    end = to
                    break
                m = mate[to]
                label[m], parent[m] = 0, to
                queue.append(m)
        while end is not None:
            v = parent[end]
            nxt = mate.get(v)
            mate[end], mate[v] = v, end
            end = nxt
    assert all(mate[mate[a]] == a and frozenset((a, mate[a])) in E for a in mate)
    return len(mate) // 2


def check_mate(mate_row, N, E, pairs):
    """mate_row (128 values) is a matching of (N, E) with exactly `pairs` pairs: an involution along E edges, 255 outside it."""
    row = [int(v) for v in mate_row]
    assert len(row) == 128
    matched = [a for a in range(128) if row[a] != 255]
    for a in matched:
        assert a in N and row[a] in N and row[row[a]] == a and frozenset((a, row[a])) in E, (a, row[a])
    assert len(matched) == 2 * pairs, (len(matched), pairs)


# ------------------------------------------------------------------------------------------------ the ring-system corpus
def _write(atoms, nb, rng):
    """A depth-first spelling of the graph (atom texts, neighbour lists; every bond implicit) from a random root with random neighbour
    order, reusing the ten ring digits; None if it needs more than ten at once."""
    n = len(atoms)
    root = int(rng.randint(n))
    parent, children, back, state = {root: None}, {a: [] for a in range(n)}, {a: [] for a in range(n)}, {}

    def visit(u):
        state[u] = 1
        order = list(nb[u])
        rng.shuffle(order)
        for v in order:
            if v == parent[u]:
                continue
            if v not in state:
                parent[v] = u
                children[u].append(v)
                visit(v)
            elif state[v] == 1:
                back[u].append(v)
                back[v].append(u)
        state[u] = 2
    visit(root)
    out, free, digit, written = [], list("0123456789"), {}, set()

    def write(u):
        out.append(atoms[u])
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
                    return False
                digit[e] = free.pop(0)
                out.append(digit[e])
        free.extend(closed)
        free.sort()
        for i, v in enumerate(children[u]):
            last = i == len(children[u]) - 1
            if not last:
                out.append("(")
            if not write(v):
                return False
            if not last:
                out.append(")")
        return True
    return "".join(out) if write(root) else None


def ring_system(rng):
    """One random polycyclic aromatic system as a string (None: the spelling is too long or needs too many digits): a cycle plus ears,
    ring sizes 3-7, up to six rings, at most 60 atoms; about 80 % of the ears join two ADJACENT degree-2 atoms (a fused ring), the
    others two arbitrary degree-2 atoms (a bridge); about 12 % of the degree-2 atoms become o, s, [nH] or n."""
    size = int(rng.randint(3, 8))
    nb = {a: [(a - 1) % size, (a + 1) % size] for a in range(size)}
    for _ in range(int(rng.randint(0, 6))):
        two = [a for a in nb if len(nb[a]) == 2]
        if rng.rand() < 0.8:
            pairs = [(a, b) for a in two for b in nb[a] if a < b and len(nb[b]) == 2]
        else:
            pairs = [(a, b) for a in two for b in two if a < b]
        if not pairs:
            continue
        a, b = pairs[int(rng.randint(len(pairs)))]
        new = int(rng.randint(3, 8)) - 2                          # the ear's atoms: with adjacent ends the new ring has 3-7 members
        if len(nb) + new > 60:
            continue
        prev = a
        for _ in range(new):
            k = len(nb)
            nb[k] = [prev]
            nb[prev].append(k)
            prev = k
        nb[prev].append(b)
        nb[b].append(prev)
    atoms = []
    for a in range(len(nb)):
        atoms.append(("o", "s", "[nH]", "n")[int(rng.randint(4))] if len(nb[a]) == 2 and rng.rand() < 0.12 else "c")
    s = _write(atoms, nb, rng)
    return s if s is not None and len(s) <= CR.CONTENT_MAX else None


def triangle_strip(n):
    """n aromatic atoms, atom k bonded to k - 1 and k - 2: n - 2 fused three-rings.  Atom k closes the digit atom k - 2 opened and opens
    another, four digits in turn.  The inner atoms have four sigma bonds and are not in N."""
    out = []
    for k in range(n):
        out.append("c" + (str((k - 2) % 4 + 1) if k >= 2 else "") + (str(k % 4 + 1) if k < n - 2 else ""))
    return "".join(out)


# two systems of more than 100 atoms in which the greedy start leaves an augmenting path through an odd ring: naive_pairs is one short
BIG_BLOSSOMS = [
    "c0cccccccc1c(ccccc2ccccccccccccccc3cccccccccccc3cccccccnc2ccoccccccc2ccccccccccccc2ccccccccccccccccccccc1)cccccccccccc0",
    "c0cc1ccccccnccc(cccccccccc2cccccccccccc2c2cccccccccccccccc2c0)ccccccccccnc0cc(ccccccccccccccccccccc0)cccccccccccccccccnccccc1",
]


def edge_rows():
    """The rows at the limits, with what the definition gives them where that is plain: (string, status or None, desc or None)."""
    return [
        ("c1" + "c" * 124 + "1", KEKULE, [125, 125, 62, 1]),          # 127 tokens: a ring of 125 aromatic atoms, the whole graph one odd cycle
        ("c1" + "c" * 123 + "1", 0, [124, 124, 62, 0]),               # a ring of 124
        ("c" * 128, CR.TOO_LONG, [0, 0, 0, 0]),
        ("CCCc1" + "c" * 66 + "1", KEKULE, [67, 67, 33, 1]),          # a ring whose closure joins atoms 3 and 69
        ("CCCc1" + "c" * 65 + "1", 0, [66, 66, 33, 0]),
        ("c1cc1" * 25, KEKULE, [75, 75, 25, 25]),                     # 25 three-rings in a chain: the bonds between them are no ring bonds
        (triangle_strip(27), 0, [4, 2, 2, 0]),                        # 25 FUSED three-rings: only the two atoms at either end are in N
        ("c1c2c3c4c5c6c7c8c9c0" + "cc" + "c0c9c8c7c6c5c4c3c2c1", 0, [22, 31, 11, 0]),      # all ten ring digits open at once
        (BIG_BLOSSOMS[0], 0, [106, 109, 53, 0]),
        (BIG_BLOSSOMS[1], KEKULE, [111, 115, 55, 1]),
    ]


_CACHE = {}


def ring_system_corpus(seed=7, rows=3000):
    """`rows` strings of ring_system (duplicates allowed; the order depends on the seed), computed once per process and shared."""
    if (seed, rows) not in _CACHE:
        rng = np.random.RandomState(seed)
        out = []
        while len(out) < rows:
            s = ring_system(rng)
            if s is not None:
                out.append(s)
        _CACHE[seed, rows] = out
    return _CACHE[seed, rows]


def ring_system_expected(seed=7, rows=3000):
    """(strings, status, desc, [(N, E)]) of ring_system_corpus, computed once per process and shared: callers leave it unchanged."""
    key = ("x", seed, rows)
    if key not in _CACHE:
        strings = ring_system_corpus(seed, rows)
        res = [kekule(s) for s in strings]
        _CACHE[key] = (strings, np.array([r[0] for r in res], np.int32), np.array([r[1] for r in res], np.int32).reshape(-1, 4),
                       [(r[2], r[3]) for r in res])
    return _CACHE[key]


def mutation_expected():
    """(strings, status, desc) of chem_ref's mutation corpus, computed once per process and shared."""
    if "m" not in _CACHE:
        strings = CR.mutation_corpus()
        _CACHE["m"] = (strings,) + expected(strings)
    return _CACHE["m"]
