"""Reference for the substructure search (mvae_smiles_substruct_rows / _corpus / _host): pure Python on rewrite_ref.atoms_of, written
from the definition of include/mvae.h ("SMILES substructure") and NOT from the kernel's method --

  the molecule is rewrite_ref's adjacency structure (a dict of neighbour -> bond order per atom), the query's likewise;
  the search is a plain recursion over the query's atoms in string order: no cursor array, no packed table, no half-edge list;
  the budget is an exception raised where the definition says the search stops.

`search(row, query, max_steps)` returns (result, map, steps): result MISS / HIT / UNDECIDED, map the first embedding (None without a
hit), steps the candidates examined.  `broken=` selects one of the deliberately wrong matchers the tests use to show that their checks
can fail.  `query_status(s)` is what the compile entry says of a query string."""
import chem_ref as CR
import rewrite_ref as RR

MISS, HIT, UNDECIDED = 0, 1, 2
QATOMS, QUERIES, STEPS = 32, 64, 65536
QUERY_ATOMS = 14
BROKEN = ("ignores_bond_class", "not_injective", "ignores_closures", "ignores_charge", "unsorted_candidates")

# the queries of the issue, with CCCCCCCN in place of the 15-carbon amine, which no row of the test corpus contains
QUERIES_22 = ["C(=O)O", "c1ccccc1", "C(=O)N", "S(=O)(=O)", "C#N", "c1ccncc1", "C[N+](C)(C)C", "C1CCNCC1", "CCCCCCCC", "c1ccc2ccccc2c1", "C1CC1",
              "C(=O)[O-]", "C(C)(C)C", "c1cc[nH]c1", "CCCCCCCN", "C1CCCCC1", "C=C", "Cl", "c1ccc(cc1)C(=O)", "C(F)C(F)", "C12C3C4C1C5C2C3C45",
              "CC(C)CC(C)CC(C)CC(C)C"]
BUDGET_QUERY, BUDGET_ROW = "C1CCCCCCCCCCCCCCC1", "C1CC1" * 25 + "CC"


def bond_class(atoms, a, b):
    """1, 2, 3, or 4 for a single bond between two aromatic atoms; 0: not bonded."""
    o = atoms[a]["nb"].get(b, 0)
    return 4 if o == 1 and atoms[a]["arom"] and atoms[b]["arom"] else o


def atom_key(a, broken=None):
    return (a["el"], a["arom"], 0 if broken == "ignores_charge" else a["chg"])


def query_status(s):
    """0 for a query, else why it is refused: the walk's status (AROMATIC is accepted), STEREO, QUERY_ATOMS."""
    st = CR.analyse(s)[0]
    if st not in (CR.OK, 5):
        return st
    if any(ch in s for ch in "@/\\"):
        return RR.STEREO
    return QUERY_ATOMS if len(RR.atoms_of(s)) > QATOMS else 0


def heavy_counts(atoms):
    out = {}
    for a in atoms:
        if a["el"] != "H":
            out[a["el"]] = out.get(a["el"], 0) + 1
    return out


class _Budget(Exception):
    pass


def search(row, query, max_steps=STEPS, broken=None):
    """row, query: strings, or the atoms_of lists of them."""
    R = RR.atoms_of(row) if isinstance(row, str) else row
    Q = RR.atoms_of(query) if isinstance(query, str) else query
    have, want = heavy_counts(R), heavy_counts(Q)
    if any(c > have.get(el, 0) for el, c in want.items()):
        return MISS, None, 0
    nq = len(Q)
    # the neighbours below i whose bonds are checked when i is placed; the anchor is the lowest
    earlier = [sorted(j for j in Q[i]["nb"] if j < i) for i in range(nq)]
    if broken == "ignores_closures":                   # the bond to the tree predecessor alone: the first one the string gave the atom
        earlier = [[j for j in list(Q[i]["nb"])[:1] if j < i] for i in range(nq)]
    m, used, steps = [None] * nq, set(), [0]

    def fits(i, c):
        if c in used and broken != "not_injective":
            return False
        if atom_key(Q[i], broken) != atom_key(R[c], broken) or len(R[c]["nb"]) < len(Q[i]["nb"]):
            return False
        for j in earlier[i]:
            have_cls = bond_class(R, m[j], c)
            if have_cls == 0 or (have_cls != bond_class(Q, j, i) and broken != "ignores_bond_class"):
                return False
        return True

    def place(i):
        if i == nq:
            return True
        if i == 0:
            cands = range(len(R))
        else:
            cands = list(R[m[earlier[i][0]]]["nb"])    # string order, as the writer's half-edge lists have it
            if broken != "unsorted_candidates":
                cands.sort()
        for c in cands:
            if steps[0] >= max_steps:
                raise _Budget()
            steps[0] += 1
            if not fits(i, c):
                continue
            m[i] = c
            used.add(c)
            if place(i + 1):
                return True
            used.discard(c)
        return False
    try:
        found = place(0)
    except _Budget:
        return UNDECIDED, None, steps[0]
    return (HIT, list(m), steps[0]) if found else (MISS, None, steps[0])


def is_embedding(R, Q, m):
    """m is injective and satisfies rules 1 and 2."""
    if len(set(m)) != len(m) or any(atom_key(Q[i]) != atom_key(R[c]) for i, c in enumerate(m)):
        return False
    return all(bond_class(Q, i, j) == bond_class(R, m[i], m[j]) for i in range(len(Q)) for j in Q[i]["nb"])


def smallest_embedding(R, Q):
    """The lexicographically smallest embedding by exhaustive enumeration over every injective assignment, pruned by nothing but rules 1
    and 2 on the atoms placed so far; None without one.  For small queries."""
    nq = len(Q)

    def extend(m):
        i = len(m)
        if i == nq:
            return m
        for c in range(len(R)):
            if c in m or atom_key(Q[i]) != atom_key(R[c]):
                continue
            if all(bond_class(Q, i, j) == bond_class(R, c, m[j]) for j in Q[i]["nb"] if j < i):
                got = extend(m + [c])
                if got is not None:
                    return got
        return None
    return extend([])


def nx_monomorphic(R, Q):
    """networkx' verdict on the same graphs with the same node and edge predicates."""
    import networkx as nx
    from networkx.algorithms import isomorphism as iso

    def graph(atoms):
        G = nx.Graph()
        for k, a in enumerate(atoms):
            G.add_node(k, key=atom_key(a))
        for k, a in enumerate(atoms):
            for j in a["nb"]:
                if j < k:
                    G.add_edge(k, j, cls=bond_class(atoms, k, j))
        return G
    gm = iso.GraphMatcher(graph(R), graph(Q), node_match=lambda a, b: a["key"] == b["key"], edge_match=lambda a, b: a["cls"] == b["cls"])
    return gm.subgraph_is_monomorphic()


_CORPUS = {}


def corpus():
    """The 1,027 status-0 rows the reference is measured on: the hand rows, 300 fragment molecules, the first 700 status-0 rows of the
    mutation corpus.  Computed once; callers leave it unchanged."""
    if "rows" not in _CORPUS:
        hand = [s for s in RR.HAND_ROWS if CR.analyse(s)[0] == CR.OK]
        mut = [s for s in CR.mutation_corpus() if s and CR.analyse(s)[0] == CR.OK][:700]
        _CORPUS["rows"] = hand + RR.fragment_corpus(300, seed=1) + mut
    return _CORPUS["rows"]
