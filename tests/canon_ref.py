"""Reference for the canonical SMILES (mvae_smiles_canon_rows / _corpus / _host): pure Python on strings, written from the rules of
include/mvae.h ("SMILES canon") and NOT from the kernel's method --

  the molecule is rewrite_ref.atoms_of's adjacency structure (a dict of neighbour -> bond order per atom) and whether the walk accepts
  the row at all is chem_ref.analyse's business, as in rewrite_ref;
  ranks are dense (the position of a key among the sorted distinct keys), keys are Python tuples compared as tuples, and a refinement
  round ranks all atoms at once with sorted(set(...)): no packed words, no permutation, no per-class sorting;
  the traversal and the emission are two plain recursions, the refusals are exceptions raised where the rules name them.

`canon(s)` returns (status, string, info, rank): the canonical spelling for status 0 and the input for every refusal; info = [atoms,
classes after the first refinement, refinement rounds in all, ties broken] and rank[k] = the canonical rank of atom k (string order),
both None where no ranks were computed (the walk's refusals and STEREO).  `all_choices(s)` follows EVERY member of the chosen class at
every tie and returns the set of strings reached: the definition promises one string only where that set has one element.  `broken=`
selects one of the deliberately wrong references the tests use to show that their checks can fail."""
import chem_ref as CR
import rewrite_ref as RR

BROKEN = ("hashed_ties", "one_round")


def invariant(atoms, a):
    """(element, aromatic, charge, bracket flag, bracket hydrogens, degree, sum of bond orders)"""
    at = atoms[a]
    return (CR.ELEMENTS.index(at["el"]), int(at["arom"]), at["chg"], int(at["bracket"]), at["h"] if at["bracket"] else 0, len(at["nb"]),
            sum(at["nb"].values()))


def dense(keys):
    order = {k: i for i, k in enumerate(sorted(set(keys)))}
    return [order[k] for k in keys]


def refine(atoms, rank, broken=None):
    """Rounds of rank := position of (rank, sorted (order, neighbour's rank)) until the classes stop growing: (rank, rounds)."""
    rounds = 0
    while True:
        keys = [(rank[a], tuple(sorted((o, rank[b]) for b, o in atoms[a]["nb"].items()))) for a in range(len(atoms))]
        if broken == "hashed_ties":
            keys = [k + (RR.mix(a + 1),) for a, k in enumerate(keys)]
        new = dense(keys)
        rounds += 1
        if len(set(new)) == len(set(rank)) or broken == "one_round":
            return new, rounds
        rank = new


def split(rank, cls, member):
    """member keeps the rank of its class, the others of the class come just above it"""
    return [r + 1 if (r > cls or (r == cls and a != member)) else r for a, r in enumerate(rank)]


def tie_class(rank):
    """the members (ascending atom number) of the class of lowest rank that has more than one, None when every class has one"""
    for cls in range(len(set(rank))):
        members = [a for a, r in enumerate(rank) if r == cls]
        if len(members) > 1:
            return cls, members
    return None


def ranks(atoms, broken=None):
    """(rank, info) with the member of lowest atom number taken at every tie"""
    n = len(atoms)
    rank, rounds = refine(atoms, dense([invariant(atoms, a) for a in range(n)]), broken)
    first, ties = len(set(rank)), 0
    while len(set(rank)) < n:
        cls, members = tie_class(rank)
        rank, more = refine(atoms, split(rank, cls, members[0]), broken)
        rounds += more
        ties += 1
    return rank, [n, first, rounds, ties]


def all_ranks(atoms):
    """every final rank list reachable by taking any member at every tie"""
    n = len(atoms)
    found, todo = [], [refine(atoms, dense([invariant(atoms, a) for a in range(n)]))[0]]
    while todo:
        rank = todo.pop()
        if len(set(rank)) == n:
            found.append(rank)
            continue
        cls, members = tie_class(rank)
        todo.extend(refine(atoms, split(rank, cls, m))[0] for m in members)
    return found


class Refused(Exception):
    pass


def spell(atoms, rank, max_content=127, have=None):
    """The "SMILES rewrite" traversal and emission with atoms compared by rank: the string, or Refused(status)."""
    root = rank.index(0)
    index, parent, children, closures = {}, {root: None}, {}, []          # closures: (ancestor, descendant)
    multi = []

    def search(a):
        index[a] = len(index)
        children[a] = []
        nb = atoms[a]["nb"]
        for b in sorted((b for b in nb if b != parent[a]), key=lambda b: (nb[b] < 2, rank[b])):
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
        raise Refused(RR.RING_MULTI)
    out, digit_of, depth = [], {}, [0]

    def put(ch):
        for c in ch:
            if have is not None and c not in have:
                raise Refused(RR.NO_TOKEN)
            if len(out) >= max_content:
                raise Refused(RR.LONG)
            out.append(c)

    def write(a):
        at = atoms[a]
        if parent[a] is not None and at["nb"][parent[a]] >= 2:
            put("=" if at["nb"][parent[a]] == 2 else "#")
        sym = at["el"].lower() if at["arom"] else at["el"]
        if at["bracket"]:
            h = at["h"]
            put("[" + sym + ("H" if h >= 1 else "") + (str(h) if h >= 2 else "") + {0: "", 1: "+", -1: "-"}[at["chg"]] + "]")
        else:
            put(sym)
        here = set()
        for d in sorted(d for d, c in digit_of.items() if c[1] == a):
            put(str(d))
            here.add(d)
            del digit_of[d]
        for c in sorted((c for c in closures if c[0] == a), key=lambda c: index[c[1]]):
            free = [d for d in (1, 2, 3, 4, 5, 6, 7, 8, 9, 0) if d not in digit_of and d not in here]
            if not free:
                raise Refused(RR.RING_DIGITS)
            digit_of[free[0]] = c
            here.add(free[0])
            put(str(free[0]))
        for k, b in enumerate(children[a]):
            if k + 1 < len(children[a]):
                if depth[0] >= 15:
                    raise Refused(RR.DEPTH)
                depth[0] += 1
                put("(")
                write(b)
                put(")")
                depth[0] -= 1
            else:
                write(b)
    write(root)
    return "".join(out)


def graph(s):
    """(status, atoms): atoms is None for a row that is refused before any rank is computed"""
    status = CR.analyse(s)[0]
    if status != CR.OK:
        return status, None
    if any(ch in s for ch in "@/\\"):
        return RR.STEREO, None
    return CR.OK, RR.atoms_of(s)


def canon(s, max_content=127, have=None, broken=None):
    status, atoms = graph(s)
    if atoms is None:
        return status, s, None, None
    rank, info = ranks(atoms, broken)
    try:
        return CR.OK, spell(atoms, rank, max_content, have), info, rank
    except Refused as r:
        return r.args[0], s, info, rank


def all_choices(s):
    """The set of strings reached over every choice at every tie (a refusal counts as the string "!<status>"); None for a row refused
    before the ranks."""
    status, atoms = graph(s)
    if atoms is None:
        return None
    out = set()
    for rank in all_ranks(atoms):
        try:
            out.add(spell(atoms, rank))
        except Refused as r:
            out.add("!%d" % r.args[0])
    return out


def isomorphic(s, rank_s, t, rank_t):
    """Whether atom a of s -> the atom of t with the same rank maps atoms and bonds of s onto those of t."""
    A, B = RR.atoms_of(s), RR.atoms_of(t)
    if len(A) != len(B) or sorted(rank_s) != sorted(rank_t):
        return False
    to = {a: rank_t.index(r) for a, r in enumerate(rank_s)}
    for a, at in enumerate(A):
        bt = B[to[a]]
        if invariant(A, a) != invariant(B, to[a]) or {to[b]: o for b, o in at["nb"].items()} != bt["nb"]:
            return False
    return True


# cage and spiro rows: many rings through every atom, large symmetry groups
CAGES = [
    "C12C3C4C1C5C2C3C45",                         # cubane
    "C1C2CC3CC1CC(C2)C3",                         # adamantane
    "C1CC2CCC1C2",                                # norbornane
    "C1CC2CCC1CC2",                               # bicyclo[2.2.2]octane
    "C1CC2(C1)CCC2",                              # spiro[3.3]heptane
    "C1CCC2(CC1)CCCCC2",                          # spiro[5.5]undecane
    "C12C3C1C23",                                 # tetrahedrane
    "C12C3C4C1C4C23",                             # prismane
    "C1C2CC1C2",                                  # bicyclo[1.1.1]pentane
    "C1C2C3CC4C1C4C23",                           # a fused cage without a name here
]


def corpus():
    """The status-0, stereo-free rows of the mutation corpus, rewrite_ref.HAND_ROWS, the chem_ref.FORMULAS strings and
    fragment_corpus(300, seed=1), in that order."""
    rows = CR.mutation_corpus() + RR.HAND_ROWS + [f[0] for f in CR.FORMULAS] + RR.fragment_corpus(300, seed=1)
    return [s for s in rows if 0 < len(s) <= 127 and graph(s)[1] is not None]
