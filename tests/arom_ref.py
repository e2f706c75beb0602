"""Reference for the aromatic normal form (mvae_smiles_aromatize_rows / _corpus / _host): pure Python on strings, written from the rules
of include/mvae.h ("Aromatic normal form") and NOT from the kernel's method.  It is a composition of the references that exist --

  whether the walk accepts the row and whether it has a stereo token is canon_ref.graph's business; the molecule is rewrite_ref.atoms_of's
  adjacency structure (a dict of neighbour -> bond order per atom);
  N and E are kekule_ref.graph's and the size of a maximum matching is networkx's;
  ring members are the ends of scaffold_ref.ring_bonds (a low-link search), the electrons are read off the dicts, and the cycles are
  networkx.simple_cycles over the subgraph of ALL bonds between candidates -- no ring-bond filter, no per-start path search, no masks;
  the output graph is a NEW list of atoms, with the hydrogens stated as the header states them;
  the ranks and the spelling are canon_ref.ranks and canon_ref.spell, applied to that list.

`aromatize(s)` returns (status, string, info, arom): the normal form for status 0 and the input for every refusal; info = [atoms, aromatic
atoms, atoms raised from upper case, double bonds lowered] and arom[k] = 1 / 0 per atom of the input, both None where the header says
zeros / 0xFF (statuses 1 - 8 and 17).  `broken=` selects one of the deliberately wrong references the tests use to show that their checks
can fail.  `kekule_spelling` writes a Kekule spelling of a row from a matching, for the tests' Kekule-invariance property."""
import functools

import networkx as nx

import canon_ref as CN
import chem_ref as CR
import kekule_ref as KR
import rewrite_ref as RR
import scaffold_ref as SR

KEKULE, NOT_AROMATIC = 7, 17
BROKEN = ("inside_doubles", "no_c_o", "no_nh", "eight_rings")
E1 = {("C", 0), ("N", 0), ("N", 1), ("O", 1), ("S", 1)}
E2 = {("N", 0): 3, ("O", 0): 2, ("S", 0): 2, ("N", -1): 2, ("C", -1): 3}


def implicit(el, arom, total):
    """The implicit hydrogens of an unbracketed atom whose bonds sum to `total` ("SMILES graph")."""
    v0 = min(v for v in CR.VALENCES[el][1] if v >= total)
    return max(0, v0 - total - 1) if arom else v0 - total


def hydrogens(at):
    return at["h"] if at["bracket"] else implicit(at["el"], at["arom"], sum(at["nb"].values()))


def electrons(atoms, N, broken=None):
    """{candidate: e}"""
    rbonds = SR.ring_bonds(atoms)
    members = {a for e in rbonds for a in e}
    out = {}
    for a, at in enumerate(atoms):
        if a not in members:
            continue
        key = (at["el"], at["chg"])
        K = sum(at["nb"].values()) + hydrogens(at) + (a in N)
        doubles = [b for b, o in at["nb"].items() if o == 2]
        dbl = len(doubles) + (a in N)
        triple = any(o == 3 for o in at["nb"].values())
        if dbl == 1 and not triple and key in E1 and K <= 4 and (a in N or frozenset((a, doubles[0])) in rbonds):
            out[a] = 1
        elif dbl == 1 and key == ("C", 0) and doubles and frozenset((a, doubles[0])) not in rbonds and atoms[doubles[0]]["el"] in "OSN":
            if broken != "no_c_o":
                out[a] = 0
        elif dbl == 0 and E2.get(key) == K:
            out[a] = 2
    return out


def aromatic_atoms(atoms, N, E, broken=None):
    e = electrons(atoms, N, broken)
    G = nx.Graph()
    G.add_nodes_from(e)
    G.add_edges_from((a, b) for a in e for b in atoms[a]["nb"] if b in e and a < b)
    partner = {}
    if broken == "inside_doubles":                # the double bond of every e = 1 atom in one Kekule structure
        for a, b in nx.max_weight_matching(KR.nx_graph(N, E), maxcardinality=True):
            partner[a], partner[b] = b, a
        for a in e:
            if e[a] == 1 and a not in N:
                partner[a] = [b for b, o in atoms[a]["nb"].items() if o == 2][0]
    top = 8 if broken == "eight_rings" else 7
    found = set()
    for cyc in nx.simple_cycles(G, length_bound=top):
        if not 5 <= len(cyc) <= top:
            continue
        total = sum(e[a] for a in cyc)
        if broken == "inside_doubles":
            total = sum(e[a] for a in cyc if e[a] != 1 or partner[a] in cyc)
        if total % 4 == 2:
            found.update(cyc)
    return found


def output_graph(atoms, ar, broken=None):
    """(the atoms of the perceived graph, bonds lowered)"""
    out, lowered = [], 0
    for a, at in enumerate(atoms):
        nb = {b: (1 if a in ar and b in ar else o) for b, o in at["nb"].items()}
        lowered += sum(1 for b, o in at["nb"].items() if o == 2 and nb[b] == 1 and a < b)
        h = hydrogens(at)
        bracket = at["bracket"] or implicit(at["el"], a in ar, sum(nb.values())) != h
        if broken == "no_nh":
            bracket = at["bracket"]
        out.append({"el": at["el"], "arom": a in ar, "bracket": bracket, "chg": at["chg"], "h": h if bracket else 0, "nb": nb})
    return out, lowered


@functools.lru_cache(maxsize=None)
def _ranked(s, broken):
    """(status, output atoms, rank, info, arom) up to the search: what does not depend on max_content or the vocabulary."""
    status, atoms = CN.graph(s)
    if atoms is None:
        return status, None, None, None, None
    N, E = KR.graph(s)
    if 2 * KR.max_pairs(N, E) != len(N):
        return KEKULE, None, None, None, None
    ar = aromatic_atoms(atoms, N, E, broken)
    lower = {a for a, at in enumerate(atoms) if at["arom"]}
    if lower - ar:
        return NOT_AROMATIC, None, None, None, None
    out, lowered = output_graph(atoms, ar, broken)
    return CR.OK, out, CN.ranks(out)[0], [len(atoms), len(ar), len(ar - lower), lowered], [int(a in ar) for a in range(len(atoms))]


def aromatize(s, max_content=127, have=None, broken=None):
    status, out, rank, info, arom = _ranked(s, broken)
    if status != CR.OK:
        return status, s, None, None
    try:
        return CR.OK, CN.spell(out, rank, max_content, have), info, arom
    except CN.Refused as r:
        return r.args[0], s, info, arom


def kekule_spelling(s, mate, seed=0, draw=0, tries=16):
    """A Kekule spelling of the status-0 row s: every atom upper case, '=' on the bonds a - mate[a] of the matching `mate` (the kekule
    entry's output row, 255 = unmatched), every atom keeping its hydrogens, written by canon_ref.spell (the rewrite's traversal and
    emission) in the order of rewrite_ref.prio(seed, draw).  A draw whose spelling would need a double closure bond is skipped; None if
    `tries` draws in a row need one."""
    atoms = RR.atoms_of(s)
    kek = []
    for a, at in enumerate(atoms):
        nb = {b: (2 if int(mate[a]) == b else o) for b, o in at["nb"].items()}
        h = hydrogens(at)
        bracket = at["bracket"] or implicit(at["el"], False, sum(nb.values())) != h
        kek.append({"el": at["el"], "arom": False, "bracket": bracket, "chg": at["chg"], "h": h if bracket else 0, "nb": nb})
    for t in range(tries):
        order = sorted(range(len(kek)), key=lambda a: (RR.prio(seed, draw + 7919 * t, a), a))
        rank = [0] * len(kek)
        for r, a in enumerate(order):
            rank[a] = r
        try:
            return CN.spell(kek, rank)
        except CN.Refused:
            continue
    return None
