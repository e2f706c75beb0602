"""Reference for the scaffold SMILES (mvae_smiles_scaffold_smiles_rows / _corpus / _host): pure Python on strings, written from the rules
of include/mvae.h ("Scaffold SMILES") and NOT from the kernel's method.  It is a composition of the references that exist --

  whether the walk accepts the row and whether it has a stereo token is canon_ref.graph's business; the molecule is rewrite_ref.atoms_of's
  adjacency structure (a dict of neighbour -> bond order per atom);
  S = Core u Exo is scaffold_ref.sets: the component criterion, a flood fill per atom, no tree predecessors and no pruning;
  the scaffold graph is a NEW list of atoms built from S -- no array is cut in place, no popcounts --, with the hydrogens stated as the
  header states them: h_S = h_row + lost, and an unbracketed atom stays one iff the implicit rule gives h_S on its new bond sum;
  the ranks and the spelling are canon_ref.ranks and canon_ref.spell, applied to that list.

`scaffold(s)` returns (status, string, info): the scaffold's canonical spelling for status 0 and "" for every other status; info =
[|S|, bonds of S, atoms that became bracket atoms, sum of lost], None where the header says zeros (statuses 1 - 8 and 14).  `broken=`
selects one of the deliberately wrong references the tests use to show that their checks can fail."""
import functools

import canon_ref as CN
import chem_ref as CR
import rewrite_ref as RR
import scaffold_ref as SR

NO_RING = 14
BROKEN = ("no_h", "keep_leaf", "copy_on_refusal")


def implicit(el, arom, total):
    """The implicit hydrogens of an unbracketed atom whose bonds sum to `total` ("SMILES graph")."""
    v0 = min(v for v in CR.VALENCES[el][1] if v >= total)
    return max(0, v0 - total - 1) if arom else v0 - total


def scaffold_graph(atoms, broken=None):
    """(the atoms of G_S in rewrite_ref's structure, info) of a molecule; ([], None) for one without a ring."""
    _, core, exo = SR.sets(atoms)
    S = core | exo
    if not S:
        return [], None
    if broken == "keep_leaf":                     # the lowest-numbered pendant atom stays
        S = S | set([a for a in range(len(atoms)) if a not in S and any(b in S for b in atoms[a]["nb"])][:1])
    new = {a: i for i, a in enumerate(sorted(S))}
    out, made, lost_sum = [], 0, 0
    for a in sorted(S):
        at = atoms[a]
        nb = {new[b]: o for b, o in at["nb"].items() if b in S}
        lost = sum(o for b, o in at["nb"].items() if b not in S)
        h_row = at["h"] if at["bracket"] else implicit(at["el"], at["arom"], sum(at["nb"].values()))
        h_s = h_row + lost
        bracket = at["bracket"] or implicit(at["el"], at["arom"], sum(nb.values())) != h_s
        if broken == "no_h":                      # the atoms are written as the row wrote them
            bracket, h_s = at["bracket"], at["h"]
        made += bracket and not at["bracket"]
        lost_sum += lost
        out.append({"el": at["el"], "arom": at["arom"], "bracket": bracket, "chg": at["chg"], "h": h_s if bracket else 0, "nb": nb})
    return out, [len(out), sum(len(a["nb"]) for a in out) // 2, made, lost_sum]


@functools.lru_cache(maxsize=None)
def _ranked(s, broken):
    """(status, atoms of G_S, rank, info) up to the search: what does not depend on max_content or the vocabulary."""
    status, atoms = CN.graph(s)
    if atoms is None:
        return status, None, None, None
    gs, info = scaffold_graph(atoms, broken)
    if not gs:
        return NO_RING, None, None, None
    return CR.OK, gs, CN.ranks(gs)[0], info


def scaffold(s, max_content=127, have=None, broken=None):
    status, gs, rank, info = _ranked(s, broken if broken in ("no_h", "keep_leaf") else None)
    text = ""
    if status == CR.OK:
        try:
            text = CN.spell(gs, rank, max_content, have)
        except CN.Refused as r:
            status = r.args[0]
    if status != CR.OK and broken == "copy_on_refusal":
        text = s
    return status, text, info
