"""Reference for the fragment feature (mvae_smiles_fragment_rows / _corpus / _host, mvae_smiles_fragment_smiles_rows / _corpus / _host):
pure Python on strings, written from the definition in include/mvae.h ("Fragments") and NOT from the kernel's method --

  the molecule is fp_ref.molecule's adjacency structure (a dict of neighbour -> bond order per atom), the status chem_ref.analyse's;
  the ring bonds are scaffold_ref.ring_bonds, the non-bridge edges of a low-link search: no tree predecessors, no closure paths;
  the cut bonds are found bond by bond over the neighbour dicts, the fragments by a flood fill over the bonds that are not cut: no
  labels handed down a spanning tree;
  the keys are scaffold_ref.graph_key over each fragment's atom set, one full run per fragment;
  the fragment strings are made the way scaffold_smiles_ref.py makes the scaffold's: a NEW list of atoms, the hydrogens as the header
  states them, canon_ref.ranks and canon_ref.spell.

`fragments(s)` returns (status, [atom sets by lowest atom], desc [4], [keys]).  `fragment_smiles(s, frag)` returns (status, string, info)."""
import functools

import numpy as np

import canon_ref as CN
import chem_ref as CR
import fp_ref as FR
import scaffold_ref as SR
import scaffold_smiles_ref as SS

F = 16
FRAG_MANY = 15
NO_FRAGMENT = 16


def cut_bonds(atoms):
    """(the cut bonds, those that only rule A cuts), as sets of frozensets {a, b}."""
    members = CR._ring_atoms(atoms)
    rbonds = SR.ring_bonds(atoms)
    deg = [len(at["nb"]) for at in atoms]

    def acyl(a):
        return a not in members and any(o == 2 and atoms[b]["el"] in ("O", "S") and deg[b] == 1 for b, o in atoms[a]["nb"].items())
    cut, only_a = set(), set()
    for a in range(len(atoms)):
        for b, order in atoms[a]["nb"].items():
            e = frozenset((a, b))
            if a > b or order != 1 or e in rbonds or deg[a] < 2 or deg[b] < 2:
                continue
            rule_r = a in members or b in members
            rule_a = (acyl(a) and atoms[b]["el"] in ("N", "O", "S")) or (acyl(b) and atoms[a]["el"] in ("N", "O", "S"))
            if rule_r or rule_a:
                cut.add(e)
                if not rule_r:
                    only_a.add(e)
    return cut, only_a


def components(atoms, cut):
    """The connected components without the cut bonds, as sets, ordered by their lowest atom."""
    seen, out = set(), []
    for start in range(len(atoms)):
        if start in seen:
            continue
        part, todo = {start}, [start]
        while todo:
            u = todo.pop()
            for v in atoms[u]["nb"]:
                if v not in part and frozenset((u, v)) not in cut:
                    part.add(v)
                    todo.append(v)
        seen |= part
        out.append(part)
    return out


@functools.lru_cache(maxsize=None)
def fragments(s):
    status = CR.analyse(s)[0]
    if status != CR.OK:
        return status, [], [0, 0, 0, 0], []
    atoms = FR.molecule(s)
    cut, only_a = cut_bonds(atoms)
    parts = components(atoms, cut)
    desc = [len(parts), len(cut), len(only_a), max(len(p) for p in parts)]
    if len(parts) > F:
        return FRAG_MANY, [], desc, []
    members, rbonds = CR._ring_atoms(atoms), SR.ring_bonds(atoms)
    return status, parts, desc, [SR.graph_key(atoms, U, members, rbonds, False) for U in parts]


def expected(strings):
    """fragments() of every string as the arrays the entries write: status int32 [B], mask int64 [B, 16, 2], desc int32 [B, 4], key
    int64 [B, 16]."""
    B = len(strings)
    status, mask = np.zeros(B, np.int32), np.zeros((B, F, 2), np.int64)
    desc, key = np.zeros((B, 4), np.int32), np.zeros((B, F), np.int64)
    for b, s in enumerate(strings):
        st, parts, d, keys = fragments(s)
        status[b], desc[b] = st, d
        for f, (U, k) in enumerate(zip(parts, keys)):
            mask[b, f], key[b, f] = SR.mask_words(U), k
    return status, mask, desc, key


_CACHE = {}


def corpus_expected():
    """(strings, expected(strings)) of chem_ref's mutation corpus, computed once per process and shared: callers leave it unchanged."""
    if "c" not in _CACHE:
        strings = CR.mutation_corpus()
        _CACHE["c"] = (strings, expected(strings))
    return _CACHE["c"]


def fragment_graph(atoms, U):
    """(the atoms of the fragment U in rewrite_ref's structure, info): scaffold_smiles_ref.scaffold_graph with U in the place of S."""
    new = {a: i for i, a in enumerate(sorted(U))}
    out, made, lost_sum = [], 0, 0
    for a in sorted(U):
        at = atoms[a]
        nb = {new[b]: o for b, o in at["nb"].items() if b in U}
        lost = sum(o for b, o in at["nb"].items() if b not in U)
        h_row = at["h"] if at["bracket"] else SS.implicit(at["el"], at["arom"], sum(at["nb"].values()))
        h_u = h_row + lost
        bracket = at["bracket"] or SS.implicit(at["el"], at["arom"], sum(nb.values())) != h_u
        made += bracket and not at["bracket"]
        lost_sum += lost
        out.append({"el": at["el"], "arom": at["arom"], "bracket": bracket, "chg": at["chg"], "h": h_u if bracket else 0, "nb": nb})
    return out, [len(out), sum(len(a["nb"]) for a in out) // 2, made, lost_sum]


@functools.lru_cache(maxsize=None)
def _ranked(s, frag):
    status, atoms = CN.graph(s)
    if atoms is None:
        return status, None, None, None
    parts = components(atoms, cut_bonds(atoms)[0])
    if frag >= len(parts):
        return NO_FRAGMENT, None, None, None
    gu, info = fragment_graph(atoms, parts[frag])
    return CR.OK, gu, CN.ranks(gu)[0], info


def fragment_smiles(s, frag=0, max_content=127, have=None):
    """(status, the canonical spelling of fragment `frag` or "", info or None where the header says zeros)."""
    status, gu, rank, info = _ranked(s, frag)
    text = ""
    if status == CR.OK:
        try:
            text = CN.spell(gu, rank, max_content, have)
        except CN.Refused as r:
            status = r.args[0]
    return status, text, info


def all_fragment_smiles(s):
    """The strings of all fragments of a row fragments() gives status 0 or FRAG_MANY; [] for any other row."""
    out = []
    for f in range(128):
        st, text, _ = fragment_smiles(s, f)
        if st != CR.OK:
            break
        out.append(text)
    return out
