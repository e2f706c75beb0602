// Where a row is cut into fragments and which fragment an atom lands in (include/mvae.h, "Fragments"): the cut set as a mask in
// registers (bit k: the tree bond k - pred(k) is cut) and the component labels from one pass up the atom numbers.  fragment.hip (the
// keys of the fragments) and fragment_smiles.hip (the string of one fragment) share it.
//   A cut bond is a bridge, and every bridge is a tree bond, so the fragments are the parts the walk's tree falls into when the cut
//   bonds are taken out of it; a closure joins two atoms of one part, because its tree path is made of ring bonds and none of them is
//   cut.  An atom's predecessor has a lower number, so the lowest atom of a part is its root and the labels, handed out at the roots in
//   atom order, number the fragments by their lowest atom.
#pragma once
#include "common.hpp"
#include "smiles_rounds.hpp"

namespace frg {

constexpr int E_N = 3, E_O = 4, E_S = 7;           // smiles_graph.hpp: H B C N O F P S Cl Br I

struct Cuts {
  smg::Mask cut;
  int acyl_only;                       // the cut bonds that rule A alone cuts
};

// D[k] := deg(k), the bonds of atom k in the row's graph; returns the cut set.  at: atom words (predecessor, bond order in bits 24-31,
// element); ring: the walk's ring members; rb: fpr::ring_bonds.
template <class Atoms, class Deg, class Clos>
SMI_HD Cuts cut_bonds(Atoms& at, Deg& D, Clos& cl, int n, int nclos, const smg::Mask& ring, const smg::Mask& rb) {
  for (int k = 0; k < n; ++k) D.set(k, 0);
  fpr::each_bond(at, cl, n, nclos, [&](int a, int b, uint32_t) {
    D.set(a, D.get(a) + 1);
    D.set(b, D.get(b) + 1);
  });
  // rule A's carbonyl-like centres: the non-ring atoms with a double bond to an O or S atom of degree 1.  A closure has order 1.
  smg::Mask acyl{0, 0};
  for (int k = 1; k < n; ++k) {
    const uint32_t w = at.get(k);
    const int p = smg::a_pred(w);
    if (p == smg::NONE || (w >> 24) != 2u) continue;
    const int ek = smg::a_elem(w), ep = smg::a_elem(at.get(p));
    if ((ek == E_O || ek == E_S) && D.get(k) == 1 && !smg::m_get(ring, p)) smg::m_set(acyl, p);
    if ((ep == E_O || ep == E_S) && D.get(p) == 1 && !smg::m_get(ring, k)) smg::m_set(acyl, k);
  }
  Cuts r{{0, 0}, 0};
  for (int k = 1; k < n; ++k) {
    const uint32_t w = at.get(k);
    const int p = smg::a_pred(w);
    if (p == smg::NONE || (w >> 24) != 1u || smg::m_get(rb, k)) continue;
    if (D.get(k) < 2 || D.get(p) < 2) continue;
    const int ek = smg::a_elem(w), ep = smg::a_elem(at.get(p));
    const bool by_ring = smg::m_get(ring, k) || smg::m_get(ring, p);
    const bool by_acyl = (smg::m_get(acyl, k) && (ep == E_N || ep == E_O || ep == E_S)) || (smg::m_get(acyl, p) && (ek == E_N || ek == E_O || ek == E_S));
    if (!by_ring && !by_acyl) continue;
    smg::m_set(r.cut, k);
    if (!by_ring) ++r.acyl_only;
  }
  return r;
}

// L[k] := the number of atom k's fragment; returns the number of fragments
template <class Atoms, class Lab>
SMI_HD int labels(Atoms& at, int n, const smg::Mask& cut, Lab& L) {
  int nf = 0;
  for (int k = 0; k < n; ++k) {
    const int p = k ? smg::a_pred(at.get(k)) : smg::NONE;
    if (p == smg::NONE || smg::m_get(cut, k)) L.set(k, nf++);
    else L.set(k, L.get(p));
  }
  return nf;
}

// the atoms whose label is f
template <class Lab>
SMI_HD smg::Mask members(Lab& L, int n, int f) {
  smg::Mask u{0, 0};
  for (int k = 0; k < n; ++k)
    if ((int)L.get(k) == f) smg::m_set(u, k);
  return u;
}

}  // namespace frg
