// The graph key of an atom subset (include/mvae.h, "Graph key") and what it runs on: the 16-bit packed atoms, the 16-bit array seen as
// the walk's closure list and as atom words, the first invariant, the degrees, the refinement rounds and the fold of the final ids.
// scaffold.hip (molecule key, scaffold key) and fragment.hip (one key per fragment) share it; scaffold.hip says how the arrays are laid out.
#pragma once
#include "common.hpp"
#include "smiles_rounds.hpp"

namespace scf {

constexpr int ROUNDS = MVAE_GRAPH_KEY_ROUNDS;

// The 16 bits of an atom word the rounds and the scaffold key's first ids read: predecessor (7 bits; atom 0 has none and is never asked),
// bond order to it (2), aromatic flag, element (4), charge + 1 (2)
SMI_HD uint16_t pack(uint32_t w) {
  return (uint16_t)((w & 0x7Fu) | ((w >> 24) & 3u) << 7 | (uint32_t)smg::a_arom(w) << 9 | (uint32_t)smg::a_elem(w) << 10 | ((w >> 22) & 3u) << 14);
}
SMI_HD uint32_t unpack(uint32_t e) {     // an atom word again, with used valence 0
  return (e & 0x7Fu) | ((e >> 10) & 0xFu) << 16 | ((e >> 9) & 1u) << 20 | ((e >> 14) & 3u) << 22 | ((e >> 7) & 3u) << 24;
}

// the 16-bit array as the walk's closure list (from the top down) and as atom words for each_bond (from the bottom up)
template <class Half>
struct TopClos {
  Half& h;
  SMI_HD int get(int c) const { return h.get(smg::ATOM_SLOTS - 1 - c); }
  SMI_HD void set(int c, uint16_t v) { h.set(smg::ATOM_SLOTS - 1 - c, v); }
};
template <class Half>
struct PackedAtoms {
  Half& h;
  SMI_HD uint32_t get(int k) const { return unpack(h.get(k)); }
};

// w_U(a) without the used valence
SMI_HD uint32_t invariant(uint32_t w, bool in_ring, uint32_t degree) {
  return (uint32_t)smg::a_elem(w) | (uint32_t)smg::a_arom(w) << 4 | (uint32_t)(smg::a_chg(w) + 1) << 5 | (uint32_t)in_ring << 7 | degree << 8;
}

// D[k] := the number of bonds of atom k inside U; returns the number of bonds inside U
template <class Atoms, class Ids, class Clos>
SMI_HD int degrees(Atoms& at, Ids& D, Clos& cl, int n, int nclos, const smg::Mask& U) {
  for (int k = 0; k < n; ++k) D.set(k, 0u);
  int nb = 0;
  fpr::each_bond(at, cl, n, nclos, [&](int a, int b, uint32_t) {
    if (!smg::m_get(U, a) || !smg::m_get(U, b)) return;
    D.set(a, D.get(a) + 1u);
    D.set(b, D.get(b) + 1u);
    ++nb;
  });
  return nb;
}

// The rounds: the first ids in I become id_8 for the atoms of U, over the bonds inside U that keep(a, b) lets through.  D: the neighbour sums.
template <class Atoms, class Ids, class Clos, class Keep>
SMI_HD void refine(Atoms& at, Ids& I, Ids& D, Clos& cl, int n, int nclos, const smg::Mask& U, const smg::Mask& rb, Keep keep) {
  for (uint32_t r = 1; r <= (uint32_t)ROUNDS; ++r) {
    for (int k = 0; k < n; ++k) D.set(k, 0u);
    // each_bond hands a tree bond as (k, pred(k)), k > pred(k), and a closure as (opener, closer), opener < closer
    fpr::each_bond(at, cl, n, nclos, [&](int a, int b, uint32_t bt) {
      if (!smg::m_get(U, a) || !smg::m_get(U, b) || !keep(a, b)) return;
      const uint32_t in_ring = a > b ? (uint32_t)smg::m_get(rb, a) : 1u;
      const uint32_t key = (bt + 8u * in_ring) * 0x7FEB352Du, ia = I.get(a), ib = I.get(b);
      D.set(a, D.get(a) + fpr::mix(ib ^ key));
      D.set(b, D.get(b) + fpr::mix(ia ^ key));
    });
    for (int k = 0; k < n; ++k)
      if (smg::m_get(U, k)) I.set(k, fpr::mix(I.get(k) * 0x9E3779B1u + r + D.get(k)));
  }
}

// what one atom's final id adds to the two sums of a key
SMI_HD void add_id(uint32_t id, uint32_t* lo, uint32_t* hi) {
  *lo += fpr::mix(id);
  *hi += fpr::mix(id ^ 0x5BD1E995u);
}

// the key of a subset of `atoms` atoms and nb bonds from the two sums over its final ids
SMI_HD uint64_t fold(uint32_t lo, uint32_t hi, int atoms, int nb) {
  lo = fpr::mix((uint32_t)atoms * 0x9E3779B1u + lo);
  hi = fpr::mix((uint32_t)nb * 0x85EBCA6Bu + hi);
  const uint64_t key = (uint64_t)lo | (uint64_t)hi << 32;
  return key ? key : 1ull;
}

// The key of the atom subset U with its nb induced bonds, from the first ids in I.  D: the neighbour sums.
template <class Atoms, class Ids, class Clos>
SMI_HD uint64_t graph_key(Atoms& at, Ids& I, Ids& D, Clos& cl, int n, int nclos, const smg::Mask& U, const smg::Mask& rb, int nb) {
  refine(at, I, D, cl, n, nclos, U, rb, [](int, int) { return true; });
  uint32_t lo = 0u, hi = 0u;
  for (int k = 0; k < n; ++k) {
    if (!smg::m_get(U, k)) continue;
    add_id(I.get(k), &lo, &hi);
  }
  return fold(lo, hi, smg::m_count(U), nb);
}

}  // namespace scf
