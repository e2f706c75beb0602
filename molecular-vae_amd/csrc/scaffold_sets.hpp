// The atom sets of the Murcko scaffold (include/mvae.h, "Murcko scaffold"): Core and S = Core u Exo from the walk's atom words and its
// ring mask, as masks in registers.  scaffold.hip (the keys of S) and scaffold_smiles.hip (the string of S) share it; scaffold.hip says
// why one pass down and one pass up the atom numbers give what repeated leaf deletion leaves.
#pragma once
#include "common.hpp"
#include "smiles_rounds.hpp"

namespace scf {

struct Sets {
  smg::Mask core, s;
  int exo;
};

template <class Atoms>
SMI_HD Sets scaffold_sets(Atoms& at, int n, const smg::Mask& ring) {
  smg::Mask one{0, 0}, two{0, 0};      // at least one / two children whose subtree holds a ring atom
  for (int k = n - 1; k >= 1; --k) {
    if (!smg::m_get(ring, k) && !smg::m_get(one, k)) continue;
    const int p = smg::a_pred(at.get(k));
    if (p == smg::NONE) continue;
    if (smg::m_get(one, p)) smg::m_set(two, p);
    else smg::m_set(one, p);
  }
  Sets r{ring, {0, 0}, 0};
  smg::Mask up{0, 0}, exo{0, 0};       // up: the part outside the atom's subtree holds a ring atom
  for (int k = 0; k < n; ++k) {
    const uint32_t w = at.get(k);
    const int p = k ? smg::a_pred(w) : smg::NONE;
    const bool sub = smg::m_get(ring, k) || smg::m_get(one, k);
    bool u = false;
    if (p != smg::NONE) u = smg::m_get(up, p) || smg::m_get(ring, p) || smg::m_get(two, p) || (smg::m_get(one, p) && !sub);
    if (u) smg::m_set(up, k);
    if (!smg::m_get(ring, k) && (smg::m_get(two, k) || (smg::m_get(one, k) && u))) smg::m_set(r.core, k);
    // a predecessor has a lower number: its Core bit is final
    if (p != smg::NONE && (w >> 24) == 2u) {
      const bool ck = smg::m_get(r.core, k), cp = smg::m_get(r.core, p);
      if (cp && !ck) smg::m_set(exo, k);
      if (ck && !cp) smg::m_set(exo, p);
    }
  }
  r.s = fpr::m_or(r.core, exo);
  r.exo = smg::m_count(exo);
  return r;
}

}  // namespace scf
