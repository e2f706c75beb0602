// The walk's graph cut down to an atom subset, every lost bond turned into a hydrogen of the atom that lost it (include/mvae.h,
// "Scaffold SMILES", Hydrogens).  scaffold_smiles.hip (the scaffold atom set) and fragment_smiles.hip (one fragment) share it; both run
// it between rew::read and rew::adjacency on the arrays of the writer (smiles_writer.hpp).
#pragma once
#include "common.hpp"
#include "smiles_writer.hpp"

namespace ssm {

// the members of m below atom k
SMI_HD int below(const smg::Mask& m, int k) {
  return k < 64 ? smg::popcount64(m.lo & ((1ull << (k & 63)) - 1ull)) : smg::popcount64(m.lo) + smg::popcount64(m.hi & ((1ull << (k & 63)) - 1ull));
}

// W and C cut down to the atoms of s: the atom words and the closure pairs moved down to 0 .. |s| - 1 in increasing atom order, in
// place (the new number of atom k is the members of s below k, never more than k).  A kept atom whose predecessor is dropped gets NONE,
// which the adjacency skips.  DROP = false: every closure lies inside s (a scaffold holds all ring atoms) and is renumbered.  DROP = true:
// a closure has both ends in s or neither, and those outside are dropped, the rest moved down the list.  Returns |s|; *nclos = the
// closures kept; *lost = the sum of the orders of the bonds with one end in s.
template <bool DROP, class Words, class Clos>
SMI_HD int cut(Words& W, Clos& C, int n, int* nclos, const smg::Mask& s, int* lost) {
  int m = 0, gone = 0;
  for (int k = 0; k < n; ++k) {
    const uint32_t w = W.get(k);
    const int p = k ? smg::a_pred(w) : rew::NONE;
    const bool in = smg::m_get(s, k), p_in = p != rew::NONE && smg::m_get(s, p);
    if (p != rew::NONE && in != p_in) gone += (int)(w >> 24) & 3;
    if (in) W.set(m++, (w & ~0xFFu) | (uint32_t)(p_in ? below(s, p) : rew::NONE));
  }
  int kept = 0;
  for (int c = 0; c < *nclos; ++c) {
    const int pr = C.get(c);
    if (DROP && !smg::m_get(s, pr & 0xFF)) continue;
    C.set(DROP ? kept : c, (uint16_t)(below(s, pr & 0xFF) | below(s, pr >> 8) << 8));
    ++kept;
  }
  *nclos = kept;
  *lost = gone;
  return m;
}

// The hydrogens of the unbracketed atoms behind the adjacency, which left lost(a) in the hydrogen field and the bond sums of the cut
// graph in P.  Returns the atoms that became bracket atoms.
template <class Words, class Bytes>
SMI_HD int hydrogens(Words& W, Bytes& P, int m) {
  int made = 0;
  for (int k = 0; k < m; ++k) {
    const uint32_t w = W.get(k);
    if (smg::a_brk(w)) continue;
    const int gone = rew::w_hyd(w), sum = P.get(k), e = smg::a_elem(w), ar = smg::a_arom(w);
    const int h = smg::implicit_h(e, ar, sum + gone) + gone;
    const uint32_t bare = w & ~(0xFu << 8);
    if (smg::implicit_h(e, ar, sum) == h) W.set(k, bare);
    else { W.set(k, bare | (uint32_t)(h & 0xF) << 8 | 1u << 21); ++made; }
  }
  return made;
}

}  // namespace ssm
