// The exact matching of "Kekulisation" (include/mvae.h) on the walk's arrays: what kekule.hip (does the row kekulise, and how) and
// smiles_aromatize.hip (the set N, and whether the row kekulises at all) share.  N, the aromatic atoms that take exactly one ring double
// bond; E, the aromatic ring bonds among them; the neighbours of an atom in E (each_nbr); one search of Edmonds' algorithm (Forest);
// and the greedy matching in bond order with the searches behind it (match).
//   The graph is never copied into an adjacency structure, and the walk's arrays stay a graph: a tree bond k - pred(k) that is in E is
//   marked in bit 31 of atom k's word (bits 26-31 belong to the recorder's byte and the walk's order is <= 3), and a closure pair is in E
//   iff both its ends are in N (a closure is a ring bond of order 1).  The neighbours of v in E are then: its predecessor if its own word
//   is marked, the marked atoms k > v whose predecessor is v, and its partners in the closure list that are in N -- one loop over
//   n - v + nclos slots.  A caller that goes on with the words clears bit 31 (rew::adjacency does).
//   The matching is exact on general graphs (aromatic systems have odd rings): Edmonds' algorithm in its O(V E)-per-search form.  It
//   starts from a greedy matching in bond order (tree bonds by atom number, then the closures), then searches once from every atom of N
//   that is still free, in atom order: a breadth-first alternating forest, a blossom contracted by giving its atoms one entry in base[].
//   A search that finds no augmenting path leaves its root free for good (no later augmentation can help it), so there are at most
//   |N| - 2 * greedy searches, and most rows need none; with one free atom at most no path can exist and none is looked for.
//   The four byte arrays (mate, parent, base, queue) may be of four types: kekule.hip has four arrays of 128, smiles_aromatize.hip lends
//   the two halves of the writer's half-edge list and two of its byte arrays.
//   Every loop carries a bound that follows from n <= 127 whatever the arrays hold, and every index goes through the slot mask.
#pragma once
#include "common.hpp"
#include "smiles_rounds.hpp"

namespace kek {

constexpr int KEKULE = MVAE_SMILES_KEKULE;
constexpr int SLOTS = smg::ATOM_SLOTS;
constexpr int FREE = smg::NONE;        // no mate / no parent
constexpr uint32_t IN_E = 1u << 31;    // atom word: the bond to the tree predecessor is in E
// smallest allowed valence by charge, one nibble per element as smg::VMAX_*: the sets of a charged atom are single values but S+ {3,5}
constexpr smg::u64 VMIN_NEG = smg::VMAX_NEG, VMIN_POS = 0xFFF34F343F0ull;

// v0: the smallest allowed valence of (element, charge) that is >= used; the walk has checked used <= the largest
SMI_HD int smallest_valence(int elem, int chg, int used) {
  const smg::u64 t = chg < 0 ? VMIN_NEG : (chg > 0 ? VMIN_POS : smg::VMIN_0);
  int v0 = (int)(t >> (4 * elem)) & 0xF;
  for (int g = 0; g < 3 && v0 < used; ++g) v0 += 2;      // {3,5}, {2,4,6}, {1,3,5}: the next allowed valence is two up
  return v0;
}

// N: the aromatic atoms whose used valence is below the smallest allowed one
template <class Words>
SMI_HD smg::Mask set_n(Words& W, int n) {
  smg::Mask N{0, 0};
  for (int k = 0; k < n; ++k) {
    const uint32_t w = W.get(k);
    if (smg::a_arom(w) && smallest_valence(smg::a_elem(w), smg::a_chg(w), smg::a_used(w)) - smg::a_used(w) >= 1) smg::m_set(N, k);
  }
  return N;
}

// f(to) for every neighbour of v in E; f returns true to stop
template <class Words, class Clos, class F>
SMI_HD void each_nbr(Words& W, Clos& cl, const smg::Mask& N, int n, int nclos, int v, F f) {
  const int end = n + (nclos < fpr::CLOSURES ? nclos : fpr::CLOSURES);
  for (int e = v; e < end; ++e) {
    int to = FREE;
    if (e < n) {
      const uint32_t w = W.get(e);
      if (!(w & IN_E)) continue;
      const int p = smg::a_pred(w);
      if (e == v) to = p;
      else if (p == v) to = e;
    } else {
      const int pr = cl.get(e - n), i = pr & 0xFF, j = pr >> 8;
      if (i == v) to = j;
      else if (j == v) to = i;
      if (to != FREE && !smg::m_get(N, to)) to = FREE;
    }
    if (to != FREE && f(to)) return;
  }
}

template <class BM, class BP, class BB, class BQ>
struct Forest {
  BM& mate;
  BP& parent;
  BB& base;
  BQ& queue;
  smg::Mask N;
  int n;

  // the base of the blossom that the edge (a, b) between two even vertices closes: the first common vertex of their paths to the root
  SMI_HD int common_base(int a, int b) const {
    smg::Mask seen{0, 0};
    for (int g = 0; g < SLOTS; ++g) {
      a = base.get(a);
      smg::m_set(seen, a);
      const int m = mate.get(a);
      if (m == FREE) break;              // the root
      a = parent.get(m);
      if (a == FREE) break;              // cannot happen: a matched even vertex was reached through its mate
    }
    for (int g = 0; g < SLOTS; ++g) {
      b = base.get(b);
      if (smg::m_get(seen, b)) return b;
      const int m = mate.get(b);
      if (m == FREE) break;
      b = parent.get(m);
      if (b == FREE) break;
    }
    return b;
  }

  // marks the bases on the path from v down to the blossom's base and turns the parents round, so that every atom of the blossom can
  // be left through either side
  SMI_HD void mark_path(int v, int b, int child, smg::Mask& blossom) {
    for (int g = 0; g < SLOTS && base.get(v) != b; ++g) {
      const int m = mate.get(v);
      if (m == FREE) break;              // cannot happen: only the root is free, and the root is the base of every blossom it is in
      smg::m_set(blossom, base.get(v));
      smg::m_set(blossom, base.get(m));
      parent.set(v, (uint8_t)child);
      child = m;
      v = parent.get(m);
      if (v == FREE) break;
    }
  }

  // One search from the free atom root.  Returns the free atom at the end of an augmenting path, FREE if there is none.
  template <class Words, class Clos>
  SMI_HD int search(Words& W, Clos& cl, int nclos, int root) {
    for (int k = 0; k < n; ++k) {
      parent.set(k, (uint8_t)FREE);
      base.set(k, (uint8_t)k);
    }
    smg::Mask even{0, 0};
    smg::m_set(even, root);
    queue.set(0, (uint8_t)root);
    int head = 0, tail = 1, found = FREE;
    // every atom enters the queue at most once (the even mask), so head < tail <= n
    while (head < tail && head < SLOTS && found == FREE) {
      const int v = queue.get(head++);
      each_nbr(W, cl, N, n, nclos, v, [&](int to) {
        if (base.get(v) == base.get(to) || mate.get(v) == to) return false;
        const int mt = mate.get(to);
        if (to == root || (mt != FREE && parent.get(mt) != FREE)) {
          // to is even too: an odd cycle.  Contract it.
          const int b = common_base(v, to);
          smg::Mask blossom{0, 0};
          mark_path(v, b, to, blossom);
          mark_path(to, b, v, blossom);
          for (int k = 0; k < n; ++k) {
            if (!smg::m_get(N, k) || !smg::m_get(blossom, base.get(k))) continue;
            base.set(k, (uint8_t)b);
            if (!smg::m_get(even, k) && tail < SLOTS) {
              smg::m_set(even, k);
              queue.set(tail++, (uint8_t)k);
            }
          }
        } else if (parent.get(to) == FREE) {
          parent.set(to, (uint8_t)v);
          if (mt == FREE) { found = to; return true; }
          if (!smg::m_get(even, mt) && tail < SLOTS) {
            smg::m_set(even, mt);
            queue.set(tail++, (uint8_t)mt);
          }
        }
        return false;
      });
    }
    return found;
  }

  // flips the path that ends in the free atom v
  SMI_HD void augment(int v) {
    for (int g = 0; g < SLOTS && v != FREE; ++g) {
      const int pv = parent.get(v);
      if (pv == FREE) break;             // cannot happen: the path leads to the root through parents
      const int next = mate.get(pv);
      mate.set(v, (uint8_t)pv);
      mate.set(pv, (uint8_t)v);
      v = next;
    }
  }
};

// E marked in the words, the greedy matching along it, and a search from every atom of N that it left free.  rb: fpr::ring_bonds of the
// row.  Returns the matched pairs (the row kekulises iff 2 * pairs == |N|); M holds the mates of atoms 0 .. n - 1, *nE = |E|.
template <class Words, class Clos, class BM, class BP, class BB, class BQ>
SMI_HD int match(Words& W, Clos& C, BM& M, BP& P, BB& Bs, BQ& Q, int n, int nclos, const smg::Mask& rb, const smg::Mask& N, int* nE) {
  const int nN = smg::m_count(N);
  int pairs = 0, edges = 0;
  for (int k = 0; k < n; ++k) M.set(k, (uint8_t)FREE);
  // An atom of N is aromatic, so "both ends aromatic" is part of "both ends in N".
  for (int k = 1; k < n; ++k) {
    const uint32_t w = W.get(k);
    const int p = smg::a_pred(w);
    const bool in_e = p != smg::NONE && (w >> 24) == 1u && smg::m_get(rb, k) && smg::m_get(N, k) && smg::m_get(N, p);
    if (!in_e) continue;
    W.set(k, w | IN_E);
    ++edges;
    if (M.get(k) == FREE && M.get(p) == FREE) { M.set(k, (uint8_t)p); M.set(p, (uint8_t)k); ++pairs; }
  }
  for (int c = 0; c < nclos; ++c) {
    const int pr = C.get(c), i = pr & 0xFF, j = pr >> 8;
    if (!smg::m_get(N, i) || !smg::m_get(N, j)) continue;
    ++edges;
    if (M.get(i) == FREE && M.get(j) == FREE) { M.set(i, (uint8_t)j); M.set(j, (uint8_t)i); ++pairs; }
  }
  if (2 * pairs < nN) {
    Forest<BM, BP, BB, BQ> f{M, P, Bs, Q, N, n};
    for (int v = 0; v < n && 2 * pairs + 1 < nN; ++v) {
      if (!smg::m_get(N, v) || M.get(v) != FREE) continue;
      const int t = f.search(W, C, nclos, v);
      if (t != FREE) { f.augment(t); ++pairs; }
    }
  }
  *nE = edges;
  return pairs;
}

}  // namespace kek
