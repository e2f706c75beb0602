// Kekulisation test of SMILES token rows (gfx950): mvae_smiles_kekule_rows / _corpus / _host.  include/mvae.h ("Kekulisation") states the
// definition: N, the aromatic atoms that take exactly one ring double bond; E, the aromatic ring bonds among them; a row kekulises iff
// (N, E) has a perfect matching.
//
// A fourth consumer of the walk of smiles_graph.hpp, with the fingerprint's recorder (smiles_rounds.hpp).  One thread per row, 64-thread
// blocks; everything indexed by a run-time atom number lives in LDS, lane-minor, never in a private array:
//   words                      128 slots x 64 lanes x 4 B = 32 KiB   the walk's atom words; then, in the low byte, the E partner down the tree
//   closure pairs               64 x 64 x 2 B             =  8 KiB   the walk's list; a pair that is not in E becomes 0xFFFF
//   mate, parent, base, queue  4 x 128 x 64 x 1 B         = 32 KiB   the matching and the alternating forest of one search
// 72 KiB per block: two blocks per CU.  Every atom SET is an smg::Mask in registers: N, the ring bonds, the forest's even vertices, the
// bases of the blossom being contracted, the ancestors in the search for its base.
//   The graph is never copied into an adjacency structure.  Once N is known, the low byte of atom k's word -- its tree predecessor --
//   is kept if the bond k - pred(k) is in E and set to NONE otherwise, and a closure pair outside E becomes (NONE, NONE); no atom has the
//   number NONE, so the neighbours of v in E are: the low byte of its word, the atoms k > v whose low byte is v, and its partners in the
//   closure list -- one loop over n - v + nclos slots (each_nbr).
//   The matching is exact on general graphs (aromatic systems have odd rings): Edmonds' algorithm in its O(V E)-per-search form.  It
//   starts from a greedy matching in bond order (tree bonds by atom number, then the closures), then searches once from every atom of N
//   that is still free, in atom order: a breadth-first alternating forest, a blossom contracted by giving its atoms one entry in base[].
//   A search that finds no augmenting path leaves its root free for good (no later augmentation can help it), so there are at most
//   |N| - 2 * greedy searches, and most rows need none; with one free atom at most no path can exist and none is looked for.
//   Every loop carries a bound that follows from n <= 127 whatever the arrays hold, and every LDS index goes through the slot mask.
#include "common.hpp"
#include "smiles_rounds.hpp"

namespace kek {

constexpr int KEKULE = MVAE_SMILES_KEKULE;
constexpr int SLOTS = smg::ATOM_SLOTS;
constexpr int FREE = smg::NONE;        // no mate / no parent
// smallest allowed valence by charge, one nibble per element as smg::VMAX_*: the sets of a charged atom are single values but S+ {3,5}
constexpr smg::u64 VMIN_NEG = smg::VMAX_NEG, VMIN_POS = 0xFFF34F343F0ull;

// v0: the smallest allowed valence of (element, charge) that is >= used; the walk has checked used <= the largest
SMI_HD int smallest_valence(int elem, int chg, int used) {
  const smg::u64 t = chg < 0 ? VMIN_NEG : (chg > 0 ? VMIN_POS : smg::VMIN_0);
  int v0 = (int)(t >> (4 * elem)) & 0xF;
  for (int g = 0; g < 3 && v0 < used; ++g) v0 += 2;      // {3,5}, {2,4,6}, {1,3,5}: the next allowed valence is two up
  return v0;
}

// f(to) for every neighbour of v in E; f returns true to stop
template <class Words, class Clos, class F>
SMI_HD void each_nbr(Words& W, Clos& cl, int n, int nclos, int v, F f) {
  const int end = n + (nclos < fpr::CLOSURES ? nclos : fpr::CLOSURES);
  for (int e = v; e < end; ++e) {
    int to = FREE;
    if (e < n) {
      const int p = (int)(W.get(e) & 0xFFu);
      if (e == v) to = p;
      else if (p == v) to = e;
    } else {
      const int pr = cl.get(e - n), i = pr & 0xFF, j = pr >> 8;
      if (i == v) to = j;
      else if (j == v) to = i;
    }
    if (to != FREE && f(to)) return;
  }
}

template <class Bytes>
struct Forest {
  Bytes &mate, &parent, &base, &queue;
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
      each_nbr(W, cl, n, nclos, v, [&](int to) {
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

// The consumer the row driver (smiles_rounds.hpp) runs.  W: the atom words; C: the closure list; M, P, Bs, Q: the byte arrays mate, parent,
// base, queue.
struct Kekule {
  template <template <class, int> class Arr>
  struct Store {
    Arr<uint32_t, SLOTS> W;
    Arr<uint16_t, fpr::CLOSURES> C;
    Arr<uint8_t, SLOTS> M, P, Bs, Q;
  };
  typedef Store<fpr::LdsMem> Lds;
  static __device__ Store<fpr::LdsArr> lane(Lds& l) { return {l.W.lane(), l.C.lane(), l.M.lane(), l.P.lane(), l.Bs.lane(), l.Q.lane()}; }
  typedef Store<fpr::HostArr> Host;
  static_assert(sizeof(Lds) == MVAE_KEKULE_LDS_BYTES, "include/mvae.h states the LDS per block");

  struct Out {
    int32_t* status;
    int32_t* desc;
    uint8_t* mate;       // optional
    bool ok() const { return status && desc; }
  };

  // One row: the walk, N and E, the matching; all outputs are written together.
  template <class S, class Src>
  static SMI_HD void row(S& s, const Src& src, int first, int end, bool end_is_eos, int V, const int32_t* tok_info, const int32_t* chem_info,
                         int eos_id, long b, const Out& o) {
    auto& W = s.W;
    auto& C = s.C;
    auto &M = s.M, &P = s.P, &Bs = s.Bs, &Q = s.Q;
    fpr::Rec<decltype(s.C)> rec(C);
    smg::Row r;
    smg::walk(W, src, first, end, end_is_eos, V, tok_info, chem_info, eos_id, &r, rec);
    int st = r.status, nN = 0, nE = 0, pairs = 0, n = 0;
    if (r.status == smg::OK) {
      n = rec.n;
      const int nclos = rec.nclos;
      const smg::Mask rb = fpr::ring_bonds(W, C, nclos);
      smg::Mask N{0, 0};
      for (int k = 0; k < n; ++k) {
        const uint32_t w = W.get(k);
        if (smg::a_arom(w) && smallest_valence(smg::a_elem(w), smg::a_chg(w), smg::a_used(w)) - smg::a_used(w) >= 1) smg::m_set(N, k);
        M.set(k, (uint8_t)FREE);
      }
      nN = smg::m_count(N);
      // E, and the greedy matching along it.  An atom of N is aromatic, so "both ends aromatic" is part of "both ends in N".
      for (int k = 1; k < n; ++k) {
        const uint32_t w = W.get(k);
        const int p = smg::a_pred(w);
        const bool in_e = p != smg::NONE && (w >> 24) == 1u && smg::m_get(rb, k) && smg::m_get(N, k) && smg::m_get(N, p);
        if (!in_e) { W.set(k, w | 0xFFu); continue; }
        ++nE;
        if (M.get(k) == FREE && M.get(p) == FREE) { M.set(k, (uint8_t)p); M.set(p, (uint8_t)k); ++pairs; }
      }
      for (int c = 0; c < nclos; ++c) {
        const int pr = C.get(c), i = pr & 0xFF, j = pr >> 8;
        if (!smg::m_get(N, i) || !smg::m_get(N, j)) { C.set(c, (uint16_t)0xFFFFu); continue; }
        ++nE;
        if (M.get(i) == FREE && M.get(j) == FREE) { M.set(i, (uint8_t)j); M.set(j, (uint8_t)i); ++pairs; }
      }
      if (2 * pairs < nN) {
        Forest<decltype(s.M)> f{M, P, Bs, Q, N, n};
        for (int v = 0; v < n && 2 * pairs + 1 < nN; ++v) {
          if (!smg::m_get(N, v) || M.get(v) != FREE) continue;
          const int t = f.search(W, C, nclos, v);
          if (t != FREE) { f.augment(t); ++pairs; }
        }
      }
      if (2 * pairs != nN) st = KEKULE;
    }
    o.status[b] = st;
    int32_t* d = o.desc + 4 * b;
    d[0] = nN; d[1] = nE; d[2] = pairs; d[3] = nN - 2 * pairs;
    if (o.mate) {
      uint8_t* m = o.mate + b * SLOTS;
      for (int k = 0; k < SLOTS; ++k) m[k] = k < n ? M.get(k) : (uint8_t)FREE;
    }
  }
};

}  // namespace kek

extern "C" {

int mvae_smiles_kekule_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, int eos_id,
                            int32_t* status, int32_t* desc, uint8_t* mate, void* stream) {
  return fpr::rows<kek::Kekule>(B, T, V, x, x_ld, tok_info, chem_info, eos_id, stream, status, desc, mate);
}

int mvae_smiles_kekule_corpus(const uint8_t* tokens, const int64_t* offsets, int64_t N, int V, const int32_t* tok_info,
                              const int32_t* chem_info, int32_t* status, int32_t* desc, uint8_t* mate, void* stream) {
  return fpr::corpus<kek::Kekule>(tokens, offsets, N, V, tok_info, chem_info, stream, status, desc, mate);
}

int mvae_smiles_kekule_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, int eos_id,
                            int32_t* status, int32_t* desc, uint8_t* mate) {
  return fpr::host<kek::Kekule>(B, T, V, x, x_ld, tok_info, chem_info, eos_id, status, desc, mate);
}

}  // extern "C"
