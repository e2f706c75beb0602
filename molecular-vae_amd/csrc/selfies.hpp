// SELFIES on the writer's arrays (include/mvae.h, "SELFIES", states the definition): the derivation of a SELFIES token row into the
// walk's graph (sf::derive), the ring bonds applied to it and the multiple ones made tree bonds (sf::apply_rings, sf::reparent), and the
// translation of a SMILES row's graph into SELFIES tokens in its own atom order (sf::kekulise, sf::sizes, sf::emit_row).  Host and device
// compile the same functions.  selfies.hip holds the two families the writer driver runs and the entries.
//   Decoding is an eleventh producer of the walk's graph: it fills the atom words W and the closure list C as smg::walk would have filled
//   them for the SMILES row it denotes, and rew::adjacency, can::ranks and rew::write take them unchanged.  Until the adjacency exists the
//   byte arrays S, D, P are free, and they hold the branch stack (root atom, end column, resume state), one level per slot: a level
//   costs a branch symbol, so the depth stays below the row length.  The deferred ring bonds wait in C, l | r << 7 | order << 14.
//   Encoding needs no stack: the atoms in increasing number are a pre-order in which every parenthesised branch is a contiguous range.
//   The matching of kekule.hpp runs on lent arrays as in smiles_aromatize.hip; the subtree sizes are in S, the last child of every atom in
//   D, the ring symbols an atom closes in P, and the output is staged in the first half of A, because C, which shares LDS with O, is read
//   until the last symbol is out.
// No runtime-indexed private array, no recursion; every loop is bounded by the row length (<= 127 symbols, atoms and ring bonds) and every
// index goes through a slot mask.
#pragma once
#include "common.hpp"
#include "kekule.hpp"
#include "smiles_writer.hpp"

namespace sf {

enum : int { CAPACITY = MVAE_SELFIES_CAPACITY };
constexpr int NONE = smg::NONE;
constexpr int E_I = 10;
// the info word of a symbol (vocab.selfies_info_table)
enum : int { K_OTHER = 0, K_ATOM, K_BRANCH, K_RING, K_NOP, K_EOS };
SMI_HD int i_kind(int32_t w) { return w & 7; }
SMI_HD int i_beta(int32_t w) { return (w >> 3) & 3; }
SMI_HD int i_elem(int32_t w) { return (w >> 5) & 0xF; }
SMI_HD int i_chg(int32_t w) { return ((w >> 9) & 3) - 1; }
SMI_HD int i_brk(int32_t w) { return (w >> 11) & 1; }
SMI_HD int i_hyd(int32_t w) { return (w >> 12) & 7; }
SMI_HD int i_len(int32_t w) { return (w >> 16) & 3; }
SMI_HD int i_index(int32_t w) { return (w >> 20) & 0xF; }
// the roles of the emit table (vocab.selfies_emit_table)
constexpr int EM_BRANCH = 495, EM_RING = 504, EM_INDEX = 513;
static_assert(EM_INDEX + 16 == MVAE_SELFIES_EMIT, "the emit table");
SMI_HD int em_atom(int beta, int elem, int chg, int h) { return (((beta - 1) * smg::E + elem) * 3 + chg + 1) * 5 + h; }

SMI_HD int min2(int a, int b) { return a < b ? a : b; }

// cap(atom): the bonds an atom of (element, charge) with h stated hydrogens can make
SMI_HD int cap(int elem, int chg, int h) { return (elem == E_I && chg == 0 ? 1 : smg::vmax(elem, chg)) - h; }

// While a row is derived, an atom word holds the bond sum in the used-valence field and the stated hydrogens in bits 26-28.
SMI_HD int w_stated(uint32_t w) { return (int)(w >> 26) & 7; }
SMI_HD int w_left(uint32_t w) { return cap(smg::a_elem(w), smg::a_chg(w), w_stated(w)) - smg::a_used(w); }
SMI_HD int w_order(uint32_t w) { return (int)(w >> 24) & 3; }
SMI_HD uint32_t w_with_bond(uint32_t w, int pred, int order) { return (w & ~(0xFFu | 3u << 24)) | (uint32_t)pred | (uint32_t)order << 24; }

struct Derived { int status, col, n, nring; };

// The derivation.  Returns the atoms in W (bond sums, no hydrogens yet) and the deferred ring bonds in C.
template <class Words, class Clos, class Bytes, class Src>
SMI_HD Derived derive(Words& W, Clos& C, Bytes& S, Bytes& D, Bytes& P, const Src& src, int first, int end, int V, const int32_t* sinfo) {
  // the row's end and the tokens that are no symbols; more than 127 symbols are refused at the 128th
  int stop = end;
  for (int t = first; t < end; ++t) {
    const long tok = src.tok(t);
    const int kind = tok < 0 || tok >= V ? K_OTHER : i_kind(sinfo[tok]);
    if (kind == K_EOS) { stop = t; break; }
    if (kind == K_OTHER || t - first >= smg::CONTENT_MAX) return {smg::SYNTAX, t, 0, 0};
  }
  int s = 0, prev = NONE, n = 0, nring = 0, depth = 0, bend = stop, t = first;
  // every step reads a symbol or leaves a branch, and a branch costs a symbol
  for (int g = 0; g < 2 * smg::ATOM_SLOTS + 2; ++g) {
    if (t >= bend) {
      if (depth == 0) break;
      --depth;
      prev = S.get(depth);
      bend = first + D.get(depth);
      s = P.get(depth);
      continue;
    }
    const int32_t w = sinfo[src.tok(t)];
    const int kind = i_kind(w), beta = i_beta(w), L = i_len(w);
    ++t;
    if (kind == K_ATOM) {
      const int c = cap(i_elem(w), i_chg(w), i_hyd(w));
      const int o = s == 0 ? 0 : min2(min2(beta, s), c);
      if (n > 0 && o < 1) return {smg::SYNTAX, t - 1, 0, 0};        // cannot happen: SelfiesVocab takes no symbol of capacity 0
      const int k = n++;
      if (prev != NONE) W.set(prev, W.get(prev) + ((uint32_t)o << 8));
      W.set(k, smg::a_make(prev, o, i_elem(w), 0, i_brk(w), i_chg(w)) | (uint32_t)o << 24 | (uint32_t)i_hyd(w) << 26);
      prev = k;
      s = c - o;
      if (s <= 0) { s = 0; t = bend; }
      continue;
    }
    if (kind != K_BRANCH && kind != K_RING) continue;    // nop
    if (kind == K_BRANCH ? s <= 1 : s == 0) continue;    // skipped: its index symbols are read as ordinary symbols
    int Q = 0;
    for (int i = 0; i < L; ++i) Q = 16 * Q + (t + i < bend ? i_index(sinfo[src.tok(t + i)]) : 0);
    t = min2(t + L, bend);
    if (kind == K_BRANCH) {
      const int b = min2(s - 1, beta);
      S.set(depth, (uint8_t)prev);
      D.set(depth, (uint8_t)(bend - first));
      P.set(depth, (uint8_t)(s - b));
      ++depth;
      bend = min2(t + Q + 1, bend);
      s = b;
    } else {
      const int o = min2(beta, s), l = prev - (Q + 1);
      // A ring bond costs its symbol and an index symbol (only the last one of a row or branch can lack it, and a branch costs a symbol
      // more), and it needs an atom in front: 127 symbols hold at most 63 of them, so the list of 64 never fills and nothing is dropped.
      if (nring < fpr::CLOSURES) C.set(nring++, (uint16_t)((l > 0 ? l : 0) | prev << 7 | o << 14));
      s -= o;
      if (s == 0) t = bend;
    }
  }
  if (n == 0) return {smg::SYNTAX, stop, 0, 0};
  return {smg::OK, -1, n, nring};
}

// The deferred ring bonds in order.  The bonds that stay are left in C[0 .. return) in the same packing.
template <class Words, class Clos>
SMI_HD int apply_rings(Words& W, Clos& C, int nring) {
  int kept = 0;
  for (int c = 0; c < nring && c < fpr::CLOSURES; ++c) {
    const int v = C.get(c), l = v & 0x7F, r = (v >> 7) & 0x7F;
    if (l == r) continue;
    const uint32_t wl = W.get(l), wr = W.get(r);
    int o = min2(v >> 14, min2(w_left(wl), w_left(wr)));
    if (o <= 0) continue;
    if (smg::a_pred(wr) == l) {        // l < r, so a tree bond between them stands in r's word
      o = min2(o, 3 - w_order(wr));
      W.set(r, wr + ((uint32_t)o << 24) + ((uint32_t)o << 8));
      W.set(l, wl + ((uint32_t)o << 8));
      continue;
    }
    int at = kept;
    for (int j = 0; j < kept; ++j)
      if ((C.get(j) & 0x3FFF) == (v & 0x3FFF)) { at = j; break; }
    if (at < kept) o = min2(o, 3 - (C.get(at) >> 14));
    else C.set(kept++, (uint16_t)(v & 0x3FFF));
    C.set(at, (uint16_t)(C.get(at) + (o << 14)));
    W.set(r, wr + ((uint32_t)o << 8));
    W.set(l, wl + ((uint32_t)o << 8));
  }
  return kept;
}

// whether atom a is atom b or one of its tree descendants
template <class Words>
SMI_HD bool below(Words& W, int a, int b) {
  for (int g = 0; g < smg::ATOM_SLOTS && a != NONE; ++g) {
    if (a == b) return true;
    a = smg::a_pred(W.get(a));
  }
  return false;
}

// A ring bond of order >= 2 becomes a tree bond: an end whose own tree bond is single, and below which the other end does not hang, takes
// the other end as its predecessor, and its old tree bond becomes the closure.  Then C holds what the walk would have left: i | j << 8.
// Returns the bonds re-parented, -1 if one could not be.
template <class Words, class Clos>
SMI_HD int reparent(Words& W, Clos& C, int kept) {
  int moved = 0;
  for (int c = 0; c < kept; ++c) {
    const int v = C.get(c), o = v >> 14;
    int l = v & 0x7F, r = (v >> 7) & 0x7F;
    if (o >= 2) {
      const uint32_t wr = W.get(r), wl = W.get(l);
      int child = NONE, other = NONE;
      if (smg::a_pred(wr) != NONE && w_order(wr) == 1 && !below(W, l, r)) { child = r; other = l; }
      else if (smg::a_pred(wl) != NONE && w_order(wl) == 1 && !below(W, r, l)) { child = l; other = r; }
      if (child == NONE) return -1;
      const uint32_t wc = W.get(child);
      l = smg::a_pred(wc);
      r = child;
      W.set(child, w_with_bond(wc, other, o));
      ++moved;
    }
    C.set(c, (uint16_t)(l | r << 8));
  }
  return moved;
}

// the words as the adjacency wants them: bonds + stated hydrogens in the used-valence field, bits 26-31 clear
template <class Words>
SMI_HD void finish_words(Words& W, int n) {
  for (int k = 0; k < n; ++k) {
    const uint32_t w = W.get(k);
    W.set(k, (w & 0x03FFFFFFu) + ((uint32_t)w_stated(w) << 8));
  }
}

// ------------------------------------------------------------------------------------------------------------------------- encode
// one 128-slot half of the half-edge list as a byte array of its own
template <class Half, int OFF>
struct HalfView {
  Half& a;
  SMI_HD int get(int i) const { return a.get(OFF + (i & (rew::SLOTS - 1))); }
  SMI_HD void set(int i, uint8_t v) { a.set(OFF + (i & (rew::SLOTS - 1)), v); }
};

constexpr int CLOS_DOUBLE = 0x80;      // closure word, bit 7: the closure is double after kekulisation (an atom number is <= 126)

// The matching of "Kekulisation" made explicit: the bonds (a, mate[a]) double, no aromatic flag.  False if there is no perfect matching.
template <class Words, class Clos, class Half, class Bytes>
SMI_HD bool kekulise(Words& W, Clos& C, Half& A, Bytes& S, Bytes& D, int n, int nclos) {
  bool any = false;
  for (int k = 0; k < n; ++k) any = any || smg::a_arom(W.get(k));
  if (!any) return true;
  const smg::Mask rb = fpr::ring_bonds(W, C, nclos);
  const smg::Mask N = kek::set_n(W, n);
  HalfView<Half, 0> mate{A};
  HalfView<Half, rew::SLOTS> parent{A};
  int edges;
  if (2 * kek::match(W, C, mate, parent, S, D, n, nclos, rb, N, &edges) != smg::m_count(N)) return false;
  for (int c = 0; c < nclos; ++c) {
    const int v = C.get(c), i = v & 0xFF, j = v >> 8;
    if (smg::m_get(N, i) && mate.get(i) == j) C.set(c, (uint16_t)(v | CLOS_DOUBLE));
  }
  for (int k = 0; k < n; ++k) {
    uint32_t w = W.get(k);
    if (smg::m_get(N, k)) {
      w += 1u << 8;
      if ((w & kek::IN_E) && mate.get(k) == smg::a_pred(w)) w = (w & ~(3u << 24)) | 2u << 24;
    }
    W.set(k, w & ~(kek::IN_E | 1u << 20));
  }
  return true;
}

SMI_HD int index_len(int Q) { return Q < 16 ? 1 : 2; }
SMI_HD int sat_add(int a, int b) { return a + b < 255 ? a + b : 255; }

// The bond sums (P), from them the hydrogens of every atom's symbol (bits 26-28 of its word) and the capacity test; the ring symbols of
// every atom (P again); the last child (D); the subtree sizes in symbols, saturating (S).  Returns the atom over its capacity, NONE if
// there is none.
template <class Words, class Clos, class Bytes>
SMI_HD int sizes(Words& W, Clos& C, Bytes& S, Bytes& D, Bytes& P, int n, int nclos) {
  for (int k = 0; k < n; ++k) { P.set(k, 0); D.set(k, (uint8_t)NONE); S.set(k, 1); }
  for (int k = 1; k < n; ++k) {
    const uint32_t w = W.get(k);
    const int p = smg::a_pred(w), o = w_order(w);
    if (p == NONE) continue;
    P.set(k, (uint8_t)(P.get(k) + o)); P.set(p, (uint8_t)(P.get(p) + o));
    D.set(p, (uint8_t)k);
  }
  for (int c = 0; c < nclos; ++c) {
    const int v = C.get(c), i = v & 0x7F, j = v >> 8, o = v & CLOS_DOUBLE ? 2 : 1;
    P.set(i, (uint8_t)(P.get(i) + o)); P.set(j, (uint8_t)(P.get(j) + o));
  }
  int over = NONE;
  for (int k = n - 1; k >= 0; --k) {
    const uint32_t w = W.get(k);
    const int e = smg::a_elem(w), chg = smg::a_chg(w), sum = P.get(k);
    int h = smg::a_brk(w) ? smg::a_used(w) - sum : 0;
    // a bracket atom with neither hydrogens nor charge, or with more than four hydrogens: no symbol says that
    if (smg::a_brk(w) && ((h == 0 && chg == 0 && e != smg::E_H) || h > 4)) h = 7;
    if (h < 7 && sum > cap(e, chg, h)) over = k;
    W.set(k, (w & 0x03FFFFFFu) | (uint32_t)h << 26);
    P.set(k, 0);
  }
  for (int c = 0; c < nclos; ++c) {
    const int v = C.get(c), i = v & 0x7F, j = v >> 8, r = i > j ? i : j, l = i > j ? j : i;
    if (l == r) continue;
    P.set(r, (uint8_t)(P.get(r) + 1));
    S.set(r, (uint8_t)sat_add(S.get(r), 1 + index_len(r - l - 1)));
  }
  for (int k = n - 1; k >= 1; --k) {
    const int p = smg::a_pred(W.get(k)), sz = S.get(k);
    if (p == NONE) continue;
    S.set(p, (uint8_t)sat_add(S.get(p), D.get(p) == k ? sz : sat_add(sz, 1 + index_len(sz - 1))));
  }
  return over;
}

template <class Out>
SMI_HD void put_index(rew::Writer<Out>& out, int Q) {
  if (Q >= 16) out.put(EM_INDEX + ((Q >> 4) & 0xF));
  out.put(EM_INDEX + (Q & 0xF));
}

// The symbols of the row in atom order.  Returns the status; branches / rings: the symbols of either kind.
template <class Words, class Clos, class Bytes, class Out>
SMI_HD int emit_row(Words& W, Clos& C, Bytes& S, Bytes& D, Bytes& P, int n, int nclos, rew::Writer<Out>& out, int* branches, int* rings) {
  *branches = 0; *rings = 0;
  for (int k = 0; k < n && out.status == smg::OK; ++k) {
    const uint32_t w = W.get(k);
    const int p = smg::a_pred(w), beta = p == NONE ? 1 : w_order(w), h = w_stated(w);
    if (beta < 1) return smg::SYNTAX;  // cannot happen: the walk bonds every atom behind the first
    if (p != NONE && D.get(p) != k) {
      const int Q = S.get(k) - 1;
      out.put(EM_BRANCH + (beta - 1) * 3 + index_len(Q) - 1);
      put_index(out, Q);
      ++*branches;
    }
    if (h == 7) out.fail(rew::NO_TOKEN);
    else out.put(em_atom(beta, smg::a_elem(w), smg::a_chg(w), h));
    // the closures whose later end is k, by their earlier end
    int last = -1;
    for (int q = P.get(k); q > 0; --q) {
      int best = NONE, dbl = 0;
      for (int c = 0; c < nclos; ++c) {
        const int v = C.get(c), i = v & 0x7F, j = v >> 8, r = i > j ? i : j, l = i > j ? j : i;
        if (r == k && l != r && l > last && l < best) { best = l; dbl = v & CLOS_DOUBLE ? 1 : 0; }
      }
      if (best == NONE) break;
      last = best;
      const int Q = k - best - 1;
      out.put(EM_RING + dbl * 3 + index_len(Q) - 1);
      put_index(out, Q);
      ++*rings;
    }
  }
  return out.status;
}

}  // namespace sf
