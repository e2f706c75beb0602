// Aromatic normal form of SMILES token rows (gfx950): mvae_smiles_aromatize_rows / _corpus / _host.  include/mvae.h ("Aromatic normal
// form") states the definition: the Kekule graph of the row (the set N of "Kekulisation" and its matching), the electrons e(a) of the
// candidate atoms, the simple cycles of 5 - 7 candidates with sum e = 2 (mod 4), the output graph with the aromatic flags and the
// lowered bonds, spelled by "SMILES canon".
//
// A tenth consumer of the walk of smiles_graph.hpp and the fifth family of the writer driver (smiles_writer.hpp), which owns the
// kernels' bodies, the launches and the host loop.  This file is the graph producer between the walk and the writer, and nothing else:
//   rew::read            the walk and the stereo test (smiles_writer.hpp)
//   kek::set_n, match    N and the exact matching (kekule.hpp, shared with kekule.hip).  Its four byte arrays are lent: mate and parent
//                        are the two halves of the half-edge list A, base is S, queue is D; the closure list C stays alive beside them.
//                        Only |matching| is used: which bond an atom of N doubles is never read
//   aro::electrons       the double-bond census (five masks in registers) and from it the candidates and their e(a) as three masks
//   aro::neighbours      the <= 3 candidate ring neighbours of every candidate, one each in S, D, P (the matching is dead by then)
//   aro::cycles          the path search from every start atom over neighbours numbered above it: the path (<= 7 atom numbers) in one
//                        64-bit register, the seven 2-bit cursors in a 32-bit one, no stack
//   aro::relabel         the aromatic flags, the lowered bond orders, and the true hydrogen count folded into the used valence, so that
//                        rew::adjacency leaves it in the hydrogen field as it leaves lost(a) for the scaffold
//   aro::hydrogens       an unbracketed atom stays one iff the implicit rule on its new flag and bond sum (the adjacency's P) gives it
//   can::ranks, rew::write   unchanged (smiles_canon.hpp); O shares C's storage and is first written by the ranks, behind the adjacency
// One thread per row, 64-thread blocks, the rewrite's 80 KiB of LDS per block (rew::Lds) with nothing added.  No runtime-indexed private
// array, no recursion; every loop is bounded by n <= 127 (the path search by STEPS) and every index goes through a slot mask.
#include "common.hpp"
#include "kekule.hpp"
#include "smiles_canon.hpp"
#include "smiles_writer.hpp"

namespace aro {

enum : int { NOT_AROMATIC = MVAE_SMILES_NOT_AROMATIC };
constexpr int E_C = smg::E_C, E_N = 3, E_O = 4, E_S = 7;
constexpr int NONE = smg::NONE;
// One start atom's search: a path has <= 7 atoms and an atom <= 3 neighbours, one of them where the path came from, so there are at
// most 1 + 3 + 6 + ... + 96 = 190 paths, and a path costs three cursor steps and one step back.
constexpr int STEPS = 1024;

// one 128-slot half of the half-edge list as a byte array of its own
template <class Half, int OFF>
struct HalfView {
  Half& a;
  SMI_HD int get(int i) const { return a.get(OFF + (i & (rew::SLOTS - 1))); }
  SMI_HD void set(int i, uint8_t v) { a.set(OFF + (i & (rew::SLOTS - 1)), v); }
};

SMI_HD void m_clear(smg::Mask& m, int i) {
  if (i < 64) m.lo &= ~(1ull << (i & 63));
  else m.hi &= ~(1ull << (i & 63));
}
SMI_HD bool m_any_outside(const smg::Mask& a, const smg::Mask& b) { return ((a.lo & ~b.lo) | (a.hi & ~b.hi)) != 0; }

struct Sets { smg::Mask cand, e1, e2; };           // the candidates; those with e = 1; those with e = 2 (the others have e = 0)

// K(a), dbl(a) and the three cases.  ring: the ring members; rb: fpr::ring_bonds; N: kek::set_n.
template <class Words>
SMI_HD Sets electrons(Words& W, int n, const smg::Mask& ring, const smg::Mask& rb, const smg::Mask& N) {
  // an atom of N has one double bond already, and it is a ring bond; a closure has order 1
  smg::Mask d1 = N, d2{0, 0}, rd = N, xd{0, 0}, tr{0, 0};      // >= 1 double, >= 2, a ring double, a non-ring double to N O S, a triple
  for (int k = 1; k < n; ++k) {
    const uint32_t w = W.get(k);
    const int p = smg::a_pred(w), o = (int)(w >> 24) & 3;
    if (p == NONE || o < 2) continue;
    if (o == 3) { smg::m_set(tr, k); smg::m_set(tr, p); continue; }
    const int ek = smg::a_elem(w), ep = smg::a_elem(W.get(p));
    if (smg::m_get(d1, k)) smg::m_set(d2, k);
    else smg::m_set(d1, k);
    if (smg::m_get(d1, p)) smg::m_set(d2, p);
    else smg::m_set(d1, p);
    if (smg::m_get(rb, k)) { smg::m_set(rd, k); smg::m_set(rd, p); }
    else {
      if (ep == E_N || ep == E_O || ep == E_S) smg::m_set(xd, k);
      if (ek == E_N || ek == E_O || ek == E_S) smg::m_set(xd, p);
    }
  }
  Sets q{{0, 0}, {0, 0}, {0, 0}};
  for (int k = 0; k < n; ++k) {
    if (!smg::m_get(ring, k)) continue;
    const uint32_t w = W.get(k);
    const int e = smg::a_elem(w), c = smg::a_chg(w), u = smg::a_used(w);
    const int K = u + (smg::m_get(N, k) ? 1 : 0) + (smg::a_brk(w) ? 0 : smg::implicit_h(e, smg::a_arom(w), u));
    const bool one = smg::m_get(d1, k) && !smg::m_get(d2, k), none = !smg::m_get(d1, k);
    if (one && !smg::m_get(tr, k) && smg::m_get(rd, k) && K <= 4 &&
        ((c == 0 && (e == E_C || e == E_N)) || (c == 1 && (e == E_N || e == E_O || e == E_S)))) {
      smg::m_set(q.cand, k);
      smg::m_set(q.e1, k);
    } else if (one && e == E_C && c == 0 && smg::m_get(xd, k)) {
      smg::m_set(q.cand, k);
    } else if (none && ((c == 0 && ((e == E_N && K == 3) || ((e == E_O || e == E_S) && K == 2))) ||
                        (c == -1 && ((e == E_N && K == 2) || (e == E_C && K == 3))))) {
      smg::m_set(q.cand, k);
      smg::m_set(q.e2, k);
    }
  }
  return q;
}

template <class Bytes>
SMI_HD void link(Bytes& S, Bytes& D, Bytes& P, int a, int b) {
  if (S.get(a) == NONE) S.set(a, (uint8_t)b);
  else if (D.get(a) == NONE) D.set(a, (uint8_t)b);
  else if (P.get(a) == NONE) P.set(a, (uint8_t)b);     // a fourth cannot happen: a candidate has at most three bonds
}

// The candidate neighbours of every atom over ring bonds, filled from S to P.  A bond of a cycle is a ring bond, so leaving the others
// out loses no cycle.
template <class Words, class Clos, class Bytes>
SMI_HD void neighbours(Words& W, Clos& C, Bytes& S, Bytes& D, Bytes& P, int n, int nclos, const smg::Mask& rb, const smg::Mask& cand) {
  for (int k = 0; k < n; ++k) { S.set(k, (uint8_t)NONE); D.set(k, (uint8_t)NONE); P.set(k, (uint8_t)NONE); }
  for (int k = 1; k < n; ++k) {
    const int p = smg::a_pred(W.get(k));
    if (p == NONE || !smg::m_get(rb, k) || !smg::m_get(cand, k) || !smg::m_get(cand, p)) continue;
    link(S, D, P, k, p);
    link(S, D, P, p, k);
  }
  for (int c = 0; c < nclos; ++c) {
    const int pr = C.get(c), i = pr & 0xFF, j = pr >> 8;
    if (!smg::m_get(cand, i) || !smg::m_get(cand, j)) continue;
    link(S, D, P, i, j);
    link(S, D, P, j, i);
  }
}

// The atoms on a simple cycle of 5, 6 or 7 candidates whose electrons sum to 2 (mod 4).  Every cycle is found from its lowest atom,
// once in each direction.
template <class Bytes>
SMI_HD smg::Mask cycles(Bytes& S, Bytes& D, Bytes& P, int n, const Sets& q) {
  smg::Mask ar{0, 0};
  for (int s = 0; s < n; ++s) {
    if (!smg::m_get(q.cand, s) || D.get(s) == NONE) continue;  // fewer than two neighbours: on no cycle
    smg::u64 path = (smg::u64)s;       // byte d: the atom at depth d
    uint32_t cursor = 0;               // bits 2 d, 2 d + 1: the next neighbour slot of the atom at depth d
    int depth = 0;
    smg::Mask on{0, 0};
    smg::m_set(on, s);
    for (int g = 0; g < STEPS; ++g) {
      const int top = (int)(path >> 8 * depth) & 0xFF, c = (int)(cursor >> 2 * depth) & 3;
      if (c == 3) {
        if (depth == 0) break;
        m_clear(on, top);
        --depth;
        continue;
      }
      cursor += 1u << 2 * depth;
      const int nb = c == 0 ? S.get(top) : (c == 1 ? D.get(top) : P.get(top));
      if (nb == NONE) continue;
      if (nb == s) {
        if (depth < 4) continue;       // fewer than 5 atoms (at depth 1 this is the bond the path came over)
        int sum = 0;
        for (int d = 0; d <= depth; ++d) {
          const int a = (int)(path >> 8 * d) & 0xFF;
          sum += smg::m_get(q.e1, a) ? 1 : (smg::m_get(q.e2, a) ? 2 : 0);
        }
        if ((sum & 3) != 2) continue;
        for (int d = 0; d <= depth; ++d) smg::m_set(ar, (int)(path >> 8 * d) & 0xFF);
        continue;
      }
      if (nb < s || nb >= n || smg::m_get(on, nb) || depth == 6) continue;
      ++depth;
      path = (path & ~(0xFFull << 8 * depth)) | (smg::u64)nb << 8 * depth;
      cursor &= ~(3u << 2 * depth);
      smg::m_set(on, nb);
    }
  }
  return ar;
}

// The output graph in the words: the flags of ar, order 1 on every bond between two atoms of ar (only an order of 2 can stand there: an
// atom with a triple bond is on no aromatic cycle), bit 31 cleared, and in the used-valence field the new bond sum plus the TRUE
// hydrogens -- bracket hydrogens, or the implicit ones by the old flag and the old bond sum.  Returns the bonds lowered.
template <class Words>
SMI_HD int relabel(Words& W, int n, const smg::Mask& ar) {
  smg::Mask low{0, 0};
  int lowered = 0;
  for (int k = 1; k < n; ++k) {
    const uint32_t w = W.get(k);
    const int p = smg::a_pred(w);
    if (p == NONE || ((w >> 24) & 3) != 2 || !smg::m_get(ar, k) || !smg::m_get(ar, p)) continue;
    smg::m_set(low, k);
    smg::m_set(low, p);
    W.set(k, (w & ~(3u << 24)) | 1u << 24);
    ++lowered;
  }
  for (int k = 0; k < n; ++k) {
    const uint32_t w = W.get(k);
    const int u = smg::a_used(w);
    const int h = smg::a_brk(w) ? 0 : smg::implicit_h(smg::a_elem(w), smg::a_arom(w), u);
    const int used = u - (smg::m_get(low, k) ? 1 : 0) + h;
    W.set(k, (w & ~(kek::IN_E | 0xFFu << 8 | 1u << 20)) | (uint32_t)(used & 0xFF) << 8 | (smg::m_get(ar, k) ? 1u << 20 : 0u));
  }
  return lowered;
}

// Behind the adjacency, which left the true hydrogens in the hydrogen field and the bond sums in P
template <class Words, class Bytes>
SMI_HD void hydrogens(Words& W, Bytes& P, int n) {
  for (int k = 0; k < n; ++k) {
    const uint32_t w = W.get(k);
    if (smg::a_brk(w)) continue;
    const int h = rew::w_hyd(w);
    if (smg::implicit_h(smg::a_elem(w), smg::a_arom(w), P.get(k)) == h) W.set(k, w & ~(0xFu << 8));
    else W.set(k, w | 1u << 21);
  }
}

// The family the writer driver runs.  info [B, 4] and arom [B, 128] may be NULL; each is written in full.
struct Aromatize {
  struct Args {
    int32_t* info;
    uint8_t* arom;
    SMI_HD int32_t* info_of(long b) const { return info ? info + 4 * b : nullptr; }
    SMI_HD uint8_t* arom_of(long b) const { return arom ? arom + rew::SLOTS * b : nullptr; }
  };

  // One row: the walk, the matching, the perception, the output graph, the ranks, the search, the emission.  Returns the status; *len
  // as rew::write gives it.  info and arom of a row whose output graph is not made (status 1 - 8 and 17) are zeros / 0xFF.
  template <class S, class Src>
  static SMI_HD int row(S& s, const Src& src, int first, int end, bool end_is_eos, int V, const int32_t* tok_info, const int32_t* chem_info,
                        const int32_t* emit, int eos_id, int max_content, long b, const Args& a, int* len) {
    *len = rew::COPY;
    int32_t* info = a.info_of(b);
    uint8_t* arom = a.arom_of(b);
    fpr::Rec<decltype(s.C)> rec(s.C);
    int st = rew::read(s.W, rec, src, first, end, end_is_eos, V, tok_info, chem_info, emit, eos_id);
    int n = 0, raised = 0, lowered = 0;
    smg::Mask ar{0, 0};
    if (st == smg::OK) {
      n = rec.n;
      const int nclos = rec.nclos < fpr::CLOSURES ? rec.nclos : fpr::CLOSURES;
      const smg::Mask rb = fpr::ring_bonds(s.W, s.C, nclos);
      const smg::Mask N = kek::set_n(s.W, n);
      HalfView<decltype(s.A), 0> mate{s.A};
      HalfView<decltype(s.A), rew::SLOTS> parent{s.A};
      int edges;
      if (2 * kek::match(s.W, s.C, mate, parent, s.S, s.D, n, nclos, rb, N, &edges) != smg::m_count(N)) st = kek::KEKULE;
      if (st == smg::OK) {
        const Sets q = electrons(s.W, n, rec.ring, rb, N);
        neighbours(s.W, s.C, s.S, s.D, s.P, n, nclos, rb, q.cand);
        ar = cycles(s.S, s.D, s.P, n, q);
        smg::Mask lower{0, 0};
        for (int k = 0; k < n; ++k)
          if (smg::a_arom(s.W.get(k))) smg::m_set(lower, k);
        if (m_any_outside(lower, ar)) st = NOT_AROMATIC;
        else {
          raised = smg::m_count(ar) - smg::m_count(lower);
          lowered = relabel(s.W, n, ar);
          rew::adjacency(s.W, s.C, s.A, s.S, s.D, s.P, n, nclos);
          hydrogens(s.W, s.P, n);
          int unused[4];
          can::ranks(s.W, s.A, s.S, s.O, s.D, s.P, n, unused);
        }
      }
    }
    const bool made = st == smg::OK;
    if (info) { info[0] = made ? n : 0; info[1] = made ? smg::m_count(ar) : 0; info[2] = raised; info[3] = lowered; }
    if (arom)
      for (int k = 0; k < rew::SLOTS; ++k) arom[k] = made && k < n ? (uint8_t)smg::m_get(ar, k) : (uint8_t)0xFF;
    if (!made) return st;
    return rew::write(can::RankOrder<decltype(s.O)>{s.O}, s.W, s.O, s.A, s.S, s.D, s.P, n, emit, max_content, len);
  }

  // info and arom of a row that is not read at all
  static SMI_HD void skipped(long b, const Args& a) {
    int32_t* info = a.info_of(b);
    uint8_t* arom = a.arom_of(b);
    if (info) { info[0] = 0; info[1] = 0; info[2] = 0; info[3] = 0; }
    if (arom)
      for (int k = 0; k < rew::SLOTS; ++k) arom[k] = (uint8_t)0xFF;
  }
};

}  // namespace aro

namespace {

static_assert(sizeof(rew::Lds) == MVAE_AROMATIZE_LDS_BYTES, "include/mvae.h states the LDS per block");
static_assert(MVAE_AROMATIZE_LDS_BYTES <= 80 * 1024, "two blocks per CU");

__global__ __launch_bounds__(64) void smiles_aromatize_rows_kernel(int B, int T, int V, const int64_t* __restrict__ x, long x_ld,
                                                                   const int32_t* __restrict__ tok_info, const int32_t* __restrict__ chem_info,
                                                                   const int32_t* __restrict__ emit, int bos_id, int eos_id, int pad_id,
                                                                   int max_content, int T_out, int64_t* __restrict__ out,
                                                                   int32_t* __restrict__ out_len, int32_t* __restrict__ status,
                                                                   int32_t* __restrict__ counts, int32_t* __restrict__ info,
                                                                   uint8_t* __restrict__ arom) {
  __shared__ rew::Lds lds;
  rew::block_rows<aro::Aromatize>(lds, B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len,
                                  status, counts, info, arom);
}

__global__ __launch_bounds__(64) void smiles_aromatize_corpus_kernel(const uint8_t* __restrict__ tokens, const int64_t* __restrict__ offsets,
                                                                     long N, const int64_t* __restrict__ rows, int B, int V,
                                                                     const int32_t* __restrict__ tok_info, const int32_t* __restrict__ chem_info,
                                                                     const int32_t* __restrict__ emit, int max_content, int stride,
                                                                     uint8_t* __restrict__ tokens_out, int64_t* __restrict__ offsets_out,
                                                                     int32_t* __restrict__ status, int32_t* __restrict__ counts,
                                                                     int32_t* __restrict__ err, int32_t* __restrict__ info,
                                                                     uint8_t* __restrict__ arom) {
  __shared__ rew::Lds lds;
  rew::block_corpus<aro::Aromatize>(lds, tokens, offsets, N, rows, B, V, tok_info, chem_info, emit, max_content, stride, tokens_out, offsets_out,
                                    status, counts, err, info, arom);
}

}  // namespace

extern "C" {

int mvae_smiles_aromatize_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info,
                               const int32_t* emit, int bos_id, int eos_id, int pad_id, int max_content, int T_out, int64_t* out,
                               int32_t* out_len, int32_t* status, int32_t* counts, int32_t* info, uint8_t* arom, void* stream) {
  return rew::rows(smiles_aromatize_rows_kernel, B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out,
                   out_len, status, counts, stream, info, arom);
}

int mvae_smiles_aromatize_corpus(const uint8_t* tokens, const int64_t* offsets, int64_t N, const int64_t* rows, int B, int V,
                                 const int32_t* tok_info, const int32_t* chem_info, const int32_t* emit, int max_content, int stride,
                                 uint8_t* tokens_out, int64_t* offsets_out, int32_t* status, int32_t* counts, int32_t* err, int32_t* info,
                                 uint8_t* arom, void* stream) {
  return rew::corpus(smiles_aromatize_corpus_kernel, tokens, offsets, N, rows, B, V, tok_info, chem_info, emit, max_content, stride, tokens_out,
                     offsets_out, status, counts, err, stream, info, arom);
}

int mvae_smiles_aromatize_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info,
                               const int32_t* emit, int bos_id, int eos_id, int pad_id, int max_content, int T_out, int64_t* out,
                               int32_t* out_len, int32_t* status, int32_t* info, uint8_t* arom) {
  return rew::host<aro::Aromatize>(B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len, status,
                                   info, arom);
}

}  // extern "C"
