// The writer of SMILES token rows that smiles_rewrite.hip and smiles_canon.hip share: the walk's graph as an adjacency in CSR form
// (rew::graph), and from it the depth-first search and the emission of the search tree in the language the syntax automaton accepts
// (rew::write), templated on the one thing the two consumers differ in -- the order of the atoms.  include/mvae.h ("SMILES rewrite")
// states the definition; "SMILES canon" replaces its (prio, atom number) by a canonical rank and nothing else.  smiles_substruct.hip
// takes the adjacency alone (rew::adjacency, he_order) and searches it instead of writing it.  Below them the writer driver: the arrays
// stated once (rew::Store), and everything around a row that the two families' kernels, launches and host loops have in common.
//
// An order policy `Ord` has one member, bool before(int a, int b): atom a comes before atom b (a strict total order on 0 .. n - 1).
// write() calls it while it picks the root and sorts the half-edges, and never once the emission has begun: a policy may therefore keep
// its state in the storage of the output row O.
//
// One thread per row; everything indexed by a run-time atom number lives in the caller's arrays (LDS, lane-minor, on the device):
//   W  words       128 x 4 B   the walk's atom words; bits 8-15 and 26-31 are rewritten once the graph is read
//   C  closures     64 x 2 B   the walk's list; dead once graph() returns, so O may share its storage
//   O  output      128 x 1 B   the output row
//   A  half-edges  256 x 1 B   neighbour | multiple-bond bit << 7, <= 252 per row
//   S, D, P        128 x 1 B   the CSR index, the search index, the search parent; D and P are free between graph() and write()
// There is no stack and no cursor array: the search returns through the parent array, and the child cursor of an atom (<= 6, the largest
// valence) sits in its word.  The open ring digits are one byte per digit in two registers, as in the walk.  Every loop carries a bound
// that follows from n <= 127 whatever the arrays hold, and every index goes through a slot mask.
#pragma once
#include "common.hpp"
#include "smiles_rounds.hpp"

namespace rew {

enum : int { STEREO = MVAE_SMILES_STEREO, RING_MULTI, RING_DIGITS, DEPTH, LONG, NO_TOKEN };
constexpr int SLOTS = smg::ATOM_SLOTS;
constexpr int HALF = 256;              // slots of the half-edge list
constexpr int NONE = smg::NONE;
constexpr int COPY = 0xFF;             // the length of a row that is copied through
// the emit table (vocab.smiles_emit_table)
constexpr int EM_ALI = 0, EM_ARO = 11, EM_L = 22, EM_R = 23, EM_LBRK = 24, EM_RBRK = 25, EM_H = 26, EM_PLUS = 27, EM_MINUS = 28, EM_DBL = 29,
              EM_TRP = 30, EM_LPAR = 31, EM_RPAR = 32, EM_DIGIT = 33, EM_STEREO = 43;
static_assert(EM_STEREO + 2 <= MVAE_REWRITE_EMIT, "the emit table");
constexpr int E_CL = 8, E_BR = 9;
// atom word once the graph is read: bits 8-11 the hydrogens of a bracket atom, 12-14 the cursor into its half-edges, 26-27 the order of
// the bond to its search parent, 28 "written in parentheses"
constexpr uint32_t W_KEEP = 0x03FF00FFu;

SMI_HD int w_cursor(uint32_t w) { return (int)(w >> 12) & 7; }
SMI_HD uint32_t w_with_cursor(uint32_t w, int c) { return (w & ~(7u << 12)) | (uint32_t)c << 12; }
SMI_HD int w_hyd(uint32_t w) { return (int)(w >> 8) & 0xF; }

// The order of the bond behind half-edge he of atom a (word w): it stands in the word of whichever end the string wrote second, and a
// closure has order 1
template <class Words>
SMI_HD int he_order(Words& W, int a, uint32_t w, int he) {
  if (!(he & 0x80)) return 1;
  const uint32_t wn = W.get(he & 0x7F);
  return smg::a_pred(wn) == a ? (int)(wn >> 24) & 3 : (int)(w >> 24) & 3;
}

// the output row under construction
template <class Bytes>
struct Writer {
  Bytes& O;
  const int32_t* emit;
  int max_content, len = 0, status = smg::OK;
  SMI_HD void fail(int st) {
    if (status == smg::OK) status = st;
  }
  SMI_HD void put(int role) {
    if (status != smg::OK) return;
    const int id = emit[role];
    if (id < 0) { fail(NO_TOKEN); return; }
    if (len >= max_content) { fail(LONG); return; }
    O.set(len++, (uint8_t)id);
  }
};

// The adjacency of the n atoms the walk left in W and the nclos closures in C, half-edges in string order (smiles_substruct.hip calls
// it behind a walk of its own: a row with a stereo token still has a graph to search).
template <class Words, class Clos, class Half, class Bytes>
SMI_HD void adjacency(Words& W, Clos& C, Half& A, Bytes& S, Bytes& D, Bytes& P, int n, int nclos) {
  // degrees into S, bond sums into P, then the exclusive prefix sum, then the half-edges with D as the fill cursor
  for (int k = 0; k <= n; ++k) { S.set(k, 0); P.set(k, 0); }
  for (int k = 1; k < n; ++k) {
    const uint32_t w = W.get(k);
    const int p = smg::a_pred(w), o = (int)(w >> 24) & 3;
    if (p == NONE) continue;
    S.set(k, (uint8_t)(S.get(k) + 1)); S.set(p, (uint8_t)(S.get(p) + 1));
    P.set(k, (uint8_t)(P.get(k) + o)); P.set(p, (uint8_t)(P.get(p) + o));
  }
  for (int c = 0; c < nclos; ++c) {
    const int pr = C.get(c), i = pr & 0xFF, j = pr >> 8;
    S.set(i, (uint8_t)(S.get(i) + 1)); S.set(j, (uint8_t)(S.get(j) + 1));
    P.set(i, (uint8_t)(P.get(i) + 1)); P.set(j, (uint8_t)(P.get(j) + 1));
  }
  int run = 0;
  for (int k = 0; k < n; ++k) {
    const uint32_t w = W.get(k);
    const int deg = S.get(k), h = smg::a_used(w) - (int)P.get(k);
    W.set(k, (w & W_KEEP) | (uint32_t)(h & 0xF) << 8);
    S.set(k, (uint8_t)run);
    D.set(k, (uint8_t)run);
    run += deg;
  }
  S.set(n, (uint8_t)run);              // run = 2 (n - 1 + nclos) <= 252: an atom and a ring digit take a token each
  for (int k = 1; k < n; ++k) {
    const uint32_t w = W.get(k);
    const int p = smg::a_pred(w), m = ((w >> 24) & 3) >= 2 ? 0x80 : 0;
    if (p == NONE) continue;
    const int ik = D.get(k), ip = D.get(p);
    A.set(ik, (uint8_t)(p | m)); D.set(k, (uint8_t)(ik + 1));
    A.set(ip, (uint8_t)(k | m)); D.set(p, (uint8_t)(ip + 1));
  }
  for (int c = 0; c < nclos; ++c) {
    const int pr = C.get(c), i = pr & 0xFF, j = pr >> 8;
    const int ii = D.get(i), ij = D.get(j);
    A.set(ii, (uint8_t)j); D.set(i, (uint8_t)(ii + 1));
    A.set(ij, (uint8_t)i); D.set(j, (uint8_t)(ij + 1));
  }
}

// The walk and the stereo test.  Returns the status; with status 0, rec holds the atoms (>= 1), the closures and the ring members
// (scaffold_smiles.hip cuts the graph down between this and the adjacency).
template <class Words, class Clos, class Src>
SMI_HD int read(Words& W, fpr::Rec<Clos>& rec, const Src& src, int first, int end, bool end_is_eos, int V, const int32_t* tok_info,
                const int32_t* chem_info, const int32_t* emit, int eos_id) {
  smg::Row r;
  smg::walk(W, src, first, end, end_is_eos, V, tok_info, chem_info, eos_id, &r, rec);
  if (r.status != smg::OK) return r.status;
  const smg::u64 stereo = (smg::u64)(uint32_t)emit[EM_STEREO] | (smg::u64)(uint32_t)emit[EM_STEREO + 1] << 32;
  for (int t = first; t < end && t - first <= smg::CONTENT_MAX; ++t) {
    const long tok = src.tok(t);
    if (tok == eos_id) break;
    if ((stereo >> (tok & 63)) & 1ull) return STEREO;
  }
  if (rec.n < 1) return smg::SYNTAX;   // cannot happen: the automaton takes no row without an atom
  return smg::OK;
}

// The walk, the stereo test and the adjacency.  Returns the status; *n_out = the atoms (>= 1 with status 0).
template <class Words, class Clos, class Half, class Bytes, class Src>
SMI_HD int graph(Words& W, Clos& C, Half& A, Bytes& S, Bytes& D, Bytes& P, const Src& src, int first, int end, bool end_is_eos, int V,
                 const int32_t* tok_info, const int32_t* chem_info, const int32_t* emit, int eos_id, int* n_out) {
  *n_out = 0;
  fpr::Rec<Clos> rec(C);
  const int st = read(W, rec, src, first, end, end_is_eos, V, tok_info, chem_info, emit, eos_id);
  if (st != smg::OK) return st;
  adjacency(W, C, A, S, D, P, rec.n, rec.nclos < fpr::CLOSURES ? rec.nclos : fpr::CLOSURES);
  *n_out = rec.n;
  return smg::OK;
}

// The root, the visiting order, the search, the emission.  Returns the status; *len = the content tokens staged in O, COPY for a row
// that is to be copied through.
template <class Ord, class Words, class Out, class Half, class Bytes>
SMI_HD int write(const Ord& ord, Words& W, Out& O, Half& A, Bytes& S, Bytes& D, Bytes& P, int n, const int32_t* emit, int max_content,
                 int* len) {
  *len = COPY;
  int root = 0;
  for (int k = 1; k < n; ++k)
    if (ord.before(k, root)) root = k;
  // every atom's half-edges in visiting order: multiple bonds first, then by the order of the other end; an insertion sort of at most 6
  for (int k = 0; k < n; ++k) {
    const int s = S.get(k), e = S.get(k + 1);
    for (int i = s + 1; i < e && i < HALF; ++i) {
      const int v = A.get(i);
      int j = i;
      for (; j > s; --j) {
        const int u = A.get(j - 1);
        const bool v_first = (v & 0x80) != (u & 0x80) ? (v & 0x80) != 0 : ord.before(v & 0x7F, u & 0x7F);
        if (!v_first) break;
        A.set(j, (uint8_t)u);
      }
      A.set(j, (uint8_t)v);
    }
  }

  // the search.  It returns through P; every step either uses up a half-edge or steps back, so there are at most run + n of them
  for (int k = 0; k < n; ++k) { D.set(k, (uint8_t)NONE); P.set(k, (uint8_t)NONE); }
  D.set(root, 0);
  bool multi = false;
  int cur = root, cnt = 1;
  for (int g = 0; g < HALF + SLOTS; ++g) {
    const uint32_t w = W.get(cur);
    const int c = w_cursor(w), at = S.get(cur) + c;
    if (at >= S.get(cur + 1)) {
      cur = P.get(cur);
      if (cur == NONE) break;
      continue;
    }
    W.set(cur, w_with_cursor(w, c + 1));
    const int he = A.get(at), nb = he & 0x7F;
    if (nb == P.get(cur)) continue;
    const int dn = D.get(nb);
    if (dn == NONE) {
      // the order of this bond stands in the word of whichever end the string wrote second
      const uint32_t wn = W.get(nb);
      const int o = smg::a_pred(wn) == cur ? (int)(wn >> 24) & 3 : (he & 0x80 ? (int)(w >> 24) & 3 : 1);
      D.set(nb, (uint8_t)cnt++);
      P.set(nb, (uint8_t)cur);
      W.set(nb, (wn & ~(3u << 26)) | (uint32_t)o << 26);
      cur = nb;
    } else if (dn < (int)D.get(cur) && (he & 0x80)) {
      multi = true;
    }
  }
  if (multi) return RING_MULTI;

  // the emission, in pre-order along the same half-edge order
  Writer<Out> out{O, emit, max_content};
  smg::u64 open_lo = ~0ull, open_hi = ~0ull;       // the descendant that closes ring digit d, one byte each, NONE = free
  int depth = 0;
  bool enter = true;
  cur = root;
  for (int g = 0; g < 2 * (HALF + SLOTS) && out.status == smg::OK; ++g) {
    uint32_t w = W.get(cur);
    const int s = S.get(cur), e = S.get(cur + 1), dc = D.get(cur);
    if (enter) {
      enter = false;
      const int o = (int)(w >> 26) & 3, elem = smg::a_elem(w);
      if (P.get(cur) != NONE && o >= 2) out.put(o == 2 ? EM_DBL : EM_TRP);
      if (smg::a_brk(w)) {
        const int h = w_hyd(w), chg = smg::a_chg(w);
        out.put(EM_LBRK);
        out.put((smg::a_arom(w) ? EM_ARO : EM_ALI) + elem);
        if (elem == E_CL) out.put(EM_L);
        if (elem == E_BR) out.put(EM_R);
        if (h >= 1) out.put(EM_H);
        if (h >= 2) out.put(EM_DIGIT + (h < 9 ? h : 9));
        if (chg != 0) out.put(chg > 0 ? EM_PLUS : EM_MINUS);
        out.put(EM_RBRK);
      } else {
        out.put((smg::a_arom(w) ? EM_ARO : EM_ALI) + elem);
        if (elem == E_CL) out.put(EM_L);
        if (elem == E_BR) out.put(EM_R);
      }
      int written = 0;
      for (int d = 0; d < 10; ++d) {
        const int sh = 8 * (d & 7);
        if (((int)((d < 8 ? open_lo : open_hi) >> sh) & 0xFF) != cur) continue;
        out.put(EM_DIGIT + d);
        written |= 1 << d;
        if (d < 8) open_lo |= 0xFFull << sh;
        else open_hi |= 0xFFull << sh;
      }
      // the closures this atom starts, by the search index of the other end
      int last = dc;
      for (int q = s; q < e; ++q) {
        int best = NONE, best_d = NONE;
        for (int i = s; i < e; ++i) {
          const int nb = A.get(i) & 0x7F, dn = D.get(nb);
          if (dn > last && dn < best_d && P.get(nb) != cur) { best = nb; best_d = dn; }
        }
        if (best == NONE) break;
        last = best_d;
        int d = -1;
        for (int t = 1; t <= 10 && d < 0; ++t) {
          const int c = t % 10, sh = 8 * (c & 7);
          if (((int)((c < 8 ? open_lo : open_hi) >> sh) & 0xFF) == NONE && !(written >> c & 1)) d = c;
        }
        if (d < 0) { out.fail(RING_DIGITS); break; }
        const int sh = 8 * (d & 7);
        if (d < 8) open_lo = (open_lo & ~(0xFFull << sh)) | (smg::u64)best << sh;
        else open_hi = (open_hi & ~(0xFFull << sh)) | (smg::u64)best << sh;
        written |= 1 << d;
        out.put(EM_DIGIT + d);
      }
      w = w_with_cursor(w, 0);
      W.set(cur, w);
    }
    // the next child, and whether another follows it
    int child = NONE, at = 0;
    bool more = false;
    for (int i = s + w_cursor(w); i < e; ++i) {
      const int nb = A.get(i) & 0x7F;
      if (P.get(nb) != cur) continue;
      if (child == NONE) { child = nb; at = i - s + 1; }
      else { more = true; break; }
    }
    if (child == NONE) {
      if (w >> 28 & 1) { out.put(EM_RPAR); --depth; }
      cur = P.get(cur);
      if (cur == NONE) break;
      continue;
    }
    W.set(cur, w_with_cursor(w, at));
    const uint32_t wc = W.get(child);
    if (more) {
      if (depth >= smi::DMAX) { out.fail(DEPTH); break; }
      ++depth;
      out.put(EM_LPAR);
      W.set(child, wc | 1u << 28);
    } else {
      W.set(child, wc & ~(1u << 28));
    }
    cur = child;
    enter = true;
  }
  if (out.status != smg::OK) return out.status;
  *len = out.len;
  return smg::OK;
}

// the columns of a padded row that a copy keeps: up to and including the first eos_id, all T without one
template <class Src>
SMI_HD int copy_len(const Src& src, int T, int eos_id) {
  for (int t = 0; t < T; ++t)
    if (src.tok(t) == eos_id) return t + 1;
  return T;
}

// The writer's arrays, stated once as the consumers of the row driver state theirs: Lds the storage of one 64-row block, Host the host
// entries' arrays, lane(lds) the calling lane's accessors.  C is dead once graph() returns and nothing writes O before, so in LDS the two
// are one 8 KiB (Front<LdsMem>); as accessors and on the host they stay two things.  W stands in Front with them so that the words keep
// the front of the block: there the compiler reads and writes them in pairs (ds_read2st64_b32), behind the 8 KiB it does not.
template <template <class, int> class Arr>
struct Front {
  Arr<uint32_t, SLOTS> W;
  Arr<uint16_t, fpr::CLOSURES> C;
  Arr<uint8_t, SLOTS> O;
};
template <>
struct Front<fpr::LdsMem> {
  fpr::LdsMem<uint32_t, SLOTS> W;
  union {
    fpr::LdsMem<uint16_t, fpr::CLOSURES> C;
    fpr::LdsMem<uint8_t, SLOTS> O;
  };
};
template <template <class, int> class Arr>
struct Store : Front<Arr> {
  Arr<uint8_t, HALF> A;
  Arr<uint8_t, SLOTS> S, D, P;
};
typedef Store<fpr::LdsMem> Lds;
typedef Store<fpr::HostArr> Host;
__device__ __forceinline__ Store<fpr::LdsArr> lane(Lds& l) {
  return {{l.W.lane(), l.C.lane(), l.O.lane()}, l.A.lane(), l.S.lane(), l.D.lane(), l.P.lane()};
}

inline bool common_ok(int V, const int32_t* tok_info, const int32_t* chem_info, const int32_t* emit, int max_content, const int32_t* status) {
  return fpr::tables_ok(V, tok_info, chem_info) && emit && status && max_content >= 1 && max_content <= smg::CONTENT_MAX;
}

inline bool rows_args_ok(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info,
                         const int32_t* emit, int bos_id, int eos_id, int pad_id, int max_content, int T_out, const int64_t* out,
                         const int32_t* out_len, const int32_t* status) {
  return common_ok(V, tok_info, chem_info, emit, max_content, status) && x && out && out_len && B >= 1 && T >= 1 && x_ld >= T && eos_id >= 0 &&
         eos_id < V && bos_id >= 0 && bos_id <= 65535 && pad_id >= 0 && pad_id <= 65535 && T_out >= 2;
}

// ---------------------------------------------------------------------------------------------------------------- the writer driver
// The row driver of smiles_rounds.hpp for the families that write a string: one thread per row, 64-thread blocks, and behind the rows a
// barrier and the block-wide copy-out.  A family R states what differs:
//   R::Args           its own arguments behind the common ones (seed, draw / info, rank).  Kernels and entries pass them one by one
//                     (F...), each pointer __restrict__ in the kernel's own list, and the driver makes the Args: as members of a
//                     by-value kernel argument they would lose the qualifier
//   R::row(store, src, first, end, end_is_eos, V, tok_info, chem_info, emit, eos_id, max_content, b, args, &len)
//                     row b into store.O; returns the status, *len as write() gives it
//   R::skipped(b, args)   what a corpus row whose id is outside [0, N) leaves in the family's own outputs
// Each family keeps two __global__ kernels of its own name whose bodies are one call of block_rows<R> / block_corpus<R>, and three
// entries that are one call of rows / corpus / host<R>.
// counts, where given, is the histogram of status & 31: int32 [16] serves the families whose statuses end at 14, the fragment family
// (fragment_smiles.hip), whose NO_FRAGMENT is 16, takes int32 [32].
// The rows are staged in LDS and copied out by the whole block behind a barrier, row r by all 64 lanes over consecutive columns (a row
// with len == COPY: the first keep columns of its source).  That read of the staging area has lanes 64 bytes apart (a 16-way bank
// conflict); it is two or three instructions per row against the several thousand of the search.
template <class R, class... F>
__device__ __forceinline__ void block_rows(Lds& lds, int B, int T, int V, const int64_t* __restrict__ x, long x_ld,
                                           const int32_t* __restrict__ tok_info, const int32_t* __restrict__ chem_info,
                                           const int32_t* __restrict__ emit, int bos_id, int eos_id, int pad_id, int max_content, int T_out,
                                           int64_t* __restrict__ out, int32_t* __restrict__ out_len, int32_t* __restrict__ status,
                                           int32_t* __restrict__ counts, F... family) {
  const int lane = threadIdx.x, b0 = blockIdx.x * 64, b = b0 + lane;
  int len = COPY, keep = 0;
  if (b < B) {
    auto store = rew::lane(lds);
    const fpr::PaddedSrc src{x + (long)b * x_ld};
    const int st = R::row(store, src, 1, T, false, V, tok_info, chem_info, emit, eos_id, max_content, (long)b, typename R::Args{family...}, &len);
    if (len == COPY) keep = copy_len(src, T, eos_id);
    status[b] = st;
    out_len[b] = len == COPY ? keep : len + 2;
    if (counts) atomicAdd(counts + (st & 31), 1);
  }
  __syncthreads();
  const int nrows = B - b0 < 64 ? B - b0 : 64;
  for (int r = 0; r < nrows; ++r) {
    const int lr = __shfl(len, r), kr = __shfl(keep, r);
    const int64_t* xr = x + (long)(b0 + r) * x_ld;
    int64_t* dst = out + (long)(b0 + r) * T_out;
    for (int t = lane; t < T_out; t += 64) {
      int64_t v = pad_id;
      if (lr == COPY) {
        if (t < kr) v = xr[t];
      } else if (t == 0) v = bos_id;
      else if (t <= lr) v = lds.O.v[((t - 1) & (SLOTS - 1)) * 64 + r];
      else if (t == lr + 1) v = eos_id;
      dst[t] = v;
    }
  }
}

// Batch member b is corpus row rows[b]; its slice of the gapped CSR, its status and the histogram are written with the row, and the
// rows go into tokens_out [B, stride] as above.
template <class R, class... F>
__device__ __forceinline__ void block_corpus(Lds& lds, const uint8_t* __restrict__ tokens, const int64_t* __restrict__ offsets, long N,
                                             const int64_t* __restrict__ rows, int B, int V, const int32_t* __restrict__ tok_info,
                                             const int32_t* __restrict__ chem_info, const int32_t* __restrict__ emit, int max_content, int stride,
                                             uint8_t* __restrict__ tokens_out, int64_t* __restrict__ offsets_out, int32_t* __restrict__ status,
                                             int32_t* __restrict__ counts, int32_t* __restrict__ err, F... family) {
  const int lane = threadIdx.x, b0 = blockIdx.x * 64, b = b0 + lane;
  int len = COPY, keep = 0;
  long lo = 0;                         // where the lane's corpus row starts in tokens
  if (b < B) {
    const long id = rows[b];
    const typename R::Args args{family...};
    int st = smg::SYNTAX;
    if (id >= 0 && id < N) {
      const long have = fpr::csr_len(offsets, id, &lo);
      auto store = rew::lane(lds);
      st = R::row(store, fpr::CsrSrc{tokens + lo}, 0, fpr::csr_end(have), true, V, tok_info, chem_info, emit, -1, max_content, (long)b, args, &len);
      if (len == COPY) {
        keep = (int)(have < stride ? have : stride);
        if (have > stride && err) atomicMax(err, 1);
      }
    } else {
      R::skipped((long)b, args);
      if (err) atomicMax(err, 2);
    }
    status[b] = st;
    offsets_out[2 * (long)b] = (long)b * stride;
    offsets_out[2 * (long)b + 1] = (long)b * stride + (len == COPY ? keep : len);
    if (b == B - 1) offsets_out[2 * (long)B] = (long)B * stride;
    if (counts) atomicAdd(counts + (st & 31), 1);
  }
  __syncthreads();
  const int nrows = B - b0 < 64 ? B - b0 : 64;
  for (int r = 0; r < nrows; ++r) {
    const int lr = __shfl(len, r), kr = __shfl(keep, r);
    const long lor = __shfl(lo, r);
    uint8_t* dst = tokens_out + (long)(b0 + r) * stride;
    for (int t = lane; t < stride; t += 64) {
      uint8_t v = 0;
      if (lr == COPY) {
        if (t < kr) v = tokens[lor + t];
      } else if (t < lr) v = lds.O.v[(t & (SLOTS - 1)) * 64 + r];
      dst[t] = v;
    }
  }
}

// The entries.  kernel: the family's __global__ function, whose parameters are those of block_rows / block_corpus behind the Lds.
// V > 64 is refused as unsupported before anything is called invalid.
template <class K, class... F>
int rows(K kernel, int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, const int32_t* emit,
         int bos_id, int eos_id, int pad_id, int max_content, int T_out, int64_t* out, int32_t* out_len, int32_t* status, int32_t* counts,
         void* stream, F... family) {
  if (V > 64) return MVAE_ERR_UNSUPPORTED;
  if (!rows_args_ok(B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len, status))
    return MVAE_ERR_INVALID;
  hipLaunchKernelGGL(kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, B, T, V, x, (long)x_ld, tok_info, chem_info, emit, bos_id,
                     eos_id, pad_id, max_content, T_out, out, out_len, status, counts, family...);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

template <class K, class... F>
int corpus(K kernel, const uint8_t* tokens, const int64_t* offsets, int64_t N, const int64_t* rows, int B, int V, const int32_t* tok_info,
           const int32_t* chem_info, const int32_t* emit, int max_content, int stride, uint8_t* tokens_out, int64_t* offsets_out, int32_t* status,
           int32_t* counts, int32_t* err, void* stream, F... family) {
  if (V > 64) return MVAE_ERR_UNSUPPORTED;
  if (!common_ok(V, tok_info, chem_info, emit, max_content, status) || !tokens || !offsets || !rows || !tokens_out || !offsets_out || N < 1 ||
      B < 1 || stride < max_content)
    return MVAE_ERR_INVALID;
  hipLaunchKernelGGL(kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, tokens, offsets, (long)N, rows, B, V, tok_info, chem_info,
                     emit, max_content, stride, tokens_out, offsets_out, status, counts, err, family...);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

// The host loop behind the checks.  selfies.hip, whose input and output vocabularies differ, states its own checks and calls this and the
// two block bodies above: to them V, the tables and emit are whatever R::row reads, and bos_id, eos_id, pad_id are the output's.
template <class R, class... F>
int host_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, const int32_t* emit,
              int bos_id, int eos_id, int pad_id, int max_content, int T_out, int64_t* out, int32_t* out_len, int32_t* status, F... family) {
  const typename R::Args args{family...};
  Host store;
  for (long b = 0; b < B; ++b) {
    const fpr::PaddedSrc src{x + b * x_ld};
    int len = COPY;
    status[b] = R::row(store, src, 1, T, false, V, tok_info, chem_info, emit, eos_id, max_content, b, args, &len);
    const int keep = len == COPY ? copy_len(src, T, eos_id) : 0;
    out_len[b] = len == COPY ? keep : len + 2;
    for (int t = 0; t < T_out; ++t) {
      int64_t v = pad_id;
      if (len == COPY) {
        if (t < keep) v = src.row[t];
      } else if (t == 0) v = bos_id;
      else if (t <= len) v = store.O.get(t - 1);
      else if (t == len + 1) v = eos_id;
      out[b * T_out + t] = v;
    }
  }
  return MVAE_OK;
}

template <class R, class... F>
int host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, const int32_t* emit, int bos_id,
         int eos_id, int pad_id, int max_content, int T_out, int64_t* out, int32_t* out_len, int32_t* status, F... family) {
  if (V > 64) return MVAE_ERR_UNSUPPORTED;
  if (!rows_args_ok(B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len, status))
    return MVAE_ERR_INVALID;
  return host_rows<R>(B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len, status, family...);
}

}  // namespace rew
