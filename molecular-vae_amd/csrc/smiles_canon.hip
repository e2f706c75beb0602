// Canonical spelling of SMILES token rows (gfx950): mvae_smiles_canon_rows / _corpus / _host.  include/mvae.h ("SMILES canon") states
// the definition: the rewrite's graph, traversal and emission (smiles_writer.hpp, shared with smiles_rewrite.hip) with the atoms compared
// by a canonical rank -- a first invariant per atom, refined by the sorted (bond order, rank) of the neighbours until the number of
// classes stops growing, ties broken one at a time by string order with a refinement after each.
//
// A sixth consumer of the walk of smiles_graph.hpp.  One thread per row, 64-thread blocks, and the rewrite's 80 KiB of LDS per block
// (rew::Lds) with nothing added: between the adjacency and the search three of its byte arrays are idle, and the ranks live there --
//   R  rank of atom a            the output row's storage (the closure list's before it; both are dead in between)
//   Q  atom at position p        the search index's storage: the atoms sorted by rank, so that a class is a run of Q
//   N  new rank of atom a        the search parent's storage
// Ranks are kept SPARSE -- rank(a) = the atoms that come before a's class, so a class of m atoms at rank r is Q[r .. r + m) -- which
// orders atoms and keys exactly as the header's dense ranks do: a round never moves an atom out of its run, it only sorts the run by key
// and cuts it where the key changes.  A key is never stored: within a class the rank is equal, so what is compared is the <= 6 neighbour
// codes (order << 7 | rank, 9 bits) sorted ascending from bit 53 of one 64-bit word, recomputed from R and the half-edges whenever it is
// needed.  No runtime-indexed private array, no recursion.  Every loop is bounded by n <= 127, the rounds by 2 n.
#include "common.hpp"
#include "smiles_writer.hpp"

namespace can {

typedef smg::u64 u64;

// atoms by canonical rank
template <class Bytes>
struct RankOrder {
  const Bytes& R;
  SMI_HD bool before(int a, int b) const { return R.get(a) < R.get(b); }
};

// The first invariant (element, aromatic, charge, bracket flag, bracket hydrogens, degree, sum of bond orders) as one number below
// 2^16, in mixed radix: a row the walk gives 0 has used valence <= 6 on every atom, so the last three are 0 .. 6.
template <class Words, class Half, class Bytes>
SMI_HD int invariant(Words& W, Half& A, Bytes& S, int a) {
  const uint32_t w = W.get(a);
  const int s = S.get(a), e = S.get(a + 1);
  int sum = 0;
  for (int i = s; i < e && i < s + 6; ++i) sum += rew::he_order(W, a, w, A.get(i));
  const int deg = e - s, h = smg::a_brk(w) ? rew::w_hyd(w) : 0;
  const int head = ((smg::a_elem(w) * 2 + smg::a_arom(w)) * 3 + smg::a_chg(w) + 1) * 2 + smg::a_brk(w);
  return ((head * 7 + (h < 6 ? h : 6)) * 7 + (deg < 6 ? (deg > 0 ? deg : 0) : 6)) * 7 + (sum < 6 ? sum : 6);
}

// The neighbour codes of atom a under the ranks R, ascending from field 5 (bits 45-53) downwards: between atoms of equal degree, integer
// order of this word is the order of the sorted tuples.
template <class Words, class Half, class Bytes, class Ranks>
SMI_HD u64 key(Words& W, Half& A, Bytes& S, Ranks& R, int a) {
  const uint32_t w = W.get(a);
  const int s = S.get(a), e = S.get(a + 1);
  u64 k = 0;
  int m = 0;
  for (int i = s; i < e && m < 6; ++i, ++m) {
    const int he = A.get(i);
    const u64 c = (u64)(rew::he_order(W, a, w, he) << 7 | (R.get(he & 0x7F) & 0x7F));
    int j = 0;                         // the codes of fields 5 .. 6 - j stay, the others move one field down
    for (; j < m; ++j)
      if (((k >> 9 * (5 - j)) & 511ull) > c) break;
    const u64 top = ~0ull << 9 * (6 - j);
    k = (k & top) | c << 9 * (5 - j) | (k & ~top) >> 9;
  }
  return k;
}

// the end of the run of Q that starts at p (the class of rank p)
template <class Bytes, class Ranks>
SMI_HD int run_end(Bytes& Q, Ranks& R, int p, int n) {
  int q = p + 1;
  while (q < n && R.get(Q.get(q)) == p) ++q;
  return q;
}

// One round: every run of Q sorted by key and cut where the key changes.  Returns the number of classes.
template <class Words, class Half, class Bytes, class Ranks>
SMI_HD int round(Words& W, Half& A, Bytes& S, Ranks& R, Bytes& Q, Bytes& N, int n) {
  int classes = 0;
  for (int p = 0; p < n;) {
    const int q = run_end(Q, R, p, n);
    if (q - p == 1) {
      N.set(Q.get(p), (uint8_t)p);
      ++classes;
      p = q;
      continue;
    }
    for (int i = p + 1; i < q; ++i) {
      const int a = Q.get(i);
      const u64 ka = key(W, A, S, R, a);
      int j = i;
      for (; j > p; --j) {
        const int u = Q.get(j - 1);
        if (!(ka < key(W, A, S, R, u))) break;
        Q.set(j, (uint8_t)u);
      }
      Q.set(j, (uint8_t)a);
    }
    u64 prev = 0;
    int first = p;
    for (int i = p; i < q; ++i) {
      const int a = Q.get(i);
      const u64 k = key(W, A, S, R, a);
      if (i == p || k != prev) { first = i; ++classes; }
      N.set(a, (uint8_t)first);
      prev = k;
    }
    p = q;
  }
  for (int a = 0; a < n; ++a) R.set(a, N.get(a));
  return classes;
}

// The canonical ranks of the n atoms into R (a permutation of 0 .. n - 1).  info = atoms, classes after the first refinement, rounds, ties.
template <class Words, class Half, class Bytes, class Ranks>
SMI_HD void ranks(Words& W, Half& A, Bytes& S, Ranks& R, Bytes& Q, Bytes& N, int n, int* info) {
  // the first invariant: its two bytes into N and R, Q sorted by it (insertion, stable), then R := where a's run starts
  for (int a = 0; a < n; ++a) {
    const int v = invariant(W, A, S, a);
    N.set(a, (uint8_t)(v >> 8));
    R.set(a, (uint8_t)v);
  }
  for (int i = 0; i < n; ++i) {
    const int v = N.get(i) << 8 | R.get(i);
    int j = i;
    for (; j > 0; --j) {
      const int u = Q.get(j - 1);
      if (!(v < (N.get(u) << 8 | R.get(u)))) break;
      Q.set(j, (uint8_t)u);
    }
    Q.set(j, (uint8_t)i);
  }
  int classes = 0, prev = -1, first = 0;
  for (int i = 0; i < n; ++i) {
    const int a = Q.get(i), v = N.get(a) << 8 | R.get(a);
    if (v != prev) { first = i; ++classes; }
    R.set(a, (uint8_t)first);
    prev = v;
  }
  // Every round but the last of a call adds a class and every tie adds one: at most n - 1 of both together, and at most n calls
  int rounds = 0, ties = 0, after_first = 0;
  for (int g = 0; g < 2 * n; ++g) {
    const int c = round(W, A, S, R, Q, N, n);
    ++rounds;
    if (c > classes) { classes = c; continue; }
    if (after_first == 0) after_first = classes;
    if (classes >= n) break;
    // the class of lowest rank with more than one member: its member of lowest atom number stays, the others come just above it
    int p = 0, q = 1;
    for (int t = 0; t < n; ++t) {
      q = run_end(Q, R, p, n);
      if (q - p > 1 || q >= n) break;
      p = q;
    }
    if (q - p < 2) break;              // cannot happen while classes < n
    int at = p;
    for (int i = p + 1; i < q; ++i)
      if (Q.get(i) < Q.get(at)) at = i;
    const int low = Q.get(at);
    Q.set(at, Q.get(p));
    Q.set(p, (uint8_t)low);
    for (int i = p + 1; i < q; ++i) R.set(Q.get(i), (uint8_t)(p + 1));
    ++ties;
    ++classes;
  }
  info[0] = n; info[1] = after_first; info[2] = rounds; info[3] = ties;
}

// One row: the graph, the ranks, the search, the emission.  Returns the status; *len as rew::write gives it.  info (4 ints) and rank (128
// bytes) may be NULL; each is written in full: zeros / 0xFF for a row that is refused before its ranks are computed.
template <class Words, class Clos, class Out, class Half, class Bytes, class Src>
SMI_HD int row(Words& W, Clos& C, Out& O, Half& A, Bytes& S, Bytes& D, Bytes& P, const Src& src, int first, int end, bool end_is_eos, int V,
               const int32_t* tok_info, const int32_t* chem_info, const int32_t* emit, int eos_id, int max_content, int* len, int32_t* info,
               uint8_t* rank) {
  *len = rew::COPY;
  int n, got[4] = {0, 0, 0, 0};
  const int st = rew::graph(W, C, A, S, D, P, src, first, end, end_is_eos, V, tok_info, chem_info, emit, eos_id, &n);
  if (st == smg::OK) ranks(W, A, S, O, D, P, n, got);
  else n = 0;
  if (info) { info[0] = got[0]; info[1] = got[1]; info[2] = got[2]; info[3] = got[3]; }
  if (rank)
    for (int k = 0; k < rew::SLOTS; ++k) rank[k] = k < n ? O.get(k) : (uint8_t)0xFF;
  if (st != smg::OK) return st;
  return rew::write(RankOrder<Out>{O}, W, O, A, S, D, P, n, emit, max_content, len);
}

// info and rank of a row that is not read at all
SMI_HD void blank(int32_t* info, uint8_t* rank) {
  if (info) { info[0] = 0; info[1] = 0; info[2] = 0; info[3] = 0; }
  if (rank)
    for (int k = 0; k < rew::SLOTS; ++k) rank[k] = (uint8_t)0xFF;
}

}  // namespace can

namespace {

static_assert(sizeof(rew::Lds) == MVAE_CANON_LDS_BYTES, "include/mvae.h states the LDS per block");
static_assert(MVAE_CANON_LDS_BYTES <= 80 * 1024, "two blocks per CU");

__global__ __launch_bounds__(64) void smiles_canon_rows_kernel(int B, int T, int V, const int64_t* __restrict__ x, long x_ld,
                                                               const int32_t* __restrict__ tok_info, const int32_t* __restrict__ chem_info,
                                                               const int32_t* __restrict__ emit, int bos_id, int eos_id, int pad_id,
                                                               int max_content, int T_out, int64_t* __restrict__ out,
                                                               int32_t* __restrict__ out_len, int32_t* __restrict__ status,
                                                               int32_t* __restrict__ counts, int32_t* __restrict__ info,
                                                               uint8_t* __restrict__ rank) {
  __shared__ rew::Lds lds;
  const int lane = threadIdx.x, b0 = blockIdx.x * 64, b = b0 + lane;
  int len = rew::COPY, keep = 0;
  if (b < B) {
    rew::LdsWords W{lds.words + lane};
    rew::LdsClos C{lds.clos + lane};
    rew::LdsBytes O{lds.out + lane}, S{lds.start + lane}, D{lds.dfs + lane}, P{lds.parent + lane};
    rew::LdsHalf A{lds.half + lane};
    const fpr::PaddedSrc src{x + (long)b * x_ld};
    const int st = can::row(W, C, O, A, S, D, P, src, 1, T, false, V, tok_info, chem_info, emit, eos_id, max_content, &len,
                            info ? info + 4 * (long)b : nullptr, rank ? rank + rew::SLOTS * (long)b : nullptr);
    if (len == rew::COPY) keep = rew::copy_len(src, T, eos_id);
    status[b] = st;
    out_len[b] = len == rew::COPY ? keep : len + 2;
    if (counts) atomicAdd(counts + (st & 15), 1);
  }
  __syncthreads();
  rew::store_rows(lds, B, b0, lane, len, keep, x, x_ld, bos_id, eos_id, pad_id, T_out, out);
}

__global__ __launch_bounds__(64) void smiles_canon_corpus_kernel(const uint8_t* __restrict__ tokens, const int64_t* __restrict__ offsets, long N,
                                                                 const int64_t* __restrict__ rows, int B, int V,
                                                                 const int32_t* __restrict__ tok_info, const int32_t* __restrict__ chem_info,
                                                                 const int32_t* __restrict__ emit, int max_content, int stride,
                                                                 uint8_t* __restrict__ tokens_out, int64_t* __restrict__ offsets_out,
                                                                 int32_t* __restrict__ status, int32_t* __restrict__ counts,
                                                                 int32_t* __restrict__ err, int32_t* __restrict__ info,
                                                                 uint8_t* __restrict__ rank) {
  __shared__ rew::Lds lds;
  const int lane = threadIdx.x, b0 = blockIdx.x * 64, b = b0 + lane;
  int len = rew::COPY, keep = 0;
  long lo = 0;
  if (b < B) {
    const long id = rows[b];
    int32_t* info_b = info ? info + 4 * (long)b : nullptr;
    uint8_t* rank_b = rank ? rank + rew::SLOTS * (long)b : nullptr;
    int st = smg::SYNTAX;
    if (id >= 0 && id < N) {
      const long have = fpr::csr_len(offsets, id, &lo);
      rew::LdsWords W{lds.words + lane};
      rew::LdsClos C{lds.clos + lane};
      rew::LdsBytes O{lds.out + lane}, S{lds.start + lane}, D{lds.dfs + lane}, P{lds.parent + lane};
      rew::LdsHalf A{lds.half + lane};
      st = can::row(W, C, O, A, S, D, P, fpr::CsrSrc{tokens + lo}, 0, fpr::csr_end(have), true, V, tok_info, chem_info, emit, -1, max_content,
                    &len, info_b, rank_b);
      if (len == rew::COPY) {
        keep = (int)(have < stride ? have : stride);
        if (have > stride && err) atomicMax(err, 1);
      }
    } else {
      can::blank(info_b, rank_b);
      if (err) atomicMax(err, 2);
    }
    rew::store_corpus_row(b, B, stride, len, keep, st, offsets_out, status, counts);
  }
  __syncthreads();
  rew::store_corpus(lds, B, b0, lane, len, keep, lo, tokens, stride, tokens_out);
}

}  // namespace

extern "C" {

int mvae_smiles_canon_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info,
                           const int32_t* emit, int bos_id, int eos_id, int pad_id, int max_content, int T_out, int64_t* out, int32_t* out_len,
                           int32_t* status, int32_t* counts, int32_t* info, uint8_t* rank, void* stream) {
  if (V > 64) return MVAE_ERR_UNSUPPORTED;
  if (!rew::rows_args_ok(B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len, status))
    return MVAE_ERR_INVALID;
  hipLaunchKernelGGL(smiles_canon_rows_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, B, T, V, x, (long)x_ld, tok_info,
                     chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len, status, counts, info, rank);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

int mvae_smiles_canon_corpus(const uint8_t* tokens, const int64_t* offsets, int64_t N, const int64_t* rows, int B, int V,
                             const int32_t* tok_info, const int32_t* chem_info, const int32_t* emit, int max_content, int stride,
                             uint8_t* tokens_out, int64_t* offsets_out, int32_t* status, int32_t* counts, int32_t* err, int32_t* info,
                             uint8_t* rank, void* stream) {
  if (V > 64) return MVAE_ERR_UNSUPPORTED;
  if (!rew::corpus_args_ok(tokens, offsets, N, rows, B, V, tok_info, chem_info, emit, max_content, stride, tokens_out, offsets_out, status))
    return MVAE_ERR_INVALID;
  hipLaunchKernelGGL(smiles_canon_corpus_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, tokens, offsets, (long)N, rows, B, V,
                     tok_info, chem_info, emit, max_content, stride, tokens_out, offsets_out, status, counts, err, info, rank);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

int mvae_smiles_canon_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info,
                           const int32_t* emit, int bos_id, int eos_id, int pad_id, int max_content, int T_out, int64_t* out, int32_t* out_len,
                           int32_t* status, int32_t* info, uint8_t* rank) {
  if (V > 64) return MVAE_ERR_UNSUPPORTED;
  if (!rew::rows_args_ok(B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len, status))
    return MVAE_ERR_INVALID;
  fpr::HostArr<uint32_t, smg::ATOM_SLOTS> W;
  fpr::HostArr<uint16_t, fpr::CLOSURES> C;
  fpr::HostArr<uint8_t, smg::ATOM_SLOTS> O, S, D, P;
  fpr::HostArr<uint8_t, rew::HALF> A;
  for (long b = 0; b < B; ++b) {
    const fpr::PaddedSrc src{x + b * x_ld};
    int len = rew::COPY;
    status[b] = can::row(W, C, O, A, S, D, P, src, 1, T, false, V, tok_info, chem_info, emit, eos_id, max_content, &len,
                         info ? info + 4 * b : nullptr, rank ? rank + rew::SLOTS * b : nullptr);
    rew::host_store_row(O, src, T, len, bos_id, eos_id, pad_id, T_out, out + b * T_out, out_len + b);
  }
  return MVAE_OK;
}

}  // extern "C"
