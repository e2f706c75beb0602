// Substructure search over SMILES token rows (gfx950): mvae_smiles_substruct_rows / _corpus / _host and the query compiler
// mvae_smiles_substruct_compile_host.  include/mvae.h ("SMILES substructure") states the definition: a query fragment is compiled once
// on the host into a packed table; row t contains query q iff an injective map of the query's atoms into the row's keeps (element,
// aromatic, charge) of every atom and the bond class of every query bond -- a monomorphism, found by a backtracking search in a fixed
// order under a step budget, so that the first embedding, the step count and "undecided" are all defined.
//
// A seventh consumer of the walk of smiles_graph.hpp, on the adjacency of smiles_writer.hpp (rew::adjacency) behind a walk of its own:
// the writer's stereo refusal does not apply, a row with '@' still has a graph to search.  One thread per row, 64-thread blocks, and the
// rewrite's 80 KiB of LDS per block with nothing added: once the adjacency stands, the search index holds the map and the cursors (32
// bytes per lane each) and the search parent's storage holds the current query's table for the whole block.  Each row's graph is built
// once and all Q queries run against it; the query loop is wave-uniform, with a barrier around the staging of each table, so lanes
// without a row stay to the end, masked.  The search is ONE flat loop, one candidate per iteration, its state (depth, cursor) in a
// register and LDS: all lanes of a wave run one body until the slowest is done.  No runtime-indexed private array, no recursion, no
// stack.  Every loop is bounded by the step budget or by n <= 127, and every run-time index goes through a slot mask.
#include "common.hpp"
#include "smiles_writer.hpp"

namespace sub {

typedef smg::u64 u64;

constexpr int QATOMS = MVAE_SUBSTRUCT_QATOMS, QUERIES = MVAE_SUBSTRUCT_QUERIES, WORDS = MVAE_SUBSTRUCT_WORDS;
constexpr int MAX_STEPS = MVAE_SUBSTRUCT_MAX_STEPS;
constexpr int Q_ATOMS = MVAE_SMILES_QUERY_ATOMS;
enum : int { MISS = 0, HIT, UNDECIDED };
// the table of one query (include/mvae.h): word 0 the atoms, 1-3 the element counts as the walk packs them, then three words per atom
constexpr int T_N = 0, T_CNT = 1, T_ATOM = 4;
static_assert(WORDS == T_ATOM + 3 * QATOMS, "include/mvae.h states the table");
static_assert(QATOMS == 32 && QUERIES == 64, "five bits per query atom, one bit of an int64 per query");

// (element, aromatic, charge) of an atom word as one number below 128: what rule 1 compares
SMI_HD int key_of(uint32_t w) { return (int)((w >> 16) & 0x1F) | (int)((w >> 22) & 3) << 5; }
// atom word 0 of the table: bits 0-6 the key, 8-10 the degree, 12-16 the anchor, 20-22 its bond class, 24-26 the other earlier neighbours
SMI_HD int q_key(uint32_t a) { return (int)a & 0x7F; }
SMI_HD int q_deg(uint32_t a) { return (int)(a >> 8) & 7; }
SMI_HD int q_anchor(uint32_t a) { return (int)(a >> 12) & 31; }
SMI_HD int q_class(uint32_t a) { return (int)(a >> 20) & 7; }
SMI_HD int q_others(uint32_t a) { return (int)(a >> 24) & 7; }

// the class of the bond behind half-edge he of atom a (word wa) whose other end has word wn: 1, 2, 3, or 4 for a single bond between
// two aromatic atoms, as fpr::each_bond has it
template <class Words>
SMI_HD int bond_class(Words& W, int a, uint32_t wa, int he, uint32_t wn) {
  const int o = rew::he_order(W, a, wa, he);
  return o == 1 && smg::a_arom(wa) && smg::a_arom(wn) ? 4 : o;
}

SMI_HD void m_clear(smg::Mask& m, int i) {
  if (i < 64) m.lo &= ~(1ull << (i & 63));
  else m.hi &= ~(1ull << (i & 63));
}

// the recorder of the query compiler: Rec's bond orders and closures, and the atoms counted as they come, because the walk calls done()
// for status 0 only and a query may have status AROMATIC
template <class Clos>
struct CountRec {
  Clos& cl;
  int nclos = 0, n = 0;
  SMI_HD explicit CountRec(Clos& c) : cl(c) {}
  SMI_HD uint32_t atom_bits(int order) {
    ++n;
    return (uint32_t)order << 24;
  }
  SMI_HD void closure(int i, int j) {
    if (nclos < fpr::CLOSURES) cl.set(nclos++, (uint16_t)(i | j << 8));
  }
  SMI_HD void done(int, const smg::Mask&) {}
};

// every atom's half-edges by ascending neighbour: an insertion sort of at most 6
template <class Half, class Bytes>
SMI_HD void sort_half_edges(Half& A, Bytes& S, int n) {
  for (int k = 0; k < n; ++k) {
    const int s = S.get(k), e = S.get(k + 1);
    for (int i = s + 1; i < e && i < rew::HALF; ++i) {
      const int v = A.get(i);
      int j = i;
      for (; j > s; --j) {
        const int u = A.get(j - 1);
        if ((u & 0x7F) < (v & 0x7F)) break;
        A.set(j, (uint8_t)u);
      }
      A.set(j, (uint8_t)v);
    }
  }
}

// The walk and, for status 0, the adjacency with sorted half-edges.  Returns the status; *n = the atoms, *lo / *hi = the walk's element
// counts.
template <class Words, class Clos, class Half, class Bytes, class Src>
SMI_HD int build(Words& W, Clos& C, Half& A, Bytes& S, Bytes& D, Bytes& P, const Src& src, int first, int end, bool end_is_eos, int V,
                 const int32_t* tok_info, const int32_t* chem_info, int eos_id, int* n, u64* lo, u64* hi) {
  *n = 0; *lo = 0; *hi = 0;
  fpr::Rec<Clos> rec(C);
  smg::Row r;
  smg::walk(W, src, first, end, end_is_eos, V, tok_info, chem_info, eos_id, &r, rec);
  if (r.status != smg::OK) return r.status;
  if (rec.n < 1) return smg::SYNTAX;   // cannot happen: the automaton takes no row without an atom
  rew::adjacency(W, C, A, S, D, P, rec.n, rec.nclos < fpr::CLOSURES ? rec.nclos : fpr::CLOSURES);
  sort_half_edges(A, S, rec.n);
  *n = rec.n; *lo = r.cnt_lo; *hi = r.cnt_hi;
  return smg::OK;
}

// One (row, query): MISS, HIT or UNDECIDED; *steps = the candidates examined.  tab.get(i): word i of the query's table.  M: the map,
// M.get(i) = m(i) for the atoms placed so far (all of them after a HIT); Cu: the next candidate of every depth.
template <class Words, class Half, class Bytes, class Small, class Tab>
SMI_HD int search(Words& W, Half& A, Bytes& S, Small& M, Small& Cu, const Tab& tab, int n, u64 cnt_lo, u64 cnt_hi, int max_steps, int* steps) {
  *steps = 0;
  const int nq = tab.get(T_N);
  if (nq < 1 || nq > QATOMS) return MISS;
  const u64 q_lo = (u64)(uint32_t)tab.get(T_CNT) | (u64)(uint32_t)tab.get(T_CNT + 1) << 32, q_hi = (u64)(uint32_t)tab.get(T_CNT + 2);
  for (int e = 0; e < 10; ++e) {
    const int sh = 8 * (e & 7);
    if (((e < 8 ? q_lo : q_hi) >> sh & 0xFF) > ((e < 8 ? cnt_lo : cnt_hi) >> sh & 0xFF)) return MISS;
  }
  smg::Mask used{0, 0};
  int depth = 0, taken = 0, res = MISS;
  Cu.set(0, 0);
  // an iteration examines a candidate (<= max_steps of them) or steps back (once per candidate that was placed, and once at the end)
  for (int g = 0; g < 2 * max_steps + 2; ++g) {
    if (depth >= nq) { res = HIT; break; }
    const uint32_t qa = (uint32_t)tab.get(T_ATOM + 3 * depth);
    const int cur = Cu.get(depth);
    int cand = cur, he = 0, ma = 0;
    bool have = cur < n;
    if (depth > 0) {
      ma = M.get(q_anchor(qa)) & 0x7F;
      const int at = S.get(ma) + cur;
      have = at < (int)S.get(ma + 1);
      he = A.get(at);
      cand = he & 0x7F;
    }
    if (!have) {
      if (depth == 0) break;
      --depth;
      m_clear(used, M.get(depth) & 0x7F);
      continue;
    }
    if (taken >= max_steps) { res = UNDECIDED; break; }
    ++taken;
    Cu.set(depth, (uint8_t)(cur + 1));
    const uint32_t wc = W.get(cand);
    const int s = S.get(cand), e = S.get(cand + 1);
    bool ok = !smg::m_get(used, cand) && key_of(wc) == q_key(qa) && e - s >= q_deg(qa);
    if (ok && depth > 0) {
      ok = bond_class(W, ma, W.get(ma), he, wc) == q_class(qa);
      const u64 others = (u64)(uint32_t)tab.get(T_ATOM + 3 * depth + 1) | (u64)(uint32_t)tab.get(T_ATOM + 3 * depth + 2) << 32;
      const int no = q_others(qa);
      for (int k = 0; k < no && k < 5 && ok; ++k) {
        const int f = (int)(others >> 8 * k) & 0xFF, mj = M.get(f & 31) & 0x7F;
        int found = 0;
        for (int i = s; i < e && i < s + 6; ++i) {
          const int h = A.get(i);
          if ((h & 0x7F) == mj) found = bond_class(W, cand, wc, h, W.get(mj));
        }
        ok = found == f >> 5;
      }
    }
    if (ok) {
      M.set(depth, (uint8_t)cand);
      smg::m_set(used, cand);
      ++depth;
      if (depth < nq) Cu.set(depth, 0);
    }
  }
  *steps = taken;
  return res;
}

// the map of one row for the query of nq atoms: 0xFF beyond nq and where there is no hit
template <class Small>
SMI_HD void store_map(const Small& M, int res, int nq, uint8_t* map) {
  for (int k = 0; k < QATOMS; ++k) map[k] = res == HIT && k < nq ? M.get(k) : (uint8_t)0xFF;
}

struct HostTab {
  const int32_t* w;
  int32_t get(int i) const { return w[i]; }
};

inline bool args_ok(int V, const int32_t* tok_info, const int32_t* chem_info, int Q, const int32_t* table, int max_steps, int map_query,
                    const int32_t* status, const int64_t* hit, const int64_t* undecided, const uint8_t* map) {
  return fpr::tables_ok(V, tok_info, chem_info) && Q >= 1 && Q <= QUERIES && table && status && hit && undecided && max_steps >= 1 &&
         max_steps <= MAX_STEPS && (!map || (map_query >= 0 && map_query < Q));
}

// One query row into its table.  Returns the query's status: 0, or why it is refused (the table is then all zeros: a query of no atoms,
// which nothing contains).
template <class Src>
inline int compile(const Src& src, int first, int end, int V, const int32_t* tok_info, const int32_t* chem_info, u64 stereo, int eos_id,
                   int32_t* t) {
  for (int i = 0; i < WORDS; ++i) t[i] = 0;
  rew::Host g;                         // the output row is not used
  auto& W = g.W;
  auto& A = g.A;
  auto& S = g.S;
  CountRec<decltype(g.C)> rec(g.C);
  smg::Row r;
  smg::walk(W, src, first, end, false, V, tok_info, chem_info, eos_id, &r, rec);
  if (r.status != smg::OK && r.status != smg::AROMATIC) return r.status;
  for (int c = first; c < end && c - first <= smg::CONTENT_MAX; ++c) {
    const long tok = src.tok(c);
    if (tok == eos_id) break;
    if ((stereo >> (tok & 63)) & 1ull) return rew::STEREO;
  }
  const int n = rec.n;
  if (n < 1) return smg::SYNTAX;       // cannot happen: the automaton takes no row without an atom
  if (n > QATOMS) return Q_ATOMS;
  rew::adjacency(W, g.C, A, S, g.D, g.P, n, rec.nclos < fpr::CLOSURES ? rec.nclos : fpr::CLOSURES);
  sort_half_edges(A, S, n);
  u64 lo = 0, hi = 0;
  for (int i = 0; i < n; ++i) {
    const int e = smg::a_elem(W.get(i));
    if (e >= 1 && e <= 8) lo += 1ull << (8 * (e - 1));
    else if (e >= 9) hi += 1ull << (8 * (e - 9));
  }
  t[T_N] = n;
  t[T_CNT] = (int32_t)(uint32_t)lo; t[T_CNT + 1] = (int32_t)(uint32_t)(lo >> 32); t[T_CNT + 2] = (int32_t)(uint32_t)hi;
  for (int i = 0; i < n; ++i) {
    const uint32_t w = W.get(i);
    const int s = S.get(i), e = S.get(i + 1);
    // the earlier neighbours in ascending order: the first is the anchor
    int lower = 0, anchor = 0, cls = 0;
    u64 others = 0;
    for (int k = s; k < e && k < s + 6; ++k) {
      const int he = A.get(k), nb = he & 0x7F;
      if (nb >= i) continue;
      const int c = bond_class(W, i, w, he, W.get(nb));
      if (lower == 0) { anchor = nb; cls = c; }
      else others |= (u64)(nb | c << 5) << 8 * (lower - 1);
      ++lower;
    }
    const int no = lower > 0 ? lower - 1 : 0;
    t[T_ATOM + 3 * i] = (int32_t)((uint32_t)key_of(w) | (uint32_t)(e - s) << 8 | (uint32_t)anchor << 12 | (uint32_t)cls << 20 | (uint32_t)no << 24);
    t[T_ATOM + 3 * i + 1] = (int32_t)(uint32_t)others;
    t[T_ATOM + 3 * i + 2] = (int32_t)(uint32_t)(others >> 32);
  }
  return smg::OK;
}

}  // namespace sub

namespace {

// the storage of one 64-row block: rew::Lds with the closure list kept apart (no output row), the map and the cursors in the search
// index's place and the staged table in the search parent's, both of which the adjacency is done with when the first query starts.
// The writer's arrays are rew::Store's own members.
struct Lds {
  decltype(rew::Lds::W) W;
  decltype(rew::Lds::C) C;
  decltype(rew::Lds::A) A;
  decltype(rew::Lds::S) S;
  union {
    decltype(rew::Lds::D) D;
    fpr::LdsMem<uint8_t, sub::QATOMS> small[2];    // [0] the map, [1] the cursors
  };
  union {
    decltype(rew::Lds::P) P;
    int32_t table[sub::WORDS];
  };
};
static_assert(sizeof(Lds) == MVAE_SUBSTRUCT_LDS_BYTES, "include/mvae.h states the LDS per block");
static_assert(MVAE_SUBSTRUCT_LDS_BYTES <= 80 * 1024, "two blocks per CU");

struct LdsTab {
  const int32_t* w;
  __device__ __forceinline__ int32_t get(int i) const { return w[i & 127]; }
};
static_assert(sub::WORDS <= 128, "the slot mask of the staged table");

// What both kernels do for the block's 64 rows; the calling lane's row is number b and is read from src (have: it exists).  Every lane
// of the block comes here and stays to the end.
template <class Src>
__device__ __forceinline__ void block_rows(Lds& lds, bool have, long b, const Src& src, int first, int end, bool end_is_eos, int V,
                                           const int32_t* __restrict__ tok_info, const int32_t* __restrict__ chem_info, int eos_id, int Q,
                                           const int32_t* __restrict__ table, int max_steps, int map_query, int32_t* __restrict__ status,
                                           int64_t* __restrict__ hit, int64_t* __restrict__ undecided, uint8_t* __restrict__ map,
                                           int32_t* __restrict__ steps, int32_t* __restrict__ counts) {
  const int lane = threadIdx.x;
  auto W = lds.W.lane();
  auto C = lds.C.lane();
  auto A = lds.A.lane();
  auto S = lds.S.lane(), D = lds.D.lane(), P = lds.P.lane();
  auto M = lds.small[0].lane(), Cu = lds.small[1].lane();
  int st = smg::SYNTAX, n = 0;
  sub::u64 lo = 0, hi = 0;
  if (have) st = sub::build(W, C, A, S, D, P, src, first, end, end_is_eos, V, tok_info, chem_info, eos_id, &n, &lo, &hi);
  const bool searched = have && st == smg::OK;
  sub::u64 hits = 0, open = 0;
  for (int q = 0; q < Q; ++q) {
    __syncthreads();                   // the adjacency, or the search of query q - 1, is done with the table's storage
    for (int i = lane; i < sub::WORDS; i += 64) lds.table[i] = table[(long)q * sub::WORDS + i];
    __syncthreads();
    const LdsTab tab{lds.table};
    int res = sub::MISS, taken = 0;
    if (searched) res = sub::search(W, A, S, M, Cu, tab, n, lo, hi, max_steps, &taken);
    if (res == sub::HIT) hits |= 1ull << q;
    if (res == sub::UNDECIDED) open |= 1ull << q;
    if (have && steps) steps[b * Q + q] = taken;
    if (have && map && q == map_query) sub::store_map(M, res, tab.get(sub::T_N), map + b * sub::QATOMS);
    if (counts) {                      // all 64 lanes are here again: one ballot and one atomic per wave and figure
      const int nh = __popcll(__ballot(res == sub::HIT)), nu = __popcll(__ballot(res == sub::UNDECIDED));
      if (lane == 0 && nh) atomicAdd(counts + 2 * q, nh);
      if (lane == 0 && nu) atomicAdd(counts + 2 * q + 1, nu);
    }
  }
  if (have) {
    status[b] = st;
    hit[b] = (int64_t)hits;
    undecided[b] = (int64_t)open;
  }
}

__global__ __launch_bounds__(64) void smiles_substruct_rows_kernel(int B, int T, int V, const int64_t* __restrict__ x, long x_ld,
                                                                   const int32_t* __restrict__ tok_info, const int32_t* __restrict__ chem_info,
                                                                   int eos_id, int Q, const int32_t* __restrict__ table, int max_steps,
                                                                   int map_query, int32_t* __restrict__ status, int64_t* __restrict__ hit,
                                                                   int64_t* __restrict__ undecided, uint8_t* __restrict__ map,
                                                                   int32_t* __restrict__ steps, int32_t* __restrict__ counts) {
  __shared__ Lds lds;
  const long b = (long)blockIdx.x * 64 + threadIdx.x;
  const bool have = b < B;
  const fpr::PaddedSrc src{x + (have ? b : 0) * x_ld};
  block_rows(lds, have, b, src, 1, T, false, V, tok_info, chem_info, eos_id, Q, table, max_steps, map_query, status, hit, undecided, map, steps,
             counts);
}

__global__ __launch_bounds__(64) void smiles_substruct_corpus_kernel(const uint8_t* __restrict__ tokens, const int64_t* __restrict__ offsets,
                                                                     long N, int V, const int32_t* __restrict__ tok_info,
                                                                     const int32_t* __restrict__ chem_info, int Q,
                                                                     const int32_t* __restrict__ table, int max_steps, int map_query,
                                                                     int32_t* __restrict__ status, int64_t* __restrict__ hit,
                                                                     int64_t* __restrict__ undecided, uint8_t* __restrict__ map,
                                                                     int32_t* __restrict__ steps, int32_t* __restrict__ counts) {
  __shared__ Lds lds;
  const long b = (long)blockIdx.x * 64 + threadIdx.x;
  const bool have = b < N;
  long lo = 0, len = 0;
  if (have) len = fpr::csr_len(offsets, b, &lo);
  block_rows(lds, have, b, fpr::CsrSrc{tokens + lo}, 0, fpr::csr_end(len), true, V, tok_info, chem_info, -1, Q, table, max_steps, map_query,
             status, hit, undecided, map, steps, counts);
}

}  // namespace

extern "C" {

int mvae_smiles_substruct_compile_host(int Q, int Tq, int V, const int64_t* xq, int64_t xq_ld, const int32_t* tok_info, const int32_t* chem_info,
                                       uint32_t stereo_lo, uint32_t stereo_hi, int eos_id, int32_t* table, int32_t* qstatus) {
  if (V > 64) return MVAE_ERR_UNSUPPORTED;
  if (!fpr::padded_rows_ok(Q, Tq, V, xq, xq_ld, tok_info, chem_info, eos_id) || Q > sub::QUERIES || !table || !qstatus) return MVAE_ERR_INVALID;
  const sub::u64 stereo = (sub::u64)stereo_lo | (sub::u64)stereo_hi << 32;
  for (long q = 0; q < Q; ++q)
    qstatus[q] = sub::compile(fpr::PaddedSrc{xq + q * xq_ld}, 1, Tq, V, tok_info, chem_info, stereo, eos_id, table + q * sub::WORDS);
  return MVAE_OK;
}

int mvae_smiles_substruct_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, int eos_id,
                               int Q, const int32_t* table, int max_steps, int map_query, int32_t* status, int64_t* hit, int64_t* undecided,
                               uint8_t* map, int32_t* steps, int32_t* counts, void* stream) {
  if (V > 64) return MVAE_ERR_UNSUPPORTED;
  if (!fpr::padded_rows_ok(B, T, V, x, x_ld, tok_info, chem_info, eos_id) ||
      !sub::args_ok(V, tok_info, chem_info, Q, table, max_steps, map_query, status, hit, undecided, map))
    return MVAE_ERR_INVALID;
  hipLaunchKernelGGL(smiles_substruct_rows_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, B, T, V, x, (long)x_ld, tok_info,
                     chem_info, eos_id, Q, table, max_steps, map_query, status, hit, undecided, map, steps, counts);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

int mvae_smiles_substruct_corpus(const uint8_t* tokens, const int64_t* offsets, int64_t N, int V, const int32_t* tok_info,
                                 const int32_t* chem_info, int Q, const int32_t* table, int max_steps, int map_query, int32_t* status,
                                 int64_t* hit, int64_t* undecided, uint8_t* map, int32_t* steps, int32_t* counts, void* stream) {
  if (V > 64) return MVAE_ERR_UNSUPPORTED;
  if (!tokens || !offsets || N < 1 || !sub::args_ok(V, tok_info, chem_info, Q, table, max_steps, map_query, status, hit, undecided, map))
    return MVAE_ERR_INVALID;
  if ((N + 63) / 64 > (int64_t)INT_MAX) return MVAE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(smiles_substruct_corpus_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, tokens, offsets, (long)N,
                     V, tok_info, chem_info, Q, table, max_steps, map_query, status, hit, undecided, map, steps, counts);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

int mvae_smiles_substruct_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, int eos_id,
                               int Q, const int32_t* table, int max_steps, int map_query, int32_t* status, int64_t* hit, int64_t* undecided,
                               uint8_t* map, int32_t* steps, int32_t* counts) {
  if (V > 64) return MVAE_ERR_UNSUPPORTED;
  if (!fpr::padded_rows_ok(B, T, V, x, x_ld, tok_info, chem_info, eos_id) ||
      !sub::args_ok(V, tok_info, chem_info, Q, table, max_steps, map_query, status, hit, undecided, map))
    return MVAE_ERR_INVALID;
  rew::Host g;                         // the output row is not used
  auto& W = g.W;
  auto& A = g.A;
  auto& S = g.S;
  fpr::HostArr<uint8_t, sub::QATOMS> M, Cu;
  for (long b = 0; b < B; ++b) {
    int n;
    sub::u64 lo, hi, hits = 0, open = 0;
    const int st = sub::build(W, g.C, A, S, g.D, g.P, fpr::PaddedSrc{x + b * x_ld}, 1, T, false, V, tok_info, chem_info, eos_id, &n, &lo, &hi);
    for (int q = 0; q < Q; ++q) {
      const sub::HostTab tab{table + (long)q * sub::WORDS};
      int res = sub::MISS, taken = 0;
      if (st == smg::OK) res = sub::search(W, A, S, M, Cu, tab, n, lo, hi, max_steps, &taken);
      if (res == sub::HIT) hits |= 1ull << q;
      if (res == sub::UNDECIDED) open |= 1ull << q;
      if (steps) steps[b * Q + q] = taken;
      if (map && q == map_query) sub::store_map(M, res, tab.get(sub::T_N), map + b * sub::QATOMS);
      if (counts) {
        counts[2 * q] += res == sub::HIT;
        counts[2 * q + 1] += res == sub::UNDECIDED;
      }
    }
    status[b] = st;
    hit[b] = (int64_t)hits;
    undecided[b] = (int64_t)open;
  }
  return MVAE_OK;
}

}  // extern "C"
