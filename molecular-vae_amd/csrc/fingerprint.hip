// Circular fingerprints of SMILES token rows and Tanimoto similarity over them (gfx950): mvae_smiles_fp_rows / _corpus / _host,
// mvae_tanimoto_knn, mvae_tanimoto_sum.  include/mvae.h ("Circular fingerprint", "Tanimoto similarity") states the definitions.
//
// Fingerprint: a second consumer of the walk of smiles_graph.hpp.  The walk runs with a recorder (smiles_rounds.hpp, shared with
// scaffold.hip, as are mix, each_bond, the LDS arrays and the token sources) that keeps what the rounds need and the
// walk itself does not: the order of the bond to the tree predecessor (bits 24-31 of the atom word) and the ring-closure pairs.  One
// thread per row, 64-thread blocks, as in smiles_graph.hip; everything indexed by a run-time atom number lives in LDS, lane-minor
// ([slot][lane]: the 64 lanes of a wave touch 64 consecutive words, lanes never share a word), never in a private array:
//   atom words            128 slots x 64 lanes x 4 B = 32 KiB
//   ids of round r - 1    128 x 64 x 4 B             = 32 KiB      the two id arrays swap roles from round to round
//   ids of round r        128 x 64 x 4 B             = 32 KiB
//   closure pairs          64 x 64 x 2 B             =  8 KiB      i | j << 8; a closure takes two of the 127 tokens, so at most 63
//   fingerprint bits       32 x 64 x 4 B             =  8 KiB      1024 bits as 32 dwords, set by a run-time bit number
// 112 KiB per block: one block per CU.  The rounds are edge-centric -- every bond (the tree bonds from the atom words, then the closure
// list) adds its two directed terms to the two ends' sums -- so there is no adjacency list, and the commutative sum needs no order.
//
// Tanimoto search: the shape of latent_knn.hip.  Lanes over TABLE rows: a lane keeps its row's 32 dwords and its popcount in VGPRs, and
// walks a tile of up to 64 queries whose 32 dwords are the same for every lane and arrive by scalar loads; a pair costs 32 AND and 32
// accumulating popcounts.  A lane reads its own 128-byte row by eight 16-byte loads (row-per-lane loads, as latent_knn.hip's): the 64
// lanes of such a load touch 64 different lines, but the eight loads of a lane are issued back to back and use every byte of its line, so
// each line is fetched once, and the load is paid once per 64 queries; staging through LDS or a tiled table would add a pass, or a second
// layout of the table, to save nothing the query tile does not already amortise.  Similarities are kept as the exact fraction (c, u)
// = (|a & b|, |a | b|) packed in one dword and compared by cross-multiplication (both <= 2048); the one f32 division happens where a
// result is written.  Each wave owns a sorted k-entry list per query of the tile in LDS behind a one-compare threshold; the four waves'
// lists, and the slots' partial lists when the table is split, are merged by (similarity descending, row ascending).
//
// Pairwise sum: lanes over the rows of b, the rows of a by scalar loads, one correctly rounded f32 division per pair, accumulated in f64
// per lane in ascending order of a's rows; a fixed tree per block, then one block adds the per-block partials in a fixed order.  No
// floating-point atomics; two runs are bitwise equal.
#include <limits.h>

#include "common.hpp"
#include "smiles_rounds.hpp"

namespace fpr {

constexpr int WORDS = MVAE_FP_WORDS;   // int64 words of a fingerprint
constexpr int DWORDS = 2 * WORDS;

template <class Bits>
SMI_HD void set_bit(Bits& bits, uint32_t id) {
  const int b = (int)(id & 1023u);
  bits.set(b >> 5, bits.get(b >> 5) | 1u << (b & 31));
}

// id_r from id_{r-1} (S -> D), and its bits
template <class Atoms, class Ids, class Clos, class Bits>
SMI_HD void hash_round(uint32_t r, Atoms& at, Ids& S, Ids& D, Clos& cl, Bits& bits, int n, int nclos) {
  for (int k = 0; k < n; ++k) D.set(k, 0u);
  each_bond(at, cl, n, nclos, [&](int a, int b, uint32_t bt) {
    const uint32_t key = bt * 0x7FEB352Du, ia = S.get(a), ib = S.get(b);
    D.set(a, D.get(a) + mix(ib ^ key));
    D.set(b, D.get(b) + mix(ia ^ key));
  });
  for (int k = 0; k < n; ++k) {
    const uint32_t id = mix(S.get(k) * 0x9E3779B1u + r + D.get(k));
    D.set(k, id);
    set_bit(bits, id);
  }
}

// The 1024 bits of a row whose walk ended OK, into bits[0 .. 32).  at: the atom words the walk left; A, B: two id arrays.
template <class Atoms, class Ids, class Clos, class Bits>
SMI_HD void rounds(Atoms& at, Ids& A, Ids& B, Clos& cl, Bits& bits, int n, int nclos, const smg::Mask& ring) {
  for (int k = 0; k < n; ++k) A.set(k, 0u);
  each_bond(at, cl, n, nclos, [&](int a, int b, uint32_t) {      // the degrees
    A.set(a, A.get(a) + 1u);
    A.set(b, A.get(b) + 1u);
  });
  for (int k = 0; k < n; ++k) {
    const uint32_t w = at.get(k);
    const uint32_t inv = (uint32_t)smg::a_elem(w) | (uint32_t)smg::a_arom(w) << 4 | (uint32_t)(smg::a_chg(w) + 1) << 5 |
                         (uint32_t)smg::m_get(ring, k) << 7 | A.get(k) << 8 | (uint32_t)smg::a_used(w) << 12;
    const uint32_t id = mix(inv);
    A.set(k, id);
    set_bit(bits, id);
  }
  hash_round(1u, at, A, B, cl, bits, n, nclos);
  hash_round(2u, at, B, A, cl, bits, n, nclos);
}

// The consumer the row driver (smiles_rounds.hpp) runs.  at: the atom words; A, B: the two id arrays; bits: the 1024 bits; cl: the closures.
struct Fp {
  template <template <class, int> class Arr>
  struct Store {
    Arr<uint32_t, smg::ATOM_SLOTS> at, A, B;
    Arr<uint32_t, DWORDS> bits;
    Arr<uint16_t, CLOSURES> cl;
  };
  typedef Store<LdsMem> Lds;
  static __device__ Store<LdsArr> lane(Lds& l) { return {l.at.lane(), l.A.lane(), l.B.lane(), l.bits.lane(), l.cl.lane()}; }
  typedef Store<HostArr> Host;

  struct Out {
    int32_t* status;
    int64_t* fp;
    bool ok() const { return status && fp; }
  };

  // One row: the walk, then the rounds; status and the 16 words are written together (zeros for a row that is not OK).
  template <class S, class Src>
  static SMI_HD void row(S& s, const Src& src, int first, int end, bool end_is_eos, int V, const int32_t* tok_info, const int32_t* chem_info,
                         int eos_id, long b, const Out& o) {
    Rec<decltype(s.cl)> rec(s.cl);
    smg::Row r;
    smg::walk(s.at, src, first, end, end_is_eos, V, tok_info, chem_info, eos_id, &r, rec);
    for (int w = 0; w < DWORDS; ++w) s.bits.set(w, 0u);
    if (r.status == smg::OK) rounds(s.at, s.A, s.B, s.cl, s.bits, rec.n, rec.nclos, rec.ring);
    o.status[b] = r.status;
    for (int w = 0; w < WORDS; ++w) o.fp[b * WORDS + w] = (int64_t)((uint64_t)s.bits.get(2 * w) | (uint64_t)s.bits.get(2 * w + 1) << 32);
  }
};

}  // namespace fpr

namespace {

// ---------------------------------------------------------------------------------------------------------------- Tanimoto
constexpr int TN_QT = 64;           // queries per block tile
constexpr int TN_ROWS = 256;        // table rows per block step: 4 waves x 64 lanes, one row per lane
constexpr int TN_BLOCKS = 512;      // workgroups the row split aims for: two per CU
constexpr int TN_MAX_SLOTS = 256;   // the merge gives a lane at most TN_MAX_SLOTS / 64 partial lists
constexpr int TN_K_MAX = 32;        // documented in include/mvae.h
constexpr int TN_NONE = INT_MAX;    // row offset of an empty list entry
constexpr long TN_NONE64 = LONG_MAX;
constexpr int TN_D = fpr::DWORDS;

struct TnPlan {
  int slots;          // partial lists per query
  long slot_rows;     // table rows per slot, a multiple of TN_ROWS
  unsigned qtiles;
};

// depends on the shape alone
TnPlan tn_plan(int Q, int64_t N) {
  TnPlan p;
  p.qtiles = (unsigned)(((long)Q + TN_QT - 1) / TN_QT);
  const long tiles = ((long)N + TN_ROWS - 1) / TN_ROWS;
  long s = (TN_BLOCKS + (long)p.qtiles - 1) / (long)p.qtiles;
  if (s > tiles) s = tiles;
  if (s > TN_MAX_SLOTS) s = TN_MAX_SLOTS;
  if (s < 1) s = 1;
  const long tps = (tiles + s - 1) / s;
  p.slots = (int)((tiles + tps - 1) / tps);
  p.slot_rows = tps * TN_ROWS;
  return p;
}

size_t tn_ws_bytes(const TnPlan& p, int Q, int k) {
  return p.slots > 1 ? (size_t)p.slots * (size_t)Q * (size_t)k * (sizeof(long) + sizeof(uint32_t)) : 0;
}

// A similarity is kept as key = c << 16 | u, the fraction c / u of the intersection and union counts (u >= 1; an empty union is the
// fraction 0 / 1); the key 0 is an empty list entry, whose row is TN_NONE.  a before b iff a's fraction is larger, or equal with the
// lower row: the cross-products of an empty entry are 0 on both sides, so it ties with everything and its row puts it last.
__device__ __forceinline__ bool tn_before(uint32_t ka, long ja, uint32_t kb, long jb) {
  const uint32_t l = (ka >> 16) * (kb & 0xFFFFu), r = (kb >> 16) * (ka & 0xFFFFu);
  return l > r || (l == r && ja < jb);
}
// the one division: correctly rounded f32 of the two integers
__device__ __forceinline__ float tn_sim(uint32_t c, uint32_t u) { return u ? __fdiv_rn((float)c, (float)u) : 0.f; }

// a lane's own table row (row-per-lane loads) and its popcount
__device__ __forceinline__ int tn_load_row(const uint32_t* __restrict__ p, uint32_t (&tr)[TN_D]) {
  int pb = 0;
#pragma unroll
  for (int d = 0; d < TN_D; d += 4) {
    const uint4 v = *reinterpret_cast<const uint4*>(p + d);
    tr[d] = v.x; tr[d + 1] = v.y; tr[d + 2] = v.z; tr[d + 3] = v.w;
    pb += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
  }
  return pb;
}

// c = |q & row|, pa = |q|; qp is the same address in every lane (scalar loads, the popcount of q on the scalar unit)
__device__ __forceinline__ void tn_pair(const uint32_t* __restrict__ qp, const uint32_t (&tr)[TN_D], int& c, int& pa) {
  c = 0;
  pa = 0;
#pragma unroll
  for (int d = 0; d < TN_D; ++d) {
    const uint32_t qd = qp[d];
    c += __popc(qd & tr[d]);
    pa += __popc(qd);
  }
}

// One wave merges `nlists` sorted lists of k entries into the first k by tn_before.  Lane l owns lists l, l + 64, ... (at most four) and a
// head position in each; a round takes the best head of all lists (a butterfly; rows are distinct) and the owner advances.
// load(list, pos, key, j) reads an entry, store(pos, key, j) receives the result ((0, TN_NONE64) once the lists ran dry).
template <class Load, class Store>
__device__ __forceinline__ void tn_wave_merge(int nlists, int k, Load load, Store store) {
  const int lane = threadIdx.x & 63;
  int h[4] = {0, 0, 0, 0};
  for (int r = 0; r < k; ++r) {
    uint32_t bk = 0u;
    long bj = TN_NONE64;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int list = lane + 64 * s;
      if (list < nlists && h[s] < k) {
        uint32_t key;
        long j;
        load(list, h[s], key, j);
        if (tn_before(key, j, bk, bj)) { bk = key; bj = j; }
      }
    }
    uint32_t wk = bk;
    long wj = bj;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t ok = (uint32_t)__shfl_xor((int)wk, o, 64);
      const long oj = __shfl_xor((long long)wj, o, 64);
      if (tn_before(ok, oj, wk, wj)) { wk = ok; wj = oj; }
    }
    if (wj != TN_NONE64) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int list = lane + 64 * s;
        if (list < nlists && h[s] < k) {
          uint32_t key;
          long j;
          load(list, h[s], key, j);
          if (j == wj) ++h[s];
        }
      }
    }
    if (lane == 0) store(r, wk, wj);
  }
}

__device__ __forceinline__ void tn_write(float* __restrict__ sim, long* __restrict__ idx, long e, uint32_t key, long j) {
  const bool none = j == TN_NONE64;
  sim[e] = none ? -1.f : tn_sim(key >> 16, key & 0xFFFFu);
  idx[e] = none ? -1 : j;
}

// grid (query tiles, slots), 256 threads.  part_k / part_j == NULL: one slot, the block writes sim / idx itself.
__global__ __launch_bounds__(256, 2) void tanimoto_knn_scan_kernel(int Q, long N, int k, const uint32_t* __restrict__ q,
                                                                   const uint32_t* __restrict__ table, const long* __restrict__ exclude,
                                                                   long slot_rows, float* __restrict__ sim, long* __restrict__ idx,
                                                                   uint32_t* __restrict__ part_k, long* __restrict__ part_j) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tn_smem[];
  uint32_t* Lk = reinterpret_cast<uint32_t*>(tn_smem);            // [4 waves][TN_QT][k] keys
  int* Lj = reinterpret_cast<int*>(Lk + 4 * TN_QT * k);           // [4 waves][TN_QT][k] row offsets from the slot's first row
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int q0 = blockIdx.x * TN_QT;
  const int nq = min(TN_QT, Q - q0);
  const long r_beg = (long)blockIdx.y * slot_rows;
  const long r_end = min(r_beg + slot_rows, N);
  for (int e = tid; e < 4 * TN_QT * k; e += 256) {
    Lk[e] = 0u;
    Lj[e] = TN_NONE;
  }
  __syncthreads();
  uint32_t* wLk = Lk + wv * TN_QT * k;
  int* wLj = Lj + wv * TN_QT * k;

  for (long c0 = r_beg + wv * 64; c0 < r_end; c0 += TN_ROWS) {
    const long row = c0 + lane;
    const bool live = row < r_end;
    const int off = (int)(row - r_beg);
    // rows past the end repeat the last one (their lanes never become candidates): the loads need no branch
    uint32_t tr[TN_D];
    const int pb = tn_load_row(table + (live ? row : r_end - 1) * TN_D, tr);
#pragma unroll 1
    for (int qi = 0; qi < nq; ++qi) {
      int c, pa;
      tn_pair(q + (long)(q0 + qi) * TN_D, tr, c, pa);
      const int u = max(pa + pb - c, 1);                            // an empty union: 0 / 1
      const long ex = exclude ? exclude[q0 + qi] : -1;
      // the list's last key: 0 while the list is not full, and then every row is a candidate.  A wave meets its rows in ascending order,
      // so a row that only ties with the last entry never displaces it: the test is strict.  A stale (smaller) threshold would only
      // admit more candidates.
      const uint32_t thr = wLk[qi * k + (k - 1)];
      const uint32_t tc = thr >> 16, tu = thr & 0xFFFFu;
      unsigned long long m = __ballot(live && row != ex && (thr == 0u || (uint32_t)c * tu > tc * (uint32_t)u));
      if (m) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const uint32_t key = (uint32_t)c << 16 | (uint32_t)u;
        uint32_t lk = lane < k ? wLk[qi * k + lane] : 0u;          // entry e of the list in lane e
        int lj = lane < k ? wLj[qi * k + lane] : TN_NONE;
        while (m) {                                                 // lowest lane = lowest row first
          const int l = __ffsll(m) - 1;
          m &= m - 1;
          const uint32_t ck = (uint32_t)__shfl((int)key, l, 64);
          const int cj = __shfl(off, l, 64);
          const int pos = __popcll(__ballot(lane < k && tn_before(lk, lj, ck, cj)));      // the list is sorted: a prefix
          if (pos < k) {
            const uint32_t uk = (uint32_t)__shfl_up((int)lk, 1, 64);
            const int uj = __shfl_up(lj, 1, 64);
            if (lane > pos) { lk = uk; lj = uj; }
            else if (lane == pos) { lk = ck; lj = cj; }
          }
        }
        if (lane < k) {
          wLk[qi * k + lane] = lk;
          wLj[qi * k + lane] = lj;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      }
    }
  }
  __syncthreads();
  // the four waves' lists of a query become one: the final answer, or this slot's partial list
  for (int qi = wv; qi < nq; qi += 4) {
    const long qg = q0 + qi;
    auto load = [&](int list, int pos, uint32_t& key, long& j) {
      const int e = (list * TN_QT + qi) * k + pos;
      key = Lk[e];
      const int o = Lj[e];
      j = o == TN_NONE ? TN_NONE64 : r_beg + o;
    };
    if (part_k) {
      const long base = ((long)blockIdx.y * Q + qg) * k;
      tn_wave_merge(4, k, load, [&](int r, uint32_t key, long j) { part_k[base + r] = key; part_j[base + r] = j; });
    } else {
      tn_wave_merge(4, k, load, [&](int r, uint32_t key, long j) { tn_write(sim, idx, qg * k + r, key, j); });
    }
  }
}

// one wave per query: the slots' partial lists, owned by the lanes in slot order, become the answer
__global__ __launch_bounds__(256) void tanimoto_knn_merge_kernel(int Q, int k, int slots, const uint32_t* __restrict__ part_k,
                                                                 const long* __restrict__ part_j, float* __restrict__ sim,
                                                                 long* __restrict__ idx) {
  const long qg = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (qg >= Q) return;
  tn_wave_merge(
      slots, k,
      [&](int list, int pos, uint32_t& key, long& j) {
        const long e = ((long)list * Q + qg) * k + pos;
        key = part_k[e];
        j = part_j[e];
      },
      [&](int r, uint32_t key, long j) { tn_write(sim, idx, qg * k + r, key, j); });
}

constexpr int TS_BLOCKS = 1024;     // workgroups the split of a's rows aims for: four per CU
constexpr int TS_A_MIN = 64;        // fewest rows of a per block

struct TsPlan {
  long btiles, achunks, a_rows;     // 256-row tiles of b; chunks of a and the rows of a per chunk
};

// depends on the shape alone
TsPlan ts_plan(int64_t M, int64_t N) {
  TsPlan p;
  p.btiles = ((long)N + TN_ROWS - 1) / TN_ROWS;
  long c = (TS_BLOCKS + p.btiles - 1) / p.btiles;
  const long most = ((long)M + TS_A_MIN - 1) / TS_A_MIN;
  if (c > most) c = most;
  if (c < 1) c = 1;
  p.a_rows = ((long)M + c - 1) / c;
  p.achunks = ((long)M + p.a_rows - 1) / p.a_rows;
  return p;
}

// a fixed tree over the 256 values of a block; the result in thread 0
__device__ __forceinline__ double ts_block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// grid (tiles of b, chunks of a), 256 threads: partial[chunk * tiles + tile]
__global__ __launch_bounds__(256) void tanimoto_sum_kernel(long M, long N, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                           int skip_diagonal, long a_rows, double* __restrict__ partial) {
  __shared__ double red[256];
  const long j = (long)blockIdx.x * TN_ROWS + threadIdx.x;
  const bool live = j < N;
  uint32_t tr[TN_D];
  const int pb = tn_load_row(b + (live ? j : N - 1) * TN_D, tr);
  const long i_beg = (long)blockIdx.y * a_rows, i_end = min(i_beg + a_rows, M);
  const long skip = skip_diagonal ? j : -1;
  double acc = 0.0;
#pragma unroll 1
  for (long i = i_beg; i < i_end; ++i) {
    int c, pa;
    tn_pair(a + i * TN_D, tr, c, pa);
    const float t = tn_sim((uint32_t)c, (uint32_t)(pa + pb - c));
    if (live && i != skip) acc += (double)t;
  }
  const double s = ts_block_sum(acc, red);
  if (threadIdx.x == 0) partial[(long)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// one block: thread t adds partials t, t + 256, ... in ascending order, then the fixed tree
__global__ __launch_bounds__(256) void tanimoto_sum_final_kernel(long n, const double* __restrict__ partial, double* __restrict__ out) {
  __shared__ double red[256];
  double acc = 0.0;
  for (long e = threadIdx.x; e < n; e += 256) acc += partial[e];
  const double s = ts_block_sum(acc, red);
  if (threadIdx.x == 0) out[0] = s;
}

}  // namespace

extern "C" {

int mvae_smiles_fp_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, int eos_id,
                        int32_t* status, int64_t* fp, void* stream) {
  return fpr::rows<fpr::Fp>(B, T, V, x, x_ld, tok_info, chem_info, eos_id, stream, status, fp);
}

int mvae_smiles_fp_corpus(const uint8_t* tokens, const int64_t* offsets, int64_t N, int V, const int32_t* tok_info, const int32_t* chem_info,
                          int32_t* status, int64_t* fp, void* stream) {
  return fpr::corpus<fpr::Fp>(tokens, offsets, N, V, tok_info, chem_info, stream, status, fp);
}

int mvae_smiles_fp_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, int eos_id,
                        int32_t* status, int64_t* fp) {
  return fpr::host<fpr::Fp>(B, T, V, x, x_ld, tok_info, chem_info, eos_id, status, fp);
}

size_t mvae_tanimoto_knn_workspace(int Q, int64_t N, int k) {
  if (Q < 1 || N < 1 || k < 1 || k > TN_K_MAX) return 0;
  return tn_ws_bytes(tn_plan(Q, N), Q, k);
}

int mvae_tanimoto_knn(int Q, int64_t N, int k, const int64_t* q, const int64_t* table, const int64_t* exclude, float* sim, int64_t* idx,
                      void* ws, size_t ws_bytes, void* stream) {
  if (!q || !table || !sim || !idx || Q < 1 || N < 1 || k < 1) return MVAE_ERR_INVALID;
  if ((uintptr_t)q % 16 || (uintptr_t)table % 16) return MVAE_ERR_INVALID;
  if (k > TN_K_MAX) return MVAE_ERR_UNSUPPORTED;
  const TnPlan p = tn_plan(Q, N);
  if (p.slot_rows >= (long)TN_NONE) return MVAE_ERR_UNSUPPORTED;        // row offsets inside a slot are 32-bit (N >= 2^39)
  uint32_t* part_k = nullptr;
  long* part_j = nullptr;
  if (p.slots > 1) {
    if (!ws || ws_bytes < tn_ws_bytes(p, Q, k)) return MVAE_ERR_WORKSPACE;
    if ((uintptr_t)ws % alignof(long)) return MVAE_ERR_INVALID;
    part_j = (long*)ws;
    part_k = (uint32_t*)(part_j + (size_t)p.slots * (size_t)Q * (size_t)k);
  }
  const size_t smem = (size_t)4 * TN_QT * k * (sizeof(uint32_t) + sizeof(int));
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tanimoto_knn_scan_kernel, dim3(p.qtiles, (unsigned)p.slots), dim3(256), smem, st, Q, (long)N, k, (const uint32_t*)q,
                     (const uint32_t*)table, (const long*)exclude, p.slot_rows, sim, (long*)idx, part_k, part_j);
  MVAE_CHECK_HIP(hipGetLastError());
  if (part_k) {
    hipLaunchKernelGGL(tanimoto_knn_merge_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, st, Q, k, p.slots, part_k, part_j, sim, (long*)idx);
    MVAE_CHECK_HIP(hipGetLastError());
  }
  return MVAE_OK;
}

size_t mvae_tanimoto_sum_workspace(int64_t M, int64_t N) {
  if (M < 1 || N < 1) return 0;
  const TsPlan p = ts_plan(M, N);
  return (size_t)p.btiles * (size_t)p.achunks * sizeof(double);
}

int mvae_tanimoto_sum(int64_t M, int64_t N, const int64_t* a, const int64_t* b, int skip_diagonal, double* out, void* ws, size_t ws_bytes,
                      void* stream) {
  if (!a || !b || !out || M < 1 || N < 1) return MVAE_ERR_INVALID;
  if ((uintptr_t)a % 16 || (uintptr_t)b % 16) return MVAE_ERR_INVALID;
  const TsPlan p = ts_plan(M, N);
  if (p.btiles > (long)INT_MAX) return MVAE_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < (size_t)p.btiles * (size_t)p.achunks * sizeof(double)) return MVAE_ERR_WORKSPACE;
  if ((uintptr_t)ws % alignof(double)) return MVAE_ERR_INVALID;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tanimoto_sum_kernel, dim3((unsigned)p.btiles, (unsigned)p.achunks), dim3(256), 0, st, (long)M, (long)N, (const uint32_t*)a,
                     (const uint32_t*)b, skip_diagonal ? 1 : 0, p.a_rows, (double*)ws);
  MVAE_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(tanimoto_sum_final_kernel, dim3(1), dim3(256), 0, st, p.btiles * p.achunks, (const double*)ws, out);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

}  // extern "C"
