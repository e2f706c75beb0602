// Token-level Levenshtein distance (gfx950): between the rows of two batches (mvae_edit_distance_rows) and as an exact k-nearest-neighbour
// search of sampled rows in the CSR corpus (mvae_edit_knn), the string-space sibling of latent_knn.hip.  include/mvae.h states the contract;
// this file states how it is kept.
//
// Distance: the bit-parallel recurrence of Myers (1999) in Hyyro's (2003) form for the full distance.  The pattern's match vectors Peq[v]
// (bit i set iff pattern token i == v) are built once; a column of the DP table is the pair of bit vectors (Pv, Mv) of its vertical +1 / -1
// deltas, one text token updates it with a dozen 64-bit logic operations and one add, and the distance follows the horizontal delta at
// the pattern's last row.  Patterns of up to 64 tokens take one 64-bit word; 65..128 take two, the horizontal delta that leaves word 0 at
// its top bit (-1 / 0 / +1) entering word 1.  A token outside [0, V) sets no bit on the pattern side and selects the all-zero vector on
// the text side, so it equals nothing and is never an index.
//
// Search layout: lanes over CORPUS rows, the queries broadcast, as in latent_knn.hip.  A block builds the match vectors of its tile of
// ED_QT queries in LDS, token-major ([v][query]), so that one 16-byte LDS read gives a lane the vectors of two neighbouring queries for its
// text token; a wave takes 64 corpus rows and walks the tile four queries at a time -- four independent recurrences per lane, which is
// what hides the latency of the LDS lookup and of the dependent 64-bit chain.  A lane streams its own row's bytes (eight byte loads ahead,
// addresses clamped into the row, so nothing outside tokens[0 : offsets[N]) is ever loaded); the loop runs to the wave's longest row and a
// lane whose row has ended only stops counting.  Whether a group takes the one-word or the two-word form depends on the queries alone:
// a uniform branch.
//
// Lists: one sorted k-entry list per (query, wave) in LDS, entry e in lane e while it is updated.  An entry is ONE 64-bit key,
// (distance << 32) | row offset inside the slot, so the order by (distance, row) is the order of the keys, the threshold test is one
// compare against the list's last key, and ties are settled exactly by it.  The four waves' lists are merged at the end of the block; when
// the corpus is split over slots, the block writes a partial list and a second launch merges the slots' lists by (distance, row).
#include <limits.h>

#include "common.hpp"
#include "launch.hpp"

namespace {

typedef unsigned long long u64;

constexpr int ED_QT = 32;            // queries per block tile
constexpr int ED_QG = 4;             // queries a lane advances together
constexpr int ED_ROWS = 256;         // corpus rows per block step: 4 waves x 64 lanes
constexpr int ED_BLOCKS = 512;       // workgroups the row split aims for: two per CU
constexpr int ED_MAX_SLOTS = 256;    // the merge gives a lane at most ED_MAX_SLOTS / 64 partial lists
constexpr int ED_K_MAX = 32;         // documented in include/mvae.h
constexpr int ED_V_MAX = 64;         // rows of a match-vector table: tokens 0..V-1 and the all-zero row V of a token that equals nothing
constexpr int ED_AHEAD = 8;          // text bytes loaded ahead per lane
constexpr long ED_NONE64 = LONG_MAX;
constexpr u64 ED_EMPTY = ((u64)MVAE_EDIT_NONE << 32) | (u64)(unsigned)INT_MAX;      // sorts behind every real (distance, offset)

struct EdPlan {
  int slots;          // partial lists per query
  long slot_rows;     // corpus rows per slot, a multiple of ED_ROWS
  unsigned qtiles;
};

// depends on the shape alone
EdPlan ed_plan(int Q, int64_t N) {
  EdPlan p;
  p.qtiles = (unsigned)(((long)Q + ED_QT - 1) / ED_QT);
  const long tiles = ((long)N + ED_ROWS - 1) / ED_ROWS;
  long s = (ED_BLOCKS + (long)p.qtiles - 1) / (long)p.qtiles;
  if (s > tiles) s = tiles;
  if (s > ED_MAX_SLOTS) s = ED_MAX_SLOTS;
  if (s < 1) s = 1;
  const long tps = (tiles + s - 1) / s;
  p.slots = (int)((tiles + tps - 1) / tps);
  p.slot_rows = tps * ED_ROWS;
  return p;
}

size_t ed_ws_bytes(const EdPlan& p, int Q, int k) {
  return p.slots > 1 ? (size_t)p.slots * (size_t)Q * (size_t)k * (sizeof(long) + sizeof(int)) : 0;
}

size_t ed_smem_bytes(int V, int k) {
  return (size_t)2 * (V + 1) * ED_QT * sizeof(u64) + (size_t)4 * ED_QT * k * sizeof(u64) + ED_QT * (sizeof(long) + sizeof(int));
}

// One text token in one 64-row block of the DP table.  Eq: the pattern rows of this block that match the token; hin: the horizontal delta
// entering above the block's first row (+1 for the table's first block: D[0][j] = j); (Pv, Mv): the column's vertical deltas, updated.
// Ph / Mh: the rows whose horizontal delta is +1 / -1, unshifted -- the caller reads the pattern's last row, or the top bit as the next
// block's hin.
__device__ __forceinline__ void ed_block(u64 Eq, int hin, u64& Pv, u64& Mv, u64& Ph, u64& Mh) {
  const u64 neg = hin < 0 ? 1ull : 0ull, pos = hin > 0 ? 1ull : 0ull;
  const u64 Xv = Eq | Mv;
  Eq |= neg;
  const u64 Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
  Ph = Mv | ~(Xh | Pv);
  Mh = Pv & Xh;
  const u64 Phs = (Ph << 1) | pos, Mhs = (Mh << 1) | neg;
  Pv = Mhs | ~(Xv | Phs);
  Mv = Phs & Xv;
}
__device__ __forceinline__ int ed_delta(u64 Ph, u64 Mh, u64 bit) { return ((Ph & bit) != 0) - ((Mh & bit) != 0); }

// The pattern side, by one wave: the content of row[1 : T] (T - 1 <= 128) cut before its first `eos`.  Returns its length m; lane v < V
// receives the match vector of token v in (w0, w1), every other lane zeros.  Columns >= T are never loaded, and the second 64 columns only
// when the first hold no `eos`.
__device__ __forceinline__ int ed_pattern(const int64_t* __restrict__ row, int T, int V, int eos, u64& w0, u64& w1) {
  const int lane = threadIdx.x & 63;
  const int L = T - 1;
  const int64_t v0 = lane < L ? row[1 + lane] : 0;
  int64_t v1 = 0;
  int m = L;
  const u64 e0 = __ballot(lane < L && v0 == (int64_t)eos);
  if (e0) {
    m = (int)__builtin_ctzll(e0);
  } else if (L > 64) {
    v1 = 64 + lane < L ? row[65 + lane] : 0;
    const u64 e1 = __ballot(64 + lane < L && v1 == (int64_t)eos);
    if (e1) m = 64 + (int)__builtin_ctzll(e1);
  }
  w0 = 0;
  w1 = 0;
  for (int v = 0; v < V; ++v) {
    const u64 b0 = __ballot(lane < m && v0 == (int64_t)v);
    const u64 b1 = __ballot(64 + lane < m && v1 == (int64_t)v);
    if (lane == v) { w0 = b0; w1 = b1; }
  }
  return m;
}

__device__ __forceinline__ bool ed_less(int da, long ja, int db, long jb) { return da < db || (da == db && ja < jb); }

// knn_wave_merge of latent_knn.hip over integer distances: one wave merges `nlists` sorted lists of k entries into the k smallest
// (distance, row), ascending.  Lane l owns lists l, l + 64, ... (at most four); an empty entry is (MVAE_EDIT_NONE, ED_NONE64).
template <class Load, class Store>
__device__ __forceinline__ void ed_wave_merge(int nlists, int k, Load load, Store store) {
  const int lane = threadIdx.x & 63;
  int h[4] = {0, 0, 0, 0};
  for (int r = 0; r < k; ++r) {
    int bd = MVAE_EDIT_NONE;
    long bj = ED_NONE64;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int list = lane + 64 * s;
      if (list < nlists && h[s] < k) {
        int d;
        long j;
        load(list, h[s], d, j);
        if (ed_less(d, j, bd, bj)) { bd = d; bj = j; }
      }
    }
    int wd = bd;
    long wj = bj;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int od = __shfl_xor(wd, o, 64);
      const long oj = __shfl_xor((long long)wj, o, 64);
      if (ed_less(od, oj, wd, wj)) { wd = od; wj = oj; }
    }
    if (wj != ED_NONE64) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int list = lane + 64 * s;
        if (list < nlists && h[s] < k) {
          int d;
          long j;
          load(list, h[s], d, j);
          if (j == wj) ++h[s];
        }
      }
    }
    if (lane == 0) store(r, wd, wj);
  }
}

// grid (query tiles, slots), 256 threads.  part_d / part_j == NULL: one slot, the block writes dist / idx itself.
__global__ __launch_bounds__(256) void edit_knn_scan_kernel(int Q, long N, int T, int V, int eos, int k, const int64_t* __restrict__ x, long x_ld,
                                                            const uint8_t* __restrict__ tokens, const int64_t* __restrict__ offsets,
                                                            const int64_t* __restrict__ exclude, long slot_rows, int* __restrict__ dist,
                                                            long* __restrict__ idx, int* __restrict__ part_d, long* __restrict__ part_j) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ed_smem[];
  u64* P0 = reinterpret_cast<u64*>(ed_smem);                        // [V + 1][ED_QT] match vectors, pattern rows 0..63
  u64* P1 = P0 + (V + 1) * ED_QT;                                   // [V + 1][ED_QT] pattern rows 64..127
  u64* Lk = P1 + (V + 1) * ED_QT;                                   // [4 waves][ED_QT][k] keys
  long* Qex = reinterpret_cast<long*>(Lk + 4 * ED_QT * k);          // [ED_QT] the row each query skips
  int* Qm = reinterpret_cast<int*>(Qex + ED_QT);                    // [ED_QT] pattern lengths
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int q0 = blockIdx.x * ED_QT;
  const int nq = min(ED_QT, Q - q0);
  const long r_beg = (long)blockIdx.y * slot_rows;
  const long r_end = min(r_beg + slot_rows, N);
  for (int e = tid; e < 2 * (V + 1) * ED_QT; e += 256) P0[e] = 0;   // P0 and P1; a query past nq stays the empty pattern
  for (int e = tid; e < 4 * ED_QT * k; e += 256) Lk[e] = ED_EMPTY;
  if (tid < ED_QT) {
    Qm[tid] = 0;
    Qex[tid] = exclude && tid < nq ? exclude[q0 + tid] : -1;
  }
  __syncthreads();
  for (int qi = wv; qi < nq; qi += 4) {
    u64 w0, w1;
    const int m = ed_pattern(x + (long)(q0 + qi) * x_ld, T, V, eos, w0, w1);
    if (lane < V) {
      P0[lane * ED_QT + qi] = w0;
      P1[lane * ED_QT + qi] = w1;
    }
    if (lane == 0) Qm[qi] = m;
  }
  __syncthreads();
  u64* wLk = Lk + wv * ED_QT * k;

  for (long c0 = r_beg + wv * 64; c0 < r_end; c0 += ED_ROWS) {
    const long row = c0 + lane;
    const bool live = row < r_end;
    const int off = (int)(row - r_beg);
    long o0 = 0;
    int len = 0;                                                     // a lane past the end holds an empty row and never becomes a candidate
    if (live) {
      o0 = offsets[row];
      const long l64 = offsets[row + 1] - o0;
      len = (int)(l64 < 0 ? 0 : l64 < (long)INT_MAX - 1 ? l64 : (long)INT_MAX - 1);
    }
    int maxlen = len;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) maxlen = max(maxlen, __shfl_xor(maxlen, o, 64));
    maxlen = __builtin_amdgcn_readfirstlane(maxlen);                 // the same in every lane: the loops below branch on the scalar side
    const uint8_t* __restrict__ tp = tokens + o0;
    const int last = len - 1;

#pragma unroll 1
    for (int g = 0; g < nq; g += ED_QG) {
      int m[ED_QG], sc[ED_QG];
      bool wide = false;
#pragma unroll
      for (int c = 0; c < ED_QG; ++c) {
        m[c] = Qm[g + c];
        sc[c] = m[c];
        wide |= m[c] > 64;
      }
      if (!wide) {
        u64 Pv[ED_QG], Mv[ED_QG], bit[ED_QG];
#pragma unroll
        for (int c = 0; c < ED_QG; ++c) {
          Pv[c] = ~0ull;
          Mv[c] = 0;
          bit[c] = m[c] > 0 ? 1ull << (m[c] - 1) : 0;
        }
#pragma unroll 1
        for (int j0 = 0; j0 < maxlen; j0 += ED_AHEAD) {
          int t[ED_AHEAD];
#pragma unroll
          for (int e = 0; e < ED_AHEAD; ++e) t[e] = len > 0 ? (int)tp[min(j0 + e, last)] : 0;
#pragma unroll
          for (int e = 0; e < ED_AHEAD; ++e) {
            const int j = j0 + e;
            if (j >= maxlen) break;
            const u64* __restrict__ pe = P0 + min(t[e], V) * ED_QT + g;
            const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(pe), b = *reinterpret_cast<const ulonglong2*>(pe + 2);
            const u64 Eq[ED_QG] = {a.x, a.y, b.x, b.y};
            const bool alive = j < len;
#pragma unroll
            for (int c = 0; c < ED_QG; ++c) {
              u64 Ph, Mh;
              ed_block(Eq[c], 1, Pv[c], Mv[c], Ph, Mh);
              const int d = ed_delta(Ph, Mh, bit[c]);
              sc[c] += alive ? d : 0;
            }
          }
        }
      } else {
#pragma unroll 1
        for (int c = 0; c < ED_QG; ++c) {
          const int mc = Qm[g + c];
          const bool two = mc > 64;
          const u64 bit = mc > 0 ? 1ull << ((mc - 1) & 63) : 0;
          u64 Pv0 = ~0ull, Mv0 = 0, Pv1 = ~0ull, Mv1 = 0;
          int s = mc;
#pragma unroll 1
          for (int j = 0; j < maxlen; ++j) {
            const int t = len > 0 ? (int)tp[min(j, last)] : 0;
            const int ti = min(t, V) * ED_QT + g + c;
            u64 Ph, Mh;
            ed_block(P0[ti], 1, Pv0, Mv0, Ph, Mh);
            if (two) {
              const int hout = ed_delta(Ph, Mh, 1ull << 63);
              ed_block(P1[ti], hout, Pv1, Mv1, Ph, Mh);
            }
            const int d = ed_delta(Ph, Mh, bit);
            s += j < len ? d : 0;
          }
#pragma unroll
          for (int cc = 0; cc < ED_QG; ++cc)
            if (cc == c) sc[cc] = s;
        }
      }
#pragma unroll
      for (int c = 0; c < ED_QG; ++c) {
        const int qi = g + c;
        if (qi >= nq) break;
        const int dd = m[c] > 0 ? sc[c] : len;                       // the empty pattern: every text token is an insertion
        const u64 key = ((u64)(unsigned)dd << 32) | (u64)(unsigned)off;
        // the list's last key: ED_EMPTY while the list is not full.  Keys are distinct (the offsets are), so "<" is the exact order by
        // (distance, row); a stale (larger) threshold would only admit more candidates
        const u64 thr = wLk[qi * k + (k - 1)];
        u64 cand = __ballot(live && row != Qex[qi] && key < thr);
        if (cand) {
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
          u64 lk = lane < k ? wLk[qi * k + lane] : ED_EMPTY;        // entry e of the list in lane e
          while (cand) {                                             // lowest lane = lowest row first
            const int l = __ffsll(cand) - 1;
            cand &= cand - 1;
            const u64 ck = __shfl(key, l, 64);
            const int pos = __popcll(__ballot(lane < k && lk < ck)); // the list is sorted: a prefix
            if (pos < k) {
              const u64 uk = __shfl_up(lk, 1, 64);
              if (lane > pos) lk = uk;
              else if (lane == pos) lk = ck;
            }
          }
          if (lane < k) wLk[qi * k + lane] = lk;
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        }
      }
    }
  }
  __syncthreads();
  // the four waves' lists of a query become one: the final answer, or this slot's partial list
  for (int qi = wv; qi < nq; qi += 4) {
    const long qg = q0 + qi;
    auto load = [&](int list, int pos, int& d, long& j) {
      const u64 key = Lk[(list * ED_QT + qi) * k + pos];
      d = (int)(key >> 32);
      j = key == ED_EMPTY ? ED_NONE64 : r_beg + (long)(unsigned)key;
    };
    if (part_d) {
      const long base = ((long)blockIdx.y * Q + qg) * k;
      ed_wave_merge(4, k, load, [&](int r, int d, long j) { part_d[base + r] = d; part_j[base + r] = j; });
    } else {
      ed_wave_merge(4, k, load, [&](int r, int d, long j) { dist[qg * k + r] = d; idx[qg * k + r] = j == ED_NONE64 ? -1 : j; });
    }
  }
}

// one wave per query: the slots' partial lists, owned by the lanes in slot order, become the answer
__global__ __launch_bounds__(256) void edit_knn_merge_kernel(int Q, int k, int slots, const int* __restrict__ part_d,
                                                             const long* __restrict__ part_j, int* __restrict__ dist, long* __restrict__ idx) {
  const long qg = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (qg >= Q) return;
  ed_wave_merge(
      slots, k,
      [&](int list, int pos, int& d, long& j) {
        const long e = ((long)list * Q + qg) * k + pos;
        d = part_d[e];
        j = part_j[e];
      },
      [&](int r, int d, long j) { dist[qg * k + r] = d; idx[qg * k + r] = j == ED_NONE64 ? -1 : j; });
}

// One wave per pair, the recurrence uniform across the wave: lane v keeps the match vector of token v, a text token fetches it by a lane
// read, and the text is walked 64 columns per load up to its first `eos` -- the bit-vector code above, tested directly at the word
// boundaries.
__global__ __launch_bounds__(256) void edit_rows_kernel(int B, int V, int eos, const int64_t* __restrict__ a, long a_ld, int Ta,
                                                        const int64_t* __restrict__ b, long b_ld, int Tb, int* __restrict__ dist) {
  const int pair = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (pair >= B) return;                                             // whole waves leave: no barrier below
  u64 w0, w1;
  const int m = ed_pattern(a + (long)pair * a_ld, Ta, V, eos, w0, w1);
  const bool two = m > 64;
  const u64 bit = m > 0 ? 1ull << ((m - 1) & 63) : 0;
  const int64_t* __restrict__ text = b + (long)pair * b_ld + 1;      // the content starts behind <bos>
  const int L = Tb - 1;
  u64 Pv0 = ~0ull, Mv0 = 0, Pv1 = ~0ull, Mv1 = 0;
  int s = m, n = 0;
  for (int j0 = 0; j0 < L; j0 += 64) {                               // columns >= Tb are never loaded
    const int i = j0 + lane;
    const int64_t v = i < L ? text[i] : 0;
    const u64 ends = __ballot(i < L && v == (int64_t)eos);
    const int stop = ends ? (int)__builtin_ctzll(ends) : min(64, L - j0);
    for (int e = 0; e < stop; ++e) {
      const int64_t t = __shfl((long long)v, e, 64);
      const bool known = t >= 0 && t < (int64_t)V;                   // anything else equals nothing and is never a lane index
      const int src = known ? (int)t : 0;
      const u64 e0 = __shfl(w0, src, 64), e1 = __shfl(w1, src, 64);
      u64 Ph, Mh;
      ed_block(known ? e0 : 0, 1, Pv0, Mv0, Ph, Mh);
      if (two) {
        const int hout = ed_delta(Ph, Mh, 1ull << 63);
        ed_block(known ? e1 : 0, hout, Pv1, Mv1, Ph, Mh);
      }
      s += ed_delta(Ph, Mh, bit);
    }
    n += stop;
    if (ends) break;
  }
  if (lane == 0) dist[pair] = m > 0 ? s : n;
}

}  // namespace

extern "C" {

int mvae_edit_distance_rows(int B, int V, int eos, const int64_t* a, int64_t a_ld, int Ta, const int64_t* b, int64_t b_ld, int Tb, int32_t* dist,
                            void* stream) {
  if (!a || !b || !dist || B < 1 || Ta < 1 || Tb < 1 || a_ld < Ta || b_ld < Tb || eos < 0 || eos > 65535 || V < 1 || V > 64)
    return MVAE_ERR_INVALID;
  if (Ta - 1 > MVAE_EDIT_PATTERN_MAX) return MVAE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(edit_rows_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, B, V, eos, a, (long)a_ld, Ta, b,
                     (long)b_ld, Tb, dist);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

size_t mvae_edit_knn_workspace(int Q, int64_t N, int k) {
  if (Q < 1 || N < 1 || k < 1 || k > ED_K_MAX) return 0;
  return ed_ws_bytes(ed_plan(Q, N), Q, k);
}

int mvae_edit_knn(int Q, int T, int V, int eos, const int64_t* x, int64_t x_ld, const uint8_t* tokens, const int64_t* offsets, int64_t N, int k,
                  const int64_t* exclude, int32_t* dist, int64_t* idx, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !tokens || !offsets || !dist || !idx || Q < 1 || N < 1 || k < 1 || T < 1 || x_ld < T || eos < 0 || eos > 65535 || V < 1 || V > 64)
    return MVAE_ERR_INVALID;
  if (k > ED_K_MAX || T - 1 > MVAE_EDIT_PATTERN_MAX) return MVAE_ERR_UNSUPPORTED;
  const EdPlan p = ed_plan(Q, N);
  if (p.slot_rows >= (long)INT_MAX) return MVAE_ERR_UNSUPPORTED;       // row offsets inside a slot are 32-bit (N >= 2^39)
  int* part_d = nullptr;
  long* part_j = nullptr;
  if (p.slots > 1) {
    if (!ws || ws_bytes < ed_ws_bytes(p, Q, k)) return MVAE_ERR_WORKSPACE;
    if ((uintptr_t)ws % alignof(long)) return MVAE_ERR_INVALID;
    part_j = (long*)ws;
    part_d = (int*)(part_j + (size_t)p.slots * (size_t)Q * (size_t)k);
  }
  const size_t smem = ed_smem_bytes(V, k);
  MVAE_CHECK_HIP(lds_opt_in<edit_knn_scan_kernel>((int)ed_smem_bytes(ED_V_MAX, ED_K_MAX)));      // V = 64 with k = 32 needs a little over the default 64 KB
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(edit_knn_scan_kernel, dim3(p.qtiles, (unsigned)p.slots), dim3(256), smem, st, Q, (long)N, T, V, eos, k, x, (long)x_ld, tokens,
                     offsets, exclude, p.slot_rows, dist, (long*)idx, part_d, part_j);
  MVAE_CHECK_HIP(hipGetLastError());
  if (part_d) {
    hipLaunchKernelGGL(edit_knn_merge_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, st, Q, k, p.slots, part_d, part_j, dist, (long*)idx);
    MVAE_CHECK_HIP(hipGetLastError());
  }
  return MVAE_OK;
}

}  // extern "C"
