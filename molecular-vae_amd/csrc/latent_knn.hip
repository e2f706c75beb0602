// Exact k nearest neighbours of latent points in a latent table (gfx950): d2(i, j) = sum_d (q[i,d] - table[j,d])^2 as a direct difference on
// the VALU, the sweep of gauss_pairwise_lse_kernel (latent.hip) with "keep the k smallest" in place of the online log-sum-exp.
//
// Layout: lanes over TABLE rows, the queries broadcast.  A wave keeps 64 table rows in registers (one per lane, DZP = dz rounded up to 32,
// zero-padded) and walks a tile of up to KNN_QT queries; a query's values are the same for every lane, so they arrive by uniform (scalar)
// loads and cost no vector register and no LDS read.  That fills the chip at Q = 1 as well as at Q = 4096: the work is split over table rows
// first.  Each wave owns one sorted k-entry list per query of the tile in LDS, entry e living in lane e while a list is updated.  The common
// case per (query, row) pair is one compare against the list's last distance; a wave enters the insertion path only when one of its 64 rows
// beats it.  Nothing is shared between waves until the end of the block, so the main loop has no barrier.
//
// Order: every distance is summed in one fixed order (four accumulators over d mod 4, each ascending in d, added as (a0 + a1) + (a2 + a3));
// the lists are ordered by (d2, row) and every merge compares (d2, row) pairs, so the result does not depend on how the rows were split
// over lanes, waves, blocks or slots, and two runs are bitwise equal.
#include <limits.h>

#include "common.hpp"

constexpr int KNN_QT = 64;          // queries per block tile
constexpr int KNN_ROWS = 256;       // table rows per block step: 4 waves x 64 lanes
constexpr int KNN_BLOCKS = 512;     // workgroups the row split aims for: two per CU
constexpr int KNN_MAX_SLOTS = 256;  // the merge gives a lane at most KNN_MAX_SLOTS / 64 partial lists
constexpr int KNN_K_MAX = 32;       // documented in include/mvae.h
constexpr int KNN_DZ_MAX = 192;     // the table row lives in registers, as PW_DZ_MAX
constexpr int KNN_NONE = INT_MAX;   // row offset of an empty list entry: (+inf, KNN_NONE) sorts behind every real (d2, row)
constexpr long KNN_NONE64 = LONG_MAX;

struct KnnPlan {
  int slots;          // partial lists per query
  long slot_rows;     // table rows per slot, a multiple of KNN_ROWS
  unsigned qtiles;
};

// depends on the shape alone
static KnnPlan knn_plan(int Q, int64_t N) {
  KnnPlan p;
  p.qtiles = (unsigned)(((long)Q + KNN_QT - 1) / KNN_QT);
  const long tiles = ((long)N + KNN_ROWS - 1) / KNN_ROWS;
  long s = (KNN_BLOCKS + (long)p.qtiles - 1) / (long)p.qtiles;
  if (s > tiles) s = tiles;
  if (s > KNN_MAX_SLOTS) s = KNN_MAX_SLOTS;
  if (s < 1) s = 1;
  const long tps = (tiles + s - 1) / s;
  p.slots = (int)((tiles + tps - 1) / tps);
  p.slot_rows = tps * KNN_ROWS;
  return p;
}

// A query's values are the same in every lane: 16 of them arrive by one scalar load into SGPRs and are used as VALU operands from there.
// The load is issued early and waited for late; between knn_sload16 and knn_swait of the same value nothing may read it, which the data
// dependence through knn_swait's in/out operand says to the compiler.
typedef float f32x16 __attribute__((ext_vector_type(16)));
// The running sums pass through the issuing statement, which keeps the arithmetic that follows it in the source behind it in the code.
__device__ __forceinline__ void knn_sload16(f32x16& v, const float* p, float& a0, float& a1, float& a2, float& a3) {
  asm volatile("s_load_dwordx16 %0, %5, 0x0" : "=s"(v), "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "s"(p) : "memory");
}
__device__ __forceinline__ void knn_swait(f32x16& v) { asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(v) : : "memory"); }

__device__ __forceinline__ bool knn_less(float da, long ja, float db, long jb) { return da < db || (da == db && ja < jb); }

// One wave merges `nlists` sorted lists of k entries into the k smallest (d2, row), ascending.  Lane l owns lists l, l + 64, ... (at most
// four) and a head position in each; a round takes the smallest head of all lists (a butterfly over (d2, row), rows are distinct) and the
// owner advances.  load(list, pos, d, j) reads an entry, store(pos, d, j) receives the result ((+inf, KNN_NONE64) once the lists ran dry).
template <class Load, class Store>
__device__ __forceinline__ void knn_wave_merge(int nlists, int k, Load load, Store store) {
  const int lane = threadIdx.x & 63;
  int h[4] = {0, 0, 0, 0};
  for (int r = 0; r < k; ++r) {
    float bd = INFINITY;
    long bj = KNN_NONE64;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int list = lane + 64 * s;
      if (list < nlists && h[s] < k) {
        float d;
        long j;
        load(list, h[s], d, j);
        if (knn_less(d, j, bd, bj)) { bd = d; bj = j; }
      }
    }
    float wd = bd;
    long wj = bj;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float od = __shfl_xor(wd, o, 64);
      const long oj = __shfl_xor((long long)wj, o, 64);
      if (knn_less(od, oj, wd, wj)) { wd = od; wj = oj; }
    }
    if (wj != KNN_NONE64) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int list = lane + 64 * s;
        if (list < nlists && h[s] < k) {
          float d;
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
template <int DZP, bool FAST>
__global__ __launch_bounds__(256, 2) void latent_knn_scan_kernel(int Q, long N, int dz, int k, const float* __restrict__ q, long ldq,
                                                                 const float* __restrict__ table, long ldt,
                                                                 const long* __restrict__ exclude, long slot_rows, float* __restrict__ dist,
                                                                 long* __restrict__ idx, float* __restrict__ part_d,
                                                                 long* __restrict__ part_j) {
  extern __shared__ __attribute__((aligned(16))) unsigned char knn_smem[];
  float* Ld = reinterpret_cast<float*>(knn_smem);                 // [4 waves][KNN_QT][k] distances
  int* Lj = reinterpret_cast<int*>(Ld + 4 * KNN_QT * k);           // [4 waves][KNN_QT][k] row offsets from the slot's first row
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int q0 = blockIdx.x * KNN_QT;
  const int nq = min(KNN_QT, Q - q0);
  const long r_beg = (long)blockIdx.y * slot_rows;
  const long r_end = min(r_beg + slot_rows, N);
  const int nt = dz - (DZP - 32);                                  // columns of the last 32 that exist (non-FAST; 1..32)
  const int tail_mask = nt >= 32 ? -1 : (1 << nt) - 1;
  for (int e = tid; e < 4 * KNN_QT * k; e += 256) {
    Ld[e] = INFINITY;
    Lj[e] = KNN_NONE;
  }
  __syncthreads();
  float* wLd = Ld + wv * KNN_QT * k;
  int* wLj = Lj + wv * KNN_QT * k;

  for (long c0 = r_beg + wv * 64; c0 < r_end; c0 += KNN_ROWS) {
    const long row = c0 + lane;
    const bool live = row < r_end;
    const int off = (int)(row - r_beg);
    // rows past the end repeat the last one (their lanes never become candidates): the loads need no branch and stay in flight together
    const float* __restrict__ tp = table + (live ? row : r_end - 1) * ldt;
    float tr[DZP];
    if (FAST) {
#pragma unroll
      for (int d = 0; d < DZP; d += 4) {
        const float4 v = *reinterpret_cast<const float4*>(tp + d);
        tr[d] = v.x; tr[d + 1] = v.y; tr[d + 2] = v.z; tr[d + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int d = 0; d < DZP - 32; ++d) tr[d] = tp[d];
      // the last 32 columns: column dz - 1 stands in past dz and the value is masked to +0 there.  Limit and mask are made opaque vector
      // values here, so that no per-column condition is hoisted out of the loops into scalar registers
      int lim, msk;
      asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %3" : "=v"(lim), "=v"(msk) : "s"(dz - 1), "s"(tail_mask));
#pragma unroll
      for (int e = 0; e < 32; ++e) {
        const int d = DZP - 32 + e;
        const float v = tp[min(d, lim)];
        tr[d] = __builtin_bit_cast(float, __builtin_bit_cast(int, v) & __builtin_amdgcn_sbfe(msk, e, 1));
      }
    }
    float tq = 0.f;                                                // non-FAST: column DZP - 32 + lane of the next query, 0 past dz
    if (!FAST) tq = lane < nt ? q[(long)q0 * ldq + (DZP - 32) + lane] : 0.f;
#pragma unroll 1
    for (int qi = 0; qi < nq; ++qi) {
      const float* __restrict__ qp = q + (long)(q0 + qi) * ldq;     // the same address in every lane: scalar loads
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      // 16 columns per step.  Steps that lie below dz for certain take their query values by one 16-dword scalar load, issued one step
      // ahead.  The last 32 columns of a shape with dz < DZP (or unaligned table rows) were read one query ahead, one column per lane and
      // 0 past dz, and are handed to the scalar side lane by lane.
      float tqn = 0.f;
      if (!FAST) {
        const int qn = min(qi + 1, nq - 1);
        tqn = lane < nt ? q[(long)(q0 + qn) * ldq + (DZP - 32) + lane] : 0.f;
      }
      constexpr int NS = DZP / 16, NA = FAST ? NS : NS - 2;
      f32x16 cur, nxt;
      if (NA > 0) knn_sload16(cur, qp, a0, a1, a2, a3);
#pragma unroll
      for (int c = 0; c < NS; ++c) {
        float v[16];
        if (c < NA) {
          knn_swait(cur);
          if (c + 1 < NA) knn_sload16(nxt, qp + 16 * (c + 1), a0, a1, a2, a3);
#pragma unroll
          for (int e = 0; e < 16; ++e) v[e] = cur[e];
        } else {
#pragma unroll
          for (int e = 0; e < 16; ++e)
            v[e] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, tq), 16 * (c - NA) + e));
        }
#pragma unroll
        for (int e = 0; e < 16; e += 4) {
          const int d = 16 * c + e;
          const float t0 = v[e] - tr[d], t1 = v[e + 1] - tr[d + 1], t2 = v[e + 2] - tr[d + 2], t3 = v[e + 3] - tr[d + 3];
          a0 = fmaf(t0, t0, a0); a1 = fmaf(t1, t1, a1); a2 = fmaf(t2, t2, a2); a3 = fmaf(t3, t3, a3);
        }
        // the sums pass through an ordered no-op: this step's arithmetic stays between its own wait and the next step's, so only two
        // 16-dword query values are ever live
        asm volatile("" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));
        if (c + 1 < NA) cur = nxt;
      }
      const float dd = (a0 + a1) + (a2 + a3);
      tq = tqn;
      const long ex = exclude ? exclude[q0 + qi] : -1;
      // the list's last distance: +inf while the list is not full.  dd <= thr lets +inf and ties through to the exact (d2, row) compare
      // below; a NaN fails it and is never a candidate.  A stale (larger) threshold would only admit more candidates.
      const float thr = wLd[qi * k + (k - 1)];
      unsigned long long m = __ballot(live && row != ex && dd <= thr);
      if (m) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        float ld = lane < k ? wLd[qi * k + lane] : INFINITY;        // entry e of the list in lane e
        int lj = lane < k ? wLj[qi * k + lane] : KNN_NONE;
        while (m) {                                                  // lowest lane = lowest row first
          const int l = __ffsll(m) - 1;
          m &= m - 1;
          const float cd = __shfl(dd, l, 64);
          const int cj = __shfl(off, l, 64);
          const int pos = __popcll(__ballot(lane < k && knn_less(ld, lj, cd, cj)));   // the list is sorted: a prefix
          if (pos < k) {
            const float ud = __shfl_up(ld, 1, 64);
            const int uj = __shfl_up(lj, 1, 64);
            if (lane > pos) { ld = ud; lj = uj; }
            else if (lane == pos) { ld = cd; lj = cj; }
          }
        }
        if (lane < k) {
          wLd[qi * k + lane] = ld;
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
    auto load = [&](int list, int pos, float& d, long& j) {
      const int e = (list * KNN_QT + qi) * k + pos;
      d = Ld[e];
      const int o = Lj[e];
      j = o == KNN_NONE ? KNN_NONE64 : r_beg + o;
    };
    if (part_d) {
      const long base = ((long)blockIdx.y * Q + qg) * k;
      knn_wave_merge(4, k, load, [&](int r, float d, long j) { part_d[base + r] = d; part_j[base + r] = j; });
    } else {
      knn_wave_merge(4, k, load, [&](int r, float d, long j) { dist[qg * k + r] = d; idx[qg * k + r] = j == KNN_NONE64 ? -1 : j; });
    }
  }
}

// one wave per query: the slots' partial lists, owned by the lanes in slot order, become the answer
__global__ __launch_bounds__(256) void latent_knn_merge_kernel(int Q, int k, int slots, const float* __restrict__ part_d,
                                                               const long* __restrict__ part_j, float* __restrict__ dist,
                                                               long* __restrict__ idx) {
  const long qg = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (qg >= Q) return;
  knn_wave_merge(
      slots, k,
      [&](int list, int pos, float& d, long& j) {
        const long e = ((long)list * Q + qg) * k + pos;
        d = part_d[e];
        j = part_j[e];
      },
      [&](int r, float d, long j) { dist[qg * k + r] = d; idx[qg * k + r] = j == KNN_NONE64 ? -1 : j; });
}

template <int DZP>
static void launch_knn_scan(bool fast, dim3 grid, size_t smem, hipStream_t st, int Q, long N, int dz, int k, const float* q, long ldq,
                            const float* table, long ldt, const long* exclude, long slot_rows, float* dist, long* idx, float* part_d,
                            long* part_j) {
  if (fast)
    hipLaunchKernelGGL((latent_knn_scan_kernel<DZP, true>), grid, dim3(256), smem, st, Q, N, dz, k, q, ldq, table, ldt, exclude, slot_rows, dist,
                       idx, part_d, part_j);
  else
    hipLaunchKernelGGL((latent_knn_scan_kernel<DZP, false>), grid, dim3(256), smem, st, Q, N, dz, k, q, ldq, table, ldt, exclude, slot_rows, dist,
                       idx, part_d, part_j);
}

static size_t knn_ws_bytes(const KnnPlan& p, int Q, int k) {
  return p.slots > 1 ? (size_t)p.slots * (size_t)Q * (size_t)k * (sizeof(long) + sizeof(float)) : 0;
}

extern "C" {

size_t mvae_latent_knn_workspace(int Q, int64_t N, int dz, int k) {
  if (Q < 1 || N < 1 || dz < 1 || k < 1 || dz > KNN_DZ_MAX || k > KNN_K_MAX) return 0;
  return knn_ws_bytes(knn_plan(Q, N), Q, k);
}

int mvae_latent_knn(int Q, int64_t N, int dz, int k, const float* q, int64_t ldq, const float* table, int64_t ldt, const int64_t* exclude,
                    float* dist, int64_t* idx, void* ws, size_t ws_bytes, void* stream) {
  if (Q < 1 || N < 1 || k < 1 || dz < 1 || ldq < dz || ldt < dz || !q || !table || !dist || !idx) return MVAE_ERR_INVALID;
  if (dz > KNN_DZ_MAX || k > KNN_K_MAX) return MVAE_ERR_UNSUPPORTED;
  const KnnPlan p = knn_plan(Q, N);
  if (p.slot_rows >= (long)KNN_NONE) return MVAE_ERR_UNSUPPORTED;       // row offsets inside a slot are 32-bit (N >= 2^39)
  float* part_d = nullptr;
  long* part_j = nullptr;
  if (p.slots > 1) {
    if (!ws || ws_bytes < knn_ws_bytes(p, Q, k)) return MVAE_ERR_WORKSPACE;
    if ((uintptr_t)ws % alignof(long)) return MVAE_ERR_INVALID;
    part_j = (long*)ws;
    part_d = (float*)(part_j + (size_t)p.slots * (size_t)Q * (size_t)k);
  }
  const int dzp = (dz + 31) / 32 * 32;
  // whole 16-byte loads of the table rows and unguarded query loads need dz == DZP and aligned table rows
  const bool fast = dz == dzp && ldt % 4 == 0 && (uintptr_t)table % 16 == 0;
  const dim3 grid(p.qtiles, (unsigned)p.slots);
  const size_t smem = (size_t)4 * KNN_QT * k * (sizeof(float) + sizeof(int));
  const hipStream_t st = (hipStream_t)stream;
  const long* ex = (const long*)exclude;
  switch (dzp / 32) {
    case 1: launch_knn_scan<32>(fast, grid, smem, st, Q, N, dz, k, q, ldq, table, ldt, ex, p.slot_rows, dist, (long*)idx, part_d, part_j); break;
    case 2: launch_knn_scan<64>(fast, grid, smem, st, Q, N, dz, k, q, ldq, table, ldt, ex, p.slot_rows, dist, (long*)idx, part_d, part_j); break;
    case 3: launch_knn_scan<96>(fast, grid, smem, st, Q, N, dz, k, q, ldq, table, ldt, ex, p.slot_rows, dist, (long*)idx, part_d, part_j); break;
    case 4: launch_knn_scan<128>(fast, grid, smem, st, Q, N, dz, k, q, ldq, table, ldt, ex, p.slot_rows, dist, (long*)idx, part_d, part_j); break;
    case 5: launch_knn_scan<160>(fast, grid, smem, st, Q, N, dz, k, q, ldq, table, ldt, ex, p.slot_rows, dist, (long*)idx, part_d, part_j); break;
    default: launch_knn_scan<192>(fast, grid, smem, st, Q, N, dz, k, q, ldq, table, ldt, ex, p.slot_rows, dist, (long*)idx, part_d, part_j); break;
  }
  MVAE_CHECK_HIP(hipGetLastError());
  if (part_d) {
    hipLaunchKernelGGL(latent_knn_merge_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, st, Q, k, p.slots, part_d, part_j, dist, (long*)idx);
    MVAE_CHECK_HIP(hipGetLastError());
  }
  return MVAE_OK;
}

}  // extern "C"
