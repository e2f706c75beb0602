// Latent-code diagnostics of mosesvae.VAE (gfx950): the importance-sampling draw of the IW likelihood, a per-group log-mean-exp, and the
// pairwise diagonal-Gaussian log-sum-exp behind the mutual information I(x; z).  Every reduction runs in a fixed order and no kernel uses
// atomics, so two runs are bitwise equal.
#include "common.hpp"
#include "kernels.hpp"

// ------------------------------------------------------------------------------------------- importance-sampling draw
// One wave per row r = b*K + k: z = mu_b + exp(logvar_b / 2) * eps_r and logw[r] = 0.5 * sum_d (eps^2 + logvar - z^2), the dimensions
// taken lane-strided and then added by the wave butterfly (a fixed order).
__global__ __launch_bounds__(256) void gauss_iw_draw_kernel(int B, int K, int dz, const float* __restrict__ mu, const float* __restrict__ logvar,
                                                            long ld, const float* __restrict__ eps, uint32_t seed, uint64_t offset,
                                                            float* __restrict__ z, float* __restrict__ logw) {
  const long R = (long)B * K;
  const int lane = threadIdx.x & 63;
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < R; r += (long)gridDim.x * 4) {
    const long b = r / K;
    float a = 0.f;
    for (int d = lane; d < dz; d += 64) {
      const float m = mu[b * ld + d], lv = logvar[b * ld + d];
      const long o = r * dz + d;
      const float e = eps ? eps[o] : normal_draw(seed, offset + (uint64_t)o);
      const float zz = m + expf(lv * 0.5f) * e;
      z[o] = zz;
      a += (e * e + lv) - zz * zz;
    }
    a = wave_sum(a);
    if (lane == 0) logw[r] = 0.5f * a;
  }
}

// ------------------------------------------------------------------------------------------- per-group log-mean-exp
// One wave per group of K values v = a + b: a max / sum / NaN pass, then the sum of exp(v - max).  A NaN stays in its group; a group of
// -inf gives -inf (and one holding +inf gives +inf) instead of the NaN of inf - inf.
__global__ __launch_bounds__(256) void group_logmeanexp_kernel(int G, int K, const float* __restrict__ a, const float* __restrict__ b, float logK,
                                                               float* __restrict__ lme, float* __restrict__ mean) {
  const int lane = threadIdx.x & 63;
  for (long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6); g < G; g += (long)gridDim.x * 4) {
    const float* pa = a + g * K;
    const float* pb = b ? b + g * K : nullptr;
    float mx = -INFINITY, sm = 0.f;
    bool nan = false;
    for (int k = lane; k < K; k += 64) {
      const float v = pb ? pa[k] + pb[k] : pa[k];
      mx = fmaxf(mx, v);
      sm += v;
      nan |= v != v;
    }
    mx = wave_max(mx);
    sm = wave_sum(sm);
    const bool any_nan = __ballot(nan) != 0;
    float s = 0.f;
    if (mx > -INFINITY && mx < INFINITY)
      for (int k = lane; k < K; k += 64) s += expf((pb ? pa[k] + pb[k] : pa[k]) - mx);
    s = wave_sum(s);
    if (lane == 0) {
      lme[g] = any_nan ? NAN : (mx > -INFINITY && mx < INFINITY) ? mx + logf(s) - logK : mx;
      mean[g] = sm / (float)K;
    }
  }
}

// ------------------------------------------------------------------------------------------- pairwise Gaussian log-sum-exp
// out[i] = logsumexp_j ( c_j - 0.5 * sum_d ((z_id - mu_jd) * s_jd)^2 ),  s_jd = exp(-logvar_jd / 2),  c_j = -0.5 * sum_d logvar_jd - dz/2 log 2 pi.
// A direct difference on the VALU (sub, mul, fma per pair and dimension): every summand is >= 0, nothing cancels.  Each lane keeps its z row
// in registers (DZP = dz rounded up to 32, zero-padded) and an online (max, sum); a workgroup of 256 rows walks the columns of its slot in
// LDS tiles of PW_TJ columns (mu and s zero-padded to DZP, so the padding adds exact zeros), read as broadcasts.  When the row blocks alone
// cannot fill the chip, the columns are split over `slots` partial (max, sum) pairs in the workspace that a second launch merges in slot
// order.  The slot count depends on the shape only.
constexpr int PW_ROWS = 256;
constexpr int PW_TJ = 32;
constexpr int PW_BLOCKS = 512;      // workgroups the column split aims for: two per CU
constexpr int PW_MIN_COLS = 64;     // fewest columns a slot gets
constexpr int PW_MAX_SLOTS = 64;
constexpr int PW_DZ_MAX = 192;      // the z row lives in registers

static void pw_plan(int Nz, int Nx, int& slots, int& cols) {
  const long rb = ((long)Nz + PW_ROWS - 1) / PW_ROWS;
  long s = (PW_BLOCKS + rb - 1) / rb;
  const long smax = ((long)Nx + PW_MIN_COLS - 1) / PW_MIN_COLS;
  if (s > smax) s = smax;
  if (s > PW_MAX_SLOTS) s = PW_MAX_SLOTS;
  if (s < 1) s = 1;
  long c = ((long)Nx + s - 1) / s;
  c = (c + PW_TJ - 1) / PW_TJ * PW_TJ;
  slots = (int)(((long)Nx + c - 1) / c);
  cols = (int)c;
}

template <int DZP>
__global__ __launch_bounds__(256, 2) void gauss_pairwise_lse_kernel(int Nz, int Nx, int dz, const float* __restrict__ z, long ldz,
                                                                    const float* __restrict__ mu, const float* __restrict__ logvar, long ldp,
                                                                    float cst, int cols, float* __restrict__ out, float2* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float smu[PW_TJ][DZP];
  __shared__ __attribute__((aligned(16))) float ssc[PW_TJ][DZP];
  __shared__ float sc[PW_TJ];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long i = (long)blockIdx.x * PW_ROWS + tid;
  const int j_beg = blockIdx.y * cols;
  const int j_end = min(j_beg + cols, Nx);
  float zr[DZP];
#pragma unroll
  for (int d = 0; d < DZP; ++d) zr[d] = (i < Nz && d < dz) ? z[i * ldz + d] : 0.f;
  float m = -INFINITY, s = 0.f;
  for (int j0 = j_beg; j0 < j_end; j0 += PW_TJ) {
    const int nj = min(PW_TJ, j_end - j0);
    __syncthreads();                                             // the previous tile is consumed
#pragma unroll 1
    for (int e = tid; e < PW_TJ * DZP; e += PW_ROWS) {
      const int jj = e / DZP, d = e - jj * DZP;
      float mv = 0.f, sv = 0.f;
      if (jj < nj && d < dz) {
        const long o = (long)(j0 + jj) * ldp + d;
        mv = mu[o];
        sv = expf(-0.5f * logvar[o]);
      }
      smu[jj][d] = mv;
      ssc[jj][d] = sv;
    }
#pragma unroll 1
    for (int jj = wv; jj < nj; jj += PW_ROWS / 64) {
      float a = 0.f;
      for (int d = lane; d < dz; d += 64) a += logvar[(long)(j0 + jj) * ldp + d];
      a = wave_sum(a);
      if (lane == 0) sc[jj] = fmaf(-0.5f, a, cst);
    }
    __syncthreads();
#pragma unroll 1
    for (int jj = 0; jj < nj; ++jj) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
      for (int d = 0; d < DZP; d += 4) {
        const float4 mv = *reinterpret_cast<const float4*>(&smu[jj][d]);
        const float4 sv = *reinterpret_cast<const float4*>(&ssc[jj][d]);
        const float t0 = (zr[d] - mv.x) * sv.x, t1 = (zr[d + 1] - mv.y) * sv.y;
        const float t2 = (zr[d + 2] - mv.z) * sv.z, t3 = (zr[d + 3] - mv.w) * sv.w;
        a0 = fmaf(t0, t0, a0); a1 = fmaf(t1, t1, a1); a2 = fmaf(t2, t2, a2); a3 = fmaf(t3, t3, a3);
        if (d % 16 == 12) __builtin_amdgcn_sched_barrier(0);    // keeps the broadcast reads near their use: the z row needs the registers
      }
      const float v = fmaf(-0.5f, (a0 + a1) + (a2 + a3), sc[jj]);
      const float mn = fmaxf(m, v);
      if (mn > -INFINITY) {
        s = s * expf(m - mn) + expf(v - mn);
        m = mn;
      }
    }
  }
  if (i >= Nz) return;
  if (part) part[(long)blockIdx.y * Nz + i] = make_float2(m, s);
  else out[i] = m > -INFINITY ? m + logf(s) : m;
}

__global__ __launch_bounds__(256) void gauss_lse_merge_kernel(int Nz, int slots, const float2* __restrict__ part, float* __restrict__ out) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < Nz; i += (long)gridDim.x * 256) {
    float M = -INFINITY;
    for (int k = 0; k < slots; ++k) M = fmaxf(M, part[(long)k * Nz + i].x);
    if (!(M > -INFINITY)) { out[i] = M; continue; }
    float S = 0.f;
    for (int k = 0; k < slots; ++k) {
      const float2 p = part[(long)k * Nz + i];
      if (p.x > -INFINITY) S += p.y * expf(p.x - M);
    }
    out[i] = M + logf(S);
  }
}

template <int DZP>
static void launch_pairwise(dim3 grid, hipStream_t st, int Nz, int Nx, int dz, const float* z, long ldz, const float* mu, const float* logvar,
                            long ldp, float cst, int cols, float* out, float2* part) {
  hipLaunchKernelGGL(gauss_pairwise_lse_kernel<DZP>, grid, dim3(PW_ROWS), 0, st, Nz, Nx, dz, z, ldz, mu, logvar, ldp, cst, cols, out, part);
}

static inline int rows_grid(long rows, int per_block) {
  long b = (rows + per_block - 1) / per_block;
  return (int)(b < 1 ? 1 : b > 4096 ? 4096 : b);
}

// ------------------------------------------------------------------------------------------- extern "C" surface
extern "C" {

int mvae_gauss_iw_draw(int B, int K, int dz, const float* mu, const float* logvar, int64_t ld, const float* eps, uint32_t seed, uint64_t offset,
                       float* z_out, float* logw_out, void* stream) {
  if (B < 1 || K < 1 || dz < 1 || ld < dz || !mu || !logvar || !z_out || !logw_out) return MVAE_ERR_INVALID;
  hipLaunchKernelGGL(gauss_iw_draw_kernel, dim3(rows_grid((long)B * K, 4)), dim3(256), 0, (hipStream_t)stream, B, K, dz, mu, logvar, (long)ld, eps,
                     seed, offset, z_out, logw_out);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

int mvae_group_logmeanexp(int G, int K, const float* a, const float* b, float* lme_out, float* mean_out, void* stream) {
  if (G < 1 || K < 1 || !a || !lme_out || !mean_out) return MVAE_ERR_INVALID;
  hipLaunchKernelGGL(group_logmeanexp_kernel, dim3(rows_grid(G, 4)), dim3(256), 0, (hipStream_t)stream, G, K, a, b, (float)log((double)K),
                     lme_out, mean_out);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

size_t mvae_gauss_pairwise_lse_workspace(int Nz, int Nx, int dz) {
  if (Nz < 1 || Nx < 1 || dz < 1) return 0;
  int slots, cols;
  pw_plan(Nz, Nx, slots, cols);
  return slots > 1 ? (size_t)slots * (size_t)Nz * sizeof(float2) : 0;
}

int mvae_gauss_pairwise_lse(int Nz, int Nx, int dz, const float* z, int64_t ldz, const float* mu, const float* logvar, int64_t ldp, float* out,
                            void* ws, size_t ws_bytes, void* stream) {
  if (Nz < 1 || Nx < 1 || dz < 1 || ldz < dz || ldp < dz || !z || !mu || !logvar || !out) return MVAE_ERR_INVALID;
  if (dz > PW_DZ_MAX) return MVAE_ERR_UNSUPPORTED;
  int slots, cols;
  pw_plan(Nz, Nx, slots, cols);
  float2* part = nullptr;
  if (slots > 1) {
    if (!ws || ws_bytes < (size_t)slots * (size_t)Nz * sizeof(float2)) return MVAE_ERR_WORKSPACE;
    if ((uintptr_t)ws % alignof(float2)) return MVAE_ERR_INVALID;
    part = (float2*)ws;
  }
  const float cst = (float)(-0.5 * dz * 1.8378770664093454835606594728112);     // -dz/2 log(2 pi)
  const dim3 grid((unsigned)(((long)Nz + PW_ROWS - 1) / PW_ROWS), (unsigned)slots);
  const hipStream_t st = (hipStream_t)stream;
  switch ((dz + 31) / 32) {
    case 1: launch_pairwise<32>(grid, st, Nz, Nx, dz, z, ldz, mu, logvar, ldp, cst, cols, out, part); break;
    case 2: launch_pairwise<64>(grid, st, Nz, Nx, dz, z, ldz, mu, logvar, ldp, cst, cols, out, part); break;
    case 3: launch_pairwise<96>(grid, st, Nz, Nx, dz, z, ldz, mu, logvar, ldp, cst, cols, out, part); break;
    case 4: launch_pairwise<128>(grid, st, Nz, Nx, dz, z, ldz, mu, logvar, ldp, cst, cols, out, part); break;
    case 5: launch_pairwise<160>(grid, st, Nz, Nx, dz, z, ldz, mu, logvar, ldp, cst, cols, out, part); break;
    default: launch_pairwise<192>(grid, st, Nz, Nx, dz, z, ldz, mu, logvar, ldp, cst, cols, out, part); break;
  }
  MVAE_CHECK_HIP(hipGetLastError());
  if (part) {
    hipLaunchKernelGGL(gauss_lse_merge_kernel, dim3(rows_grid(Nz, 256)), dim3(256), 0, st, Nz, slots, part, out);
    MVAE_CHECK_HIP(hipGetLastError());
  }
  return MVAE_OK;
}

}  // extern "C"
