// Valence check and molecular formula of SMILES token rows (gfx950): mvae_smiles_graph_rows over padded int64 rows, mvae_smiles_graph_corpus
// over the CSR corpus, mvae_smiles_graph_host on host pointers.  include/mvae.h ("SMILES graph") states the rules; smiles_graph.hpp is the
// walk, written once; this file is where the per-atom state lives and how rows map to threads.
//
// One thread per row, 64-thread blocks, as in smiles_syntax_check_kernel: a row is a sequential parse of a few dozen tokens and the rows
// are independent.  The per-atom state -- one 32-bit word per atom: predecessor, used valence, element / aromatic / bracket / charge -- is
// indexed by a run-time atom number, so it lives in LDS and not in a private array (which would go to scratch): 128 atoms x 64 lanes x
// 4 bytes = 32 KiB per block, atom-major ([atom][lane]), so the 64 lanes of a wave that touch the same atom number touch 64 consecutive
// words -- one word per bank pair, no conflict -- and lanes that touch different atoms never share a word.  Everything else the walk keeps
// is a handful of 64-bit masks and packed words in registers.
#include <limits.h>

#include "common.hpp"
#include "smiles_graph.hpp"

namespace {

struct LdsAtoms {
  uint32_t* base;      // &lds[lane]
  __device__ __forceinline__ uint32_t get(int i) const { return base[(i & (smg::ATOM_SLOTS - 1)) * 64]; }
  __device__ __forceinline__ void set(int i, uint32_t w) { base[(i & (smg::ATOM_SLOTS - 1)) * 64] = w; }
};

struct HostAtoms {
  uint32_t w[smg::ATOM_SLOTS];
  uint32_t get(int i) const { return w[i & (smg::ATOM_SLOTS - 1)]; }
  void set(int i, uint32_t v) { w[i & (smg::ATOM_SLOTS - 1)] = v; }
};

struct PaddedSrc {
  const int64_t* row;
  __host__ __device__ __forceinline__ long tok(int t) const { return (long)row[t]; }
};

struct CsrSrc {
  const uint8_t* row;
  __device__ __forceinline__ long tok(int t) const { return (long)row[t]; }
};

__global__ __launch_bounds__(64) void smiles_graph_rows_kernel(int B, int T, int V, const int64_t* __restrict__ x, long x_ld,
                                                               const int32_t* __restrict__ tok_info, const int32_t* __restrict__ chem_info, int eos_id,
                                                               int32_t* __restrict__ status, int32_t* __restrict__ bad_pos,
                                                               int32_t* __restrict__ desc, int32_t* __restrict__ formula) {
  __shared__ uint32_t lds[smg::ATOM_SLOTS * 64];
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  LdsAtoms at{lds + threadIdx.x};
  smg::Row r;
  smg::walk(at, PaddedSrc{x + (long)b * x_ld}, 1, T, false, V, tok_info, chem_info, eos_id, &r);
  smg::store(r, b, status, bad_pos, desc, formula);
}

__global__ __launch_bounds__(64) void smiles_graph_corpus_kernel(const uint8_t* __restrict__ tokens, const int64_t* __restrict__ offsets, long N, int V,
                                                                 const int32_t* __restrict__ tok_info, const int32_t* __restrict__ chem_info,
                                                                 int32_t* __restrict__ status, int32_t* __restrict__ bad_pos,
                                                                 int32_t* __restrict__ desc, int32_t* __restrict__ formula) {
  __shared__ uint32_t lds[smg::ATOM_SLOTS * 64];
  const long b = (long)blockIdx.x * 64 + threadIdx.x;
  if (b >= N) return;
  const long lo = offsets[b], hi = offsets[b + 1];
  const long len = hi > lo ? hi - lo : 0;
  LdsAtoms at{lds + threadIdx.x};
  smg::Row r;
  smg::walk(at, CsrSrc{tokens + lo}, 0, (int)(len < INT_MAX - 1 ? len : INT_MAX - 1), true, V, tok_info, chem_info, -1, &r);
  smg::store(r, b, status, bad_pos, desc, formula);
}

bool graph_rows_args_ok(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, int eos_id,
                        const int32_t* status) {
  return x && tok_info && chem_info && status && B >= 1 && T >= 1 && V >= 1 && x_ld >= T && eos_id >= 0 && eos_id < V;
}

}  // namespace

extern "C" {

int mvae_smiles_graph_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, int eos_id,
                           int32_t* status, int32_t* bad_pos, int32_t* desc, int32_t* formula, void* stream) {
  if (V > 64) return MVAE_ERR_UNSUPPORTED;
  if (!graph_rows_args_ok(B, T, V, x, x_ld, tok_info, chem_info, eos_id, status)) return MVAE_ERR_INVALID;
  hipLaunchKernelGGL(smiles_graph_rows_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, B, T, V, x, (long)x_ld, tok_info, chem_info,
                     eos_id, status, bad_pos, desc, formula);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

int mvae_smiles_graph_corpus(const uint8_t* tokens, const int64_t* offsets, int64_t N, int V, const int32_t* tok_info, const int32_t* chem_info,
                             int32_t* status, int32_t* bad_pos, int32_t* desc, int32_t* formula, void* stream) {
  if (V > 64) return MVAE_ERR_UNSUPPORTED;
  if (!tokens || !offsets || !tok_info || !chem_info || !status || N < 1 || V < 1) return MVAE_ERR_INVALID;
  if ((N + 63) / 64 > (int64_t)INT_MAX) return MVAE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(smiles_graph_corpus_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, tokens, offsets, (long)N, V,
                     tok_info, chem_info, status, bad_pos, desc, formula);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

int mvae_smiles_graph_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, int eos_id,
                           int32_t* status, int32_t* bad_pos, int32_t* desc, int32_t* formula) {
  if (V > 64) return MVAE_ERR_UNSUPPORTED;
  if (!graph_rows_args_ok(B, T, V, x, x_ld, tok_info, chem_info, eos_id, status)) return MVAE_ERR_INVALID;
  HostAtoms at;
  for (long b = 0; b < B; ++b) {
    smg::Row r;
    smg::walk(at, PaddedSrc{x + b * x_ld}, 1, T, false, V, tok_info, chem_info, eos_id, &r);
    smg::store(r, b, status, bad_pos, desc, formula);
  }
  return MVAE_OK;
}

}  // extern "C"
