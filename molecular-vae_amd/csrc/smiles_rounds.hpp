// What the consumers of the SMILES graph walk share.  For those that work on the finished graph (fingerprint.hip, scaffold.hip, kekule.hip,
// smiles_rewrite.hip, smiles_canon.hip): the mix function, the recorder that keeps bond orders and ring-closure pairs, the loop over all bonds, the ring bonds.
// For all of them: lane-minor LDS storage for everything indexed by a run-time atom number (and its host twin), the two token sources, how
// a CSR row is read, and the row driver -- rows_kernel<C> / corpus_kernel<C> and the host side rows<C> / corpus<C> / host<C> -- which is
// the one place that maps a row to a thread and refuses arguments before a launch (smiles_graph.hip, fingerprint.hip, scaffold.hip,
// kekule.hip, fragment.hip).  smiles_rewrite.hip and smiles_canon.hip copy out block-wide after their rows: theirs is the writer driver of
// smiles_writer.hpp, built the same way on the same storage types.  Definitions: include/mvae.h, "Circular fingerprint".
#pragma once
#include <limits.h>

#include "common.hpp"
#include "smiles_graph.hpp"

namespace fpr {

constexpr int CLOSURES = 64;           // slots of the closure list

SMI_HD uint32_t mix(uint32_t h) {
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}

// the recorder the walk runs with (smg::NoRec states the three calls)
template <class Clos>
struct Rec {
  Clos& cl;
  int nclos = 0, n = 0;
  smg::Mask ring{0, 0};
  SMI_HD explicit Rec(Clos& c) : cl(c) {}
  SMI_HD uint32_t atom_bits(int order) const { return (uint32_t)order << 24; }
  SMI_HD void closure(int i, int j) {
    if (nclos < CLOSURES) cl.set(nclos++, (uint16_t)(i | j << 8));
  }
  SMI_HD void done(int atoms, const smg::Mask& members) { n = atoms; ring = members; }
};

// f(a, b, bt) for every bond: atom k's bond to its tree predecessor, then the closure pairs
template <class Atoms, class Clos, class F>
SMI_HD void each_bond(Atoms& at, Clos& cl, int n, int nclos, F f) {
  for (int k = 1; k < n; ++k) {
    const uint32_t w = at.get(k);
    const int p = smg::a_pred(w);
    if (p == smg::NONE) continue;
    const uint32_t order = w >> 24;
    f(k, p, order == 1 && smg::a_arom(w) && smg::a_arom(at.get(p)) ? 4u : order);
  }
  for (int c = 0; c < nclos; ++c) {
    const int v = cl.get(c), i = v & 0xFF, j = v >> 8;
    f(i, j, smg::a_arom(at.get(i)) && smg::a_arom(at.get(j)) ? 4u : 1u);
  }
}

SMI_HD smg::Mask m_or(const smg::Mask& a, const smg::Mask& b) { return smg::Mask{a.lo | b.lo, a.hi | b.hi}; }
SMI_HD smg::Mask m_first(int n) {      // atoms 0 .. n - 1, n <= 127
  return smg::Mask{n >= 64 ? ~0ull : (1ull << n) - 1ull, n > 64 ? (1ull << (n - 64)) - 1ull : 0ull};
}

// bit k: the tree bond k - pred(k) lies on a cycle, that is, some closure's tree path steps over it
template <class Atoms, class Clos>
SMI_HD smg::Mask ring_bonds(Atoms& at, Clos& cl, int nclos) {
  smg::Mask rb{0, 0};
  for (int c = 0; c < nclos; ++c) {
    const int v = cl.get(c);
    int a = v & 0xFF, b = v >> 8;
    for (int g = 0; g < 2 * smg::ATOM_SLOTS && a != b; ++g) {
      if (a > b) { smg::m_set(rb, a); a = smg::a_pred(at.get(a)); }
      else { smg::m_set(rb, b); b = smg::a_pred(at.get(b)); }
    }
  }
  return rb;
}

// [slot][lane]: the 64 lanes of a wave touch 64 consecutive elements, lanes never share one
template <class T, int SLOTS>
struct LdsArr {
  T* base;             // &lds[lane]
  __device__ __forceinline__ T get(int i) const { return base[(i & (SLOTS - 1)) * 64]; }
  __device__ __forceinline__ void set(int i, T v) { base[(i & (SLOTS - 1)) * 64] = v; }
};

template <class T, int SLOTS>
struct HostArr {
  T w[SLOTS];
  T get(int i) const { return w[i & (SLOTS - 1)]; }
  void set(int i, T v) { w[i & (SLOTS - 1)] = v; }
};

// the block's storage behind an LdsArr
template <class T, int SLOTS>
struct LdsMem {
  T v[SLOTS * 64];
  __device__ __forceinline__ LdsArr<T, SLOTS> lane() { return {v + threadIdx.x}; }
};

struct PaddedSrc {
  const int64_t* row;
  __host__ __device__ __forceinline__ long tok(int t) const { return (long)row[t]; }
};

struct CsrSrc {
  const uint8_t* row;
  __device__ __forceinline__ long tok(int t) const { return (long)row[t]; }
};

// The tokens of CSR row b, whose first one is tokens[*lo]; a row with offsets[b + 1] < offsets[b] reads as empty.  csr_end: that count as
// the walk's `end`.
__device__ __forceinline__ long csr_len(const int64_t* __restrict__ offsets, long b, long* lo) {
  *lo = offsets[b];
  const long hi = offsets[b + 1];
  return hi > *lo ? hi - *lo : 0;
}
__device__ __forceinline__ int csr_end(long len) { return (int)(len < INT_MAX - 1 ? len : INT_MAX - 1); }

// ------------------------------------------------------------------------------------------------------------------ the row driver
// One thread per row, 64-thread blocks, nothing after the row.  A consumer C states what differs:
//   C::Lds, C::Host   its arrays, listed once as Store<Arr> and instantiated with LdsMem and with HostArr
//   C::lane(lds)      Store<LdsArr>: the calling lane's accessors
//   C::Out            the output pointers, in the order of the entry's arguments; ok(): the required ones are there
//   C::row(store, src, first, end, end_is_eos, V, tok_info, chem_info, eos_id, b, out)      the walk and what follows, all outputs of row b
// A padded row starts behind <bos> and ends at eos_id; a CSR row has no specials and its end acts as <eos>.  The kernels take the output
// pointers one by one (P...), each __restrict__, and make the Out themselves: as members of a by-value struct they would lose the qualifier.
template <class C, class... P>
__global__ __launch_bounds__(64) void rows_kernel(int B, int T, int V, const int64_t* __restrict__ x, long x_ld,
                                                  const int32_t* __restrict__ tok_info, const int32_t* __restrict__ chem_info, int eos_id,
                                                  P* __restrict__... out) {
  __shared__ typename C::Lds lds;
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  auto store = C::lane(lds);
  C::row(store, PaddedSrc{x + (long)b * x_ld}, 1, T, false, V, tok_info, chem_info, eos_id, (long)b, typename C::Out{out...});
}

template <class C, class... P>
__global__ __launch_bounds__(64) void corpus_kernel(const uint8_t* __restrict__ tokens, const int64_t* __restrict__ offsets, long N, int V,
                                                    const int32_t* __restrict__ tok_info, const int32_t* __restrict__ chem_info,
                                                    P* __restrict__... out) {
  __shared__ typename C::Lds lds;
  const long b = (long)blockIdx.x * 64 + threadIdx.x;
  if (b >= N) return;
  long lo;
  const long len = csr_len(offsets, b, &lo);
  auto store = C::lane(lds);
  C::row(store, CsrSrc{tokens + lo}, 0, csr_end(len), true, V, tok_info, chem_info, -1, b, typename C::Out{out...});
}

inline bool tables_ok(int V, const int32_t* tok_info, const int32_t* chem_info) { return tok_info && chem_info && V >= 1; }

inline bool padded_rows_ok(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, int eos_id) {
  return x && tables_ok(V, tok_info, chem_info) && B >= 1 && T >= 1 && x_ld >= T && eos_id >= 0 && eos_id < V;
}

// V > 64 is refused as unsupported before anything is called invalid
template <class C, class... P>
int rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, int eos_id, void* stream,
         P*... out) {
  if (V > 64) return MVAE_ERR_UNSUPPORTED;
  if (!padded_rows_ok(B, T, V, x, x_ld, tok_info, chem_info, eos_id) || !typename C::Out{out...}.ok()) return MVAE_ERR_INVALID;
  hipLaunchKernelGGL((rows_kernel<C, P...>), dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, B, T, V, x, (long)x_ld, tok_info, chem_info,
                     eos_id, out...);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

template <class C, class... P>
int corpus(const uint8_t* tokens, const int64_t* offsets, int64_t N, int V, const int32_t* tok_info, const int32_t* chem_info, void* stream,
           P*... out) {
  if (V > 64) return MVAE_ERR_UNSUPPORTED;
  if (!tokens || !offsets || !tables_ok(V, tok_info, chem_info) || !typename C::Out{out...}.ok() || N < 1) return MVAE_ERR_INVALID;
  if ((N + 63) / 64 > (int64_t)INT_MAX) return MVAE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL((corpus_kernel<C, P...>), dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, tokens, offsets, (long)N, V,
                     tok_info, chem_info, out...);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

template <class C, class... P>
int host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, int eos_id, P*... outs) {
  const typename C::Out out{outs...};
  if (V > 64) return MVAE_ERR_UNSUPPORTED;
  if (!padded_rows_ok(B, T, V, x, x_ld, tok_info, chem_info, eos_id) || !out.ok()) return MVAE_ERR_INVALID;
  typename C::Host store;
  for (long b = 0; b < B; ++b) C::row(store, PaddedSrc{x + b * x_ld}, 1, T, false, V, tok_info, chem_info, eos_id, b, out);
  return MVAE_OK;
}

}  // namespace fpr
