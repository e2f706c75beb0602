// The exact corpus index behind MosesDeviceDataset.lookup and moses_generate(novel_against=...): an open-addressing hash table over the rows
// of the CSR corpus (uint8 tokens, int64 offsets -- the layout mvae_moses_collate reads), built by one launch and probed by one launch per
// batch of sampled rows.  include/mvae.h states the contract; this file states how it is kept.
//
// A slot is one 64-bit word: all ones = empty, otherwise (tag << 40) | row with a 24-bit tag from the row's hash and the 40-bit id of the
// lowest corpus row with that content seen so far.  The tag sits above the row id, so for two rows of equal content (equal hash, equal tag)
// the unsigned order of the words is the order of the row ids and "keep the lower row" is one atomic min; and most occupied slots of another
// content are passed on the tag alone, without reading the occupant's bytes.  A hit is always confirmed on the bytes.
//
// The hash is position-wise: h = H0 ^ XOR_i mix(i, token_i), two 32-bit words.  XOR does not care about the order of its terms, so one
// thread can fold a corpus row byte by byte (build) and a wave can fold a sampled row 64 columns at a time and combine the lanes (probe) and
// both get the same value; a uint8 corpus token and an int64 sample token with the same id give the same term.
//
// Work mapping.  build: one thread per corpus row -- 1.6 M rows of ~35 bytes are plenty of threads, consecutive rows are contiguous in the
//   CSR so the 64 rows of a wave are one ~2 KB span that its byte loads share line by line, and the table traffic (one random 8-byte atomic
//   per row and chain step) is the same in every mapping.  A wave per row would leave half the lanes idle on a 35-byte row.
// probe: one wave per sampled row -- a batch has a few thousand rows of T int64 columns (800 B each at T = 100), so a thread per row would
//   be 64 waves of strided 8-byte loads with a serial search for <eos>; a wave reads 512 contiguous bytes per load, finds the <eos> with
//   one ballot and compares a candidate row 64 tokens at a time.  The walk through the table is wave-uniform.
//
// No thread ever waits for another.  An insertion walks forward from its home slot: a relaxed agent-scope load is only a hint -- an empty
// slot is claimed, and thereby confirmed empty, by the compare-and-swap alone; what the CAS returns when it fails is the occupant, handled
// like any other: another tag or other bytes -> next slot, equal bytes -> atomic min and done.  The content that owns a slot never changes
// (only rows of that content min into it), slots never empty again, and all rows of one content walk the same sequence, so whichever of
// them claims the first slot that was empty for it is found by all the others: one slot per distinct content, and the claims counted are
// the distinct rows whatever the order.  Both walks are bounded by n_slots steps, so a launch ends whatever the table holds.
#include "common.hpp"
#include "kernels.hpp"

namespace {

typedef unsigned long long u64;
constexpr u64 CI_EMPTY = ~0ull;
constexpr int CI_ROW_BITS = 40;
constexpr u64 CI_ROW_MASK = (1ull << CI_ROW_BITS) - 1;

// one (position, token) term of the row hash: token in [0, 255]; positions from 2^24 on wrap, alike on both sides
__device__ __forceinline__ void ci_term(uint32_t pos, uint32_t tok, uint32_t& lo, uint32_t& hi) {
  const uint32_t key = (pos << 8) | tok;
  lo ^= drop_hash_u32(0x243F6A88u, key);
  hi ^= drop_hash_u32(0x85A308D3u, key);
}
constexpr uint32_t CI_H0_LO = 0x13198A2Eu, CI_H0_HI = 0x03707344u;      // the empty row's hash
__device__ __forceinline__ u64 ci_home(uint32_t lo, uint32_t hi, u64 mask) { return (((u64)(hi & 0xFFu) << 32) | lo) & mask; }
__device__ __forceinline__ u64 ci_tag(uint32_t hi) { return (u64)(hi >> 8); }

__device__ __forceinline__ u64 slot_load(u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(256) void corpus_index_build_kernel(const uint8_t* __restrict__ tokens, const int64_t* __restrict__ offsets, long N,
                                                                 u64* slots, u64 n_slots, u64* n_distinct) {
  const u64 mask = n_slots - 1;
  for (long base = (long)blockIdx.x * 256; base < N; base += (long)gridDim.x * 256) {      // wave-uniform trip count: the ballot below
    const long r = base + threadIdx.x;
    bool claimed = false;
    if (r < N) {
      const long o0 = offsets[r], len = offsets[r + 1] - o0;
      uint32_t lo = CI_H0_LO, hi = CI_H0_HI;
      for (long i = 0; i < len; ++i) ci_term((uint32_t)i, tokens[o0 + i], lo, hi);
      const u64 val = (ci_tag(hi) << CI_ROW_BITS) | (u64)r;
      u64 pos = ci_home(lo, hi, mask);
      for (u64 step = 0; step < n_slots; ++step, pos = (pos + 1) & mask) {
        u64 cur = slot_load(slots + pos);
        if (cur == CI_EMPTY) {
          u64 expected = CI_EMPTY;
          if (__hip_atomic_compare_exchange_strong(slots + pos, &expected, val, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
            claimed = true;
            break;
          }
          cur = expected;                                        // somebody else's row got here first: an occupant like any other
        }
        if ((cur >> CI_ROW_BITS) != (val >> CI_ROW_BITS)) continue;
        const long occ = (long)(cur & CI_ROW_MASK);              // a row id some thread of this launch wrote: inside [0, N)
        if (occ >= N) continue;                                  // (cannot happen behind the memset; no access outside the corpus if it did)
        const long p0 = offsets[occ];
        if (offsets[occ + 1] - p0 != len) continue;
        bool same = true;
        for (long i = 0; i < len && same; ++i) same = tokens[p0 + i] == tokens[o0 + i];
        if (!same) continue;
        __hip_atomic_fetch_min(slots + pos, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
    }
    if (n_distinct) {                                            // one add per wave, not per row
      const u64 won = __ballot(claimed);
      if ((threadIdx.x & 63) == 0 && won) atomicAdd(n_distinct, (u64)__popcll(won));
    }
  }
}

__global__ __launch_bounds__(256) void corpus_index_probe_kernel(const uint8_t* __restrict__ tokens, const int64_t* __restrict__ offsets, long N,
                                                                 const u64* __restrict__ slots, u64 n_slots, int B, int T,
                                                                 const int64_t* __restrict__ x, long x_ld, int eos, int64_t* match) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;                                            // whole waves leave: no barrier below
  const int64_t* row = x + (long)b * x_ld + 1;                   // the content starts behind <bos>
  const int L = T - 1;
  uint32_t lo = 0, hi = 0;
  int len = L;
  bool bad = false;
  for (int j0 = 0; j0 < L; j0 += 64) {                           // columns >= T are never loaded
    const int i = j0 + lane;
    const int64_t v = i < L ? row[i] : 0;
    const u64 ends = __ballot(i < L && v == (int64_t)eos);
    const int stop = ends ? j0 + (int)__builtin_ctzll(ends) : L;    // what this chunk holds at or behind the first <eos> is dropped here
    if (i < stop) {
      if (v < 0 || v > 255) bad = true;                          // can equal no corpus token; never hashed, never an index
      else ci_term((uint32_t)i, (uint32_t)v, lo, hi);
    }
    if (ends) { len = stop; break; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { lo ^= __shfl_xor(lo, o, 64); hi ^= __shfl_xor(hi, o, 64); }
  lo ^= CI_H0_LO; hi ^= CI_H0_HI;
  long found = -1;
  if (!__any(bad)) {
    const u64 mask = n_slots - 1, tag = ci_tag(hi);
    u64 pos = ci_home(lo, hi, mask);
    for (u64 step = 0; step < n_slots; ++step, pos = (pos + 1) & mask) {
      const u64 cur = slots[pos];                                // one address for the wave
      if (cur == CI_EMPTY) break;
      if ((cur >> CI_ROW_BITS) != tag) continue;
      const long occ = (long)(cur & CI_ROW_MASK);
      if (occ >= N) continue;                                    // not a table of this corpus: still no access outside it
      const long p0 = offsets[occ];
      if (offsets[occ + 1] - p0 != (long)len) continue;
      bool same = true;
      for (int j0 = 0; j0 < len && same; j0 += 64) {
        const int i = j0 + lane;
        same = !__any(i < len && row[i] != (int64_t)tokens[p0 + i]);
      }
      if (same) { found = occ; break; }
    }
  }
  if (lane == 0) match[b] = found;
}

bool ci_bad_table(const void* tokens, const void* offsets, int64_t N, const void* slots, int64_t n_slots) {
  return !tokens || !offsets || !slots || N < 1 || N > (int64_t)CI_ROW_MASK || n_slots <= N || (n_slots & (n_slots - 1)) != 0;
}

}  // namespace

int launch_corpus_index_build(const uint8_t* tokens, const int64_t* offsets, int64_t N, int64_t* slots, int64_t n_slots, int64_t* n_distinct,
                              hipStream_t st) {
  if (ci_bad_table(tokens, offsets, N, slots, n_slots)) return MVAE_ERR_INVALID;
  MVAE_CHECK_HIP(hipMemsetAsync(slots, 0xFF, (size_t)n_slots * sizeof(int64_t), st));       // every slot empty
  if (n_distinct) MVAE_CHECK_HIP(hipMemsetAsync(n_distinct, 0, sizeof(int64_t), st));
  const int64_t blocks = (N + 255) / 256;
  hipLaunchKernelGGL(corpus_index_build_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, tokens, offsets, (long)N,
                     (u64*)slots, (u64)n_slots, (u64*)n_distinct);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

int launch_corpus_index_probe(const uint8_t* tokens, const int64_t* offsets, int64_t N, const int64_t* slots, int64_t n_slots, int B, int T,
                              const int64_t* x, int64_t x_ld, int eos, int64_t* match, hipStream_t st) {
  if (ci_bad_table(tokens, offsets, N, slots, n_slots)) return MVAE_ERR_INVALID;
  if (!x || !match || B < 1 || T < 1 || x_ld < T || eos < 0 || eos > 65535) return MVAE_ERR_INVALID;
  hipLaunchKernelGGL(corpus_index_probe_kernel, dim3((B + 3) / 4), dim3(256), 0, st, tokens, offsets, (long)N, (const u64*)slots, (u64)n_slots, B,
                     T, x, (long)x_ld, eos, match);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}
