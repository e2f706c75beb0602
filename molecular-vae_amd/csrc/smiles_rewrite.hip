// Randomised respelling of SMILES token rows (gfx950): mvae_smiles_rewrite_rows / _corpus / _host.  include/mvae.h ("SMILES rewrite")
// states the definition: the walk's graph, a priority per atom from a counter hash, a depth-first search from the atom of least priority
// with multiple bonds first, and the emission of the search tree in pre-order in the language the syntax automaton accepts.
//
// A fifth consumer of the walk of smiles_graph.hpp, with the fingerprint's recorder (smiles_rounds.hpp), and the first that writes a
// string.  The graph, the search and the emission are smiles_writer.hpp's, shared with smiles_canon.hip; this file states the order of
// the atoms -- (prio, atom number) -- and the kernels.  One thread per row, 64-thread blocks; everything indexed by a run-time atom
// number lives in LDS, lane-minor, never in a private array:
//   words                128 slots x 64 lanes x 4 B = 32 KiB   the walk's atom words; bits 8-15 and 26-31 are rewritten once the graph is read
//   closure pairs         64 x 64 x 2 B             =  8 KiB   the walk's list; once the adjacency is built, the SAME storage holds the
//                                                              output row (128 bytes per lane)
//   half-edges           256 x 64 x 1 B             = 16 KiB   the adjacency in CSR form: neighbour | multiple-bond bit << 7, <= 252 per row
//   start, dfs, parent   3 x 128 x 64 x 1 B         = 24 KiB   the CSR index, the search index, the search parent
// 80 KiB per block: two blocks per CU.  The output row is staged in LDS so that the global stores are done by the whole wave: row r of
// the block is written by all 64 lanes over consecutive columns.
#include "common.hpp"
#include "smiles_writer.hpp"

namespace rew {

SMI_HD uint32_t prio(uint32_t base, int a) { return fpr::mix(base ^ ((uint32_t)a * 0x85EBCA6Bu)); }

// atoms by (prio, number)
struct HashOrder {
  uint32_t base;
  SMI_HD bool before(int a, int b) const {
    const uint32_t pa = prio(base, a), pb = prio(base, b);
    return pa < pb || (pa == pb && a < b);
  }
};

// One row: the walk, the adjacency, the search, the emission.  Returns the status; *len = the content tokens staged in O, COPY for a
// row that is to be copied through.  O may share C's storage: C is not read once the adjacency is built.
template <class Words, class Clos, class Out, class Half, class Bytes, class Src>
SMI_HD int row(Words& W, Clos& C, Out& O, Half& A, Bytes& S, Bytes& D, Bytes& P, const Src& src, int first, int end, bool end_is_eos, int V,
               const int32_t* tok_info, const int32_t* chem_info, const int32_t* emit, int eos_id, uint32_t base, int max_content, int* len) {
  *len = COPY;
  int n;
  const int st = graph(W, C, A, S, D, P, src, first, end, end_is_eos, V, tok_info, chem_info, emit, eos_id, &n);
  if (st != smg::OK) return st;
  return write(HashOrder{base}, W, O, A, S, D, P, n, emit, max_content, len);
}

// mix(seed * 0x9E3779B1 + draw_b): what prio() of row b starts from
SMI_HD uint32_t draw_base(uint32_t seed, const uint32_t* draw, long b) {
  return fpr::mix(seed * 0x9E3779B1u + (draw ? draw[b] : (uint32_t)b));
}

}  // namespace rew

namespace {

using rew::LdsBytes;
using rew::LdsClos;
using rew::LdsHalf;
using rew::LdsWords;
typedef rew::Lds RewLds;
static_assert(sizeof(RewLds) == MVAE_REWRITE_LDS_BYTES, "include/mvae.h states the LDS per block");

__global__ __launch_bounds__(64) void smiles_rewrite_rows_kernel(int B, int T, int V, const int64_t* __restrict__ x, long x_ld,
                                                                 const int32_t* __restrict__ tok_info, const int32_t* __restrict__ chem_info,
                                                                 const int32_t* __restrict__ emit, int bos_id, int eos_id, int pad_id,
                                                                 uint32_t seed, const uint32_t* __restrict__ draw, int max_content, int T_out,
                                                                 int64_t* __restrict__ out, int32_t* __restrict__ out_len,
                                                                 int32_t* __restrict__ status, int32_t* __restrict__ counts) {
  __shared__ RewLds lds;
  const int lane = threadIdx.x, b0 = blockIdx.x * 64, b = b0 + lane;
  int len = rew::COPY, keep = 0;
  if (b < B) {
    LdsWords W{lds.words + lane};
    LdsClos C{lds.clos + lane};
    LdsBytes O{lds.out + lane}, S{lds.start + lane}, D{lds.dfs + lane}, P{lds.parent + lane};
    LdsHalf A{lds.half + lane};
    const fpr::PaddedSrc src{x + (long)b * x_ld};
    const int st = rew::row(W, C, O, A, S, D, P, src, 1, T, false, V, tok_info, chem_info, emit, eos_id, rew::draw_base(seed, draw, b),
                            max_content, &len);
    if (len == rew::COPY) keep = rew::copy_len(src, T, eos_id);
    status[b] = st;
    out_len[b] = len == rew::COPY ? keep : len + 2;
    if (counts) atomicAdd(counts + (st & 15), 1);
  }
  __syncthreads();
  rew::store_rows(lds, B, b0, lane, len, keep, x, x_ld, bos_id, eos_id, pad_id, T_out, out);
}

__global__ __launch_bounds__(64) void smiles_rewrite_corpus_kernel(const uint8_t* __restrict__ tokens, const int64_t* __restrict__ offsets, long N,
                                                                   const int64_t* __restrict__ rows, int B, int V,
                                                                   const int32_t* __restrict__ tok_info, const int32_t* __restrict__ chem_info,
                                                                   const int32_t* __restrict__ emit, uint32_t seed,
                                                                   const uint32_t* __restrict__ draw, int max_content, int stride,
                                                                   uint8_t* __restrict__ tokens_out, int64_t* __restrict__ offsets_out,
                                                                   int32_t* __restrict__ status, int32_t* __restrict__ counts,
                                                                   int32_t* __restrict__ err) {
  __shared__ RewLds lds;
  const int lane = threadIdx.x, b0 = blockIdx.x * 64, b = b0 + lane;
  int len = rew::COPY, keep = 0;
  long lo = 0;
  if (b < B) {
    const long id = rows[b];
    int st = smg::SYNTAX;
    if (id >= 0 && id < N) {
      const long have = fpr::csr_len(offsets, id, &lo);
      LdsWords W{lds.words + lane};
      LdsClos C{lds.clos + lane};
      LdsBytes O{lds.out + lane}, S{lds.start + lane}, D{lds.dfs + lane}, P{lds.parent + lane};
      LdsHalf A{lds.half + lane};
      st = rew::row(W, C, O, A, S, D, P, fpr::CsrSrc{tokens + lo}, 0, fpr::csr_end(have), true, V, tok_info, chem_info, emit, -1,
                    rew::draw_base(seed, draw, b), max_content, &len);
      if (len == rew::COPY) {
        keep = (int)(have < stride ? have : stride);
        if (have > stride && err) atomicMax(err, 1);
      }
    } else if (err) {
      atomicMax(err, 2);
    }
    rew::store_corpus_row(b, B, stride, len, keep, st, offsets_out, status, counts);
  }
  __syncthreads();
  rew::store_corpus(lds, B, b0, lane, len, keep, lo, tokens, stride, tokens_out);
}

}  // namespace

extern "C" {

int mvae_smiles_rewrite_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info,
                             const int32_t* emit, int bos_id, int eos_id, int pad_id, uint32_t seed, const uint32_t* draw, int max_content,
                             int T_out, int64_t* out, int32_t* out_len, int32_t* status, int32_t* counts, void* stream) {
  if (V > 64) return MVAE_ERR_UNSUPPORTED;
  if (!rew::rows_args_ok(B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len, status))
    return MVAE_ERR_INVALID;
  hipLaunchKernelGGL(smiles_rewrite_rows_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, B, T, V, x, (long)x_ld, tok_info,
                     chem_info, emit, bos_id, eos_id, pad_id, seed, draw, max_content, T_out, out, out_len, status, counts);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

int mvae_smiles_rewrite_corpus(const uint8_t* tokens, const int64_t* offsets, int64_t N, const int64_t* rows, int B, int V,
                               const int32_t* tok_info, const int32_t* chem_info, const int32_t* emit, uint32_t seed, const uint32_t* draw,
                               int max_content, int stride, uint8_t* tokens_out, int64_t* offsets_out, int32_t* status, int32_t* counts,
                               int32_t* err, void* stream) {
  if (V > 64) return MVAE_ERR_UNSUPPORTED;
  if (!rew::corpus_args_ok(tokens, offsets, N, rows, B, V, tok_info, chem_info, emit, max_content, stride, tokens_out, offsets_out, status))
    return MVAE_ERR_INVALID;
  hipLaunchKernelGGL(smiles_rewrite_corpus_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, tokens, offsets, (long)N, rows, B, V,
                     tok_info, chem_info, emit, seed, draw, max_content, stride, tokens_out, offsets_out, status, counts, err);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

int mvae_smiles_rewrite_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info,
                             const int32_t* emit, int bos_id, int eos_id, int pad_id, uint32_t seed, const uint32_t* draw, int max_content,
                             int T_out, int64_t* out, int32_t* out_len, int32_t* status) {
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
    status[b] = rew::row(W, C, O, A, S, D, P, src, 1, T, false, V, tok_info, chem_info, emit, eos_id, rew::draw_base(seed, draw, b), max_content,
                         &len);
    rew::host_store_row(O, src, T, len, bos_id, eos_id, pad_id, T_out, out + b * T_out, out_len + b);
  }
  return MVAE_OK;
}

}  // extern "C"
