// Canonical spelling of SMILES token rows (gfx950): mvae_smiles_canon_rows / _corpus / _host.  include/mvae.h ("SMILES canon") states
// the definition: the rewrite's graph, traversal and emission (smiles_writer.hpp, shared with smiles_rewrite.hip) with the atoms compared
// by a canonical rank -- a first invariant per atom, refined by the sorted (bond order, rank) of the neighbours until the number of
// classes stops growing, ties broken one at a time by string order with a refinement after each.
//
// A sixth consumer of the walk of smiles_graph.hpp, and the second family of the writer driver (smiles_writer.hpp), which owns the
// kernels' bodies, the launches and the host loop: smiles_canon.hpp (shared with scaffold_smiles.hip) states the ranks as the family
// can::Canon, and this file names its two kernels and three entries.  One thread per row, 64-thread blocks, and the rewrite's 80 KiB of LDS per block
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
#include "smiles_canon.hpp"
#include "smiles_writer.hpp"

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
  rew::block_rows<can::Canon>(lds, B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len, status,
                              counts, info, rank);
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
  rew::block_corpus<can::Canon>(lds, tokens, offsets, N, rows, B, V, tok_info, chem_info, emit, max_content, stride, tokens_out, offsets_out,
                                status, counts, err, info, rank);
}

}  // namespace

extern "C" {

int mvae_smiles_canon_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info,
                           const int32_t* emit, int bos_id, int eos_id, int pad_id, int max_content, int T_out, int64_t* out, int32_t* out_len,
                           int32_t* status, int32_t* counts, int32_t* info, uint8_t* rank, void* stream) {
  return rew::rows(smiles_canon_rows_kernel, B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len,
                   status, counts, stream, info, rank);
}

int mvae_smiles_canon_corpus(const uint8_t* tokens, const int64_t* offsets, int64_t N, const int64_t* rows, int B, int V,
                             const int32_t* tok_info, const int32_t* chem_info, const int32_t* emit, int max_content, int stride,
                             uint8_t* tokens_out, int64_t* offsets_out, int32_t* status, int32_t* counts, int32_t* err, int32_t* info,
                             uint8_t* rank, void* stream) {
  return rew::corpus(smiles_canon_corpus_kernel, tokens, offsets, N, rows, B, V, tok_info, chem_info, emit, max_content, stride, tokens_out,
                     offsets_out, status, counts, err, stream, info, rank);
}

int mvae_smiles_canon_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info,
                           const int32_t* emit, int bos_id, int eos_id, int pad_id, int max_content, int T_out, int64_t* out, int32_t* out_len,
                           int32_t* status, int32_t* info, uint8_t* rank) {
  return rew::host<can::Canon>(B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len, status, info,
                               rank);
}

}  // extern "C"
