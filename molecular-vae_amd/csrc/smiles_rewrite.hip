// Randomised respelling of SMILES token rows (gfx950): mvae_smiles_rewrite_rows / _corpus / _host.  include/mvae.h ("SMILES rewrite")
// states the definition: the walk's graph, a priority per atom from a counter hash, a depth-first search from the atom of least priority
// with multiple bonds first, and the emission of the search tree in pre-order in the language the syntax automaton accepts.
//
// A fifth consumer of the walk of smiles_graph.hpp, with the fingerprint's recorder (smiles_rounds.hpp), and the first that writes a
// string.  The graph, the search, the emission, the arrays (rew::Store) and the writer driver -- the kernels' bodies, the launches and
// the host loop -- are smiles_writer.hpp's, shared with smiles_canon.hip; this file states the order of the atoms, (prio, atom number),
// as the family rew::Respell, and names its two kernels and three entries.  One thread per row, 64-thread blocks; everything indexed by
// a run-time atom number lives in LDS, lane-minor, never in a private array:
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

// mix(seed * 0x9E3779B1 + draw_b): what prio() of row b starts from
SMI_HD uint32_t draw_base(uint32_t seed, const uint32_t* draw, long b) {
  return fpr::mix(seed * 0x9E3779B1u + (draw ? draw[b] : (uint32_t)b));
}

// The family the writer driver (smiles_writer.hpp) runs
struct Respell {
  struct Args {
    uint32_t seed;
    const uint32_t* draw;  // optional
  };

  // One row: the walk, the adjacency, the search, the emission.  Returns the status; *len = the content tokens staged in s.O, COPY for a
  // row that is to be copied through.
  template <class S, class Src>
  static SMI_HD int row(S& s, const Src& src, int first, int end, bool end_is_eos, int V, const int32_t* tok_info, const int32_t* chem_info,
                        const int32_t* emit, int eos_id, int max_content, long b, const Args& a, int* len) {
    *len = COPY;
    const uint32_t base = draw_base(a.seed, a.draw, b);
    int n;
    const int st = graph(s.W, s.C, s.A, s.S, s.D, s.P, src, first, end, end_is_eos, V, tok_info, chem_info, emit, eos_id, &n);
    if (st != smg::OK) return st;
    return write(HashOrder{base}, s.W, s.O, s.A, s.S, s.D, s.P, n, emit, max_content, len);
  }
  static SMI_HD void skipped(long, const Args&) {}
};

}  // namespace rew

namespace {

static_assert(sizeof(rew::Lds) == MVAE_REWRITE_LDS_BYTES, "include/mvae.h states the LDS per block");

__global__ __launch_bounds__(64) void smiles_rewrite_rows_kernel(int B, int T, int V, const int64_t* __restrict__ x, long x_ld,
                                                                 const int32_t* __restrict__ tok_info, const int32_t* __restrict__ chem_info,
                                                                 const int32_t* __restrict__ emit, int bos_id, int eos_id, int pad_id,
                                                                 int max_content, int T_out, int64_t* __restrict__ out,
                                                                 int32_t* __restrict__ out_len, int32_t* __restrict__ status,
                                                                 int32_t* __restrict__ counts, uint32_t seed, const uint32_t* __restrict__ draw) {
  __shared__ rew::Lds lds;
  rew::block_rows<rew::Respell>(lds, B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len, status,
                                counts, seed, draw);
}

__global__ __launch_bounds__(64) void smiles_rewrite_corpus_kernel(const uint8_t* __restrict__ tokens, const int64_t* __restrict__ offsets, long N,
                                                                   const int64_t* __restrict__ rows, int B, int V,
                                                                   const int32_t* __restrict__ tok_info, const int32_t* __restrict__ chem_info,
                                                                   const int32_t* __restrict__ emit, int max_content, int stride,
                                                                   uint8_t* __restrict__ tokens_out, int64_t* __restrict__ offsets_out,
                                                                   int32_t* __restrict__ status, int32_t* __restrict__ counts,
                                                                   int32_t* __restrict__ err, uint32_t seed, const uint32_t* __restrict__ draw) {
  __shared__ rew::Lds lds;
  rew::block_corpus<rew::Respell>(lds, tokens, offsets, N, rows, B, V, tok_info, chem_info, emit, max_content, stride, tokens_out, offsets_out,
                                  status, counts, err, seed, draw);
}

}  // namespace

extern "C" {

int mvae_smiles_rewrite_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info,
                             const int32_t* emit, int bos_id, int eos_id, int pad_id, uint32_t seed, const uint32_t* draw, int max_content,
                             int T_out, int64_t* out, int32_t* out_len, int32_t* status, int32_t* counts, void* stream) {
  return rew::rows(smiles_rewrite_rows_kernel, B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out,
                   out_len, status, counts, stream, seed, draw);
}

int mvae_smiles_rewrite_corpus(const uint8_t* tokens, const int64_t* offsets, int64_t N, const int64_t* rows, int B, int V,
                               const int32_t* tok_info, const int32_t* chem_info, const int32_t* emit, uint32_t seed, const uint32_t* draw,
                               int max_content, int stride, uint8_t* tokens_out, int64_t* offsets_out, int32_t* status, int32_t* counts,
                               int32_t* err, void* stream) {
  return rew::corpus(smiles_rewrite_corpus_kernel, tokens, offsets, N, rows, B, V, tok_info, chem_info, emit, max_content, stride, tokens_out,
                     offsets_out, status, counts, err, stream, seed, draw);
}

int mvae_smiles_rewrite_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info,
                             const int32_t* emit, int bos_id, int eos_id, int pad_id, uint32_t seed, const uint32_t* draw, int max_content,
                             int T_out, int64_t* out, int32_t* out_len, int32_t* status) {
  return rew::host<rew::Respell>(B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len, status,
                                 seed, draw);
}

}  // extern "C"
