// Murcko scaffolds of SMILES token rows as canonical token rows (gfx950): mvae_smiles_scaffold_smiles_rows / _corpus / _host.
// include/mvae.h ("Scaffold SMILES") states the definition: the scaffold atom set S of "Murcko scaffold", the row's graph cut down to
// it with every lost bond turned into hydrogens, spelled by "SMILES canon".
//
// An eighth consumer of the walk of smiles_graph.hpp and the third family of the writer driver (smiles_writer.hpp), which owns the
// kernels' bodies, the launches and the host loop.  This file is the graph producer between the walk and the writer, and nothing else:
//   rew::read            the walk and the stereo test (smiles_writer.hpp)
//   scf::scaffold_sets   S as a mask in registers, from the atom words and the ring mask (scaffold_sets.hpp, shared with scaffold.hip)
//   ssm::cut             the atom words and the closure pairs of S moved down to 0 .. |S| - 1 in increasing atom order, in place: the
//                        new number of atom k is the members of S below k (a popcount), never more than k (smiles_cut.hpp, shared
//                        with fragment_smiles.hip)
//   rew::adjacency       on the cut arrays: it leaves used valence - bond sum in the hydrogen field, which for a bracket atom is h_S
//                        already and for an unbracketed one is lost(a)
//   ssm::hydrogens       an unbracketed atom stays one iff the implicit rule on its bond sum in G_S (the adjacency's P) gives h_S
//   can::ranks, rew::write   unchanged (smiles_canon.hpp)
// One thread per row, 64-thread blocks, the rewrite's 80 KiB of LDS per block (rew::Lds) with nothing added.  No runtime-indexed private
// array, no recursion; every loop is bounded by n <= 127 and every index goes through a slot mask.
#include "common.hpp"
#include "scaffold_sets.hpp"
#include "smiles_canon.hpp"
#include "smiles_cut.hpp"
#include "smiles_writer.hpp"

namespace ssm {

enum : int { NO_RING = MVAE_SMILES_NO_RING };

// The family the writer driver runs.  info [B, 4] may be NULL; it is written in full.
struct ScaffoldSmiles {
  struct Args {
    int32_t* info;
    SMI_HD int32_t* info_of(long b) const { return info ? info + 4 * b : nullptr; }
  };

  // One row: the walk, S, the cut, the hydrogens, the ranks, the search, the emission.  Returns the status; *len = the content tokens
  // staged in O, 0 for a row without a scaffold: never a copy.
  template <class S, class Src>
  static SMI_HD int row(S& s, const Src& src, int first, int end, bool end_is_eos, int V, const int32_t* tok_info, const int32_t* chem_info,
                        const int32_t* emit, int eos_id, int max_content, long b, const Args& a, int* len) {
    *len = 0;
    int32_t* info = a.info_of(b);
    fpr::Rec<decltype(s.C)> rec(s.C);
    int st = rew::read(s.W, rec, src, first, end, end_is_eos, V, tok_info, chem_info, emit, eos_id);
    if (st == smg::OK && !(rec.ring.lo | rec.ring.hi)) st = NO_RING;
    int m = 0, bonds = 0, made = 0, lost = 0;
    if (st == smg::OK) {
      int nclos = rec.nclos < fpr::CLOSURES ? rec.nclos : fpr::CLOSURES;
      const scf::Sets sets = scf::scaffold_sets(s.W, rec.n, rec.ring);
      m = cut<false>(s.W, s.C, rec.n, &nclos, sets.s, &lost);
      rew::adjacency(s.W, s.C, s.A, s.S, s.D, s.P, m, nclos);
      bonds = s.S.get(m) >> 1;
      made = hydrogens(s.W, s.P, m);
      int unused[4];
      can::ranks(s.W, s.A, s.S, s.O, s.D, s.P, m, unused);
    }
    if (info) { info[0] = m; info[1] = bonds; info[2] = made; info[3] = lost; }
    if (st != smg::OK) return st;
    st = rew::write(can::RankOrder<decltype(s.O)>{s.O}, s.W, s.O, s.A, s.S, s.D, s.P, m, emit, max_content, len);
    if (st != smg::OK) *len = 0;
    return st;
  }

  // info of a row that is not read at all
  static SMI_HD void skipped(long b, const Args& a) {
    int32_t* info = a.info_of(b);
    if (info) { info[0] = 0; info[1] = 0; info[2] = 0; info[3] = 0; }
  }
};

}  // namespace ssm

namespace {

static_assert(sizeof(rew::Lds) == MVAE_SCAFFOLD_SMILES_LDS_BYTES, "include/mvae.h states the LDS per block");
static_assert(MVAE_SCAFFOLD_SMILES_LDS_BYTES <= 80 * 1024, "two blocks per CU");

__global__ __launch_bounds__(64) void smiles_scaffold_smiles_rows_kernel(int B, int T, int V, const int64_t* __restrict__ x, long x_ld,
                                                                         const int32_t* __restrict__ tok_info,
                                                                         const int32_t* __restrict__ chem_info, const int32_t* __restrict__ emit,
                                                                         int bos_id, int eos_id, int pad_id, int max_content, int T_out,
                                                                         int64_t* __restrict__ out, int32_t* __restrict__ out_len,
                                                                         int32_t* __restrict__ status, int32_t* __restrict__ counts,
                                                                         int32_t* __restrict__ info) {
  __shared__ rew::Lds lds;
  rew::block_rows<ssm::ScaffoldSmiles>(lds, B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len,
                                       status, counts, info);
}

__global__ __launch_bounds__(64) void smiles_scaffold_smiles_corpus_kernel(const uint8_t* __restrict__ tokens, const int64_t* __restrict__ offsets,
                                                                           long N, const int64_t* __restrict__ rows, int B, int V,
                                                                           const int32_t* __restrict__ tok_info,
                                                                           const int32_t* __restrict__ chem_info, const int32_t* __restrict__ emit,
                                                                           int max_content, int stride, uint8_t* __restrict__ tokens_out,
                                                                           int64_t* __restrict__ offsets_out, int32_t* __restrict__ status,
                                                                           int32_t* __restrict__ counts, int32_t* __restrict__ err,
                                                                           int32_t* __restrict__ info) {
  __shared__ rew::Lds lds;
  rew::block_corpus<ssm::ScaffoldSmiles>(lds, tokens, offsets, N, rows, B, V, tok_info, chem_info, emit, max_content, stride, tokens_out,
                                         offsets_out, status, counts, err, info);
}

}  // namespace

extern "C" {

int mvae_smiles_scaffold_smiles_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info,
                                     const int32_t* emit, int bos_id, int eos_id, int pad_id, int max_content, int T_out, int64_t* out,
                                     int32_t* out_len, int32_t* status, int32_t* counts, int32_t* info, void* stream) {
  return rew::rows(smiles_scaffold_smiles_rows_kernel, B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out,
                   out_len, status, counts, stream, info);
}

int mvae_smiles_scaffold_smiles_corpus(const uint8_t* tokens, const int64_t* offsets, int64_t N, const int64_t* rows, int B, int V,
                                       const int32_t* tok_info, const int32_t* chem_info, const int32_t* emit, int max_content, int stride,
                                       uint8_t* tokens_out, int64_t* offsets_out, int32_t* status, int32_t* counts, int32_t* err, int32_t* info,
                                       void* stream) {
  return rew::corpus(smiles_scaffold_smiles_corpus_kernel, tokens, offsets, N, rows, B, V, tok_info, chem_info, emit, max_content, stride,
                     tokens_out, offsets_out, status, counts, err, stream, info);
}

int mvae_smiles_scaffold_smiles_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info,
                                     const int32_t* emit, int bos_id, int eos_id, int pad_id, int max_content, int T_out, int64_t* out,
                                     int32_t* out_len, int32_t* status, int32_t* info) {
  return rew::host<ssm::ScaffoldSmiles>(B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len,
                                        status, info);
}

}  // extern "C"
