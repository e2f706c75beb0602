// One fragment of SMILES token rows as canonical token rows (gfx950): mvae_smiles_fragment_smiles_rows / _corpus / _host.
// include/mvae.h ("Fragments") states the definition: fragment number `frag` of the row, the row's graph cut down to it with every
// lost bond turned into hydrogens ("Scaffold SMILES"), spelled by "SMILES canon".  This library's own rule: not BRICS, not RECAP.
//
// The fourth family of the writer driver (smiles_writer.hpp), which owns the kernels' bodies, the launches and the host loop.  This file
// is the graph producer between the walk and the writer, and nothing else:
//   rew::read            the walk and the stereo test (smiles_writer.hpp)
//   frg::cut_bonds, frg::labels   the cut set as a mask in registers and the fragment of every atom (fragment_sets.hpp, shared with
//                        fragment.hip); the degrees stand in S and the labels in D, which are free until the adjacency
//   ssm::cut<true>       the atom words and the closure pairs cut down to the fragment in place; the closures of other fragments are
//                        dropped (smiles_cut.hpp, shared with scaffold_smiles.hip)
//   rew::adjacency, ssm::hydrogens, can::ranks, rew::write   as in scaffold_smiles.hip
// One thread per row, 64-thread blocks, the rewrite's 80 KiB of LDS per block (rew::Lds) with nothing added.  No runtime-indexed private
// array, no recursion; every loop is bounded by n <= 127 and every index goes through a slot mask.
#include "common.hpp"
#include "fragment_sets.hpp"
#include "smiles_canon.hpp"
#include "smiles_cut.hpp"
#include "smiles_writer.hpp"

namespace fsm {

enum : int { NO_FRAGMENT = MVAE_SMILES_NO_FRAGMENT };

// The family the writer driver runs.  info [B, 4] may be NULL; it is written in full.
struct FragmentSmiles {
  struct Args {
    int frag;
    int32_t* info;
    SMI_HD int32_t* info_of(long b) const { return info ? info + 4 * b : nullptr; }
  };

  // One row: the walk, the cut set, the labels, the cut, the hydrogens, the ranks, the search, the emission.  Returns the status;
  // *len = the content tokens staged in O, 0 for a row without that fragment: never a copy.
  template <class S, class Src>
  static SMI_HD int row(S& s, const Src& src, int first, int end, bool end_is_eos, int V, const int32_t* tok_info, const int32_t* chem_info,
                        const int32_t* emit, int eos_id, int max_content, long b, const Args& a, int* len) {
    *len = 0;
    int32_t* info = a.info_of(b);
    fpr::Rec<decltype(s.C)> rec(s.C);
    int st = rew::read(s.W, rec, src, first, end, end_is_eos, V, tok_info, chem_info, emit, eos_id);
    int m = 0, bonds = 0, made = 0, lost = 0;
    if (st == smg::OK) {
      int nclos = rec.nclos < fpr::CLOSURES ? rec.nclos : fpr::CLOSURES;
      const smg::Mask rb = fpr::ring_bonds(s.W, s.C, nclos);
      const frg::Cuts cuts = frg::cut_bonds(s.W, s.S, s.C, rec.n, nclos, rec.ring, rb);
      const int nf = frg::labels(s.W, rec.n, cuts.cut, s.D);
      if (a.frag >= nf) st = NO_FRAGMENT;
      else {
        const smg::Mask u = frg::members(s.D, rec.n, a.frag);
        m = ssm::cut<true>(s.W, s.C, rec.n, &nclos, u, &lost);
        rew::adjacency(s.W, s.C, s.A, s.S, s.D, s.P, m, nclos);
        bonds = s.S.get(m) >> 1;
        made = ssm::hydrogens(s.W, s.P, m);
        int unused[4];
        can::ranks(s.W, s.A, s.S, s.O, s.D, s.P, m, unused);
      }
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

}  // namespace fsm

namespace {

static_assert(sizeof(rew::Lds) == MVAE_FRAGMENT_SMILES_LDS_BYTES, "include/mvae.h states the LDS per block");
static_assert(MVAE_FRAGMENT_SMILES_LDS_BYTES <= 80 * 1024, "two blocks per CU");

__global__ __launch_bounds__(64) void smiles_fragment_smiles_rows_kernel(int B, int T, int V, const int64_t* __restrict__ x, long x_ld,
                                                                         const int32_t* __restrict__ tok_info,
                                                                         const int32_t* __restrict__ chem_info, const int32_t* __restrict__ emit,
                                                                         int bos_id, int eos_id, int pad_id, int max_content, int T_out,
                                                                         int64_t* __restrict__ out, int32_t* __restrict__ out_len,
                                                                         int32_t* __restrict__ status, int32_t* __restrict__ counts, int frag,
                                                                         int32_t* __restrict__ info) {
  __shared__ rew::Lds lds;
  rew::block_rows<fsm::FragmentSmiles>(lds, B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len,
                                       status, counts, frag, info);
}

__global__ __launch_bounds__(64) void smiles_fragment_smiles_corpus_kernel(const uint8_t* __restrict__ tokens, const int64_t* __restrict__ offsets,
                                                                           long N, const int64_t* __restrict__ rows, int B, int V,
                                                                           const int32_t* __restrict__ tok_info,
                                                                           const int32_t* __restrict__ chem_info, const int32_t* __restrict__ emit,
                                                                           int max_content, int stride, uint8_t* __restrict__ tokens_out,
                                                                           int64_t* __restrict__ offsets_out, int32_t* __restrict__ status,
                                                                           int32_t* __restrict__ counts, int32_t* __restrict__ err, int frag,
                                                                           int32_t* __restrict__ info) {
  __shared__ rew::Lds lds;
  rew::block_corpus<fsm::FragmentSmiles>(lds, tokens, offsets, N, rows, B, V, tok_info, chem_info, emit, max_content, stride, tokens_out,
                                         offsets_out, status, counts, err, frag, info);
}

}  // namespace

extern "C" {

// frag < 0 is refused with the other arguments: no row has such a fragment, and the driver's own checks come first
int mvae_smiles_fragment_smiles_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info,
                                     const int32_t* emit, int bos_id, int eos_id, int pad_id, int max_content, int T_out, int64_t* out,
                                     int32_t* out_len, int32_t* status, int32_t* counts, int frag, int32_t* info, void* stream) {
  if (V <= 64 && frag < 0) return MVAE_ERR_INVALID;
  return rew::rows(smiles_fragment_smiles_rows_kernel, B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out,
                   out_len, status, counts, stream, frag, info);
}

int mvae_smiles_fragment_smiles_corpus(const uint8_t* tokens, const int64_t* offsets, int64_t N, const int64_t* rows, int B, int V,
                                       const int32_t* tok_info, const int32_t* chem_info, const int32_t* emit, int max_content, int stride,
                                       uint8_t* tokens_out, int64_t* offsets_out, int32_t* status, int32_t* counts, int32_t* err, int frag,
                                       int32_t* info, void* stream) {
  if (V <= 64 && frag < 0) return MVAE_ERR_INVALID;
  return rew::corpus(smiles_fragment_smiles_corpus_kernel, tokens, offsets, N, rows, B, V, tok_info, chem_info, emit, max_content, stride,
                     tokens_out, offsets_out, status, counts, err, stream, frag, info);
}

int mvae_smiles_fragment_smiles_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info,
                                     const int32_t* emit, int bos_id, int eos_id, int pad_id, int max_content, int T_out, int64_t* out,
                                     int32_t* out_len, int32_t* status, int frag, int32_t* info) {
  if (V <= 64 && frag < 0) return MVAE_ERR_INVALID;
  return rew::host<fsm::FragmentSmiles>(B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len,
                                        status, frag, info);
}

}  // extern "C"
