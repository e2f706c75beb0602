// Valence check and molecular formula of SMILES token rows (gfx950): mvae_smiles_graph_rows over padded int64 rows, mvae_smiles_graph_corpus
// over the CSR corpus, mvae_smiles_graph_host on host pointers.  include/mvae.h ("SMILES graph") states the rules; smiles_graph.hpp is the
// walk, written once; this file is where the per-atom state lives; smiles_rounds.hpp's row driver maps rows to threads.
//
// One thread per row, 64-thread blocks, as in smiles_syntax_check_kernel: a row is a sequential parse of a few dozen tokens and the rows
// are independent.  The per-atom state -- one 32-bit word per atom: predecessor, used valence, element / aromatic / bracket / charge -- is
// indexed by a run-time atom number, so it lives in LDS and not in a private array (which would go to scratch): 128 atoms x 64 lanes x
// 4 bytes = 32 KiB per block, atom-major ([atom][lane]), so the 64 lanes of a wave that touch the same atom number touch 64 consecutive
// words -- one word per bank pair, no conflict -- and lanes that touch different atoms never share a word.  Everything else the walk keeps
// is a handful of 64-bit masks and packed words in registers.
#include "common.hpp"
#include "smiles_rounds.hpp"

namespace smg {

// The consumer the row driver (smiles_rounds.hpp) runs: the walk alone, without a recorder
struct Check {
  template <template <class, int> class Arr>
  struct Store {
    Arr<uint32_t, ATOM_SLOTS> at;
  };
  typedef Store<fpr::LdsMem> Lds;
  static __device__ Store<fpr::LdsArr> lane(Lds& l) { return {l.at.lane()}; }
  typedef Store<fpr::HostArr> Host;

  struct Out {
    int32_t* status;
    int32_t *bad_pos, *desc, *formula;       // optional
    bool ok() const { return status != nullptr; }
  };

  template <class S, class Src>
  static SMI_HD void row(S& s, const Src& src, int first, int end, bool end_is_eos, int V, const int32_t* tok_info, const int32_t* chem_info,
                         int eos_id, long b, const Out& o) {
    Row r;
    walk(s.at, src, first, end, end_is_eos, V, tok_info, chem_info, eos_id, &r);
    store(r, b, o.status, o.bad_pos, o.desc, o.formula);
  }
};

}  // namespace smg

extern "C" {

int mvae_smiles_graph_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, int eos_id,
                           int32_t* status, int32_t* bad_pos, int32_t* desc, int32_t* formula, void* stream) {
  return fpr::rows<smg::Check>(B, T, V, x, x_ld, tok_info, chem_info, eos_id, stream, status, bad_pos, desc, formula);
}

int mvae_smiles_graph_corpus(const uint8_t* tokens, const int64_t* offsets, int64_t N, int V, const int32_t* tok_info, const int32_t* chem_info,
                             int32_t* status, int32_t* bad_pos, int32_t* desc, int32_t* formula, void* stream) {
  return fpr::corpus<smg::Check>(tokens, offsets, N, V, tok_info, chem_info, stream, status, bad_pos, desc, formula);
}

int mvae_smiles_graph_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, int eos_id,
                           int32_t* status, int32_t* bad_pos, int32_t* desc, int32_t* formula) {
  return fpr::host<smg::Check>(B, T, V, x, x_ld, tok_info, chem_info, eos_id, status, bad_pos, desc, formula);
}

}  // extern "C"
