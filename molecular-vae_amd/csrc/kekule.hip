// Kekulisation test of SMILES token rows (gfx950): mvae_smiles_kekule_rows / _corpus / _host.  include/mvae.h ("Kekulisation") states the
// definition: N, the aromatic atoms that take exactly one ring double bond; E, the aromatic ring bonds among them; a row kekulises iff
// (N, E) has a perfect matching.
//
// A fourth consumer of the walk of smiles_graph.hpp, with the fingerprint's recorder (smiles_rounds.hpp).  One thread per row, 64-thread
// blocks; everything indexed by a run-time atom number lives in LDS, lane-minor, never in a private array:
//   words                      128 slots x 64 lanes x 4 B = 32 KiB   the walk's atom words; bit 31: the bond to the predecessor is in E
//   closure pairs               64 x 64 x 2 B             =  8 KiB   the walk's list
//   mate, parent, base, queue  4 x 128 x 64 x 1 B         = 32 KiB   the matching and the alternating forest of one search
// 72 KiB per block: two blocks per CU.  Every atom SET is an smg::Mask in registers: N, the ring bonds, the forest's even vertices, the
// bases of the blossom being contracted, the ancestors in the search for its base.
//   N, the neighbours in E, the forest and the matching are kekule.hpp's, shared with smiles_aromatize.hip; this file states the arrays
//   and the outputs.
#include "common.hpp"
#include "kekule.hpp"
#include "smiles_rounds.hpp"

namespace kek {

// The consumer the row driver (smiles_rounds.hpp) runs.  W: the atom words; C: the closure list; M, P, Bs, Q: the byte arrays mate, parent,
// base, queue.
struct Kekule {
  template <template <class, int> class Arr>
  struct Store {
    Arr<uint32_t, SLOTS> W;
    Arr<uint16_t, fpr::CLOSURES> C;
    Arr<uint8_t, SLOTS> M, P, Bs, Q;
  };
  typedef Store<fpr::LdsMem> Lds;
  static __device__ Store<fpr::LdsArr> lane(Lds& l) { return {l.W.lane(), l.C.lane(), l.M.lane(), l.P.lane(), l.Bs.lane(), l.Q.lane()}; }
  typedef Store<fpr::HostArr> Host;
  static_assert(sizeof(Lds) == MVAE_KEKULE_LDS_BYTES, "include/mvae.h states the LDS per block");

  struct Out {
    int32_t* status;
    int32_t* desc;
    uint8_t* mate;       // optional
    bool ok() const { return status && desc; }
  };

  // One row: the walk, N and E, the matching; all outputs are written together.
  template <class S, class Src>
  static SMI_HD void row(S& s, const Src& src, int first, int end, bool end_is_eos, int V, const int32_t* tok_info, const int32_t* chem_info,
                         int eos_id, long b, const Out& o) {
    auto& W = s.W;
    auto& C = s.C;
    auto &M = s.M, &P = s.P, &Bs = s.Bs, &Q = s.Q;
    fpr::Rec<decltype(s.C)> rec(C);
    smg::Row r;
    smg::walk(W, src, first, end, end_is_eos, V, tok_info, chem_info, eos_id, &r, rec);
    int st = r.status, nN = 0, nE = 0, pairs = 0, n = 0;
    if (r.status == smg::OK) {
      n = rec.n;
      const int nclos = rec.nclos;
      const smg::Mask rb = fpr::ring_bonds(W, C, nclos);
      const smg::Mask N = set_n(W, n);
      nN = smg::m_count(N);
      pairs = match(W, C, M, P, Bs, Q, n, nclos, rb, N, &nE);
      if (2 * pairs != nN) st = KEKULE;
    }
    o.status[b] = st;
    int32_t* d = o.desc + 4 * b;
    d[0] = nN; d[1] = nE; d[2] = pairs; d[3] = nN - 2 * pairs;
    if (o.mate) {
      uint8_t* m = o.mate + b * SLOTS;
      for (int k = 0; k < SLOTS; ++k) m[k] = k < n ? M.get(k) : (uint8_t)FREE;
    }
  }
};

}  // namespace kek

extern "C" {

int mvae_smiles_kekule_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, int eos_id,
                            int32_t* status, int32_t* desc, uint8_t* mate, void* stream) {
  return fpr::rows<kek::Kekule>(B, T, V, x, x_ld, tok_info, chem_info, eos_id, stream, status, desc, mate);
}

int mvae_smiles_kekule_corpus(const uint8_t* tokens, const int64_t* offsets, int64_t N, int V, const int32_t* tok_info,
                              const int32_t* chem_info, int32_t* status, int32_t* desc, uint8_t* mate, void* stream) {
  return fpr::corpus<kek::Kekule>(tokens, offsets, N, V, tok_info, chem_info, stream, status, desc, mate);
}

int mvae_smiles_kekule_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, int eos_id,
                            int32_t* status, int32_t* desc, uint8_t* mate) {
  return fpr::host<kek::Kekule>(B, T, V, x, x_ld, tok_info, chem_info, eos_id, status, desc, mate);
}

}  // extern "C"
