// Murcko scaffolds and graph keys of SMILES token rows (gfx950): mvae_smiles_scaffold_rows / _corpus / _host.  include/mvae.h ("Murcko
// scaffold", "Graph key") states the definitions.
//
// A third consumer of the walk of smiles_graph.hpp, next to smiles_graph.hip and fingerprint.hip, with the fingerprint's recorder
// (smiles_rounds.hpp): bond orders in bits 24-31 of the atom words, the ring-closure pairs in a list, the ring mask at <eos>.  One thread
// per row, 64-thread blocks; everything indexed by a run-time atom number lives in LDS, lane-minor, never in a private array:
//   words                 128 slots x 64 lanes x 4 B = 32 KiB      the walk's atom words; once they are packed, the neighbour sums
//   ids                   128 x 64 x 4 B             = 32 KiB      id_{r-1}, overwritten by id_r once the sums are complete
//   packed atoms + pairs  128 x 64 x 2 B             = 16 KiB      closure c in slot 127 - c, packed atom k in slot k
// 80 KiB per block: two blocks per CU.  The rounds need three things per atom -- predecessor, bond order, aromatic flag -- and the first
// ids two more -- element, charge --: 16 bits (scf::pack).  So the walk's 32-bit words are read for the ring bonds, the sets and the
// molecule key's first ids (the only reader of the used valence), packed, and their storage becomes the sums.  An atom costs one of the
// 127 tokens and a closure two, so n + nclos <= 127 and the closure pairs, which the walk appends from slot 127 down, never meet the
// packed atoms.  The shared each_bond runs over the packed atoms through an adaptor that hands it atom words again.
// Every atom SET is an smg::Mask in registers: the ring members (the walk's), the tree bonds that are ring bonds (bit k: the bond
// k - pred(k)), Core, S.
//   Ring bonds: every closure walks its tree path again, as the walk did for the ring members, and marks the bonds it steps over.
//   Core without pruning: a non-ring atom has only bridges, and every bridge is a tree bond, so what is left when it is removed are its
//   children's subtrees and the rest.  One pass down the atom numbers counts, saturating at two, the children whose subtree holds a ring
//   atom (two masks); one pass up hands every atom whether the rest outside its subtree holds one.  A non-ring atom is a linker iff two
//   of those parts hold ring atoms -- the component criterion of the definition, which is what repeated leaf deletion leaves.
//   Keys: the rounds are edge-centric as the fingerprint's, restricted to the bonds inside the subset; the molecule key and the scaffold
//   key run one after the other through the same two arrays.
#include "common.hpp"
#include "graph_key.hpp"
#include "scaffold_sets.hpp"
#include "smiles_rounds.hpp"

namespace scf {

using fpr::m_or;
using fpr::m_first;
using fpr::ring_bonds;

// The consumer the row driver (smiles_rounds.hpp) runs.  W: the walk's atom words and then the sums; I: the ids; H: the 16-bit array.
struct Scaffold {
  template <template <class, int> class Arr>
  struct Store {
    Arr<uint32_t, smg::ATOM_SLOTS> W, I;
    Arr<uint16_t, smg::ATOM_SLOTS> H;
  };
  typedef Store<fpr::LdsMem> Lds;
  static __device__ Store<fpr::LdsArr> lane(Lds& l) { return {l.W.lane(), l.I.lane(), l.H.lane()}; }
  typedef Store<fpr::HostArr> Host;
  static_assert(sizeof(Lds) == MVAE_SCAFFOLD_LDS_BYTES, "include/mvae.h states the LDS per block");

  struct Out {
    int32_t* status;
    int64_t* mask;       // optional
    int32_t* desc;
    int64_t* key;
    bool ok() const { return status && desc && key; }
  };

  // One row: the walk, the sets, the two keys; all outputs are written together (zeros for a row that is not OK).
  template <class S, class Src>
  static SMI_HD void row(S& mem, const Src& src, int first, int end, bool end_is_eos, int V, const int32_t* tok_info, const int32_t* chem_info,
                         int eos_id, long b, const Out& o) {
    typedef decltype(mem.H) Half;
    auto &W = mem.W, &I = mem.I;
    auto& H = mem.H;
    TopClos<Half> cl{H};
    fpr::Rec<TopClos<Half>> rec(cl);
    smg::Row r;
    smg::walk(W, src, first, end, end_is_eos, V, tok_info, chem_info, eos_id, &r, rec);
    smg::Mask s{0, 0};
    int d0 = 0, d1 = 0, d2 = 0, d3 = 0;
    uint64_t kmol = 0, kscaf = 0;
    if (r.status == smg::OK) {
      const int n = rec.n, nclos = rec.nclos;
      const smg::Mask ring = rec.ring, all = m_first(n);
      const bool has_ring = (ring.lo | ring.hi) != 0;
      const smg::Mask rb = ring_bonds(W, cl, nclos);
      Sets st{{0, 0}, {0, 0}, 0};
      if (has_ring) st = scaffold_sets(W, n, ring);
      // the molecule key's first ids, the only reader of the used valence; then the words give way to the sums
      const int nb = degrees(W, I, cl, n, nclos, all);
      for (int k = 0; k < n; ++k) {
        const uint32_t w = W.get(k);
        I.set(k, fpr::mix(invariant(w, smg::m_get(ring, k), I.get(k)) | (uint32_t)smg::a_used(w) << 12));
        H.set(k, pack(w));
      }
      PackedAtoms<Half> at{H};
      kmol = graph_key(at, I, W, cl, n, nclos, all, rb, nb);
      if (has_ring) {
        s = st.s;
        d1 = degrees(at, W, cl, n, nclos, s);
        for (int k = 0; k < n; ++k)
          if (smg::m_get(s, k)) I.set(k, fpr::mix(invariant(at.get(k), smg::m_get(ring, k), W.get(k))));
        kscaf = graph_key(at, I, W, cl, n, nclos, s, rb, d1);
        d0 = smg::m_count(s);
        d2 = smg::m_count(st.core) - smg::m_count(ring);
        d3 = st.exo;
      }
    }
    o.status[b] = r.status;
    if (o.mask) { o.mask[2 * b] = (int64_t)s.lo; o.mask[2 * b + 1] = (int64_t)s.hi; }
    int32_t* d = o.desc + 4 * b;
    d[0] = d0; d[1] = d1; d[2] = d2; d[3] = d3;
    o.key[2 * b] = (int64_t)kmol; o.key[2 * b + 1] = (int64_t)kscaf;
  }
};

}  // namespace scf

extern "C" {

int mvae_smiles_scaffold_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, int eos_id,
                              int32_t* status, int64_t* mask, int32_t* desc, int64_t* key, void* stream) {
  return fpr::rows<scf::Scaffold>(B, T, V, x, x_ld, tok_info, chem_info, eos_id, stream, status, mask, desc, key);
}

int mvae_smiles_scaffold_corpus(const uint8_t* tokens, const int64_t* offsets, int64_t N, int V, const int32_t* tok_info,
                                const int32_t* chem_info, int32_t* status, int64_t* mask, int32_t* desc, int64_t* key, void* stream) {
  return fpr::corpus<scf::Scaffold>(tokens, offsets, N, V, tok_info, chem_info, stream, status, mask, desc, key);
}

int mvae_smiles_scaffold_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, int eos_id,
                              int32_t* status, int64_t* mask, int32_t* desc, int64_t* key) {
  return fpr::host<scf::Scaffold>(B, T, V, x, x_ld, tok_info, chem_info, eos_id, status, mask, desc, key);
}

}  // extern "C"
