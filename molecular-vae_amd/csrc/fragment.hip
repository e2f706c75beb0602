// The fragments of SMILES token rows and their graph keys (gfx950): mvae_smiles_fragment_rows / _corpus / _host.  include/mvae.h
// ("Fragments") states where a row is cut and what comes out; "Graph key" states the key.  This library's own rule: not BRICS, not RECAP.
//
// A ninth consumer of the walk of smiles_graph.hpp, on the row driver of smiles_rounds.hpp, with the arrays of scaffold.hip and nothing
// added: one thread per row, 64-thread blocks, 80 KiB of LDS per block, two blocks per CU.
//   words                 128 slots x 64 lanes x 4 B = 32 KiB      the walk's atom words; once they are packed, the neighbour sums; once the
//                                                                   rounds are over, per atom: degree inside its fragment | label << 8 |
//                                                                   next atom of the fragment << 16
//   ids                   128 x 64 x 4 B             = 32 KiB      deg(a), then id_{r-1}, overwritten by id_r once the sums are complete
//   packed atoms + pairs  128 x 64 x 2 B             = 16 KiB      as in scaffold.hip; once the labels stand, per fragment: its lowest
//                                                                   atom | its atoms << 8
// The cut set is one smg::Mask in registers (frg::cut_bonds, fragment_sets.hpp).  The eight rounds run ONCE per row, over all atoms, with
// the cut tree bonds left out of each_bond: no bond joins two fragments, so every atom ends with the id that a run over its fragment alone
// would give it, and one walk along each fragment's atom list sums them into that fragment's key.  The lists are threaded through the
// words by one pass down the atom numbers, so all fragments together cost one pass over the atoms, not F.  A row with more than F
// fragments skips the rounds.  No runtime-indexed private array, no recursion; every loop is bounded by n <= 127 and every index goes
// through a slot mask.
#include "common.hpp"
#include "fragment_sets.hpp"
#include "graph_key.hpp"
#include "smiles_rounds.hpp"

namespace frg {

constexpr int F = MVAE_FRAGMENT_MAX;
enum : int { MANY = MVAE_SMILES_FRAG_MANY };

// bits 8-15 of the words as the labels of frg::labels
template <class Words>
struct LabelField {
  Words& w;
  SMI_HD int get(int k) const { return (int)(w.get(k) >> 8) & 0xFF; }
  SMI_HD void set(int k, int v) { w.set(k, (w.get(k) & 0xFFu) | (uint32_t)v << 8); }
};

// The consumer the row driver (smiles_rounds.hpp) runs.  W: the walk's atom words, then the sums, then the lists; I: the ids; H: the
// 16-bit array.
struct Fragment {
  template <template <class, int> class Arr>
  struct Store {
    Arr<uint32_t, smg::ATOM_SLOTS> W, I;
    Arr<uint16_t, smg::ATOM_SLOTS> H;
  };
  typedef Store<fpr::LdsMem> Lds;
  static __device__ Store<fpr::LdsArr> lane(Lds& l) { return {l.W.lane(), l.I.lane(), l.H.lane()}; }
  typedef Store<fpr::HostArr> Host;
  static_assert(sizeof(Lds) == MVAE_FRAGMENT_LDS_BYTES, "include/mvae.h states the LDS per block");
  static_assert(MVAE_FRAGMENT_LDS_BYTES <= 80 * 1024, "two blocks per CU");

  struct Out {
    int32_t* status;
    int64_t* mask;       // optional
    int32_t* desc;
    int64_t* key;
    bool ok() const { return status && desc && key; }
  };

  // One row: the walk, the cut set, the rounds, the labels, the keys; all outputs are written together (zeros for a row that is not OK).
  template <class S, class Src>
  static SMI_HD void row(S& mem, const Src& src, int first, int end, bool end_is_eos, int V, const int32_t* tok_info, const int32_t* chem_info,
                         int eos_id, long b, const Out& o) {
    typedef decltype(mem.H) Half;
    auto &W = mem.W, &I = mem.I;
    auto& H = mem.H;
    scf::TopClos<Half> cl{H};
    fpr::Rec<scf::TopClos<Half>> rec(cl);
    smg::Row r;
    smg::walk(W, src, first, end, end_is_eos, V, tok_info, chem_info, eos_id, &r, rec);
    int status = r.status, nf = 0, ncut = 0, acyl = 0, largest = 0, written = 0;
    if (status == smg::OK) {
      const int n = rec.n, nclos = rec.nclos;
      const smg::Mask ring = rec.ring;
      const smg::Mask rb = fpr::ring_bonds(W, cl, nclos);
      const Cuts cuts = cut_bonds(W, I, cl, n, nclos, ring, rb);
      const smg::Mask cut = cuts.cut;
      ncut = smg::m_count(cut);
      acyl = cuts.acyl_only;
      nf = ncut + 1;                   // atom 0 and the lower end of every cut bond start a fragment
      if (nf > F) status = MANY;
      // the first ids on the degrees inside the fragments; then the words give way to the sums
      for (int k = 1; k < n; ++k) {
        if (!smg::m_get(cut, k)) continue;
        const int p = smg::a_pred(W.get(k));
        I.set(k, I.get(k) - 1u);
        I.set(p, I.get(p) - 1u);
      }
      for (int k = 0; k < n; ++k) {
        const uint32_t w = W.get(k);
        I.set(k, fpr::mix(scf::invariant(w, smg::m_get(ring, k), I.get(k))));
        H.set(k, scf::pack(w));
      }
      scf::PackedAtoms<Half> at{H};
      const auto uncut = [&](int a, int c) { return !(a > c && smg::m_get(cut, a)); };     // a tree bond comes as (k, pred(k)), k > pred(k)
      if (status == smg::OK) scf::refine(at, I, W, cl, n, nclos, fpr::m_first(n), rb, uncut);
      // the degrees inside the fragments again, the labels beside them
      for (int k = 0; k < n; ++k) W.set(k, 0u);
      fpr::each_bond(at, cl, n, nclos, [&](int a, int c, uint32_t) {
        if (!uncut(a, c)) return;
        W.set(a, W.get(a) + 1u);
        W.set(c, W.get(c) + 1u);
      });
      LabelField<decltype(mem.W)> lab{W};
      labels(at, n, cut, lab);
      // the packed atoms and the pairs are dead: H[l] := lowest atom | atoms << 8 of fragment l, every atom pointing to the next higher one
      for (int l = 0; l < nf; ++l) H.set(l, (uint16_t)smg::NONE);
      for (int k = n - 1; k >= 0; --k) {
        const uint32_t w = W.get(k);
        const int l = (int)(w >> 8) & 0xFF, e = H.get(l);
        W.set(k, (w & 0xFFFFu) | (uint32_t)(e & 0xFF) << 16);
        H.set(l, (uint16_t)(k | ((e >> 8) + 1) << 8));
      }
      for (int l = 0; l < nf; ++l) {
        const int size = H.get(l) >> 8;
        if (size > largest) largest = size;
      }
      if (status == smg::OK) written = nf;
    }
    o.status[b] = status;
    int64_t* key = o.key + (long)F * b;
    int64_t* mask = o.mask ? o.mask + 2L * F * b : nullptr;
    for (int f = 0; f < F; ++f) {
      uint64_t kf = 0;
      smg::Mask u{0, 0};
      if (f < written) {
        const int e = H.get(f), size = e >> 8;
        uint32_t lo = 0u, hi = 0u, deg = 0u;
        int k = e & 0xFF;
        for (int g = 0; g < size && g < smg::ATOM_SLOTS; ++g) {
          const uint32_t w = W.get(k);
          scf::add_id(I.get(k), &lo, &hi);
          deg += w & 0xFFu;
          smg::m_set(u, k & (smg::ATOM_SLOTS - 1));
          k = (int)(w >> 16) & 0xFF;
        }
        kf = scf::fold(lo, hi, size, (int)(deg >> 1));
      }
      key[f] = (int64_t)kf;
      if (mask) { mask[2 * f] = (int64_t)u.lo; mask[2 * f + 1] = (int64_t)u.hi; }
    }
    int32_t* d = o.desc + 4 * b;
    const bool told = status == smg::OK || status == MANY;
    d[0] = told ? nf : 0; d[1] = told ? ncut : 0; d[2] = told ? acyl : 0; d[3] = told ? largest : 0;
  }
};

}  // namespace frg

extern "C" {

int mvae_smiles_fragment_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, int eos_id,
                              int32_t* status, int64_t* mask, int32_t* desc, int64_t* key, void* stream) {
  return fpr::rows<frg::Fragment>(B, T, V, x, x_ld, tok_info, chem_info, eos_id, stream, status, mask, desc, key);
}

int mvae_smiles_fragment_corpus(const uint8_t* tokens, const int64_t* offsets, int64_t N, int V, const int32_t* tok_info,
                                const int32_t* chem_info, int32_t* status, int64_t* mask, int32_t* desc, int64_t* key, void* stream) {
  return fpr::corpus<frg::Fragment>(tokens, offsets, N, V, tok_info, chem_info, stream, status, mask, desc, key);
}

int mvae_smiles_fragment_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info, int eos_id,
                              int32_t* status, int64_t* mask, int32_t* desc, int64_t* key) {
  return fpr::host<frg::Fragment>(B, T, V, x, x_ld, tok_info, chem_info, eos_id, status, mask, desc, key);
}

}  // extern "C"
