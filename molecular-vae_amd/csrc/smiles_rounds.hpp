// What the consumers of the SMILES graph walk that work on the finished graph share (fingerprint.hip, scaffold.hip, kekule.hip): the mix
// function, the recorder that keeps bond orders and ring-closure pairs, the loop over all bonds, the ring bonds, lane-minor LDS storage for everything
// indexed by a run-time atom number (and its host twin), and the two token sources.  Definitions: include/mvae.h, "Circular fingerprint".
#pragma once
#include "smiles_graph.hpp"

namespace fpr {

constexpr int CLOSURES = 64;           // slots of the closure list

SMI_HD uint32_t mix(uint32_t h) {
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}

// the recorder the walk runs with (smg::NoRec states the three calls)
template <class Clos>
struct Rec {
  Clos& cl;
  int nclos = 0, n = 0;
  smg::Mask ring{0, 0};
  SMI_HD explicit Rec(Clos& c) : cl(c) {}
  SMI_HD uint32_t atom_bits(int order) const { return (uint32_t)order << 24; }
  SMI_HD void closure(int i, int j) {
    if (nclos < CLOSURES) cl.set(nclos++, (uint16_t)(i | j << 8));
  }
  SMI_HD void done(int atoms, const smg::Mask& members) { n = atoms; ring = members; }
};

// f(a, b, bt) for every bond: atom k's bond to its tree predecessor, then the closure pairs
template <class Atoms, class Clos, class F>
SMI_HD void each_bond(Atoms& at, Clos& cl, int n, int nclos, F f) {
  for (int k = 1; k < n; ++k) {
    const uint32_t w = at.get(k);
    const int p = smg::a_pred(w);
    if (p == smg::NONE) continue;
    const uint32_t order = w >> 24;
    f(k, p, order == 1 && smg::a_arom(w) && smg::a_arom(at.get(p)) ? 4u : order);
  }
  for (int c = 0; c < nclos; ++c) {
    const int v = cl.get(c), i = v & 0xFF, j = v >> 8;
    f(i, j, smg::a_arom(at.get(i)) && smg::a_arom(at.get(j)) ? 4u : 1u);
  }
}

SMI_HD smg::Mask m_or(const smg::Mask& a, const smg::Mask& b) { return smg::Mask{a.lo | b.lo, a.hi | b.hi}; }
SMI_HD smg::Mask m_first(int n) {      // atoms 0 .. n - 1, n <= 127
  return smg::Mask{n >= 64 ? ~0ull : (1ull << n) - 1ull, n > 64 ? (1ull << (n - 64)) - 1ull : 0ull};
}

// bit k: the tree bond k - pred(k) lies on a cycle, that is, some closure's tree path steps over it
template <class Atoms, class Clos>
SMI_HD smg::Mask ring_bonds(Atoms& at, Clos& cl, int nclos) {
  smg::Mask rb{0, 0};
  for (int c = 0; c < nclos; ++c) {
    const int v = cl.get(c);
    int a = v & 0xFF, b = v >> 8;
    for (int g = 0; g < 2 * smg::ATOM_SLOTS && a != b; ++g) {
      if (a > b) { smg::m_set(rb, a); a = smg::a_pred(at.get(a)); }
      else { smg::m_set(rb, b); b = smg::a_pred(at.get(b)); }
    }
  }
  return rb;
}

// [slot][lane]: the 64 lanes of a wave touch 64 consecutive elements, lanes never share one
template <class T, int SLOTS>
struct LdsArr {
  T* base;             // &lds[lane]
  __device__ __forceinline__ T get(int i) const { return base[(i & (SLOTS - 1)) * 64]; }
  __device__ __forceinline__ void set(int i, T v) { base[(i & (SLOTS - 1)) * 64] = v; }
};

template <class T, int SLOTS>
struct HostArr {
  T w[SLOTS];
  T get(int i) const { return w[i & (SLOTS - 1)]; }
  void set(int i, T v) { w[i & (SLOTS - 1)] = v; }
};

struct PaddedSrc {
  const int64_t* row;
  __host__ __device__ __forceinline__ long tok(int t) const { return (long)row[t]; }
};

struct CsrSrc {
  const uint8_t* row;
  __device__ __forceinline__ long tok(int t) const { return (long)row[t]; }
};

}  // namespace fpr
