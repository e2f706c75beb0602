// The canonical rank of the atoms of a graph the writer holds (rew::adjacency's arrays), and the family can::Canon that the writer driver
// runs: what smiles_canon.hip (the rank of a row's graph) and scaffold_smiles.hip (the rank of its scaffold graph) share.
// include/mvae.h ("SMILES canon") states the definition; smiles_canon.hip says where the ranks live.
#pragma once
#include "common.hpp"
#include "smiles_writer.hpp"

namespace can {

typedef smg::u64 u64;

// atoms by canonical rank
template <class Bytes>
struct RankOrder {
  const Bytes& R;
  SMI_HD bool before(int a, int b) const { return R.get(a) < R.get(b); }
};

// The first invariant (element, aromatic, charge, bracket flag, bracket hydrogens, degree, sum of bond orders) as one number below
// 2^16, in mixed radix: a row the walk gives 0 has used valence <= 6 on every atom, so the last three are 0 .. 6.
template <class Words, class Half, class Bytes>
SMI_HD int invariant(Words& W, Half& A, Bytes& S, int a) {
  const uint32_t w = W.get(a);
  const int s = S.get(a), e = S.get(a + 1);
  int sum = 0;
  for (int i = s; i < e && i < s + 6; ++i) sum += rew::he_order(W, a, w, A.get(i));
  const int deg = e - s, h = smg::a_brk(w) ? rew::w_hyd(w) : 0;
  const int head = ((smg::a_elem(w) * 2 + smg::a_arom(w)) * 3 + smg::a_chg(w) + 1) * 2 + smg::a_brk(w);
  return ((head * 7 + (h < 6 ? h : 6)) * 7 + (deg < 6 ? (deg > 0 ? deg : 0) : 6)) * 7 + (sum < 6 ? sum : 6);
}

// The neighbour codes of atom a under the ranks R, ascending from field 5 (bits 45-53) downwards: between atoms of equal degree, integer
// order of this word is the order of the sorted tuples.
template <class Words, class Half, class Bytes, class Ranks>
SMI_HD u64 key(Words& W, Half& A, Bytes& S, Ranks& R, int a) {
  const uint32_t w = W.get(a);
  const int s = S.get(a), e = S.get(a + 1);
  u64 k = 0;
  int m = 0;
  for (int i = s; i < e && m < 6; ++i, ++m) {
    const int he = A.get(i);
    const u64 c = (u64)(rew::he_order(W, a, w, he) << 7 | (R.get(he & 0x7F) & 0x7F));
    int j = 0;                         // the codes of fields 5 .. 6 - j stay, the others move one field down
    for (; j < m; ++j)
      if (((k >> 9 * (5 - j)) & 511ull) > c) break;
    const u64 top = ~0ull << 9 * (6 - j);
    k = (k & top) | c << 9 * (5 - j) | (k & ~top) >> 9;
  }
  return k;
}

// the end of the run of Q that starts at p (the class of rank p)
template <class Bytes, class Ranks>
SMI_HD int run_end(Bytes& Q, Ranks& R, int p, int n) {
  int q = p + 1;
  while (q < n && R.get(Q.get(q)) == p) ++q;
  return q;
}

// One round: every run of Q sorted by key and cut where the key changes.  Returns the number of classes.
template <class Words, class Half, class Bytes, class Ranks>
SMI_HD int round(Words& W, Half& A, Bytes& S, Ranks& R, Bytes& Q, Bytes& N, int n) {
  int classes = 0;
  for (int p = 0; p < n;) {
    const int q = run_end(Q, R, p, n);
    if (q - p == 1) {
      N.set(Q.get(p), (uint8_t)p);
      ++classes;
      p = q;
      continue;
    }
    for (int i = p + 1; i < q; ++i) {
      const int a = Q.get(i);
      const u64 ka = key(W, A, S, R, a);
      int j = i;
      for (; j > p; --j) {
        const int u = Q.get(j - 1);
        if (!(ka < key(W, A, S, R, u))) break;
        Q.set(j, (uint8_t)u);
      }
      Q.set(j, (uint8_t)a);
    }
    u64 prev = 0;
    int first = p;
    for (int i = p; i < q; ++i) {
      const int a = Q.get(i);
      const u64 k = key(W, A, S, R, a);
      if (i == p || k != prev) { first = i; ++classes; }
      N.set(a, (uint8_t)first);
      prev = k;
    }
    p = q;
  }
  for (int a = 0; a < n; ++a) R.set(a, N.get(a));
  return classes;
}

// The canonical ranks of the n atoms into R (a permutation of 0 .. n - 1).  info = atoms, classes after the first refinement, rounds, ties.
template <class Words, class Half, class Bytes, class Ranks>
SMI_HD void ranks(Words& W, Half& A, Bytes& S, Ranks& R, Bytes& Q, Bytes& N, int n, int* info) {
  // the first invariant: its two bytes into N and R, Q sorted by it (insertion, stable), then R := where a's run starts
  for (int a = 0; a < n; ++a) {
    const int v = invariant(W, A, S, a);
    N.set(a, (uint8_t)(v >> 8));
    R.set(a, (uint8_t)v);
  }
  for (int i = 0; i < n; ++i) {
    const int v = N.get(i) << 8 | R.get(i);
    int j = i;
    for (; j > 0; --j) {
      const int u = Q.get(j - 1);
      if (!(v < (N.get(u) << 8 | R.get(u)))) break;
      Q.set(j, (uint8_t)u);
    }
    Q.set(j, (uint8_t)i);
  }
  int classes = 0, prev = -1, first = 0;
  for (int i = 0; i < n; ++i) {
    const int a = Q.get(i), v = N.get(a) << 8 | R.get(a);
    if (v != prev) { first = i; ++classes; }
    R.set(a, (uint8_t)first);
    prev = v;
  }
  // Every round but the last of a call adds a class and every tie adds one: at most n - 1 of both together, and at most n calls
  int rounds = 0, ties = 0, after_first = 0;
  for (int g = 0; g < 2 * n; ++g) {
    const int c = round(W, A, S, R, Q, N, n);
    ++rounds;
    if (c > classes) { classes = c; continue; }
    if (after_first == 0) after_first = classes;
    if (classes >= n) break;
    // the class of lowest rank with more than one member: its member of lowest atom number stays, the others come just above it
    int p = 0, q = 1;
    for (int t = 0; t < n; ++t) {
      q = run_end(Q, R, p, n);
      if (q - p > 1 || q >= n) break;
      p = q;
    }
    if (q - p < 2) break;              // cannot happen while classes < n
    int at = p;
    for (int i = p + 1; i < q; ++i)
      if (Q.get(i) < Q.get(at)) at = i;
    const int low = Q.get(at);
    Q.set(at, Q.get(p));
    Q.set(p, (uint8_t)low);
    for (int i = p + 1; i < q; ++i) R.set(Q.get(i), (uint8_t)(p + 1));
    ++ties;
    ++classes;
  }
  info[0] = n; info[1] = after_first; info[2] = rounds; info[3] = ties;
}

// The family the writer driver (smiles_writer.hpp) runs.  info [B, 4] and rank [B, 128] may be NULL; each is written in full.
struct Canon {
  struct Args {
    int32_t* info;
    uint8_t* rank;
    SMI_HD int32_t* info_of(long b) const { return info ? info + 4 * b : nullptr; }
    SMI_HD uint8_t* rank_of(long b) const { return rank ? rank + rew::SLOTS * b : nullptr; }
  };

  // One row: the graph, the ranks, the search, the emission.  Returns the status; *len as rew::write gives it.  info and rank of a row
  // that is refused before its ranks are computed are zeros / 0xFF.
  template <class S, class Src>
  static SMI_HD int row(S& s, const Src& src, int first, int end, bool end_is_eos, int V, const int32_t* tok_info, const int32_t* chem_info,
                        const int32_t* emit, int eos_id, int max_content, long b, const Args& a, int* len) {
    *len = rew::COPY;
    int32_t* info = a.info_of(b);
    uint8_t* rank = a.rank_of(b);
    int n, got[4] = {0, 0, 0, 0};
    const int st = rew::graph(s.W, s.C, s.A, s.S, s.D, s.P, src, first, end, end_is_eos, V, tok_info, chem_info, emit, eos_id, &n);
    if (st == smg::OK) ranks(s.W, s.A, s.S, s.O, s.D, s.P, n, got);
    else n = 0;
    if (info) { info[0] = got[0]; info[1] = got[1]; info[2] = got[2]; info[3] = got[3]; }
    if (rank)
      for (int k = 0; k < rew::SLOTS; ++k) rank[k] = k < n ? s.O.get(k) : (uint8_t)0xFF;
    if (st != smg::OK) return st;
    return rew::write(RankOrder<decltype(s.O)>{s.O}, s.W, s.O, s.A, s.S, s.D, s.P, n, emit, max_content, len);
  }

  // info and rank of a row that is not read at all
  static SMI_HD void skipped(long b, const Args& a) {
    int32_t* info = a.info_of(b);
    uint8_t* rank = a.rank_of(b);
    if (info) { info[0] = 0; info[1] = 0; info[2] = 0; info[3] = 0; }
    if (rank)
      for (int k = 0; k < rew::SLOTS; ++k) rank[k] = (uint8_t)0xFF;
  }
};

}  // namespace can
