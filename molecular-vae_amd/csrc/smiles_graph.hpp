// SMILES graph walk shared by the device kernels and the host entry of smiles_graph.hip (rules: include/mvae.h, "SMILES graph").  A second
// automaton on top of smiles_syntax.hpp: while smi::step decides whether the row is well-formed, the walk below keeps the molecular graph
// the tokens spell -- atoms, their tree predecessors, the valence they have used, ring closures -- and enforces the rules that need no
// kekulisation.  Host and device compile the same functions.  The per-atom state is ONE 32-bit word per atom in storage the caller
// provides (`Atoms`: get(i) / set(i, w); LDS on the device, a local array on the host); everything else -- ring membership, aromatic
// atoms, the ring partners of the current atom, the branch stack, the openers of the ten ring digits, the element counts -- is a 64-bit
// mask or a packed word in registers, never a runtime-indexed private array.
#pragma once
#include "smiles_syntax.hpp"

namespace smg {

typedef unsigned long long u64;

enum : int { OK = 0, SYNTAX, VALENCE, CHARGE, RING_BOND, AROMATIC, TOO_LONG };
constexpr int E = 11;                 // H B C N O F P S Cl Br I
constexpr int E_H = 0, E_C = 2;
constexpr int NDESC = 8;
constexpr int CONTENT_MAX = 127;      // content tokens of a row the graph is kept for; also the most atoms a row can have
constexpr int ATOM_SLOTS = 128;       // words of per-atom storage the caller provides
constexpr int NONE = 0xFF;            // no predecessor / no current atom

// largest allowed valence, one nibble per element (element e at bits 4e), 0xF = no entry; smallest allowed valence at charge 0
constexpr u64 VMAX_NEG = 0x00012012340ull, VMAX_0 = 0x51165123431ull, VMAX_POS = 0xFFF54F343F0ull, VMIN_0 = 0x11123123431ull;
constexpr int NO_ENTRY = 0xF;

SMI_HD int vmax(int elem, int chg) {
  const u64 t = chg < 0 ? VMAX_NEG : (chg > 0 ? VMAX_POS : VMAX_0);
  return (int)(t >> (4 * elem)) & 0xF;
}

// atom word: bits 0-7 the tree predecessor (NONE for the first atom), 8-15 the valence used (bonds + bracket hydrogens), 16-19 the
// element, 20 aromatic, 21 bracket atom, 22-23 charge + 1; bits 24-31 are free for a recorder (below)
SMI_HD uint32_t a_make(int pred, int used, int elem, int arom, int brk, int chg) {
  return (uint32_t)pred | (uint32_t)used << 8 | (uint32_t)elem << 16 | (uint32_t)arom << 20 | (uint32_t)brk << 21 | (uint32_t)(chg + 1) << 22;
}
SMI_HD int a_pred(uint32_t w) { return (int)(w & 0xFF); }
SMI_HD int a_used(uint32_t w) { return (int)(w >> 8) & 0xFF; }
SMI_HD int a_elem(uint32_t w) { return (int)(w >> 16) & 0xF; }
SMI_HD int a_arom(uint32_t w) { return (int)(w >> 20) & 1; }
SMI_HD int a_brk(uint32_t w) { return (int)(w >> 21) & 1; }
SMI_HD int a_chg(uint32_t w) { return ((int)(w >> 22) & 3) - 1; }
SMI_HD bool a_fits(uint32_t w) { return a_used(w) <= vmax(a_elem(w), a_chg(w)); }

// the implicit hydrogens of an unbracketed atom of element e whose bonds sum to `sum`
SMI_HD int implicit_h(int e, int arom, int sum) {
  int v0 = (int)(VMIN_0 >> (4 * e)) & 0xF;
  while (v0 < sum) v0 += 2;           // {3,5}, {2,4,6}, {1,3,5}: the next allowed valence is two up
  const int h = v0 - sum;
  return arom ? (h > 0 ? h - 1 : 0) : h;
}

struct Mask { u64 lo, hi; };          // one bit per atom
SMI_HD void m_set(Mask& m, int i) {
  if (i < 64) m.lo |= 1ull << (i & 63);
  else m.hi |= 1ull << (i & 63);
}
SMI_HD bool m_get(const Mask& m, int i) { return (((i < 64 ? m.lo : m.hi) >> (i & 63)) & 1ull) != 0; }
SMI_HD int popcount64(u64 v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(v);
#else
  return __builtin_popcountll(v);
#endif
}
SMI_HD int m_count(const Mask& m) { return popcount64(m.lo) + popcount64(m.hi); }

// what a row comes to; the counts are meaningful for status OK only
struct Row {
  int status, bad_pos;
  int heavy, bonds, rings, ring_atoms, arom, hyd, charge, hetero;
  u64 cnt_lo, cnt_hi;                 // atoms of element e = 1 .. 10, one byte each: e - 1 = 0 .. 7 in cnt_lo, 8 .. 9 in cnt_hi
};

// What a second consumer of the walk wants kept beyond the checks and the counts (fingerprint.hip).  The walk calls
//   atom_bits(order)  at a new atom: bits 24-31 of its atom word (the order of the bond to its tree predecessor is not stored otherwise);
//   closure(i, j)     at every ring-closure bond it accepts (those exist only as the `partner` mask of the current atom);
//   done(n, ring)     at <eos> of a row whose status is OK: the number of atoms and the ring members.
// NoRec keeps nothing: every call is empty and the walk compiles to what it was without a recorder.
struct NoRec {
  SMI_HD uint32_t atom_bits(int) const { return 0u; }
  SMI_HD void closure(int, int) {}
  SMI_HD void done(int, const Mask&) {}
};

// The graph under construction.  `at` holds the atom words 0 .. n - 1.
template <class Atoms, class Rec = NoRec>
struct Graph {
  Atoms& at;
  Rec& rec;
  int status = OK, bad = -1;          // the first graph error and the column of its token
  int n = 0, cur = NONE, order = 1;   // atoms so far, the current atom, the pending bond order
  int nring = 0, hsum = 0, charge = 0;
  Mask ring{0, 0}, arom{0, 0}, partner{0, 0};      // ring members, aromatic atoms, the atoms a ring digit has joined to the current one
  u64 stack_lo = 0, stack_hi = 0;     // the branch stack, one byte per level, the top in the low byte of stack_lo
  u64 open_lo = 0, open_hi = 0;       // the atom that opened ring digit d, one byte each: 0 .. 7 in open_lo, 8 .. 9 in open_hi
  int k_elem = 0, k_arom = 0, k_h = 0, k_sign = 0, k_mag = -1;      // the bracket atom being read

  SMI_HD Graph(Atoms& a, Rec& r) : at(a), rec(r) {}

  SMI_HD void fail(int st, int col) {
    if (status == OK) { status = st; bad = col; }
  }

  // a new atom, bonded with the pending order to the current one
  SMI_HD void new_atom(int elem, int ar, int brk, int chg, int h, int col) {
    if (n >= CONTENT_MAX) return;     // cannot happen: one atom takes at least one of the CONTENT_MAX tokens
    const int k = n++;
    int used = h;
    if (cur != NONE) {
      const uint32_t pw = at.get(cur) + ((uint32_t)order << 8);
      at.set(cur, pw);
      used += order;
      if (!a_fits(pw)) fail(VALENCE, col);
    }
    const uint32_t w = a_make(cur, used, elem, ar, brk, chg) | rec.atom_bits(order);
    at.set(k, w);
    if (!a_fits(w)) fail(VALENCE, col);
    if (ar) m_set(arom, k);
    charge += chg;
    hsum += h;
    cur = k;
    order = 1;
    partner = Mask{0, 0};
  }

  SMI_HD void ring_digit(int d, bool closing, int col) {
    const int sh = 8 * (d & 7);
    if (!closing) {
      if (d < 8) open_lo = (open_lo & ~(0xFFull << sh)) | ((u64)cur << sh);
      else open_hi = (open_hi & ~(0xFFull << sh)) | ((u64)cur << sh);
      return;
    }
    const int i = (int)((d < 8 ? open_lo : open_hi) >> sh) & 0xFF, j = cur;
    uint32_t wj = at.get(j);
    if (a_pred(wj) == i || m_get(partner, i)) { fail(RING_BOND, col); return; }
    const uint32_t wi = at.get(i) + (1u << 8);
    wj += 1u << 8;
    at.set(i, wi);
    at.set(j, wj);
    if (!a_fits(wi) || !a_fits(wj)) fail(VALENCE, col);
    m_set(partner, i);
    ++nring;
    rec.closure(i, j);
    // the tree path i .. j through the lowest common ancestor: a predecessor has a lower index than its atom, so the higher of the two
    // ends steps up until they meet
    int a = i, b = j;
    for (int g = 0; g < 2 * ATOM_SLOTS && a != b; ++g) {
      if (a > b) { m_set(ring, a); a = a_pred(at.get(a)); }
      else { m_set(ring, b); b = a_pred(at.get(b)); }
    }
    m_set(ring, a);
  }

  // One token the automaton has accepted in mode m (the mode in front of it).  cls / info: its tok_info class and word; chem: its
  // chem_info word; closing: for a ring digit outside brackets, whether the digit was open.
  SMI_HD void token(int m, int cls, int32_t info, int32_t chem, bool closing, int col) {
    if (m >= smi::KOPEN) {
      switch (cls) {
        case smi::C_ATOM:  k_elem = chem & 0xF; k_arom = (chem >> 4) & 1; break;
        case smi::C_H:     if (m == smi::KOPEN) { k_elem = E_H; k_arom = 0; } else k_h = 1; break;
        case smi::C_TAIL:  k_elem = chem & 0xF; break;
        case smi::C_PLUS:  k_sign = 1; break;
        case smi::C_MINUS: k_sign = -1; break;
        case smi::C_DIGIT: if (m == smi::KH) k_h = (info >> 16) & 0xF; else k_mag = (info >> 16) & 0xF; break;
        case smi::C_RBRK: {
          const int chg = k_sign * (k_mag >= 0 ? k_mag : 1);
          if (chg < -1 || chg > 1 || vmax(k_elem, chg) == NO_ENTRY) fail(CHARGE, col);      // decided before the atom is bonded
          else new_atom(k_elem, k_arom, 1, chg, k_h, col);
          break;
        }
        default: break;
      }
      return;
    }
    switch (cls) {
      case smi::C_ATOM: new_atom(chem & 0xF, (chem >> 4) & 1, 0, 0, 0, col); break;
      case smi::C_TAIL: {
        const uint32_t w = (at.get(cur) & ~(0xFu << 16)) | (uint32_t)(chem & 0xF) << 16;
        at.set(cur, w);
        if (!a_fits(w)) fail(VALENCE, col);
        break;
      }
      case smi::C_LBRK: k_elem = 0; k_arom = 0; k_h = 0; k_sign = 0; k_mag = -1; break;
      case smi::C_BOND:
      case smi::C_MINUS: order = (chem >> 8) & 3; break;
      case smi::C_DIGIT: ring_digit((info >> 16) & 0xF, closing, col); break;
      case smi::C_LPAR:
        stack_hi = (stack_hi << 8) | (stack_lo >> 56);
        stack_lo = (stack_lo << 8) | (u64)cur;
        break;
      case smi::C_RPAR:
        cur = (int)(stack_lo & 0xFF);
        stack_lo = (stack_lo >> 8) | (stack_hi << 56);
        stack_hi >>= 8;
        break;
      default: break;
    }
  }

  // The checks and the counts at <eos> (column col).
  SMI_HD void finish(int col, Row* r) {
    if ((arom.lo & ~ring.lo) | (arom.hi & ~ring.hi)) { fail(AROMATIC, col); return; }
    int heavy = 0, hetero = 0, hyd = hsum;
    u64 lo = 0, hi = 0;
    for (int k = 0; k < n; ++k) {
      const uint32_t w = at.get(k);
      const int e = a_elem(w);
      if (e == E_H) ++hyd;
      else {
        ++heavy;
        if (e != E_C) ++hetero;
        if (e <= 8) lo += 1ull << (8 * (e - 1));
        else hi += 1ull << (8 * (e - 9));
      }
      if (!a_brk(w)) hyd += implicit_h(e, a_arom(w), a_used(w));
    }
    r->heavy = heavy; r->bonds = n - 1 + nring; r->rings = nring; r->ring_atoms = m_count(ring); r->arom = m_count(arom);
    r->hyd = hyd; r->charge = charge; r->hetero = hetero; r->cnt_lo = lo; r->cnt_hi = hi;
  }
};

// One row.  src.tok(t) is the token at column t, first <= t < end.  end_is_eos: the end of the row acts as <eos> at column `end` (the CSR
// corpus); else only the id eos_id ends the row (pass eos_id = -1 with end_is_eos: no id does).  An id that tok_info calls EOS and that is
// not eos_id is refused, as mvae_smiles_syntax_check refuses it.  rec: the recorder (NoRec: the overload below).
template <class Atoms, class Src, class Rec>
SMI_HD void walk(Atoms& at, const Src& src, int first, int end, bool end_is_eos, int V, const int32_t* tok_info, const int32_t* chem_info,
                 int eos_id, Row* r, Rec& rec) {
  smi::State s{smi::START, 0, smi::NO_PREV, 0, 0};
  Graph<Atoms, Rec> g(at, rec);
  int syn_bad = end, eos_col = -1;
  const int last = end_is_eos ? end + 1 : end;
  for (int t = first; t < last; ++t) {
    long tok = 0;
    int32_t info = smi::C_EOS, chem = 0;
    if (t < end) {
      tok = src.tok(t);
      if (tok < 0 || tok >= V) { syn_bad = t; break; }
      info = tok_info[tok];
      chem = chem_info[tok];
      if (tok == eos_id) info = smi::C_EOS;
      else if ((info & 0xFF) == smi::C_EOS) info = smi::C_OTHER;
    }
    smi::State nx;
    if (!smi::step(s, (int)tok, info, &nx)) { syn_bad = t; break; }
    const int cls = info & 0xFF;
    if (cls == smi::C_EOS) { syn_bad = -1; eos_col = t; break; }
    if (g.status == OK && t - first < CONTENT_MAX)
      g.token(s.mode, cls, info, chem, cls == smi::C_DIGIT && (s.open >> ((info >> 16) & 0xF) & 1) != 0, t);
    s = nx;
  }
  *r = Row{OK, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (syn_bad != -1) { r->status = SYNTAX; r->bad_pos = syn_bad; return; }
  if (eos_col - first > CONTENT_MAX) { r->status = TOO_LONG; r->bad_pos = eos_col; return; }
  if (g.status == OK) g.finish(eos_col, r);
  if (g.status != OK) { *r = Row{g.status, g.bad, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }
  else rec.done(g.n, g.ring);
}

template <class Atoms, class Src>
SMI_HD void walk(Atoms& at, const Src& src, int first, int end, bool end_is_eos, int V, const int32_t* tok_info, const int32_t* chem_info,
                 int eos_id, Row* r) {
  NoRec rec;
  walk(at, src, first, end, end_is_eos, V, tok_info, chem_info, eos_id, r, rec);
}

// Row b of the outputs; a row that is not OK gets zeros in desc and formula.
SMI_HD void store(const Row& r, long b, int32_t* status, int32_t* bad_pos, int32_t* desc, int32_t* formula) {
  status[b] = r.status;
  if (bad_pos) bad_pos[b] = r.bad_pos;
  if (desc) {
    int32_t* d = desc + b * NDESC;
    d[0] = r.heavy; d[1] = r.bonds; d[2] = r.rings; d[3] = r.ring_atoms; d[4] = r.arom; d[5] = r.hyd; d[6] = r.charge; d[7] = r.hetero;
  }
  if (formula) {
    int32_t* f = formula + b * E;
    f[0] = r.hyd;
    for (int e = 1; e <= 8; ++e) f[e] = (int)(r.cnt_lo >> (8 * (e - 1))) & 0xFF;
    f[9] = (int)r.cnt_hi & 0xFF;
    f[10] = (int)(r.cnt_hi >> 8) & 0xFF;
  }
}

}  // namespace smg
