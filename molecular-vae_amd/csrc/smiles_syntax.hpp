// SMILES syntax automaton shared by the constrained sampling step and the syntax-check kernel (layout and grammar: include/mvae.h,
// "SMILES syntax").  A conservative, character-level subset of OpenSMILES: everything it accepts is well-formed (balanced branches,
// closed rings and brackets, no dangling bond, a bracket-atom grammar), not everything well-formed is accepted.  Syntax only: valence and
// aromaticity are not its business.  Host and device compile the same functions; there is no table in memory besides the caller's tok_info.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMI_HD __host__ __device__ inline
#else
#define SMI_HD inline
#endif

namespace smi {

// modes (word 0, bits 0-7 of the packed state)
enum : int { START = 0, ATOM, ATOMX, RING, BOND, OPEN, CLOSE, KOPEN, KSYM, KSYMX, KCHI1, KCHI2, KH, KHN, KCHG, KCHGN, END, ERROR };
// token classes (bits 0-7 of a tok_info word)
enum : int { C_OTHER = 0, C_ATOM, C_TAIL, C_H, C_BOND, C_MINUS, C_PLUS, C_AT, C_DIGIT, C_LPAR, C_RPAR, C_LBRK, C_RBRK, C_EOS };
constexpr int DMAX = 15;          // open branches
constexpr int NO_PREV = 0xFF;

constexpr unsigned bit(int m) { return 1u << m; }
constexpr unsigned M_ATOMISH = bit(ATOM) | bit(ATOMX) | bit(RING);
constexpr unsigned M_AFTER = M_ATOMISH | bit(CLOSE);                                  // where '(' , ')' and <eos> may follow
constexpr unsigned M_BONDABLE = M_AFTER | bit(OPEN);
constexpr unsigned M_SYM = bit(KSYM) | bit(KSYMX);
constexpr unsigned M_CHI = M_SYM | bit(KCHI1) | bit(KCHI2);                           // where the hydrogen count may follow
constexpr unsigned M_CHARGEABLE = M_CHI | bit(KH) | bit(KHN);
constexpr unsigned M_PRE = bit(START) | bit(BOND) | bit(OPEN);                        // an atom is owed before anything else

struct State { int mode, depth, prev, open, cur; };

SMI_HD State unpack(int32_t w0, int32_t w1) { return State{w0 & 0xFF, (w0 >> 8) & 0xFF, (w0 >> 16) & 0xFF, w1 & 0x3FF, (w1 >> 16) & 0x3FF}; }
SMI_HD int32_t pack0(const State& s) { return s.mode | (s.depth << 8) | (s.prev << 16); }
SMI_HD int32_t pack1(const State& s) { return s.open | (s.cur << 16); }

// s --tok--> *out; false when the token is not allowed in s (then *out is unspecified).  info = tok_info[tok].
SMI_HD bool step(const State& s, int tok, int32_t info, State* out) {
  const int cls = info & 0xFF, m = s.mode;
  if (m >= END) return false;
  const unsigned mb = 1u << m;
  const bool tail_ok = ((info >> 8) & 0xFF) == s.prev + 1;                            // (prev NO_PREV never matches)
  State n = s;
  n.prev = tok;
  bool ok = false;
  if (m >= KOPEN) {                                                                   // inside [...]
    switch (cls) {
      case C_ATOM:  ok = m == KOPEN; n.mode = KSYM; break;
      case C_H:     ok = m == KOPEN || (mb & M_CHI); n.mode = m == KOPEN ? KHN : KH; break;
      case C_RBRK:  ok = m != KOPEN; n.mode = ATOMX; n.cur = 0; break;
      case C_TAIL:  ok = m == KSYM && tail_ok; n.mode = KSYMX; break;
      case C_AT:    ok = (mb & (M_SYM | bit(KCHI1))) != 0; n.mode = m == KCHI1 ? KCHI2 : KCHI1; break;
      case C_PLUS:
      case C_MINUS: ok = (mb & M_CHARGEABLE) != 0; n.mode = KCHG; break;
      case C_DIGIT: ok = m == KH || m == KCHG; n.mode = m == KH ? KHN : KCHGN; break;
      default: break;
    }
  } else {
    switch (cls) {
      case C_ATOM:  ok = true; n.mode = ATOM; n.cur = 0; break;
      case C_LBRK:  ok = true; n.mode = KOPEN; n.cur = 0; break;
      case C_TAIL:  ok = m == ATOM && tail_ok; n.mode = ATOMX; break;
      case C_BOND:
      case C_MINUS: ok = (mb & M_BONDABLE) != 0; n.mode = BOND; break;
      case C_DIGIT: {
        const int b = 1 << ((info >> 16) & 0xF);
        ok = (mb & M_ATOMISH) && !(s.cur & b) && b < 1024;
        n.mode = RING; n.open = s.open ^ b; n.cur = s.cur | b;
        break;
      }
      case C_LPAR:  ok = (mb & M_AFTER) && s.depth < DMAX; n.mode = OPEN; n.depth = s.depth + 1; break;
      case C_RPAR:  ok = (mb & M_AFTER) && s.depth > 0; n.mode = CLOSE; n.depth = s.depth - 1; break;
      case C_EOS:   ok = (mb & M_AFTER) && s.depth == 0 && s.open == 0; n.mode = END; n.depth = 0; n.open = 0; n.cur = 0; break;
      default: break;
    }
  }
  *out = n;
  return ok;
}

SMI_HD int popcount10(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc((unsigned)v);
#else
  return __builtin_popcount((unsigned)v);
#endif
}

// tokens still required to finish from s, <eos> included
SMI_HD int need(const State& s) {
  const int m = s.mode;
  if (m >= END) return 0;
  const int n = popcount10(s.open);
  if (m >= KOPEN) return (m == KOPEN ? 2 : 1) + n + s.depth + 1;
  const int pre = (int)((M_PRE >> m) & 1u);
  const int extra = (pre == 0 && n > 0 && ((s.open & s.cur) != 0 || m == CLOSE)) ? 1 : 0;
  return pre + n + extra + s.depth + 1;
}

// The automaton over a prefix: toks[0 .. n) from the initial state.  Returns the index of the first refused token (an id outside [0, V) is
// one), -1 when every token is taken.  *out = the state reached; after a refusal the state in front of the refused token, its mode ERROR.
SMI_HD int walk(const int32_t* toks, int n, int V, const int32_t* tok_info, State* out) {
  State s{START, 0, NO_PREV, 0, 0};
  int bad = -1;
  for (int t = 0; t < n; ++t) {
    const int tok = toks[t];
    State nx;
    if (tok < 0 || tok >= V || !step(s, tok, tok_info[tok], &nx)) { bad = t; s.mode = ERROR; break; }
    s = nx;
  }
  *out = s;
  return bad;
}

}  // namespace smi
