"""References for the SMILES syntax feature (mvae_moses_sample_syntax_step, mvae_smiles_syntax_check, vocab.smiles_token_table).

1. `valid_smiles(s)`: an INDEPENDENT validator of the accepted language -- not an automaton over (mode, depth, ...), but
     a regular expression for bracket atoms; the string collapsed to the alphabet {A (atom), ~ (bond), ( ) digits};
     a regular expression for the forbidden neighbours; a scan for branch depth and ring pairing.
2. `step` / `need`: the automaton as the issue states it, in plain Python over characters ('$' = <eos>), with helpers that pack a state
   into the int32 [2] layout of include/mvae.h and list the tokens allowed in a state -- the tests build device states with them.
Syntax only: neither formulation knows about valence or aromaticity."""
import re

import numpy as np

# ------------------------------------------------------------------------------------------------ 1. the independent validator
_SYM = r"(?:Cl|Br|[BCNOPSFIbcnops])"
_BRACKET = re.compile(r"\[(?:" + _SYM + r"@{0,2}(?:H[0-9]?)?|H)(?:[+-][0-9]?)?\]")
_FORBIDDEN = re.compile(r"~~|~\)|~\(|~[0-9]|~$|\(\)|\([0-9]|\(\(|\)[0-9]|\($")
DEPTH_MAX = 15


def collapse(s):
    """s over {A, ~, (, ), digits}, or None when a character is left that belongs to no atom or bond."""
    s = _BRACKET.sub("A", s)                                   # (A is no SMILES character, so a bracket atom never merges with a neighbour)
    s = re.sub(r"Cl|Br", "A", s)
    s = re.sub(r"[BCNOPSFIbcnops]", "A", s)
    s = re.sub(r"[=#:/\\-]", "~", s)
    return s if re.fullmatch(r"[A~()0-9]*", s) else None


def valid_smiles(s):
    t = collapse(s)
    if t is None or not t.startswith("A") or _FORBIDDEN.search(t):
        return False
    depth, open_rings, on_atom = 0, set(), set()
    for ch in t:
        if ch == "A":
            on_atom = set()
        elif ch == "(":
            depth += 1
            if depth > DEPTH_MAX:
                return False
        elif ch == ")":
            depth -= 1
            if depth < 0:
                return False
        elif ch.isdigit():
            if ch in on_atom:                                  # a ring may not close on the atom that opened it, nor a digit serve it twice
                return False
            on_atom.add(ch)
            open_rings ^= {ch}
    return depth == 0 and not open_rings


def row_string(ids, vocab):
    """The string a token row (bos first) spells up to its first <eos>, or None when it has no <eos> or a special token before it."""
    ids = [int(t) for t in ids]
    if vocab.eos not in ids[1:]:
        return None
    body = ids[1:1 + ids[1:].index(vocab.eos)]
    chars = [vocab.i2c.get(t, "<?>") for t in body]
    return None if any(len(c) != 1 for c in chars) else "".join(chars)


def row_valid(ids, vocab):
    s = row_string(ids, vocab)
    return s is not None and valid_smiles(s)


# ------------------------------------------------------------------------------------------------ 2. the automaton of the issue
A = set("BCNOPSFIbcnops"); BONDS = set("=#:/\\"); DIG = set("0123456789"); TAIL = {'l': 'C', 'r': 'B'}
START, ATOM, ATOMX, RING, BOND, OPEN, CLOSE, KOPEN, KSYM, KSYMX, KCHI1, KCHI2, KH, KHN, KCHG, KCHGN, END = range(17)
ERROR = 17
ATOMISH = (ATOM, ATOMX, RING); DMAX = 15
S0 = (START, 0, 0, 0, None)


def step(s, ch):                      # -> next state, or None when ch is not allowed
    m, d, o, c, p = s
    if m == END: return None
    if m >= KOPEN:                     # inside [...]
        if m == KOPEN:
            if ch in A: return (KSYM, d, o, c, ch)
            if ch == 'H': return (KHN, d, o, c, ch)
            return None
        if ch == ']': return (ATOMX, d, o, 0, ch)
        if m == KSYM and ch in TAIL and TAIL[ch] == p: return (KSYMX, d, o, c, ch)
        if ch == '@':
            if m in (KSYM, KSYMX): return (KCHI1, d, o, c, ch)
            if m == KCHI1: return (KCHI2, d, o, c, ch)
            return None
        if ch == 'H' and m in (KSYM, KSYMX, KCHI1, KCHI2): return (KH, d, o, c, ch)
        if ch in '+-' and m in (KSYM, KSYMX, KCHI1, KCHI2, KH, KHN): return (KCHG, d, o, c, ch)
        if ch in DIG:
            if m == KH: return (KHN, d, o, c, ch)
            if m == KCHG: return (KCHGN, d, o, c, ch)
        return None
    if ch in A: return (ATOM, d, o, 0, ch)
    if ch == '[': return (KOPEN, d, o, 0, ch)
    if ch in TAIL: return (ATOMX, d, o, c, ch) if (m == ATOM and TAIL[ch] == p) else None
    if ch in BONDS or ch == '-': return (BOND, d, o, c, ch) if m in ATOMISH + (CLOSE, OPEN) else None
    if ch in DIG:
        b = 1 << int(ch)
        return (RING, d, o ^ b, c | b, ch) if (m in ATOMISH and not c & b) else None
    if ch == '(': return (OPEN, d + 1, o, c, ch) if (m in ATOMISH + (CLOSE,) and d < DMAX) else None
    if ch == ')': return (CLOSE, d - 1, o, c, ch) if (m in ATOMISH + (CLOSE,) and d > 0) else None
    if ch == '$': return (END, 0, 0, 0, ch) if (m in ATOMISH + (CLOSE,) and d == 0 and o == 0) else None
    return None                      # everything else, <bos>/<pad>/<unk> included


def need(s):                         # tokens still required to finish, <eos> included
    m, d, o, c, p = s
    if m == END: return 0
    n = bin(o).count('1')
    if m >= KOPEN: return (2 if m == KOPEN else 1) + n + d + 1
    pre = 1 if m in (START, BOND, OPEN) else 0
    extra = 1 if (pre == 0 and n > 0 and ((o & c) != 0 or m == CLOSE)) else 0
    return pre + n + extra + d + 1


def accepts(s):
    """The automaton's verdict on a string (without <eos>)."""
    st = S0
    for ch in s + "$":
        st = step(st, ch)
        if st is None:
            return False
    return st[0] == END


def token_chars(vocab):
    """id -> the character the automaton sees: the symbol itself, '$' for <eos>, None for every other special.  A tail whose head the
    vocabulary lacks and an unpaired '(' ')' '[' ']' are None too (vocab.smiles_token_table makes them OTHER)."""
    out = []
    for i in range(len(vocab)):
        c = vocab.i2c[i]
        if i == vocab.eos:
            c = "$"
        elif len(c) != 1:
            c = None
        elif c in TAIL and TAIL[c] not in vocab.c2i:
            c = None
        elif c in "()" and not ("(" in vocab.c2i and ")" in vocab.c2i):
            c = None
        elif c in "[]" and not ("[" in vocab.c2i and "]" in vocab.c2i):
            c = None
        out.append(c)
    return out


def allowed_ids(s, chars, left):
    """The token ids allowed in state s when `left` = max_len - 1 - step tokens remain after the one being chosen (the feasibility rule)."""
    out = []
    for i, c in enumerate(chars):
        if c is None:
            continue
        n = step(s, c)
        if n is not None and need(n) <= left:
            out.append(i)
    return out


def pack_state(s, vocab):
    """(mode, depth, open, cur, prev char) -> the two int32 words of include/mvae.h."""
    m, d, o, c, p = s
    pid = 0xFF if p is None else (vocab.eos if p == "$" else vocab.c2i[p])
    return (m | d << 8 | pid << 16, o | c << 16)


def first_refusal(ids, chars):
    """mvae_smiles_syntax_check's bad_pos for one token row (bos first): the index of the first refused token, len(ids) when the row runs
    out without <eos>, -1 when END is reached."""
    st = S0
    for t in range(1, len(ids)):
        i = int(ids[t])
        c = chars[i] if 0 <= i < len(chars) else None
        n = step(st, c) if c is not None else None
        if n is None:
            return t
        st = n
        if st[0] == END:
            return -1
    return len(ids)


def random_walk(chars, max_len, rs):
    """One uniformly random constrained walk: at step i = 1 .. max_len - 1 a uniform draw among the allowed ids.  Returns (ids without
    bos, states after each token); raises AssertionError when an allowed set is empty."""
    st, ids, states = S0, [], []
    for i in range(1, max_len):
        al = allowed_ids(st, chars, max_len - 1 - i)
        assert al, (st, i, max_len)
        t = al[rs.randint(len(al))]
        st = step(st, chars[t])
        ids.append(t); states.append(st)
        if st[0] == END:
            break
    return ids, states


def random_prefix(chars, n_tokens, rs, max_len=64):
    """A state reached by n_tokens random legal tokens that do not end the string (feasible within max_len), and the ids that lead there."""
    st, ids = S0, []
    for i in range(1, n_tokens + 1):
        al = [t for t in allowed_ids(st, chars, max_len - 1 - i) if chars[t] != "$"]
        if not al:
            break
        t = al[rs.randint(len(al))]
        st = step(st, chars[t]); ids.append(t)
    return st, ids


def np_states(states, vocab):
    return np.array([pack_state(s, vocab) for s in states], np.int32).reshape(-1, 2)
