"""Float64 reference for mosesvae.VAE.decode(syntax=True) (test helper): beam_ref's decoder and its candidate, tie and finished-beam rules,
applied to the tokens the plain-Python automaton of syntax_ref allows (mvae_moses_beam_syntax_step):
  - an active beam in automaton state s proposes its best min(K, allowed) tokens among allowed_ids(s, chars, max_len - 1 - step), at
    score + log p with log p the log-softmax over ALL tokens (no renormalisation); a finished beam proposes itself once;
  - the best K candidates of a molecule survive in the order (score desc, parent beam asc, token asc); a slot without a candidate
    becomes (-inf, parent 0, pad), and a token the automaton refuses puts the row's state in ERROR (None here), which allows nothing;
  - a finished parent's state is carried unchanged.
The margin is the smallest gap between consecutive finite scores among the best K + 1 candidates over the ALLOWED tokens of the active
beams (and the finished beams' own scores).  With syntax=False every token is allowed and the search is beam_ref.beam_search."""
import numpy as np

import beam_ref as BR
import syntax_ref as SY


def beam_search(p, z, K, max_len, vocab, syntax=True, n_layers=3):
    """One molecule.  Returns (ids [K, max_len] int64, ends [K], scores [K], margin) in the kernel's order."""
    bos, eos, pad = vocab.bos, vocab.eos, vocab.pad
    dec = BR.Decoder(p, z, n_layers)
    V = dec.E.shape[0]
    chars = SY.token_chars(vocab) if syntax else None
    score = np.full(K, -np.inf); score[0] = 0.0
    fin = np.zeros(K, bool)
    ends = np.full(K, max_len, np.int64)
    ids = np.full((K, max_len), pad, np.int64); ids[:, 0] = bos
    last = np.full(K, bos, np.int64)
    states = [SY.S0] * K                                     # None = ERROR
    hs = dec.h0(K)
    margin = np.inf
    for step in range(1, max_len):
        logp, new = dec.step(last, hs)
        cands, full = [], []
        for r in range(K):
            if fin[r]:
                cands.append((score[r], r, pad))
                full.append(score[r])
                continue
            if syntax:
                allowed = [] if states[r] is None else SY.allowed_ids(states[r], chars, max_len - 1 - step)
            else:
                allowed = list(range(V))
            c = score[r] + logp[r]
            full.extend(c[allowed].tolist())
            for v in sorted(allowed, key=lambda v: (-c[v], v))[:min(K, V)]:
                cands.append((c[v], r, v))
        cands.sort(key=lambda t: (-t[0], t[1], t[2]))
        top = sorted(full, reverse=True)[:K + 1]
        fin_top = [t for t in top if np.isfinite(t)]
        if len(fin_top) > 1:
            margin = min(margin, float(np.min(-np.diff(fin_top))))
        sel = cands[:K]
        sel += [(-np.inf, 0, pad)] * (K - len(sel))          # dead slots
        par = np.array([s[1] for s in sel]); tok = np.array([s[2] for s in sel])
        pfin = fin[par]
        tok = np.where(pfin, pad, tok)
        if syntax:
            nxt = []
            for k in range(K):
                s = states[par[k]]
                if not pfin[k]:
                    ch = chars[tok[k]]
                    s = SY.step(s, ch) if (s is not None and ch is not None) else None
                nxt.append(s)
            states = nxt
        ids = ids[par]; ids[:, step] = tok
        ends = np.where(pfin, ends[par], np.where(tok == eos, step + 1, ends[par]))
        fin = pfin | (tok == eos)
        score = np.array([s[0] for s in sel])
        hs = [h[par] for h in new]
        last = tok
    return ids, ends, score, margin
