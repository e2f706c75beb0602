"""Float64 reference for mosesvae.VAE.decode / score (test helper): the decoder run one token at a time through the oracle's GRU layer
(T = 1, all lengths 1) and linear head, with the candidate, tie and finished-beam rules of mvae_moses_beam_step:
  - an active beam proposes its top-K tokens at score + log p, a finished beam proposes itself once (token pad, score unchanged);
  - the best K candidates of a molecule survive in the order (score desc, parent beam asc, token asc);
  - at step 1 beams 1..K-1 start at -inf; end = step + 1 at the first <eos>, max_len if it never comes.
Each step also reports the smallest gap between consecutive finite scores among the best K + 1 candidates of ALL tokens of the active
beams: where that margin exceeds the f32 path's error, the f32 search must choose the same beams in the same order."""
import numpy as np

from oracle import np_oracle as O


def _logsoftmax(y):
    mx = y.max(-1, keepdims=True)
    return y - (mx + np.log(np.exp(y - mx).sum(-1, keepdims=True)))


class Decoder:
    """The decoder half of mosesvae.VAE in float64 for ONE latent z [d_z]: step(tokens [n], states) -> (log p [n, V], new states)."""

    def __init__(self, p, z, n_layers=3):
        self.p = {k: np.asarray(v, np.float64) for k, v in p.items()}
        self.z = np.asarray(z, np.float64)
        self.NL = n_layers
        self.E = self.p["x_emb.weight"]

    def h0(self, n):
        h = O.linear(self.z[None], self.p["decoder_lat.weight"], self.p["decoder_lat.bias"])
        return [np.repeat(h, n, 0) for _ in range(self.NL)]

    def step(self, toks, hs):
        n = len(toks)
        x = np.concatenate([self.E[np.asarray(toks)], np.repeat(self.z[None], n, 0)], 1)[None]      # [1, n, V + d_z]
        new = []
        for l in range(self.NL):
            p = self.p
            _, h, _ = O.gru_layer_fwd(x, np.ones(n, np.int64), p[f"decoder_rnn.weight_ih_l{l}"], p[f"decoder_rnn.weight_hh_l{l}"],
                                      p[f"decoder_rnn.bias_ih_l{l}"], p[f"decoder_rnn.bias_hh_l{l}"], hs[l])
            new.append(h)
            x = h[None]
        y = O.linear(new[-1], self.p["decoder_fc.weight"], self.p["decoder_fc.bias"])
        return _logsoftmax(y), new


def beam_search(p, z, K, max_len, bos, eos, pad, n_layers=3):
    """One molecule.  Returns (ids [K, max_len] int64, ends [K], scores [K], margin): the K hypotheses in the kernel's order and the
    smallest decision margin over all steps (inf when no decision was close)."""
    dec = Decoder(p, z, n_layers)
    V = dec.E.shape[0]
    score = np.full(K, -np.inf); score[0] = 0.0
    fin = np.zeros(K, bool)
    ends = np.full(K, max_len, np.int64)
    ids = np.full((K, max_len), pad, np.int64); ids[:, 0] = bos
    last = np.full(K, bos, np.int64)
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
            c = score[r] + logp[r]
            full.extend(c.tolist())
            for v in sorted(range(V), key=lambda v: (-c[v], v))[:min(K, V)]:
                cands.append((c[v], r, v))
        cands.sort(key=lambda t: (-t[0], t[1], t[2]))
        top = sorted(full, reverse=True)[:K + 1]
        fin_top = [t for t in top if np.isfinite(t)]
        if len(fin_top) > 1:
            margin = min(margin, float(np.min(-np.diff(fin_top))))
        sel = cands[:K]
        par = np.array([s[1] for s in sel]); tok = np.array([s[2] for s in sel])
        pfin = fin[par]
        tok = np.where(pfin, pad, tok)
        ids = ids[par]; ids[:, step] = tok
        ends = np.where(pfin, ends[par], np.where(tok == eos, step + 1, ends[par]))
        fin = pfin | (tok == eos)
        score = np.array([s[0] for s in sel])
        hs = [h[par] for h in new]
        last = tok
    return ids, ends, score, margin


def teacher_forced(p, z, ids, n_layers=3):
    """log p of each token ids[1:] given its prefix (float64) and the top-2 gap of every step's log p: (logp [n-1], chosen [n-1], gap [n-1])."""
    dec = Decoder(p, z, n_layers)
    hs = dec.h0(1)
    out, best, gap = [], [], []
    for t in range(len(ids) - 1):
        logp, hs = dec.step([ids[t]], hs)
        lp = logp[0]
        out.append(lp[ids[t + 1]])
        best.append(int(lp.argmax()))
        s = np.sort(lp)
        gap.append(s[-1] - s[-2])
    return np.array(out), np.array(best), np.array(gap)
