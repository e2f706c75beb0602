"""Float64 reference for the filtered sampling step (mvae_moses_sample_filtered_step) and its loop (test helper), built on the float64
decoder of tests/beam_ref.py:
  - the classes of a row are ranked in the total order (p descending, class id ascending); before(v) = mass ranked before v;
  - keep = {rank < top_k} & {before(v) < top_p * sum(p)} (rank 0 always kept), both on the unfiltered p;
  - the draw is the first kept class, in class-id order, with cumsum(q)_v > u * sum(q), q = keep ? p : 0;
  - the hash is 64-bit FNV-1a over the token ids.
Each decision also reports its margin, so that an fp32 kernel is compared only where the decision is numerically meaningful:
  (a) top-k: log p of rank k-1 minus log p of rank k;  (b) top-p: min over ranks >= 1 of |before(v) - top_p|;
  (c) draw: min_v |cumsum(q)_v - u * sum(q)|;  (b) and (c) with p normalised to sum 1.  A filter that is off has margin +inf."""
import numpy as np

import beam_ref as BR
from oracle import np_oracle as O

FNV_BASIS, FNV_PRIME, M64 = 0xcbf29ce484222325, 0x100000001b3, (1 << 64) - 1


def _rows(p):
    p = np.asarray(p, np.float64)
    p = p[None] if p.ndim == 1 else p
    return p / p.sum(1, keepdims=True)


def _ranked(p):
    """p [n, V] -> (order [n, V]: class at each rank, rank [n, V]: rank of each class, ps: p by rank, before: mass before each rank)."""
    n, V = p.shape
    ids = np.arange(V)[None].repeat(n, 0)
    order = np.lexsort((ids, -p), axis=1)
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, ids, 1)
    ps = np.take_along_axis(p, order, 1)
    return order, rank, ps, np.cumsum(ps, 1) - ps


def _k_on(top_k, V):
    return top_k is not None and 0 < top_k < V


def _p_on(top_p):
    return top_p is not None and top_p < 1.0


def filter_keep(p, top_k=None, top_p=None):
    """keep [n, V] (or [V] for a single row) of the filter rule above; top_k None / 0 / >= V and top_p None / >= 1 are off."""
    one = np.asarray(p).ndim == 1
    p = _rows(p)
    V = p.shape[1]
    _, rank, _, before = _ranked(p)
    keep_s = np.ones(p.shape, bool)                        # by rank
    if _k_on(top_k, V):
        keep_s &= np.arange(V)[None] < top_k
    if _p_on(top_p):
        keep_s &= before < top_p
        keep_s[:, 0] = True
    keep = np.take_along_axis(keep_s, rank, 1)
    return keep[0] if one else keep


def filter_margins(p, top_k=None, top_p=None):
    """(a [n], b [n]): the top-k and top-p margins of each row (+inf where the filter is off)."""
    p = _rows(p)
    n, V = p.shape
    _, _, ps, before = _ranked(p)
    a, b = np.full(n, np.inf), np.full(n, np.inf)
    if _k_on(top_k, V):
        with np.errstate(divide="ignore"):
            a = np.log(ps[:, top_k - 1]) - np.log(ps[:, top_k])
    if _p_on(top_p):
        b = np.abs(before[:, 1:] - top_p).min(1)
    return a, b


def draw(p, keep, u):
    """The class drawn at uniform u [n] from q = keep ? p : 0: the first kept class with cumsum(q) > u * sum(q); the last kept class if
    none is (u * sum(q) rounding up to sum(q))."""
    p = _rows(p)
    keep = np.asarray(keep, bool).reshape(p.shape)
    u = np.atleast_1d(np.asarray(u, np.float64))
    c = np.cumsum(p * keep, 1)
    above = keep & (c > (u * c[:, -1])[:, None])
    V = p.shape[1]
    last = V - 1 - np.argmax(keep[:, ::-1], 1)
    return np.where(above.any(1), np.argmax(above, 1), last)


def draw_margin(p, keep, u):
    """(c [n]): min_v |cumsum(q)_v - u * sum(q)|, p normalised to sum 1."""
    p = _rows(p)
    keep = np.asarray(keep, bool).reshape(p.shape)
    u = np.atleast_1d(np.asarray(u, np.float64))
    c = np.cumsum(p * keep, 1)
    return np.abs(c - (u * c[:, -1])[:, None]).min(1)


def fnv1a64(ids):
    """64-bit FNV-1a over a sequence of small integers (one "byte" each), as an unsigned Python int."""
    h = FNV_BASIS
    for t in ids:
        h = ((h ^ int(t)) * FNV_PRIME) & M64
    return h


def as_int64(h):
    """An unsigned 64-bit value as the int64 a torch tensor holds."""
    return h - (1 << 64) if h >= (1 << 63) else h


class BatchDecoder(BR.Decoder):
    """beam_ref.Decoder with one latent PER ROW: z [n, d_z]; step(tokens [n], states) -> (log p [n, V], new states)."""

    def h0(self, n=None):
        h = O.linear(self.z, self.p["decoder_lat.weight"], self.p["decoder_lat.bias"])
        return [h.copy() for _ in range(self.NL)]

    def step(self, toks, hs):
        x = np.concatenate([self.E[np.asarray(toks)], self.z], 1)[None]
        n = len(toks)
        new = []
        for l in range(self.NL):
            p = self.p
            _, h, _ = O.gru_layer_fwd(x, np.ones(n, np.int64), p[f"decoder_rnn.weight_ih_l{l}"], p[f"decoder_rnn.weight_hh_l{l}"],
                                      p[f"decoder_rnn.bias_ih_l{l}"], p[f"decoder_rnn.bias_hh_l{l}"], hs[l])
            new.append(h)
            x = h[None]
        y = O.linear(new[-1], self.p["decoder_fc.weight"], self.p["decoder_fc.bias"])
        return BR._logsoftmax(y), new


def softmax_temp(logp, temp):
    y = np.asarray(logp, np.float64) / temp
    e = np.exp(y - y.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def teacher_forced_sampling(p64, z, x, temp, top_k, top_p, u_of_step):
    """Teacher-force the float64 decoder on the token rows x [B, max_len] (bos first) with one latent per row.  For every step i = 1 ..
    max_len-1 returns the reference draw, log(q_w / sum q) of the GIVEN token x[:, i] (-inf if the reference dropped it) and the three
    margins: dict of [B, max_len-1] arrays "tok", "logq", "a", "b", "c", and "logp" (the model's log p of the given token, temp = 1)."""
    x = np.asarray(x)
    B, T = x.shape
    dec = BatchDecoder(p64, z)
    hs = dec.h0()
    out = {k: np.zeros((B, T - 1)) for k in ("logq", "a", "b", "c", "logp")}
    out["tok"] = np.zeros((B, T - 1), np.int64)
    for i in range(1, T):
        logp, hs = dec.step(x[:, i - 1], hs)
        p = softmax_temp(logp, temp)
        keep = filter_keep(p, top_k, top_p)
        u = u_of_step(i)
        a, b = filter_margins(p, top_k, top_p)
        q = p * keep
        qw = np.take_along_axis(q, x[:, i:i + 1], 1)[:, 0]
        with np.errstate(divide="ignore"):
            out["logq"][:, i - 1] = np.log(qw / q.sum(1))
        out["logp"][:, i - 1] = np.take_along_axis(logp, x[:, i:i + 1], 1)[:, 0]
        out["tok"][:, i - 1] = draw(p, keep, u)
        out["a"][:, i - 1], out["b"][:, i - 1], out["c"][:, i - 1] = a, b, draw_margin(p, keep, u)
    return out
