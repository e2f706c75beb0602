"""Float64 reference of a torch.nn.GRU stack AS THE STEP KERNELS SEE IT (mvae_rnn_fwd / mvae_rnn_bwd, cell = GRU): plain numpy on the CPU.

Two implementations of the same stack, checked against each other and against torch.nn.GRU by tests/test_gru_ref_host.py:

  gru_stack(...)                         float64 (or float32) math on `oracle.np_oracle.gru_layer_fwd / gru_layer_bwd`, nothing rounded
  gru_stack(..., storage_round=fn)       the same expressions written out here, with `fn` applied to every tensor the kernels keep in the
                                         storage type, at the point where they store it; with fn = identity it returns what the oracle form
                                         returns, bit for bit.  fn = bf16_round gives what a kernel with exact arithmetic would produce.

What the bf16 kernels store rounded, and what they read back (include/mvae.h, csrc/rnn.hip):
  forward   hs[t] (the emitted h_t, zeros past a length), hdrop[t] = h_t * keep / (1 - p) (rounded once, from the unrounded h_t), the saved
            gate slots r, z, n, W_hn h + b_hn; the weights and h0 arrive in bf16.  The contraction of step t reads the STORED h_{t-1}; the
            element-wise update h_t = (1 - z) n + z h_{t-1} reads the fp32 state, which is never rounded.
  backward  dG (all four slots, each rounded on its own).  The cell reads the stored gates and the stored h_{t-1} (h0 at t = 0) and contracts
            the stored dG_{t+1} and dG^{l+1}_t; the carried gradient, dy, dh_last and dh0 are fp32.

The layer-0 input is any sum of: a real sequence x0 [T, B, in0] through w_ih[0]; a pre-activation addend per step [T, B, 3H] or time-invariant
[B, 3H]; table rows table[index[b, t]] ([rows, 3H]).  Addends are gate-ordered (r, z, n) like W_ih x.  Both forms feed them through the oracle
as extra input columns against an identity block, x_aug = [x0 | addend], w_aug = [W_ih | I]: the input gradient of those columns is then dG's
(r, z, n) slots exactly (a sum of one value and zeros), which is how the oracle form gets at dG without restating the cell.

The 4-slot layout of the library (models.py "RNN stacks", mvae.h bias comment) is written out below and NOT imported from the package:
  W_ih rows  -> slots (r, z, n, 0)            W_hh rows -> slots (r, z, 0, n)         bias -> (b_ir + b_hr, b_iz + b_hz, b_in, b_hn)
  saved gates = [r | z | n | W_hn h + b_hn]   dG = [dpr | dpz | dpn | dpn * r]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import np_oracle as O          # noqa: E402


# ------------------------------------------------------------------------------------------------ 4-slot layout
def pack_w_ih(w):
    """torch W_ih [3H, in] (rows r, z, n) -> [4H, in], slots (r, z, n, 0)."""
    H = w.shape[0] // 3
    out = np.zeros((4 * H,) + w.shape[1:], w.dtype)
    out[0:H] = w[0:H]; out[H:2 * H] = w[H:2 * H]; out[2 * H:3 * H] = w[2 * H:3 * H]
    return out


def pack_w_hh(w):
    """torch W_hh [3H, H] (rows r, z, n) -> [4H, H], slots (r, z, 0, n)."""
    H = w.shape[0] // 3
    out = np.zeros((4 * H,) + w.shape[1:], w.dtype)
    out[0:H] = w[0:H]; out[H:2 * H] = w[H:2 * H]; out[3 * H:4 * H] = w[2 * H:3 * H]
    return out


def pack_bias(b_ih, b_hh):
    """-> [4H]: (b_ir + b_hr, b_iz + b_hz, b_in, b_hn)."""
    H = b_ih.shape[0] // 3
    out = np.zeros(4 * H, b_ih.dtype)
    out[0:H] = b_ih[0:H] + b_hh[0:H]; out[H:2 * H] = b_ih[H:2 * H] + b_hh[H:2 * H]
    out[2 * H:3 * H] = b_ih[2 * H:]; out[3 * H:] = b_hh[2 * H:]
    return out


def pack_addend(a):
    """gate-ordered addend [..., 3H] -> [..., 4H] (slot 3 zero: an input-side term has no W_hn h part)."""
    H = a.shape[-1] // 3
    out = np.zeros(a.shape[:-1] + (4 * H,), a.dtype)
    out[..., :3 * H] = a
    return out


def unslot_ih(a4):
    """the W_ih-side rows of a 4-slot array [4H, ...] -> torch's [3H, ...]: slots 0, 1, 2."""
    H = a4.shape[0] // 4
    return np.concatenate([a4[0:H], a4[H:2 * H], a4[2 * H:3 * H]], 0)


def unslot_hh(a4):
    """the W_hh-side rows of a 4-slot array [4H, ...] -> torch's [3H, ...]: slots 0, 1, 3."""
    H = a4.shape[0] // 4
    return np.concatenate([a4[0:H], a4[H:2 * H], a4[3 * H:4 * H]], 0)


def gates_to_slots(r, z, n, hn):
    return np.concatenate([r, z, n, hn], -1)


def dG_to_slots(dgx, dgh):
    """dgx = [dpr | dpz | dpn], dgh = [dpr | dpz | dpn * r]  ->  [dpr | dpz | dpn | dpn * r]."""
    H = dgx.shape[-1] // 3
    return np.concatenate([dgx, dgh[..., 2 * H:]], -1)


def bf16_round(a):
    """round to nearest-even bf16 and back, in a's dtype."""
    a = np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy().astype(a.dtype)


def bf16_ulp(x):
    """spacing of bf16 numbers at |x| (8 significant bits)."""
    x = float(abs(x))
    return 0.0 if x == 0.0 else 2.0 ** (np.floor(np.log2(x)) - 7)


# ------------------------------------------------------------------------------------------------ one layer, storage form
def _layer_fwd_storage(x, lengths, w_ih, w_hh, b_ih, b_hh, h0, rq):
    """oracle.gru_layer_fwd with the kernel's stores: same expressions in the same order, `rq` where the kernel rounds."""
    T, B, _ = x.shape
    H = w_hh.shape[1]
    dt = x.dtype
    y = np.zeros((T, B, H), dt); y_raw = np.zeros((T, B, H), dt)
    hs = np.zeros((T + 1, B, H), dt)              # the fp32 recurrent state (never rounded after h0)
    hk = np.zeros((T, B, H), dt)                  # the stored h_{t-1} the contraction (and the backward cell) reads
    hs[0] = rq(h0)                                # h0 arrives in the storage type
    r_a = np.zeros((T, B, H), dt); z_a = np.zeros((T, B, H), dt)
    n_a = np.zeros((T, B, H), dt); hn_a = np.zeros((T, B, H), dt)
    gx = (x.reshape(T * B, -1) @ w_ih.T + b_ih).reshape(T, B, 3 * H)
    for t in range(T):
        h = hs[t]
        hk[t] = rq(h)
        gh = hk[t] @ w_hh.T + b_hh
        r = O.sigmoid(gx[t, :, 0:H] + gh[:, 0:H])
        z = O.sigmoid(gx[t, :, H:2 * H] + gh[:, H:2 * H])
        n = np.tanh(gx[t, :, 2 * H:] + r * gh[:, 2 * H:])
        hnew = (1.0 - z) * n + z * h
        m = (t < lengths)[:, None]
        hs[t + 1] = np.where(m, hnew, h)
        y_raw[t] = np.where(m, hnew, 0.0)
        y[t] = rq(y_raw[t])
        r_a[t], z_a[t], n_a[t], hn_a[t] = rq(r), rq(z), rq(n), rq(gh[:, 2 * H:])
    return y, hs[T], (x, lengths, hk, r_a, z_a, n_a, hn_a, w_ih, w_hh), y_raw


def _layer_bwd_storage(dy, dh_last, cache, rq):
    """oracle.gru_layer_bwd on the stored gates / stored h_{t-1}, dG rounded where the kernel stores it (before anything contracts it)."""
    x, lengths, hk, r_a, z_a, n_a, hn_a, w_ih, w_hh = cache
    T, B, H = dy.shape
    dt = dy.dtype
    dgx = np.zeros((T, B, 3 * H), dt)
    dgh = np.zeros((T, B, 3 * H), dt)
    dh = dh_last.copy()
    for t in range(T - 1, -1, -1):
        m = (t < lengths)[:, None]
        r, z, n, hn, h = r_a[t], z_a[t], n_a[t], hn_a[t], hk[t]
        dhn = np.where(m, dh + dy[t], 0.0)
        dn = dhn * (1.0 - z)
        dz = dhn * (h - n)
        dpn = dn * (1.0 - n * n)
        dr = dpn * hn
        dpr = dr * r * (1.0 - r)
        dpz = dz * z * (1.0 - z)
        dgx[t] = rq(np.concatenate([dpr, dpz, dpn], 1))
        dgh[t] = rq(np.concatenate([dpr, dpz, dpn * r], 1))
        dh = np.where(m, dhn * z + dgh[t] @ w_hh, dh)
    dgx2, dgh2 = dgx.reshape(T * B, 3 * H), dgh.reshape(T * B, 3 * H)
    dx = (dgx2 @ w_ih).reshape(T, B, -1)
    dw_ih = dgx2.T @ x.reshape(T * B, -1)
    dw_hh = dgh2.T @ hk.reshape(T * B, H)
    return dx, dh, dw_ih, dw_hh, dgx2.sum(0), dgh2.sum(0), dgx, dgh


# ------------------------------------------------------------------------------------------------ the stack
def layer0_addend(T, B, H, dt, add_step=None, add_const=None, table=None, index=None):
    """Sum of the layer-0 pre-activation addends [T, B, 3H] (None when there is none): table row first, then the per-sequence terms, as the
    step epilogue forms it."""
    a = None
    if table is not None:
        a = np.asarray(table, dt)[np.asarray(index)[:, :T].T]                      # [T, B, 3H]
    for extra in (None if add_const is None else np.broadcast_to(np.asarray(add_const, dt)[None], (T, B, 3 * H)),
                  None if add_step is None else np.asarray(add_step, dt)):
        if extra is not None:
            a = extra.copy() if a is None else a + extra
    return a


def gru_stack(params, lengths, T, B, x0=None, add_step=None, add_const=None, table=None, index=None, h0=None, dy=None, dh_last=None,
              drop_mask=None, drop_p=0.0, storage_round=None, math_dtype=np.float64, backward=True):
    """params: per layer dict(w_ih [3H, in] (layer 0: None without x0), w_hh [3H, H], b_ih [3H], b_hh [3H]) in torch's layout.
    lengths [B] (descending) or None; h0 / dh_last: per-layer lists of [B, H] (or None = zeros); dy [T, B, H] gradient on the top layer's
    output (or None); drop_mask [NL-1, T, B, H] keep bytes with drop_p.  storage_round: None = the oracle form, else the storage form.
    Returns a list of per-layer dicts: y, hdrop (None on the last layer / without dropout), h_last, gates [T, B, 4H], x_in (the rows the layer
    contracted with W_ih: x0 or the stored output below, None for an addend-only layer 0), h_prev [T, B, H], and with backward: dG
    [T, B, 4H], dh0, dW_hh, dW_ih (None for an addend-only layer 0), db_ih, db_hh, dx (gradient on x_in)."""
    dt = math_dtype
    NL = len(params)
    H = params[0]["w_hh"].shape[1]
    lengths = np.full(B, T, np.int64) if lengths is None else np.asarray(lengths, np.int64)
    scale = dt(1.0) / (dt(1.0) - dt(drop_p)) if drop_p > 0.0 else dt(1.0)
    eye = np.eye(3 * H, dtype=dt)
    rq = storage_round
    out, caches = [], []
    x_in = None if x0 is None else np.asarray(x0, dt)
    for l in range(NL):
        p = params[l]
        add = layer0_addend(T, B, H, dt, add_step, add_const, table, index) if l == 0 else None
        if add is None:
            add = np.zeros((T, B, 3 * H), dt)
        n_in = 0 if x_in is None else x_in.shape[2]
        x_aug = add if x_in is None else np.concatenate([x_in, add], 2)
        w_aug = eye if x_in is None else np.concatenate([np.asarray(p["w_ih"], dt), eye], 1)
        w_hh, b_ih, b_hh = np.asarray(p["w_hh"], dt), np.asarray(p["b_ih"], dt), np.asarray(p["b_hh"], dt)
        h0l = np.zeros((B, H), dt) if h0 is None or h0[l] is None else np.asarray(h0[l], dt)
        if rq is None:
            y, h_last, cache = O.gru_layer_fwd(x_aug, lengths, w_aug, w_hh, b_ih, b_hh, h0l)
            y_raw, h_prev = y, cache[2][:T]
        else:
            y, h_last, cache, y_raw = _layer_fwd_storage(x_aug, lengths, w_aug, w_hh, b_ih, b_hh, h0l, rq)
            h_prev = cache[2]
        hdrop = None
        if l + 1 < NL and drop_mask is not None:
            hdrop = y_raw * (np.asarray(drop_mask[l], dt) * scale)
            if rq is not None:
                hdrop = rq(hdrop)
        out.append(dict(y=y, hdrop=hdrop, h_last=h_last, gates=gates_to_slots(*cache[3:7]), x_in=x_in, h_prev=h_prev, n_in=n_in))
        caches.append(cache)
        x_in = hdrop if hdrop is not None else y
    if not backward:
        return out
    dyl = np.zeros((T, B, H), dt) if dy is None else np.asarray(dy, dt)
    for l in range(NL - 1, -1, -1):
        o = out[l]
        dhl = np.zeros((B, H), dt) if dh_last is None or dh_last[l] is None else np.asarray(dh_last[l], dt)
        if rq is None:
            dx_aug, dh0l, dw_aug, dw_hh, db_ih, db_hh = O.gru_layer_bwd(dyl, dhl, caches[l])
            dgx = dx_aug[:, :, o["n_in"]:]                       # through the identity block: dG's (r, z, n) slots themselves
            dgh = np.concatenate([dgx[:, :, :2 * H], dgx[:, :, 2 * H:] * caches[l][3]], 2)      # dpn * r, the oracle's own expression
        else:
            dx_aug, dh0l, dw_aug, dw_hh, db_ih, db_hh, dgx, dgh = _layer_bwd_storage(dyl, dhl, caches[l], rq)
        n_in = o["n_in"]
        o.update(dG=dG_to_slots(dgx, dgh), dh0=dh0l, dW_hh=dw_hh, dW_ih=(dw_aug[:, :n_in] if n_in else None), db_ih=db_ih, db_hh=db_hh,
                 dx=(dx_aug[:, :, :n_in] if n_in else None))
        if l > 0:
            dyl = dx_aug[:, :, :n_in]
            if drop_mask is not None:
                dyl = dyl * (np.asarray(drop_mask[l - 1], dt) * scale)
    return out
