"""Float64 reference of a torch.nn.LSTM stack AS THE STEP KERNELS SEE IT (mvae_rnn_fwd / mvae_rnn_bwd, cell = LSTM): plain numpy on the CPU,
the LSTM counterpart of tests/gru_ref.py.  tests/test_lstm_ref_host.py checks it against torch.nn.LSTM and the numpy oracle;
tests/test_gpu_lstm_kernels.py compares the kernels with it.

Two implementations of the same stack:

  lstm_stack(...)                        the oracle form: float64 (or float32) math on `oracle.np_oracle.lstm_layer_fwd / lstm_layer_bwd`,
                                         nothing rounded -- torch.nn.LSTM with a zero initial state, gate order i, f, g, o
  lstm_stack(..., storage_round=fn)      the storage form: the same expressions written out here, with `fn` applied to every tensor the
                                         kernels keep in the storage type, at the point where they store it; with fn = identity it returns
                                         what the oracle form returns, bit for bit.  fn = bf16_round gives what a kernel with exact
                                         arithmetic would produce.

What the bf16 kernels store rounded, and what they read back (the epilogues of lstm_step_fwd_kernel and bwd_cell_group in csrc/rnn.hip):
  forward   hs[t] (the contraction of step t + 1 and of the layer above read the STORED value), cs[t] (a rounded copy: the carried cell state
            c is fp32 and never rounded), the saved gates i, f, g, o (rounded copies: c and h are computed from the unrounded gates),
            hdrop[t] = h_t * keep / (1 - p), rounded once from the unrounded h_t.  The weights arrive in the storage type.
  backward  the cell reads the STORED gates, cs[t] and cs[t-1] and takes tanh of the stored c; dG (four slots) is rounded on store and the
            next contraction reads the stored dG; the carried dc is fp32.  dy is fp32; dy_a and dy_w are storage-type operands contracted
            in fp32 (the caller forms dy = dy + dy_a . dy_w^T in the math type from operands exact in the storage type).

The layer-0 input is a pre-activation addend: per step [T, B, 4H], time-invariant [B, 4H], table rows table[index[b, t]] ([rows, 4H], ids
clamped to [0, rows) as include/mvae.h says), or a sum of them.  Both forms feed it through the layer as input columns against an identity
block, x_aug = [x_in | addend], w_aug = [W_ih | I]: the input gradient of those columns is then dG itself.

This module also holds what the GPU test and the host test share: the seeded case builder with its input conditions (build_case), the host
products (host_products) and the comparison with its bounds (check_slabs).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import np_oracle as O          # noqa: E402

GATES = ("i", "f", "g", "o")


def bf16_round(a):
    """round to nearest-even bf16 and back, in a's dtype."""
    a = np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy().astype(a.dtype)


def f32_round(a):
    a = np.asarray(a)
    return a.astype(np.float32).astype(a.dtype)


def bf16_ulp(x):
    """spacing of bf16 numbers at |x| (8 significant bits)."""
    x = float(abs(x))
    return 0.0 if x == 0.0 else 2.0 ** (np.floor(np.log2(x)) - 7)


def dropout_keep_mask(seed, shape, p):
    """mvae_dropout_keep (include/mvae.h) restated: keep byte of element `flat index` of an [NL-1, T, B, H] array."""
    idx = np.arange(int(np.prod(shape)), dtype=np.uint64)
    m = np.uint64(0xFFFFFFFF)
    h = ((idx * np.uint64(0x9E3779B1)) & m) ^ np.uint64(seed & 0xFFFFFFFF)
    h ^= h >> np.uint64(16); h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13); h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return (h >= np.uint64(int(float(np.float32(p)) * 4294967296.0))).astype(np.uint8).reshape(shape)


# ------------------------------------------------------------------------------------------------ one layer, storage form
def _layer_fwd_storage(x, w_ih, w_hh, b, rq):
    """oracle.lstm_layer_fwd with the kernel's stores: same expressions in the same order, `rq` where the kernel rounds."""
    T, B, _ = x.shape
    H = w_hh.shape[1]
    dt = x.dtype
    y = np.zeros((T, B, H), dt); y_raw = np.zeros((T, B, H), dt)
    c_all = np.zeros((T, B, H), dt)
    gates = np.zeros((T, B, 4 * H), dt)
    h = np.zeros((B, H), dt)                      # the STORED h_{t-1}: what the contraction reads
    c = np.zeros((B, H), dt)                      # the fp32 carried cell state: never rounded
    gx = x.reshape(T * B, -1) @ w_ih.T + (b + np.zeros_like(b))
    gx = gx.reshape(T, B, 4 * H)
    for t in range(T):
        pre = gx[t] + h @ w_hh.T
        i = O.sigmoid(pre[:, 0:H])
        f = O.sigmoid(pre[:, H:2 * H])
        g = np.tanh(pre[:, 2 * H:3 * H])
        o = O.sigmoid(pre[:, 3 * H:4 * H])
        c = f * c + i * g
        y_raw[t] = o * np.tanh(c)
        h = rq(y_raw[t])
        y[t] = h
        c_all[t] = rq(c)
        gates[t, :, 0:H] = rq(i)
        gates[t, :, H:2 * H] = rq(f)
        gates[t, :, 2 * H:3 * H] = rq(g)
        gates[t, :, 3 * H:4 * H] = rq(o)
    return y, (x, y, c_all, gates, w_ih, w_hh), y_raw


def _layer_bwd_storage(dy, cache, rq, mut, l):
    """oracle.lstm_layer_bwd on the stored gates / cell states, dG rounded where the kernel stores it (before anything contracts it)."""
    x, y, c_all, gates, w_ih, w_hh = cache
    T, B, H = dy.shape
    dt = dy.dtype
    dpre = np.zeros((T, B, 4 * H), dt)
    dh_next = np.zeros((B, H), dt)
    dc_next = np.zeros((B, H), dt)
    for t in range(T - 1, -1, -1):
        i = gates[t, :, 0:H]
        f = gates[t, :, H:2 * H]
        g = gates[t, :, 2 * H:3 * H]
        o = gates[t, :, 3 * H:4 * H]
        c = c_all[t]
        c_prev = c_all[t - 1] if t > 0 else np.zeros_like(c)
        if mut.get("df_uses_c_t"):
            c_prev = c
        if mut.get("drop_dc_at") == (l, t):
            dc_next = np.zeros((B, H), dt)
        tc = np.tanh(c)
        dh = dy[t] + dh_next
        do = dh * tc
        dc = dh * o * (1.0 - tc * tc) + dc_next
        di = dc * g
        dg = dc * i
        df = dc * c_prev
        dc_next = dc * f
        dpre[t, :, 0:H] = rq(di * i * (1.0 - i))
        dpre[t, :, H:2 * H] = rq(df * f * (1.0 - f))
        dpre[t, :, 2 * H:3 * H] = rq(dg * (1.0 - g * g))
        dpre[t, :, 3 * H:4 * H] = rq(do * o * (1.0 - o))
        dh_next = dpre[t] @ w_hh
    dp2 = dpre.reshape(T * B, 4 * H)
    dx = (dp2 @ w_ih).reshape(T, B, -1)
    dw_ih = dp2.T @ x.reshape(T * B, -1)
    h_prev = np.concatenate([np.zeros((1, B, H), dt), y[:-1]], 0).reshape(T * B, H)
    dw_hh = dp2.T @ h_prev
    db = dp2.sum(0)
    return dx, dw_ih, dw_hh, db


# ------------------------------------------------------------------------------------------------ the stack
def layer0_addend(T, B, H, dt, add_step=None, add_const=None, table=None, index=None, clamp=True):
    """Sum of the layer-0 pre-activation addends [T, B, 4H] (None when there is none): table row first, then the per-sequence terms, as the
    step epilogue forms it.  Table ids are clamped to [0, rows)."""
    a = None
    if table is not None:
        tb = np.asarray(table, dt)
        ids = np.asarray(index)[:, :T].T
        a = tb[np.clip(ids, 0, tb.shape[0] - 1)] if clamp else np.take(tb, ids, axis=0, mode="wrap")      # [T, B, 4H]
    for extra in (None if add_const is None else np.broadcast_to(np.asarray(add_const, dt)[None], (T, B, 4 * H)),
                  None if add_step is None else np.asarray(add_step, dt)):
        if extra is not None:
            a = extra.copy() if a is None else a + extra
    return a


def host_products(dG, h_self, x_in):
    """What the models' weight-gradient GEMMs form from the saved tensors, in float64: dG^T . h_prev (h_prev = the layer's own output shifted
    by one step, zeros at t = 0), dG^T . x_in (None for an addend-only layer 0) and colsum(dG).  dG [T, B, 4H], h_self / x_in [T, B, H]."""
    T, B, G4 = dG.shape
    d2 = np.asarray(dG, np.float64).reshape(T * B, G4)
    hs = np.asarray(h_self, np.float64)
    hprev = np.concatenate([np.zeros((1,) + hs.shape[1:]), hs[:-1]], 0).reshape(T * B, -1)
    return dict(p_hh=d2.T @ hprev, p_ih=None if x_in is None else d2.T @ np.asarray(x_in, np.float64).reshape(T * B, -1), p_b=d2.sum(0))


def lstm_stack(params, T, B, add_step=None, add_const=None, table=None, index=None, dy=None, drop_mask=None, drop_p=0.0, storage_round=None,
               math_dtype=np.float64, backward=True, _mutate=None):
    """params: per layer dict(w_ih [4H, H] (layer 0: None), w_hh [4H, H], b [4H] = b_ih + b_hh (None = zeros)) in torch's layout (rows i, f, g,
    o).  Layer 0 is fed by addends only.  dy [T, B, H]: the gradient on the top layer's output (the caller adds a product dy_a . dy_w^T to
    it).  drop_mask [NL-1, T, B, H] keep bytes with drop_p.  storage_round: None = the oracle form, else the storage form.
    _mutate: deliberately WRONG variants of the storage form (tests/test_lstm_ref_host.py: they play a broken kernel's part).
    Returns a list of per-layer dicts: hs, cs, gates [T, B, 4H], hdrop (None on the last layer / without dropout), pre (the pre-activations),
    x_in (the rows the layer contracted with W_ih: the stored output below or its dropped copy; None for layer 0), and with backward: dG
    [T, B, 4H], dW_hh, dW_ih (None for layer 0), db in the math type, and p_hh, p_ih, p_b = host_products of the layer's own tensors."""
    dt = math_dtype
    mut = _mutate or {}
    NL = len(params)
    H = params[0]["w_hh"].shape[1]
    scale = dt(1.0) / (dt(1.0) - dt(drop_p)) if drop_p > 0.0 else dt(1.0)
    eye = np.eye(4 * H, dtype=dt)
    rq = storage_round
    assert rq is not None or not mut
    out, caches = [], []
    x_in = None
    for l in range(NL):
        p = params[l]
        add = layer0_addend(T, B, H, dt, add_step, add_const, table, index, clamp=not mut.get("wrap_ids")) if l == 0 else None
        if add is None:
            add = np.zeros((T, B, 4 * H), dt)
        n_in = 0 if x_in is None else x_in.shape[2]
        x_aug = add if x_in is None else np.concatenate([x_in, add], 2)
        w_aug = eye if x_in is None else np.concatenate([np.asarray(p["w_ih"], dt), eye], 1)
        w_hh = np.asarray(p["w_hh"], dt)
        b = np.zeros(4 * H, dt) if p.get("b") is None else np.asarray(p["b"], dt)
        if rq is None:
            y, cache = O.lstm_layer_fwd(x_aug, w_aug, w_hh, b, np.zeros_like(b))
            y_raw = y
        else:
            y, cache, y_raw = _layer_fwd_storage(x_aug, w_aug, w_hh, b, rq)
        h_prev = np.concatenate([np.zeros((1, B, H), dt), y[:-1]], 0)
        pre = (x_aug.reshape(T * B, -1) @ w_aug.T + b + h_prev.reshape(T * B, H) @ w_hh.T).reshape(T, B, 4 * H)
        hdrop = None
        if l + 1 < NL and drop_mask is not None:
            hdrop = y_raw * (np.asarray(drop_mask[l], dt) * scale)
            if rq is not None:
                hdrop = rq(hdrop)
        out.append(dict(hs=y, cs=cache[2], gates=cache[3], hdrop=hdrop, pre=pre, x_in=x_in, n_in=n_in))
        caches.append(cache)
        x_in = hdrop if hdrop is not None else y
    if not backward:
        return out
    dyl = np.zeros((T, B, H), dt) if dy is None else np.asarray(dy, dt)
    for l in range(NL - 1, -1, -1):
        o = out[l]
        if rq is None:
            dx_aug, dw_aug, dw_hh, db = O.lstm_layer_bwd(dyl, caches[l])
        else:
            dx_aug, dw_aug, dw_hh, db = _layer_bwd_storage(dyl, caches[l], rq, mut, l)
        n_in = o["n_in"]
        dG = dx_aug[:, :, n_in:]                                # through the identity block: dG itself (a sum of one value and zeros)
        o.update(dG=dG, dW_hh=dw_hh, dW_ih=(dw_aug[:, :n_in] if n_in else None), db=db)
        o.update(host_products(dG, o["hs"], o["x_in"]))
        if l > 0:
            dyl = dx_aug[:, :, :n_in]
            if drop_mask is not None:
                dyl = dyl * (np.asarray(drop_mask[l - 1], dt) * (dt(1.0) if mut.get("no_drop_scale_bwd") else scale))
    return out


# ------------------------------------------------------------------------------------------------ comparison
def _slabs(o, drop):
    """(name, array, slab axes) of everything compared in one layer's dict: per time step for the sequences, whole for the products."""
    H = o["hs"].shape[2]
    yield "hs", o["hs"], (1, 2)
    if o.get("cs") is not None:                   # (a forward-only call saves neither; a tensor the reference has and `got` lacks is a KeyError)
        yield "cs", o["cs"], (1, 2)
    for k, g in enumerate(GATES):
        if o.get("gates") is not None:
            yield f"gate_{g}", o["gates"][:, :, k * H:(k + 1) * H], (1, 2)
    if drop and o.get("hdrop") is not None:
        yield "hdrop", o["hdrop"], (1, 2)
    if o.get("dG") is not None:
        for k, g in enumerate(GATES):
            yield f"dG_{g}", o["dG"][:, :, k * H:(k + 1) * H], (1, 2)


PRODUCTS = (("p_hh", "dW_hh"), ("p_ih", "dW_ih"), ("p_b", "db"))


def check_slabs(got, ref, ref32=None, drop=False, only=None):
    """Element-wise |got - ref| <= bound for every tensor of every layer, the bound taken per (layer, time step) slab; the host products of
    `got` (p_hh, p_ih, p_b) against ref's parameter gradients (dW_hh, dW_ih, db), one slab each.
      ref32 is None (f32 kernels)  ref = the oracle form;                   bound = 2e-5 * max|ref| of the slab
      ref32 given   (bf16 kernels) ref = the storage form in float64 math,  floor = max|ref32 - ref| of the slab (ref32 = the storage form in
                                   float32 math; for the products, ref32's own host products), bound = 4 * floor + one bf16 ulp of max|ref|
    got / ref / ref32: lists of per-layer dicts as lstm_stack returns them.  A NaN in `got` fails.
    Returns (bad, floors): bad = list of failure records (empty = pass); floors = {tensor kind: the largest slab floor in bf16 ulps of that
    slab's maximum} (empty without ref32)."""
    bad, floors = [], {}
    ulp = np.vectorize(bf16_ulp)

    def cmp(name, kind, g, r, r32, axes):
        g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
        assert g.shape == r.shape, (name, g.shape, r.shape)
        mx = np.abs(r).max(axis=axes, keepdims=True)
        if r32 is None:
            bound = 2e-5 * mx
        else:
            floor = np.abs(np.asarray(r32, np.float64) - r).max(axis=axes, keepdims=True)
            bound = 4.0 * floor + ulp(mx)
            rel = np.where(mx > 0, floor / np.maximum(ulp(mx), 1e-300), 0.0)
            floors[kind] = max(floors.get(kind, 0.0), float(rel.max()))
        err = np.abs(g - r)
        ok = err <= bound                                        # NaN in got: False
        if not ok.all():
            i = np.unravel_index(np.argmax(np.where(ok, 0.0, np.where(np.isnan(err), np.inf, err))), err.shape)
            bad.append((name, f"{int((~ok).sum())} of {ok.size} elements", "worst at", tuple(int(v) for v in i), "got", float(g[i]), "ref", float(r[i]),
                        "bound", float(np.broadcast_to(bound, err.shape)[i])))

    for l, (g, r) in enumerate(zip(got, ref)):
        r32 = None if ref32 is None else ref32[l]
        s32 = {} if r32 is None else {n: a for n, a, _ in _slabs(r32, drop)}
        gs = {n: a for n, a, _ in _slabs(g, drop)}
        for name, a, axes in _slabs(r, drop):
            if only is None or name in only:
                cmp(f"{name}[{l}]", name, gs[name], a, s32.get(name), axes)
        if r.get("dG") is None or only is not None:
            continue
        for pk, wk in PRODUCTS:
            if r[wk] is None:
                assert g.get(pk) is None
                continue
            cmp(f"{pk}[{l}]", pk, g[pk], r[wk], None if r32 is None else r32[pk], tuple(range(np.ndim(r[wk]))))
    return bad, floors


# ------------------------------------------------------------------------------------------------ the cases
# (name, dtype, T, B, H, NL, layer-0 input, extras): the eleven cases of tests/test_gpu_lstm_kernels.py
CASES = {
    1: dict(dtname="f32", T=4, B=6, H=20, NL=2, add="step"),
    2: dict(dtname="f32", T=1, B=6, H=72, NL=1, add="step"),
    3: dict(dtname="f32", T=6, B=37, H=72, NL=3, add=None, table_rows=35),
    4: dict(dtname="f32", T=3, B=9, H=72, NL=4, add="const"),
    5: dict(dtname="f32", T=4, B=200, H=64, NL=2, add="step"),
    6: dict(dtname="bf16", T=9, B=6, H=32, NL=2, add="step"),
    7: dict(dtname="bf16", T=5, B=130, H=128, NL=3, add="step"),
    8: dict(dtname="bf16", T=4, B=256, H=128, NL=3, add="const"),
    9: dict(dtname="bf16", T=4, B=128, H=128, NL=3, add="step", drop_p=0.25, drop_seed=0x5EED1234),
    10: dict(dtname="bf16", T=1, B=9, H=64, NL=2, add="step"),
    11: dict(dtname="bf16", T=5, B=70, H=64, NL=2, add="const", table_rows=23),
}


def build_case(dtname, T, B, H, NL, seed=1, add="step", table_rows=0, bad_ids=False, dy=True, dy_a=False, drop_p=0.0, drop_seed=0):
    """Seeded inputs (float64 arrays holding values exact in the type the kernel reads them in) and the references.  The recipe keeps the
    gates off their rails so that a wrong slot, factor or carry changes the result: weights U(+-3 / sqrt(H)) rounded to the storage type,
    upper-layer bias sums U(+-1.5), a layer-0 addend N(0, 1) (a table + a time-invariant addend: N(0, 1/2) each), dy N(0, 1); asserted below
    for every layer: >= 90 % of i, f, o inside (0.02, 0.98) and of |g| below 0.98, and a standard deviation of the pre-activations of every
    (layer, step) of at least 0.5.
    dy_a: the output gradient (also) as a product dy_a [T, B, 35] . dy_w [H, 35]^T of storage-type operands.  bad_ids: some table ids below 0
    and at or above the number of rows (the kernels clamp them)."""
    bf16 = dtname == "bf16"
    q = bf16_round if bf16 else f32_round
    rs = np.random.RandomState(seed)
    a = 3.0 / np.sqrt(H)
    ps = []
    for l in range(NL):
        ps.append(dict(w_ih=q(rs.uniform(-a, a, (4 * H, H))) if l else None, w_hh=q(rs.uniform(-a, a, (4 * H, H))),
                       b=f32_round(rs.uniform(-1.5, 1.5, 4 * H)) if l else None))
    c = dict(bf16=bf16, T=T, B=B, H=H, NL=NL, ps=ps, drop_p=drop_p, drop_seed=drop_seed)
    both = 1.0 / np.sqrt(2.0) if (table_rows and add) else 1.0
    c["add_step"] = f32_round(both * rs.standard_normal((T, B, 4 * H))) if add == "step" else None
    c["add_const"] = f32_round(both * rs.standard_normal((B, 4 * H))) if add == "const" else None
    c["table"] = f32_round(both * rs.standard_normal((table_rows, 4 * H))) if table_rows else None
    c["index"] = rs.randint(0, table_rows, (B, T + 3)) if table_rows else None
    if bad_ids:
        c["index"][::5, ::2] = -1 - rs.randint(0, 3, c["index"][::5, ::2].shape)
        c["index"][1::7, 1::2] = table_rows + rs.randint(0, 3, c["index"][1::7, 1::2].shape)
        assert (c["index"][:, :T] < 0).any() and (c["index"][:, :T] >= table_rows).any()
    c["dy"] = f32_round(rs.standard_normal((T, B, H))) if dy else None
    dy_tot = c["dy"]
    c["dy_a"] = c["dy_w"] = None
    if dy_a:
        C = 35
        c["dy_a"], c["dy_w"] = q(rs.standard_normal((T, B, C))), q(rs.standard_normal((H, C)) / np.sqrt(C))
        prod = (c["dy_a"].reshape(T * B, C) @ c["dy_w"].T).reshape(T, B, H)
        c["dy_prod"] = prod
        dy_tot = prod if dy_tot is None else dy_tot + prod
    c["dy_tot"] = dy_tot
    c["mask"] = dropout_keep_mask(drop_seed, (NL - 1, T, B, H), drop_p) if drop_p > 0 else None
    kw = dict(add_step=c["add_step"], add_const=c["add_const"], table=c["table"], index=c["index"], dy=dy_tot, drop_mask=c["mask"], drop_p=drop_p)
    c["kw"] = kw
    if not bf16:
        c["ref"] = lstm_stack(ps, T, B, **kw)
        c["ref32"] = None
    else:
        c["ref"] = lstm_stack(ps, T, B, storage_round=bf16_round, **kw)
        c["ref32"] = lstm_stack(ps, T, B, storage_round=bf16_round, math_dtype=np.float32, **kw)
    c["conditions"] = input_conditions(c["ref"])
    for l, (unsat, sd) in enumerate(c["conditions"]):
        assert unsat >= 0.9 and sd >= 0.5, ("input conditions", l, unsat, sd)
    return c


def input_conditions(ref):
    """per layer: (the smaller of the fractions of i, f, o inside (0.02, 0.98) and of |g| below 0.98, the smallest standard deviation of the
    pre-activations over the (layer, step) slabs)."""
    out = []
    for o in ref:
        H = o["hs"].shape[2]
        g = o["gates"]
        ifo = np.concatenate([g[:, :, :2 * H], g[:, :, 3 * H:]], 2)
        unsat = min(float(((ifo > 0.02) & (ifo < 0.98)).mean()), float((np.abs(g[:, :, 2 * H:3 * H]) < 0.98).mean()))
        out.append((unsat, float(o["pre"].std(axis=(1, 2)).min())))
    return out
