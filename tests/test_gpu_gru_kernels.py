"""The GRU form of mvae_rnn_fwd / mvae_rnn_bwd called directly (ops.rnn_fwd / ops.rnn_bwd, cell = GRU) on seeded inputs, every tensor it
writes compared element by element with tests/gru_ref.py -- the kernel-level counterpart of `_lstm_case` for the cell that mosesvae.VAE and
models2d.VAE run on.  Thirteen cases chosen from the dispatcher (rnn_fwd_impl / rnn_bwd_impl in csrc/rnn.hip, rnn_gru_rowres_* in
csrc/rnn_rowres.hip; K-step ke = 32 elements for f32, 64 for bf16); each test says which branch it reaches.

What is compared, per layer: hs, the final fp32 state hstate[(T-1) & 1], the four saved gate slots, hdrop, the four dG slots, dh0, and the
host products dG^T . h_prev, dG^T . x_in and colsum(dG) against the reference's dW_hh, dW_ih, db_ih / db_hh.  No element is left out, with one
exception: the saved gate slots of rows whose sequence has finished -- the backward never reads them (the forward contracts a zero / kept
h_{t-1} there and discards the cell), so they are unspecified.
Exact parts: rows past a length are +0 in hs, hdrop and dG; pad columns stay zero; guard rows behind every buffer keep their sentinel; the
final state of a finished row is its state at its last valid step; a forward-only call and a second run are bit-identical; the hashed and
the injected dropout mask give bit-identical results.

Bounds (element-wise, never derived from what the kernel returns):
  f32   |got - ref| <= 2e-5 * max|ref| per (layer, time step) slab, ref = the float64 oracle form (what `_lstm_case` holds the f32 kernels to).
  bf16  ref = the bf16-STORAGE form of the reference in float64 math: same roundings at the same places, so the storage noise that the model
        tests' 3e-2 / 8e-2 bounds absorb is gone.  What is left is fp32 arithmetic (and fast exp / rcp) against float64, which now and then
        flips a bf16 rounding.  The test computes that floor on the CPU per case, tensor and (layer, step) slab as
            floor = max|ref(storage, float32 math) - ref(storage, float64 math)|
        and allows  4 * floor + one bf16 ulp of max|ref| in the slab.  The factor 4: the float32 reference sums K in numpy's order, the
        kernel in MFMA-tile order (and per K-segment), so the kernel's fp32 result is a different sample of the same rounding noise, not the
        same one; a flipped rounding upstream then propagates through up to T steps and the layers above.  A real error (wrong factor, slot,
        mask, carry) is of the order of the value itself, i.e. >= 100 ulp.
        Floors observed, as the largest slab's floor in bf16 ulps of that slab's maximum (CPU figures, printed by every test with `-s`),
        range over the bf16 cases 4-13:
            forward   hs, hdrop 0 .. 1.0;  saved gates r, z, n, W_hn h + b_hn 0 .. 1.0;  final fp32 state 0 .. 0.08
            backward  dG slots r 0 .. 1.0, z 0 .. 1.5, n 0 .. 1.0, n*r 0 .. 1.0;  dh0 0 .. 0.43
            products  dG^T . h_prev 0 .. 0.16, dG^T . x_in 0 .. 0.14, colsum(dG) 0 .. 0.16
        i.e. the backward's floor is the forward's: single flipped bf16 roundings (one ulp is 3.9e-3 of a value near 1), a slab of dG_z once
        with an element off by one and a half.  The smallest case (T=9, B=6) has floor 0 throughout: there the bound is the one ulp alone.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gru_ref as R                                  # noqa: E402
from molecular_vae_amd import ops, _lib as L         # noqa: E402

dev = torch.device("cuda")
SENT = 7.0
GUARD = 8
F32, BF16 = torch.float32, torch.bfloat16


def _t(a, dt=F32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)).astype(np.float32)).to(dev).to(dt)


def _q(a, dt):
    """numpy float64 array rounded to what a tensor of `dt` holds."""
    a = np.asarray(a, np.float64)
    return R.bf16_round(a) if dt == BF16 else a.astype(np.float32).astype(np.float64)


def _lengths(rs, T, B):
    """descending, include T and 1 (the header requires the order; pack_sequence semantics)."""
    if T == 1:
        return np.ones(B, np.int64)
    ln = np.sort(rs.randint(1, T + 1, B))[::-1].copy()
    ln[0], ln[-1] = T, 1
    return ln


@functools.lru_cache(maxsize=2)
def _case(dtname, T, B, H, NL, seed=1, in0=0, add=None, table=False, lens=True, h0=True, dy=True, dh_last=False, dy_a=False, drop_p=0.0,
          drop_seed=0):
    """Seeded inputs (float64 arrays holding values exact in the type the kernel reads them in) and the references.  Cached: the knob
    variants of one case share it."""
    dt = BF16 if dtname == "bf16" else F32
    rs = np.random.RandomState(seed)
    a = 1.0 / np.sqrt(H)
    ps = []
    for l in range(NL):
        n_in = in0 if l == 0 else H
        ps.append(dict(w_ih=_q(rs.uniform(-a, a, (3 * H, n_in)), dt) if (l > 0 or in0) else None, w_hh=_q(rs.uniform(-a, a, (3 * H, H)), dt),
                       b_ih=_q(rs.uniform(-a, a, 3 * H), F32), b_hh=_q(rs.uniform(-a, a, 3 * H), F32)))
    c = dict(dt=dt, T=T, B=B, H=H, NL=NL, in0=in0, ps=ps, drop_p=drop_p, drop_seed=drop_seed)
    c["lengths"] = _lengths(rs, T, B) if lens else None
    ln = c["lengths"] if lens else np.full(B, T)
    c["x0"] = _q(rs.standard_normal((T, B, in0)), dt) if in0 else None
    c["add_step"] = _q(0.5 * rs.standard_normal((T, B, 3 * H)), F32) if add == "step" else None
    c["add_const"] = _q(0.5 * rs.standard_normal((B, 3 * H)), F32) if add == "const" else None
    V = 23
    c["table"] = _q(0.5 * rs.standard_normal((V, 3 * H)), F32) if table else None
    c["index"] = rs.randint(0, V, (B, T + 3)) if table else None
    c["h0"] = [_q(rs.uniform(-0.8, 0.8, (B, H)), dt) for _ in range(NL)] if h0 else None
    c["dy"] = _q(rs.standard_normal((T, B, H)), F32) if dy else None
    c["dh_last"] = [_q(rs.standard_normal((B, H)), F32) for _ in range(NL)] if dh_last else None
    dy_tot = c["dy"]
    if dy_a:
        C = 35
        A = _q(0.3 * rs.standard_normal((T, B, C)), dt)
        A[np.arange(T)[:, None] >= ln[None, :]] = 0.0              # rows of finished sequences must be zero in dy_a (mvae.h)
        c["dy_a"], c["dy_w"] = A, _q(0.3 * rs.standard_normal((H, C)), dt)
        prod = (A.reshape(T * B, C) @ c["dy_w"].T).reshape(T, B, H)
        dy_tot = prod if dy_tot is None else dy_tot + prod
    c["mask"] = ops.dropout_keep_mask(drop_seed, (NL - 1, T, B, H), drop_p) if drop_p > 0 else None
    kw = dict(x0=c["x0"], add_step=c["add_step"], add_const=c["add_const"], table=c["table"], index=c["index"], h0=c["h0"], dy=dy_tot,
              dh_last=c["dh_last"], drop_mask=c["mask"], drop_p=drop_p)
    if dt == F32:
        c["ref"] = R.gru_stack(ps, c["lengths"], T, B, **kw)
        c["ref32"] = None
    else:
        c["ref"] = R.gru_stack(ps, c["lengths"], T, B, storage_round=R.bf16_round, **kw)
        c["ref32"] = R.gru_stack(ps, c["lengths"], T, B, storage_round=R.bf16_round, math_dtype=np.float32, **kw)
    # a saturated gate hides derivative errors: r and z must stay inside (0.02, 0.98) for at least 90 % of the valid elements
    valid = (np.arange(T)[:, None] < ln[None, :])
    for o in c["ref"]:
        rz = o["gates"][:, :, :2 * H][valid]
        assert ((rz > 0.02) & (rz < 0.98)).mean() >= 0.9
    return c


def _buf(rows, ld, cols, dt):
    """[rows + GUARD, ld]: NaN where the kernel must write, zero pad columns, a sentinel in the rows behind."""
    b = torch.zeros(rows + GUARD, ld, device=dev, dtype=dt)
    b[:rows, :cols] = float("nan")
    b[rows:] = SENT
    return b


def _padded(a, rows, ld, dt):
    out = torch.zeros(rows, ld, device=dev, dtype=dt)
    out[:a.shape[0], :a.shape[1]] = _t(a, dt)
    return out


def _run(c, gates=True, drop=None, zero_padded_k=False, ld=None, backward=True):
    """One forward (+ backward) call on fresh buffers.  drop: None / 'inject' (mask bytes) / 'hash' (seed).  ld = (ldh, ldw) override."""
    dt, T, B, H, NL, in0 = c["dt"], c["T"], c["B"], c["H"], c["NL"], c["in0"]
    TB, G4 = T * B, 4 * H
    H8 = (H + 7) // 8 * 8
    ldh, ldw = ld if ld else (H8 + 8, H8)
    ldh0, ldg = ldh, (G4 + 7) // 8 * 8 + 8
    before = dict(ops.PERSIST_STATS)
    ps = c["ps"]
    w_hh = [_padded(R.pack_w_hh(p["w_hh"]), G4, ldw, dt) for p in ps]
    w_ih = [(_padded(R.pack_w_ih(ps[0]["w_ih"]), G4, in0, dt) if in0 else None)] + [_padded(R.pack_w_ih(p["w_ih"]), G4, ldw, dt) for p in ps[1:]]
    ldw_ih = [in0 if in0 else ldw] + [ldw] * (NL - 1)
    bias = [_t(R.pack_bias(p["b_ih"], p["b_hh"])) for p in ps]
    h0 = [_padded(h, B, ldh0, dt) for h in c["h0"]] if c["h0"] is not None else None
    lengths = torch.from_numpy(c["lengths"].astype(np.int32)).to(dev) if c["lengths"] is not None else None
    x0 = _t(c["x0"].reshape(TB, in0), dt) if in0 else None
    add0, tstride = None, 0
    if c["add_step"] is not None:
        add0, tstride = _t(R.pack_addend(c["add_step"])), B * G4
    if c["add_const"] is not None:
        add0 = _t(R.pack_addend(c["add_const"]))
    table = _t(R.pack_addend(c["table"])) if c["table"] is not None else None
    index = torch.from_numpy(c["index"]).to(dev) if c["index"] is not None else None
    hs = [_buf(TB, ldh, H, dt) for _ in range(NL)]
    gt = [_buf(TB, G4, G4, dt) for _ in range(NL)] if gates else None
    cstate = [_buf(2 * B, H, H, F32) for _ in range(NL)]
    hdrop = mask_d = None
    if drop:
        hdrop = [_buf(TB, ldh, H, dt) for _ in range(NL - 1)] + [None]
        mask_d = [torch.from_numpy(c["mask"][l].copy()).to(dev) for l in range(NL - 1)] if drop == "inject" else None
    dkw = dict(drop_p=c["drop_p"], drop_seed=c["drop_seed"]) if drop else {}
    ops.rnn_fwd(L.CELL_GRU, dt, T, B, H, add0, tstride, w_ih, ldw_ih, w_hh, [ldw] * NL, bias, hs, ldh, None, gt, cstate, x0=x0, x0_ld=in0, in0=in0,
                h0=h0, ldh0=ldh0 if h0 else 0, lengths=lengths, zero_padded_k=zero_padded_k, hdrop=hdrop, drop_mask=mask_d,
                add_table=table, add_index=index, **dkw)
    out = dict(hs=hs, gates=gt, cstate=cstate, hdrop=hdrop, ldh=ldh, ldg=ldg)
    if backward and gates:
        w_hhT = [_t(R.pack_w_hh(p["w_hh"]).T, dt) for p in ps]
        w_ihT = [None] + [_t(R.pack_w_ih(p["w_ih"]).T, dt) for p in ps[1:]]
        dG = [_buf(TB, ldg, G4, dt) for _ in range(NL)]
        dstate = [_buf(2 * B, H, H, F32) for _ in range(NL)]
        dh0 = [_buf(B, H, H, F32) for _ in range(NL)] if c.get("want_dh0", True) else None
        dy = _t(c["dy"].reshape(TB, H)) if c["dy"] is not None else None
        dh_last = [_t(g) for g in c["dh_last"]] if c["dh_last"] is not None else None
        akw = {}
        if "dy_a" in c:
            dy_a = torch.zeros(TB + GUARD, 128, device=dev, dtype=dt); dy_a[:TB, :c["dy_a"].shape[2]] = _t(c["dy_a"].reshape(TB, -1), dt)
            dy_w = torch.zeros(H, 128, device=dev, dtype=dt); dy_w[:, :c["dy_w"].shape[1]] = _t(c["dy_w"], dt)
            akw = dict(dy_a=dy_a[:TB], dy_w=dy_w, dy_k=128)
        ops.rnn_bwd(L.CELL_GRU, dt, T, B, H, w_hhT, [G4] * NL, w_ihT, [G4] * NL, dy, H if dy is not None else 0, hs, ldh, None, gt, dG, dstate,
                    ldg=ldg, h0=h0, ldh0=ldh0 if h0 else 0, lengths=lengths, dh_last=dh_last, dh0=dh0, drop_mask=mask_d, **akw, **dkw)
        out.update(dG=dG, dstate=dstate, dh0=dh0)
    torch.cuda.synchronize()
    # the GRU form has no schedule with bounded spins: nothing may have been counted as one
    assert all(ops.PERSIST_STATS[k] == before[k] for k in ("launches", "rowres_pipe", "bwd_launches", "failures", "reruns"))
    return out


def _bits(x):
    return x.view(torch.int16 if x.dtype == BF16 else torch.int32)


def _same(a, b, keys):
    """bit-identical (NaNs and signed zeros included)."""
    for k in keys:
        if a.get(k) is None:
            assert b.get(k) is None
            continue
        for l, (x, y) in enumerate(zip(a[k], b[k])):
            if x is not None:
                assert torch.equal(_bits(x), _bits(y)), (k, l)


ALL_KEYS = ("hs", "hdrop", "gates", "cstate", "dG", "dstate", "dh0")


def _np(x):
    return x.double().cpu().numpy()


class _Report:
    def __init__(self, c):
        self.c, self.bad, self.floors = c, [], {}

    def cmp(self, name, got, ref, ref32, slab_axes):
        """element-wise |got - ref| <= bound, the bound taken per slab (the axes NOT in slab_axes index the slabs)."""
        mx = np.abs(ref).max(axis=slab_axes, keepdims=True) if ref.size else np.zeros(())
        if self.c["dt"] == F32:
            bound = 2e-5 * mx
        else:
            floor = np.abs(ref32.astype(np.float64) - ref).max(axis=slab_axes, keepdims=True) if ref.size else np.zeros(())
            bound = 4.0 * floor + np.vectorize(R.bf16_ulp)(mx)
            kind = name.rstrip("0123456789").split("[")[0]
            if floor.size:
                with np.errstate(divide="ignore", invalid="ignore"):
                    rel = np.where(mx > 0, floor / np.vectorize(R.bf16_ulp)(np.maximum(mx, 1e-300)), 0.0)
                self.floors[kind] = max(self.floors.get(kind, 0.0), float(rel.max()))
        err = np.abs(got - ref)
        ok = err <= bound                                        # NaN in got: False
        if not ok.all():
            i = np.unravel_index(np.argmax(np.where(ok, 0.0, np.where(np.isnan(err), np.inf, err))), err.shape)
            self.bad.append((name, f"{int((~ok).sum())} of {ok.size} elements", "worst at", tuple(int(v) for v in i), "got", float(got[i]), "ref", float(ref[i]),
                             "bound", float(np.broadcast_to(bound, err.shape)[i])))


def _check(c, o, drop=False):
    dt, T, B, H, NL = c["dt"], c["T"], c["B"], c["H"], c["NL"]
    TB, G4, ldh, ldg = T * B, 4 * H, o["ldh"], o["ldg"]
    ref, ref32 = c["ref"], c["ref32"] or [None] * NL
    ln = c["lengths"] if c["lengths"] is not None else np.full(B, T)
    valid = np.arange(T)[:, None] < ln[None, :]                   # [T, B]
    rep = _Report(c)
    g32 = lambda r, k: None if r is None or r[k] is None else r[k]
    x_got = c["x0"]
    for l in range(NL):
        r, r32 = ref[l], ref32[l]
        # ---- pads, guards, finished rows: exact
        for key, cols in (("hs", H), ("hdrop", H), ("dG", G4)):
            if o.get(key) is None or o[key][l] is None:
                continue
            buf = o[key][l]
            assert float(buf[:TB, cols:].abs().sum()) == 0.0, (key, l, "pad columns must stay zero")
            assert bool((buf[TB:] == SENT).all()), (key, l, "rows behind the buffer were written")
            fin = _bits(buf)[:TB, :cols].reshape(T, B, cols)[torch.from_numpy(~valid).to(dev)]
            assert bool((fin == 0).all()), (key, l, "rows past a sequence's length must be +0")
        for key in ("gates", "cstate", "dstate", "dh0"):
            if o.get(key) is not None and o[key][l] is not None:
                assert bool((o[key][l][-GUARD:] == SENT).all()), (key, l, "rows behind the buffer were written")
        hs = _np(o["hs"][l][:TB, :H]).reshape(T, B, H)
        rep.cmp(f"hs{l}", hs, r["y"], g32(r32, "y"), (1, 2))
        hfin_t = o["cstate"][l][((T - 1) & 1) * B:((T - 1) & 1) * B + B]
        rep.cmp(f"hstate{l}", _np(hfin_t), r["h_last"], g32(r32, "h_last"), (0, 1))
        # the final state of a row is its state at its last valid step: hs there is that state, rounded to the storage type
        last = o["hs"][l][:TB, :H].reshape(T, B, H)[torch.from_numpy(ln - 1).to(dev), torch.arange(B, device=dev)]
        assert torch.equal(_bits(hfin_t.to(dt).contiguous()), _bits(last.contiguous())), (l, "final state != state at the last valid step")
        if o["gates"] is not None:
            g = _np(o["gates"][l][:TB]).reshape(T, B, G4)
            for k, nm in enumerate(("r", "z", "n", "hn")):      # finished rows are skipped: the backward never reads their saved gates
                sl = slice(k * H, (k + 1) * H)
                vm = valid[:, :, None]
                rep.cmp(f"gate_{nm}{l}", np.where(vm, g[:, :, sl], 0.0), np.where(vm, r["gates"][:, :, sl], 0.0),
                        None if r32 is None else np.where(vm, r32["gates"][:, :, sl], 0.0), (1, 2))
        hd = None
        if drop and l + 1 < NL:
            hd = _np(o["hdrop"][l][:TB, :H]).reshape(T, B, H)
            rep.cmp(f"hdrop{l}", hd, r["hdrop"], g32(r32, "hdrop"), (1, 2))
        if o.get("dG") is not None:
            dG = _np(o["dG"][l][:TB, :G4]).reshape(T, B, G4)
            for k, nm in enumerate(("r", "z", "n", "nr")):
                sl = slice(k * H, (k + 1) * H)
                rep.cmp(f"dG_{nm}{l}", dG[:, :, sl], r["dG"][:, :, sl], None if r32 is None else r32["dG"][:, :, sl], (1, 2))
            if o["dh0"] is not None:
                rep.cmp(f"dh0_{l}", _np(o["dh0"][l][:B]), r["dh0"], g32(r32, "dh0"), (0, 1))
            # host products from the kernel's own tensors, as the models' weight-gradient GEMMs form them
            d2 = dG.reshape(TB, G4)
            h0l = c["h0"][l] if c["h0"] is not None else np.zeros((B, H))
            hprev = np.concatenate([h0l[None], hs[:-1]], 0).reshape(TB, H)
            rep.cmp(f"dWhh{l}", R.unslot_hh(d2.T @ hprev), r["dW_hh"], g32(r32, "dW_hh"), (0, 1))
            rep.cmp(f"db_ih{l}", R.unslot_ih(d2.sum(0)), r["db_ih"], g32(r32, "db_ih"), (0,))
            rep.cmp(f"db_hh{l}", R.unslot_hh(d2.sum(0)), r["db_hh"], g32(r32, "db_hh"), (0,))
            if x_got is not None:
                rep.cmp(f"dWih{l}", R.unslot_ih(d2.T @ x_got.reshape(TB, -1)), r["dW_ih"], g32(r32, "dW_ih"), (0, 1))
        x_got = hd if hd is not None else hs
    if rep.floors:
        print(f"\n[gru floors, in bf16 ulps of the slab maximum] T={T} B={B} H={H} NL={NL}: " + ", ".join(f"{k}={v:.2f}" for k, v in sorted(rep.floors.items())))
    assert not rep.bad, rep.bad
    return rep


def _gru_case(c, drop=None, twice=True, **kw):
    """Run, compare everything with the reference; a second run on fresh buffers must reproduce the first bit for bit."""
    o = _run(c, drop=drop, **kw)
    _check(c, o, drop=bool(drop))
    if twice:
        _same(o, _run(c, drop=drop, **kw), ALL_KEYS)
    return o


# ------------------------------------------------------------------------------------------------ the cases
def test_case01_f32_input_sequence_ragged_lengths_generic_tiles():
    """f32, T=4 B=6 H=20 NL=2, layer 0 a REAL sequence x0 (in0 = 8) through w_ih[0], h0 given, ragged lengths (cases 1 and 4-8 also pass a
    dh_last: it is the only gradient a finished row carries, so without it a lost carry would go unseen).  Forward: H % 32 != 0 -> no
    LDS-direct pipe, H % 8 != 0 -> scalar epilogue; backward: 32 x 32 tiles (small f32 stack), 4H % 32 != 0 -> generic loop, gru3 off."""
    T, B, H, NL = 4, 6, 20, 2
    assert H % 32 and H % 8 and (4 * H) % 32 and (B + 63) // 64 * ((H + 63) // 64) * NL < 256
    _gru_case(_case("f32", T, B, H, NL, seed=1, in0=8, dh_last=True))


def test_case02_f32_pipelined_addend_per_step_dh_last_and_dy():
    """f32, T=5 B=200 H=64 NL=2, a per-step addend, no lengths, dh_last + dy.  H % 32 == 0 and 4H % 32 == 0: both passes pipelined, vector
    epilogues, the zero gate-slot block skipped as a K hole (gru3 on)."""
    T, B, H, NL = 5, 200, 64, 2
    assert H % 32 == 0 and H % 8 == 0
    _gru_case(_case("f32", T, B, H, NL, seed=2, add="step", lens=False, h0=False, dh_last=True))


def test_case03_f32_single_step_single_layer_dh0():
    """f32, T=1 B=9 H=64 NL=1: the t = -1 pseudo-cell that produces dh0 runs right behind the only step (carry of t = 0 in dstate[0])."""
    _gru_case(_case("f32", 1, 9, 64, 1, seed=3, add="const"))


@pytest.mark.parametrize("H", [96, 192])
def test_case04_05_bf16_ragged_batch_pipe_without_and_with_k_hole(H):
    """bf16, T=6 B=130 NL=3, lengths, h0, dh0.  4H % 64 == 0: pipelined backward.  H = 96: H % 64 != 0 -> gru3 OFF with the pipe on (the whole
    4H contraction incl. the zero slot; forward: generic loop); H = 192: gru3 on, the K hole in both passes' pipelined loops."""
    assert (4 * H) % 64 == 0 and (H % 64 == 0) == (H == 192)
    _gru_case(_case("bf16", 6, 130, H, 3, seed=4 + H, add="step", dh_last=True))


@pytest.mark.parametrize("zpk", [True, False], ids=["zero_padded_k", "plain"])
def test_case06_bf16_padded_k_pipe_against_generic_loop(zpk):
    """bf16, T=4 B=37 H=72 NL=2, ldh = ldh0 = ldw = 128 with zero pads.  zero_padded_k: the forward contracts whole K-steps over the pads
    (LDS-direct pipe); without it the generic loop over K = 72 -- same reference, same bounds.  Backward (both): 4H % 64 != 0 -> generic
    loop with the vector epilogue."""
    assert 72 % 64 and (4 * 72) % 64 and 72 % 8 == 0
    _gru_case(_case("bf16", 4, 37, 72, 2, seed=6, add="step", dh_last=True), zero_padded_k=zpk, ld=(128, 128))


@pytest.mark.parametrize("split", ["0", "1", "2", "1284", "644", "2562", "1281", "641", "2561"])
def test_case07_bf16_every_backward_schedule(split, monkeypatch):
    """bf16, T=5 B=256 H=128 NL=3, lengths, h0, dh0, dy: fused 64 x 64 (0), the default choice (1), segment split (2, 2562), half-segment
    split (1284, 644) with the element-wise second launch, the unsplit wave-specialised tiles (1281, 641, 2561) -- each with the t = -1
    pseudo-cell under the same schedule."""
    monkeypatch.setenv("MVAE_BWD_SPLIT", split)
    _gru_case(_case("bf16", 5, 256, 128, 3, seed=7, add="step", dh_last=True))


@pytest.mark.parametrize("split", ["1", "2", "1284", "1281"])
def test_case08_bf16_dropout_factor_in_each_backward_form(split, monkeypatch):
    """Case 7 + inter-layer dropout p = 0.2: the factor in the forward's hdrop, in the fused backward tile, in the split schedules'
    element-wise launch; 1281 (an instantiation without the factor) must fall back to one that has it.  The mask derived on the device from
    the seed and the same mask injected as bytes give bit-identical results."""
    monkeypatch.setenv("MVAE_BWD_SPLIT", split)
    c = _case("bf16", 5, 256, 128, 3, seed=7, add="step", dh_last=True, drop_p=0.2, drop_seed=0x5EED1234)
    keep = c["mask"].mean()
    assert 0.75 < keep < 0.85
    a = _gru_case(c, drop="inject")
    b = _gru_case(c, drop="hash", twice=False)
    _same(a, b, ALL_KEYS)


@pytest.mark.parametrize("with_dy", [False, True], ids=["product", "product+dy"])
def test_case09_bf16_output_gradient_as_a_product(with_dy):
    """Case 7's shape with the output gradient as dy_a . dy_w^T (dy_k = 128, rows of finished sequences zero), alone and added to a dy
    tensor: the top cell's second K-segment is contracted in full (seg1_full: no GRU zero block there)."""
    _gru_case(_case("bf16", 5, 256, 128, 3, seed=9, add="step", dy=with_dy, dy_a=True))


@pytest.mark.parametrize("env", [{"MVAE_BJ": "64"}, {"MVAE_BM": "128", "MVAE_NBUF_FWD": "4", "MVAE_NBUF_BWD": "5"},
                                 {"MVAE_BM": "64", "MVAE_NBUF_FWD": "5", "MVAE_NBUF_BWD": "3"}, {"MVAE_BM": "64", "MVAE_NBUF_FWD": "2"}],
                         ids=["BJ64", "BM128-ring4-5", "BM64-ring5-3", "BM64-ring2"])
def test_case10_bf16_forward_tile_and_ring_variants(env, monkeypatch):
    """bf16, T=4 B=200 H=192 NL=3: the tile / ring-depth variants of test_lstm_tile_variants_vs_oracle that exist for the GRU branch (only
    instantiated ring depths: the FWD_CASE / BWD_CASE lists), incl. the wave-specialised 128 x (64 x 4) tile and the 2-deep ring the bench
    shape picks."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _gru_case(_case("bf16", 4, 200, 192, 3, seed=10, add="step"))


def _rowres_case(B, dy):
    c = dict(_case("bf16", 9, B, 256, 1, seed=11 + B, table=True, dy=dy, dh_last=True))
    c["want_dh0"] = False                 # the row-resident backward serves calls without dh0 (the MOSES encoder's)
    return c


@pytest.mark.parametrize("variant", ["default", "safe", "forward_only"])
def test_case11_bf16_row_resident_gru256(variant, monkeypatch):
    """bf16, T=9 B=64 H=256 NL=1, token table only, lengths, dh_last only: gru_rowres_fwd_kernel / gru_rowres_bwd_kernel (one launch per
    pass), also with full waits (MVAE_GRU_ROWRES_SAFE=1) and as a forward-only call.  Proof of the branch: that schedule keeps the state
    and the carried gradient in registers -- it writes one half of hstate and nothing of dstate."""
    if variant == "safe":
        monkeypatch.setenv("MVAE_GRU_ROWRES_SAFE", "1")
    c = _rowres_case(64, dy=False)
    B = 64
    o = _gru_case(c)
    assert bool(torch.isnan(o["cstate"][0][((9 - 2) & 1) * B:((9 - 2) & 1) * B + B]).all()) and bool(torch.isnan(o["dstate"][0][:2 * B]).all())
    if variant == "forward_only":
        f = _run(c, gates=False)
        _same(o, f, ("hs", "cstate"))


@pytest.mark.parametrize("variant", ["B6", "dy"])
def test_case12_bf16_gru256_falls_back_to_the_wavefront(variant):
    """Case 11's shape where the row-resident schedule does not serve: B % 4 != 0 (both passes), and a gradient on the output sequence
    (backward only).  The wavefront schedule writes both halves of its ping-pong state."""
    B = 6 if variant == "B6" else 64
    c = _rowres_case(B, dy=(variant == "dy"))
    o = _gru_case(c)
    assert not bool(torch.isnan(o["dstate"][0][:2 * B]).any())
    assert bool(torch.isnan(o["cstate"][0][:2 * B]).any()) == (variant == "dy")


def test_case13_bf16_moses_decoder_call():
    """bf16, T=3 B=512 H=512 NL=3: token table + time-invariant addend + h0 + lengths + dh0, the output gradient as a product -- the MOSES
    decoder's call at the schedules the default dispatch picks at that batch."""
    _gru_case(_case("bf16", 3, 512, 512, 3, seed=13, add="const", table=True, dy=False, dy_a=True))
