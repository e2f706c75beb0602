"""The LSTM form of mvae_rnn_fwd / mvae_rnn_bwd called directly (ops.rnn_fwd / ops.rnn_bwd, cell = LSTM) on seeded inputs, every tensor it
writes compared element by element with tests/lstm_ref.py -- the LSTM counterpart of test_gpu_gru_kernels.py.  Eleven cases chosen from the
dispatcher (rnn_fwd_impl / rnn_bwd_impl in csrc/rnn.hip, rnn_rowres_fwd / rnn_rowres_bwd in csrc/rnn_rowres.hip; K-step ke = 32 elements for
f32, 64 for bf16); each test says which branch it reaches.  The inputs follow lstm_ref.build_case's recipe, which keeps the gates of every
layer off their rails (asserted there and, without a GPU, in test_lstm_ref_host.py).

What is compared, per layer: hs, cs, the four saved gate slots, hdrop where there is dropout, the four dG slots, and the host products
dG^T . h_prev, dG^T . x_in and colsum(dG) against the reference's dW_hh, dW_ih and db.  No element is left out.
Exact parts: pad columns of hs, hdrop and dG are +0; guard rows behind every buffer keep their sentinel; a second run into fresh buffers is
bit-identical; a forward-only call gives the training call's hs bit for bit where both take the same kernel; the hashed and the injected
dropout mask give bit-identical results; h0 / dh_last / dh0 with the LSTM cell are refused before anything is written.

Bounds (lstm_ref.check_slabs; element-wise, never derived from what the kernel returns -- the ones test_gpu_gru_kernels.py established):
  f32   |got - ref| <= 2e-5 * max|ref| per (layer, time step) slab, ref = the float64 oracle form.
  bf16  ref = the bf16-STORAGE form of the reference in float64 math: same roundings at the same places.  What is left is fp32 arithmetic
        (and fast exp / rcp) against float64, which now and then flips a bf16 rounding.  That floor is computed on the CPU per case, tensor
        and (layer, step) slab as
            floor = max|ref(storage, float32 math) - ref(storage, float64 math)|
        and the kernel is allowed  4 * floor + one bf16 ulp of max|ref| in the slab.  The factor 4 (the GRU test's argument, which holds
        here unchanged): the float32 reference sums K in numpy's order, the kernel in MFMA-tile order (and per K-segment), so the kernel's
        fp32 result is a different sample of the same rounding noise, not the same one; a flipped rounding upstream then propagates through
        up to T steps and the layers above.  A real error (wrong factor, slot, carry) is of the order of the value itself, i.e. >= 100 ulp;
        test_lstm_ref_host.py shows every such mutant rejected.
        Floors observed, as the largest slab's floor in bf16 ulps of that slab's maximum (CPU figures: they come from the two CPU references
        alone and are printed by every bf16 test with `-s`), range over the bf16 cases 6-11 and their dy / dy_a / dropout variants:
            forward   hs 0 .. 1.0;  cs 0 .. 1.0;  saved gates i, f, g, o 0 .. 1.0;  hdrop (case 9) 0.5
            backward  dG slots i 0 .. 1.0, f 0 .. 1.0, g 0 .. 1.0, o 0 .. 1.0
            products  dG^T . h_prev 0 .. 0.22, dG^T . x_in 0 .. 0.10, colsum(dG) 0 .. 0.16
        i.e. single flipped bf16 roundings (0.5: a flip below the slab's top binade); the small cases 6 (B = 6) and 10 (T = 1) have floor 0
        throughout: there the bound is the one ulp alone.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lstm_ref as R                                 # noqa: E402
from molecular_vae_amd import ops, _lib as L         # noqa: E402

dev = torch.device("cuda")
SENT = 7.0
GUARD = 8
F32, BF16 = torch.float32, torch.bfloat16


def _t(a, dt=F32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)).astype(np.float32)).to(dev).to(dt)


@functools.lru_cache(maxsize=3)
def _case(n, **over):
    """lstm_ref.build_case of case n (cached: the knob variants of one case share the references, which stay unchanged)."""
    return R.build_case(**dict(R.CASES[n], seed=n, **over))


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


def _run(c, drop=None, persist=None, Hp=None, backward=True, save=True, sink=None, **refuse):
    """One forward (+ backward) call on fresh buffers.  drop: None / 'inject' (mask bytes) / 'hash' (seed).  Hp: ldh = ldw = Hp with zero
    pads and zero_padded_k (else ldh = H + 8, ldw = H as `_lstm_case` has them); ldg = 4H + 8.  save=False: the forward-only call.
    persist: the schedules with bounded spins (True: required in the forward; None: where served; False: never).  refuse: h0 / dh_last / dh0
    lists handed through (the calls must fail; `sink` then receives the buffers the failed call was given)."""
    dt = BF16 if c["bf16"] else F32
    T, B, H, NL = c["T"], c["B"], c["H"], c["NL"]
    TB, G4 = T * B, 4 * H
    ldh, ldw, ldg = (Hp, Hp, G4 + 8) if Hp else (H + 8, H, G4 + 8)
    ps = c["ps"]
    w_hh = [_padded(p["w_hh"], G4, ldw, dt) for p in ps]
    w_ih = [None] + [_padded(p["w_ih"], G4, ldw, dt) for p in ps[1:]]
    bias = [None] + [_t(p["b"]) for p in ps[1:]]
    add0, tstride = None, 0
    if c["add_step"] is not None:
        add0, tstride = _t(c["add_step"]), B * G4
    if c["add_const"] is not None:
        add0 = _t(c["add_const"])
    table = _t(c["table"]) if c["table"] is not None else None
    index = torch.from_numpy(c["index"]).to(dev) if c["index"] is not None else None
    hs = [_buf(TB, ldh, H, dt) for _ in range(NL)]
    cs = [_buf(TB, H, H, dt) for _ in range(NL)] if save else None
    gt = [_buf(TB, G4, G4, dt) for _ in range(NL)] if save else None
    spare = torch.full((TB, G4), SENT, device=dev, dtype=dt)          # a forward-only call has no gates buffer: nothing may land in this one
    cstate = [_buf(2 * B, H, H, F32) for _ in range(NL)]
    hdrop = mask_d = None
    if drop:
        hdrop = [_buf(TB, ldh, H, dt) for _ in range(NL - 1)] + [None]
        mask_d = [torch.from_numpy(c["mask"][l].copy()).to(dev) for l in range(NL - 1)] if drop == "inject" else None
    dkw = dict(drop_p=c["drop_p"], drop_seed=c["drop_seed"]) if drop else {}
    before = dict(ops.PERSIST_STATS)
    out = sink if sink is not None else {}
    out.update(hs=hs, cs=cs, gates=gt, cstate=cstate, hdrop=hdrop, ldh=ldh, ldg=ldg, spare=spare)
    ops.rnn_fwd(L.CELL_LSTM, dt, T, B, H, add0, tstride, w_ih, [ldw] * NL, w_hh, [ldw] * NL, bias, hs, ldh, cs, gt, cstate, zero_padded_k=bool(Hp),
                hdrop=hdrop, drop_mask=mask_d, add_table=table, add_index=index, persist=persist, h0=refuse.get("h0"), ldh0=ldh if refuse.get("h0") else 0, **dkw)
    if backward and save:
        w_hhT = [_t(p["w_hh"].T, dt) for p in ps]
        w_ihT = [None] + [_t(p["w_ih"].T, dt) for p in ps[1:]]
        dG = [_buf(TB, ldg, G4, dt) for _ in range(NL)]
        dstate = [_buf(2 * B, H, H, F32) for _ in range(NL)]
        dy = _t(c["dy"].reshape(TB, H)) if c["dy"] is not None else None
        akw = {}
        if c["dy_a"] is not None:
            dy_a = torch.zeros(TB + GUARD, 128, device=dev, dtype=dt); dy_a[:TB, :c["dy_a"].shape[2]] = _t(c["dy_a"].reshape(TB, -1), dt)
            dy_w = torch.zeros(H, 128, device=dev, dtype=dt); dy_w[:, :c["dy_w"].shape[1]] = _t(c["dy_w"], dt)
            akw = dict(dy_a=dy_a[:TB], dy_w=dy_w, dy_k=128)
        out.update(dG=dG, dstate=dstate)
        ops.rnn_bwd(L.CELL_LSTM, dt, T, B, H, w_hhT, [G4] * NL, w_ihT, [G4] * NL, dy, H if dy is not None else 0, hs, ldh, cs, gt, dG, dstate, ldg=ldg,
                    drop_mask=mask_d, persist=(False if persist is False else None), dh_last=refuse.get("dh_last"), dh0=refuse.get("dh0"), **akw, **dkw)
    torch.cuda.synchronize()
    out["rowres_pipe"] = ops.PERSIST_STATS["rowres_pipe"] - before["rowres_pipe"]
    # bf16 LSTM stacks of these sizes are not served by the weights-resident passes, and nothing may have given up
    assert all(ops.PERSIST_STATS[k] == before[k] for k in ("launches", "bwd_launches"))
    return out


def _bits(x):
    return x.view(torch.int16 if x.dtype == BF16 else torch.int32)


ALL_KEYS = ("hs", "cs", "gates", "hdrop", "dG", "cstate", "dstate")


def _same(a, b, keys=ALL_KEYS):
    """bit-identical (NaNs and signed zeros included)."""
    for k in keys:
        if a.get(k) is None:
            assert b.get(k) is None
            continue
        for l, (x, y) in enumerate(zip(a[k], b[k])):
            if x is not None:
                assert torch.equal(_bits(x), _bits(y)), (k, l)


def _np(x):
    return x.double().cpu().numpy()


def _exact(c, o):
    """pads are +0, guard rows keep their sentinel."""
    T, B, H, NL = c["T"], c["B"], c["H"], c["NL"]
    TB, G4 = T * B, 4 * H
    for l in range(NL):
        for key, cols in (("hs", H), ("hdrop", H), ("dG", G4)):
            if o.get(key) is None or o[key][l] is None:
                continue
            buf = o[key][l]
            assert bool((_bits(buf)[:TB, cols:] == 0).all()), (key, l, "pad columns must stay +0")
        for key in ALL_KEYS:
            if o.get(key) is not None and o[key][l] is not None:
                assert bool((o[key][l][-GUARD:] == SENT).all()), (key, l, "rows behind the buffer were written")
    assert bool((o["spare"] == SENT).all())


def _got(c, o, drop):
    """the kernel's tensors in lstm_stack's layout, with the host products formed from them."""
    T, B, H, NL = c["T"], c["B"], c["H"], c["NL"]
    TB, G4 = T * B, 4 * H
    got, x_in = [], None
    for l in range(NL):
        g = dict(hs=_np(o["hs"][l][:TB, :H]).reshape(T, B, H), hdrop=None)
        if o["cs"] is not None:
            g.update(cs=_np(o["cs"][l][:TB]).reshape(T, B, H), gates=_np(o["gates"][l][:TB]).reshape(T, B, G4))
        if drop and l + 1 < NL:
            g["hdrop"] = _np(o["hdrop"][l][:TB, :H]).reshape(T, B, H)
        if o.get("dG") is not None:
            g["dG"] = _np(o["dG"][l][:TB, :G4]).reshape(T, B, G4)
            g.update(R.host_products(g["dG"], g["hs"], x_in))
        got.append(g)
        x_in = g["hdrop"] if g["hdrop"] is not None else g["hs"]
    return got


def _check(c, o, drop=False, only=None):
    _exact(c, o)
    bad, floors = R.check_slabs(_got(c, o, drop), c["ref"], c["ref32"], drop=drop, only=only)
    if floors:
        print(f"\n[lstm floors, in bf16 ulps of the slab maximum] T={c['T']} B={c['B']} H={c['H']} NL={c['NL']}: "
              + ", ".join(f"{k}={v:.2f}" for k, v in sorted(floors.items())))
    assert not bad, bad


def _lstm(c, drop=None, twice=True, fwd_only=None, **kw):
    """Run, compare everything with the reference; a second run on fresh buffers must reproduce the first bit for bit.  fwd_only: also the
    forward-only call -- 'same' = its hs equals the training call's bit for bit (same kernel, save stores skipped), 'ref' = its hs is held to
    the reference (it takes another schedule than the training call)."""
    o = _run(c, drop=drop, **kw)
    _check(c, o, drop=bool(drop))
    if twice:
        _same(o, _run(c, drop=drop, **kw))
    if fwd_only:
        f = _run(c, drop=drop, save=False, **kw)
        if fwd_only == "same":
            _exact(c, f)
            _same(o, f, ("hs", "hdrop"))
        else:
            _check(c, f, only=("hs",))
    return o


def _env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------------------------------------ the cases
def test_case01_f32_odd_width_generic_loops():
    """f32, T=4 B=6 H=20 NL=2, addend per step.  Forward: H % 32 != 0 -> no LDS-direct pipe (lstm_step_fwd_kernel<float, 32, 32, 0>), H % 8
    != 0 -> element-wise epilogue (partial 8-unit groups); backward: small f32 stack -> 32 x 32 tile, 4H % 32 != 0 -> generic loop
    (lstm_step_bwd_kernel<float, 32, 32, 0>).  The forward-only call takes the same kernel."""
    H = 20
    assert H % 32 and H % 8 and (4 * H) % 32
    _lstm(_case(1), fwd_only="same")


def test_case02_f32_row_resident_single_layer_single_step():
    """f32, T=1 B=6 H=72 NL=1: rnn_rowres_fwd layer by layer (one layer: lstm_rowres_fwd_kernel<72, false, 320>), rnn_rowres_bwd as
    lstm_rowres_bwd_all_kernel with nl = 1 (no dx, no scratch), ragged 4-row group (B = 6).  Proof of the branch: the row-resident
    schedule keeps c in registers and never writes cstate / dstate."""
    o = _lstm(_case(2))
    assert bool(torch.isnan(o["cstate"][0][:12]).all()) and bool(torch.isnan(o["dstate"][0][:12]).all())


@pytest.mark.parametrize("variant", ["default", "layerwise", "hoisted", "persist", "bad_ids", "rows65", "forward_only"])
def test_case03_f32_row_resident_token_table(variant, monkeypatch):
    """f32, T=6 B=37 H=72 NL=3, layer 0 = a 35-row table + ids, ldh = ldw = 96 with zero pads (zero_padded_k), ragged last 4-row group.
      default / persist   the layer-concurrent forms where they are served (lstm_rowres_fwd_pipe_kernel<72, true>, lstm_rowres_bwd_pipe_kernel),
                          persist: the forward REQUIRED to take it -- PERSIST_STATS['rowres_pipe'] grows
      layerwise / hoisted MVAE_ROWRES_PIPE=0 with MVAE_ROWRES_HOIST=0 / 1: lstm_rowres_fwd_kernel<72, false, 320, true> for layer 0, upper
                          layers contracting [x | h] per step / taking the hoisted x . W_ih^T GEMM as their addend; lstm_rowres_bwd_all_kernel
      bad_ids             ids below 0 and >= 35: clamped to the table
      rows65              a table over RR_TBL_ROWS = 64: the forward falls to the wavefront schedule (padded-K LDS-direct f32 loop,
                          lstm_step_fwd_kernel<float, 32, 32, 4>, table rows added in the vector epilogue); the backward stays row-resident
      forward_only        no save buffers: the wavefront schedule again -- its hs is held to the reference (another schedule than the
                          training call's, so not bit-identical to it)"""
    over = {"bad_ids": dict(bad_ids=True), "rows65": dict(table_rows=65)}.get(variant, {})
    c = _case(3, **over)
    if variant in ("layerwise", "hoisted"):
        _env(monkeypatch, {"MVAE_ROWRES_PIPE": "0", "MVAE_ROWRES_HOIST": "0" if variant == "layerwise" else "1"})
    o = _lstm(c, Hp=96, persist=True if variant == "persist" else None, fwd_only="ref" if variant == "forward_only" else None)
    if variant == "persist":
        assert o["rowres_pipe"] >= 1
    if variant in ("layerwise", "hoisted"):
        assert o["rowres_pipe"] == 0
    written = not bool(torch.isnan(o["cstate"][0][:2 * c["B"]]).any())
    assert written == (variant == "rows65")          # only the wavefront forward keeps the cell state in cstate


@pytest.mark.parametrize("persist", [False, True], ids=["layer_by_layer", "persist"])
def test_case04_f32_four_layer_row_resident_stack(persist):
    """f32, T=3 B=9 H=72 NL=4, a time-invariant addend (tstride 0).  Forward: layer by layer with the hoisted projection (persist False) or
    lstm_rowres_fwd_pipe_kernel<72, false> over 4 x 3 workgroups (persist True: required, PERSIST_STATS['rowres_pipe'] grows).  Backward:
    NL > 3 keeps it off the layer-concurrent form -- lstm_rowres_bwd_all_kernel, layer 1 reusing the dx buffer layer 3 wrote."""
    o = _lstm(_case(4), persist=persist)
    assert o["rowres_pipe"] == (1 if persist else 0)        # the forward only: the backward never reports a status record at NL = 4


@pytest.mark.parametrize("nbuf", ["4", "0"])
@pytest.mark.parametrize("bm", [None, "64", "128"])
def test_case05_f32_mfma_lds_direct_loop(bm, nbuf, monkeypatch):
    """f32, T=4 B=200 H=64 NL=2: H % 32 == 0 -> the f32 MFMA LDS-direct forward loop (ring of 4) or the register-staged one
    (MVAE_NBUF_FWD=0) on 32- (default at this size), 64- and 128-row tiles with a ragged last tile: lstm_step_fwd_kernel<float, BM, 32,
    4 | 0>; backward lstm_step_bwd_kernel<float, 32, 32, 4> / <float, 64 | 128, 64, 4>."""
    _env(monkeypatch, dict({"MVAE_NBUF_FWD": nbuf}, **({"MVAE_BM": bm} if bm else {})))
    _lstm(_case(5), fwd_only="same" if bm is None else None)


def test_case06_bf16_register_staged_forward_pipelined_backward():
    """bf16, T=9 B=6 H=32 NL=2: H % 64 != 0 -> lstm_step_fwd_kernel<bf16, 64, 32, 0> (generic loop, vector epilogue); 4H % 64 == 0 ->
    lstm_step_bwd_kernel<bf16, 64, 64, 4> (pipelined)."""
    assert 32 % 64 and (4 * 32) % 64 == 0
    _lstm(_case(6), fwd_only="same")


CASE7_ENVS = {"default": {}, "BJ64": {"MVAE_BJ": "64"}, "BM128-ring4-5": {"MVAE_BM": "128", "MVAE_NBUF_FWD": "4", "MVAE_NBUF_BWD": "5"},
              "BM64-ring5-3": {"MVAE_BM": "64", "MVAE_BJ": "32", "MVAE_NBUF_FWD": "5", "MVAE_NBUF_BWD": "3"},
              "BM64-ring2-noGM": {"MVAE_BM": "64", "MVAE_BJ": "32", "MVAE_NBUF_FWD": "2", "MVAE_FWD_GM": "0"},
              "fwd-ring0": {"MVAE_NBUF_FWD": "0"}, "bwd-ring0": {"MVAE_NBUF_BWD": "0"}, "bwd-ring6": {"MVAE_NBUF_BWD": "6"},
              "GM256256": {"MVAE_FWD_GM": "256256"}, "GM256128": {"MVAE_FWD_GM": "256128"}, "GM128128": {"MVAE_FWD_GM": "128128"},
              "GM128064": {"MVAE_FWD_GM": "128064"}}


@pytest.mark.parametrize("env", sorted(CASE7_ENVS))
def test_case07_bf16_lds_direct_tiles_rings_and_gate_major(env, monkeypatch):
    """bf16, T=5 B=130 H=128 NL=3: LDS-direct loops, a ragged last row tile in every tile height.  default: lstm_step_fwd_kernel<bf16, 64,
    32, 3> + lstm_step_bwd_kernel<bf16, 64, 64, 4>; BJ64: the wave-specialised 128 x (64 x 4) forward tile; BM / ring knobs: the 128- and
    64-row tiles at ring depths 4 / 5 / 2 forward and 5 / 3 backward; fwd-ring0 / bwd-ring0: the generic loops; bwd-ring6; GM*: the four
    gate-major forward tiles lstm_step_fwd_gm_kernel<256 | 128, 256 | 128 | 64, .>.  B % 128 != 0 keeps the backward off the split forms
    (case 8 has those).  Each with the forward-only call on the same forward kernel."""
    _env(monkeypatch, CASE7_ENVS[env])
    _lstm(_case(7), fwd_only="same")


@pytest.mark.parametrize("split", ["0", "1", "2", "1284", "644", "2562", "1281", "641", "2561"])
@pytest.mark.parametrize("grad", ["dy", "dy_a", "dy+dy_a"])
def test_case08_bf16_every_backward_schedule(grad, split, monkeypatch):
    """bf16, T=4 B=256 H=128 NL=3, a time-invariant addend; the output gradient as a tensor, as the product dy_a . dy_w^T (C = 35 padded to
    dy_k = 128, the top cell's second K-segment) and as both.  MVAE_BWD_SPLIT: 0 fused 64 x 64; 1 the default choice; 2, 2562 the segment
    split (128 x 128 / 256 x 128 partial tiles + lstm_bwd_epi_kernel); 1284, 644 the half-segment split; 1281, 641, 2561 the unsplit
    wave-specialised tiles with the fused epilogue -- <.., 0, 1> with dy, <.., 0, 2> (the no-dy instantiation) with dy_a alone."""
    monkeypatch.setenv("MVAE_BWD_SPLIT", split)
    _lstm(_case(8, dy=grad != "dy_a", dy_a=grad != "dy"))


@pytest.mark.parametrize("split", ["0", "1", "2", "1284"])
def test_case09_bf16_dropout_lstm_hdrop_branch(split, monkeypatch):
    """bf16, T=4 B=128 H=128 NL=3, inter-layer dropout p = 0.25: the LSTM branch of the forward epilogue that writes hdrop (the gate-major
    tile is excluded under dropout: lstm_step_fwd_kernel<bf16, 64, 32, 3>), the factor in the fused backward tile (0, 1:
    lstm_step_bwd_kernel<bf16, 64, 64, 4, false, true>) and in the split schedules' element-wise launch (2, 1284).  The mask derived on the
    device from the seed and the same mask injected as bytes give bit-identical results."""
    monkeypatch.setenv("MVAE_BWD_SPLIT", split)
    c = _case(9)
    assert 0.7 < c["mask"].mean() < 0.8
    a = _lstm(c, drop="inject")
    b = _run(c, drop="hash")
    _same(a, b)


def test_case10_bf16_single_step():
    """bf16, T=1 B=9 H=64 NL=2: one launch per layer diagonal, no recurrent operand at all (A1 = NULL at t = 0), no dc carry."""
    _lstm(_case(10), fwd_only="same")


@pytest.mark.parametrize("gm", [None, "128064"])
def test_case11_bf16_token_table_epilogue(gm, monkeypatch):
    """bf16, T=5 B=70 H=64 NL=2, layer 0 = table rows + a time-invariant addend: the table branch of lstm_step_fwd_kernel<bf16, 64, 32, 3>'s
    epilogue with the LSTM cell.  MVAE_FWD_GM=128064 must be ignored with a table (the gate-major tile has no table epilogue): same bits."""
    c = _case(11)
    base = _lstm(c, fwd_only="same")
    if gm:
        monkeypatch.setenv("MVAE_FWD_GM", gm)
        _same(base, _lstm(c, twice=False))


@pytest.mark.parametrize("what", ["h0", "dh_last", "dh0"])
def test_lstm_refuses_initial_state_and_state_gradients(what):
    """mvae_rnn_fwd (h0) and mvae_rnn_bwd (dh_last, dh0) return MVAE_ERR_UNSUPPORTED for the LSTM cell before anything is enqueued: the
    buffers the refused call was given are untouched."""
    c = _case(1)
    B, H, NL = c["B"], c["H"], c["NL"]
    TB = c["T"] * B
    given = [None] + [torch.zeros(B, H + 8 if what == "h0" else H, device=dev, dtype=F32) for _ in range(NL - 1)]      # one non-NULL entry is enough
    sink = {}
    with pytest.raises(L.MvaeError, match=r"-3"):
        _run(c, sink=sink, **{what: given})
    torch.cuda.synchronize()
    if what == "h0":
        assert "dG" not in sink and all(bool(torch.isnan(b[:TB, :H]).all()) for b in sink["hs"] + sink["cs"] + sink["gates"])
    else:
        assert all(bool(torch.isnan(b[:TB, :4 * H]).all()) for b in sink["dG"]) and all(bool(torch.isnan(b[:2 * B]).all()) for b in sink["dstate"])
