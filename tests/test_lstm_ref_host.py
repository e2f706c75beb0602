"""CPU tests of tests/lstm_ref.py, the float64 reference the LSTM step-kernel tests (test_gpu_lstm_kernels.py) compare against: the stack
against torch.nn.LSTM in float64 with autograd and against the numpy oracle, inter-layer dropout against a stack of nn.LSTMCell, the storage
form against the oracle form, the input conditions of all eleven GPU cases -- and the evidence that the comparison bites: deliberately wrong
references in the kernel's place, every one of which check_slabs must reject."""
import copy

import numpy as np
import pytest
import torch

import lstm_ref as R
from oracle import np_oracle as O


def _params(rs, NL, H):
    a = 1.0 / np.sqrt(H)
    return [dict(w_ih=rs.uniform(-a, a, (4 * H, H)) if l else None, w_hh=rs.uniform(-a, a, (4 * H, H)), b=rs.uniform(-a, a, 4 * H)) for l in range(NL)]


def _relmax(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


@pytest.mark.parametrize("shape", [(7, 6, 9, 3), (1, 5, 8, 2)], ids=["T7", "T1"])
def test_float64_stack_matches_torch_lstm_and_the_numpy_oracle(shape):
    """Layer 0's addend is the projection of a real input sequence x (addend = x . W_ih0^T + b0): outputs, dW, db of every layer and dx
    (= dG[0] . W_ih0) within 1e-10 of torch.nn.LSTM's autograd in float64, relative to the tensor's largest element; the same against
    oracle.np_oracle.lstm_fwd / lstm_bwd."""
    T, B, H, NL = shape
    In = 5
    rs = np.random.RandomState(T)
    ps = _params(rs, NL, H)
    w0, b_ih0, b_hh0 = rs.uniform(-0.4, 0.4, (4 * H, In)), rs.uniform(-0.3, 0.3, 4 * H), rs.uniform(-0.3, 0.3, 4 * H)
    x, dy = rs.standard_normal((T, B, In)), rs.standard_normal((T, B, H))
    add = (x.reshape(T * B, In) @ w0.T + (b_ih0 + b_hh0)).reshape(T, B, 4 * H)
    ps[0]["b"] = None
    ref = R.lstm_stack(ps, T, B, add_step=add, dy=dy)

    m = torch.nn.LSTM(In, H, NL).double()
    tp = {}
    with torch.no_grad():
        for l in range(NL):
            tp[f"g.weight_ih_l{l}"] = w0 if l == 0 else ps[l]["w_ih"]
            tp[f"g.weight_hh_l{l}"] = ps[l]["w_hh"]
            tp[f"g.bias_ih_l{l}"] = b_ih0 if l == 0 else ps[l]["b"]
            tp[f"g.bias_hh_l{l}"] = b_hh0 if l == 0 else np.zeros(4 * H)
            for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                getattr(m, f"{k}_l{l}").copy_(torch.from_numpy(tp[f"g.{k}_l{l}"]))
    xt = torch.from_numpy(x).requires_grad_(True)
    y, _ = m(xt)
    (y * torch.from_numpy(dy)).sum().backward()
    errs = {"y": _relmax(ref[-1]["hs"], y.detach().numpy()), "dx": _relmax(ref[0]["dG"].reshape(T * B, -1) @ w0, xt.grad.numpy().reshape(T * B, In)),
            "dW_ih0": _relmax(ref[0]["dG"].reshape(T * B, -1).T @ x.reshape(T * B, In), m.weight_ih_l0.grad.numpy())}
    for l in range(NL):
        if T > 1:
            errs[f"dW_hh{l}"] = _relmax(ref[l]["dW_hh"], getattr(m, f"weight_hh_l{l}").grad.numpy())
        else:
            assert not ref[l]["dW_hh"].any() and not getattr(m, f"weight_hh_l{l}").grad.numpy().any()
        errs[f"db{l}"] = _relmax(ref[l]["db"], getattr(m, f"bias_ih_l{l}").grad.numpy())
        if l:
            errs[f"dW_ih{l}"] = _relmax(ref[l]["dW_ih"], getattr(m, f"weight_ih_l{l}").grad.numpy())
    # the numpy oracle (what `_lstm_case` of test_gpu_parity.py compares with)
    yo, caches = O.lstm_fwd(x, tp, "g", NL)
    grads = {}
    dxo = O.lstm_bwd(dy, caches, grads, "g")
    errs["oracle dx"] = _relmax(ref[0]["dG"].reshape(T * B, -1) @ w0, dxo.reshape(T * B, In))
    for l in range(NL):
        errs[f"oracle h{l}"] = _relmax(ref[l]["hs"], caches[l][1]); errs[f"oracle c{l}"] = _relmax(ref[l]["cs"], caches[l][2])
        errs[f"oracle gates{l}"] = _relmax(ref[l]["gates"], caches[l][3]); errs[f"oracle db{l}"] = _relmax(ref[l]["db"], grads[f"g.bias_ih_l{l}"])
        if T > 1:
            errs[f"oracle dW_hh{l}"] = _relmax(ref[l]["dW_hh"], grads[f"g.weight_hh_l{l}"])
    bad = {k: v for k, v in errs.items() if not v <= 1e-10}
    assert not bad, bad
    # the host products are the parameter gradients: what the GPU test forms from the kernel's tensors
    for l in range(NL):
        assert _relmax(ref[l]["p_b"], ref[l]["db"]) <= 1e-12 and np.abs(ref[l]["p_hh"] - ref[l]["dW_hh"]).max() <= 1e-12 * max(np.abs(ref[l]["dW_hh"]).max(), 1.0)
        assert (ref[l]["p_ih"] is None) == (l == 0) and (l == 0 or _relmax(ref[l]["p_ih"], ref[l]["dW_ih"]) <= 1e-12)


def test_inter_layer_dropout_against_a_stack_of_lstm_cells():
    """torch's own mask cannot be injected: nn.LSTMCell per layer and step, layer l + 1 reading h_l * keep / (1 - p); autograd returns the
    factor on the way back."""
    T, B, H, NL, p = 4, 3, 5, 3, 0.3
    rs = np.random.RandomState(5)
    ps = _params(rs, NL, H)
    add, dy = rs.standard_normal((T, B, 4 * H)), rs.standard_normal((T, B, H))
    mask = (rs.uniform(size=(NL - 1, T, B, H)) >= p).astype(np.uint8)
    ref = R.lstm_stack(ps, T, B, add_step=add, dy=dy, drop_mask=mask, drop_p=p)
    cells = []
    for l in range(NL):
        cell = torch.nn.LSTMCell(4 * H if l == 0 else H, H).double()
        with torch.no_grad():
            cell.weight_ih.copy_(torch.eye(4 * H, dtype=torch.float64) if l == 0 else torch.from_numpy(ps[l]["w_ih"]))
            cell.weight_hh.copy_(torch.from_numpy(ps[l]["w_hh"])); cell.bias_ih.copy_(torch.from_numpy(ps[l]["b"])); cell.bias_hh.zero_()
        cells.append(cell)
    seq = [torch.from_numpy(add[t]) for t in range(T)]
    for l in range(NL):
        h = c = torch.zeros(B, H, dtype=torch.float64)
        outs = []
        for t in range(T):
            h, c = cells[l](seq[t], (h, c))
            outs.append(h)
        assert _relmax(ref[l]["hs"], torch.stack(outs).detach().numpy()) <= 1e-10
        if l + 1 < NL:
            seq = [o * torch.from_numpy(mask[l][t].astype(np.float64)) / (1.0 - p) for t, o in enumerate(outs)]
            assert _relmax(ref[l]["hdrop"], torch.stack(seq).detach().numpy()) <= 1e-10
    (torch.stack(outs) * torch.from_numpy(dy)).sum().backward()
    assert ref[-1]["hdrop"] is None
    for l in range(NL):
        assert _relmax(ref[l]["dW_hh"], cells[l].weight_hh.grad.numpy()) <= 1e-10 and _relmax(ref[l]["db"], cells[l].bias_ih.grad.numpy()) <= 1e-10
        if l:
            assert _relmax(ref[l]["dW_ih"], cells[l].weight_ih.grad.numpy()) <= 1e-10
    plain = R.lstm_stack(ps, T, B, add_step=add, dy=dy)
    assert _relmax(plain[0]["dW_hh"], ref[0]["dW_hh"]) > 1e-2          # the factor is really there


@pytest.mark.parametrize("drop", [False, True])
def test_storage_form_without_rounding_is_the_oracle_form_bit_for_bit(drop):
    T, B, H, NL, V = 6, 5, 8, 3, 9
    rs = np.random.RandomState(8)
    ps = _params(rs, NL, H)
    idx = rs.randint(-2, V + 2, (B, T + 1))
    kw = dict(add_step=rs.standard_normal((T, B, 4 * H)), add_const=rs.standard_normal((B, 4 * H)), table=rs.standard_normal((V, 4 * H)), index=idx,
              dy=rs.standard_normal((T, B, H)))
    if drop:
        kw.update(drop_mask=(rs.uniform(size=(NL - 1, T, B, H)) >= 0.25).astype(np.uint8), drop_p=0.25)
    a = R.lstm_stack(ps, T, B, **kw)
    b = R.lstm_stack(ps, T, B, storage_round=lambda v: v, **kw)
    for l in range(NL):
        for k in a[l]:
            if isinstance(a[l][k], np.ndarray):
                assert np.array_equal(a[l][k], b[l][k]), (l, k)
    # table ids are clamped to [0, rows)
    assert (idx[:, :T] < 0).any() and (idx[:, :T] >= V).any()
    cl = R.lstm_stack(ps, T, B, **dict(kw, index=np.clip(idx, 0, V - 1)))
    assert np.array_equal(cl[NL - 1]["dG"], a[NL - 1]["dG"])
    # ... and rounding changes it by about the storage type's precision, not more (and not nothing)
    c = R.lstm_stack(ps, T, B, storage_round=R.bf16_round, **kw)
    e = _relmax(c[NL - 1]["hs"], a[NL - 1]["hs"])
    assert 1e-4 < e < 3e-2, e
    for k in ("hs", "cs", "gates", "dG"):
        assert np.array_equal(R.bf16_round(c[0][k]), c[0][k]), k
    f32 = R.lstm_stack(ps, T, B, storage_round=R.bf16_round, math_dtype=np.float32, **kw)
    assert f32[0]["dG"].dtype == np.float32 and f32[0]["p_hh"].dtype == np.float64 and _relmax(f32[NL - 1]["hs"], c[NL - 1]["hs"]) < 1e-2


def test_dropout_hash_and_bf16_helpers():
    assert R.bf16_round(np.array([1.0 + 2.0 ** -9, 1.0 + 2.0 ** -8 + 2.0 ** -12, 3.0])).tolist() == [1.0, 1.0 + 2.0 ** -7, 3.0]
    assert R.bf16_ulp(1.0) == 2.0 ** -7 and R.bf16_ulp(0.99) == 2.0 ** -8 and R.bf16_ulp(-3.0) == 2.0 ** -6 and R.bf16_ulp(0.0) == 0.0
    m = R.dropout_keep_mask(0x5EED1234, (2, 4, 16, 32), 0.25)
    assert m.dtype == np.uint8 and 0.7 < m.mean() < 0.8
    # element 0 by hand: idx = 0 -> h = seed, then the three mixing rounds of the header
    h = 0x5EED1234
    h ^= h >> 16; h = (h * 0x85EBCA6B) & 0xFFFFFFFF; h ^= h >> 13; h = (h * 0xC2B2AE35) & 0xFFFFFFFF; h ^= h >> 16
    assert int(m.flat[0]) == int(h >= int(0.25 * 2 ** 32))


@pytest.mark.parametrize("n", sorted(R.CASES))
def test_input_conditions_of_every_gpu_case(n):
    """build_case asserts the caps (>= 90 % unsaturated, pre-activation standard deviation >= 0.5 per (layer, step)); the recipe gives far
    more, which is what keeps a permuted gate slot or a lost carry visible."""
    c = R.build_case(**R.CASES[n])
    for l, (unsat, sd) in enumerate(c["conditions"]):
        assert unsat >= 0.9 and sd >= 0.5, (n, l, unsat, sd)
    if c["bf16"]:
        bad, floors = R.check_slabs(c["ref32"], c["ref"], c["ref32"], drop=c["drop_p"] > 0)
        assert not bad and floors


# ------------------------------------------------------------------------------------------------ the checks can fail
def _mutants(c, kind):
    """(name, outputs of a deliberately wrong 'kernel') for a built case: the storage reference in float32 math with one defect each."""
    T, B, NL, ps, kw = c["T"], c["B"], c["NL"], c["ps"], c["kw"]
    rq = R.bf16_round if c["bf16"] else R.f32_round
    run = lambda ps_=ps, mut=None, **over: R.lstm_stack(ps_, T, B, storage_round=rq, math_dtype=np.float32, _mutate=mut, **dict(kw, **over))
    yield "honest", run()
    H = c["H"]
    sw = copy.deepcopy(ps)
    for k in ("w_ih", "w_hh", "b"):
        a = sw[1][k].copy(); a[0:H], a[H:2 * H] = sw[1][k][H:2 * H], sw[1][k][0:H]; sw[1][k] = a
    yield "i and f slots swapped in layer 1", run(sw)
    yield "c_t for c_{t-1} in df", run(mut=dict(df_uses_c_t=True))
    yield "dc carry dropped at one step", run(mut=dict(drop_dc_at=(NL - 1, T // 2)))
    if kind == "drop":
        yield "1 / (1 - p) omitted in the backward", run(mut=dict(no_drop_scale_bwd=True))
    if kind == "dy_a":
        dy = c["dy_tot"].copy(); dy[T - 1] -= c["dy_prod"][T - 1]
        yield "dy_a product left out at the last step", run(dy=dy)
    if kind == "table":
        yield "table id not clamped", run(mut=dict(wrap_ids=True))
    o = run()
    o[NL - 1]["hs"] = o[NL - 1]["hs"].copy(); o[NL - 1]["hs"][T - 1, B - 1, :] = np.nan
    yield "one row of the last batch tile unwritten", o


@pytest.mark.parametrize("case", ["f32-table", "bf16-dy_a", "bf16-drop"])
def test_check_slabs_rejects_every_mutant_and_passes_the_honest_float32_form(case):
    """A mutated reference plays the kernel's part.  f32: case 3 with out-of-range table ids (bound 2e-5 of the slab maximum against the
    float64 oracle form); bf16: case 8 with dy + dy_a and case 9 (dropout) against the float64 storage form with the floor-derived bound.
    The unmutated float32 storage reference passes both; every mutant must be rejected."""
    if case == "f32-table":
        c, kind = R.build_case(**dict(R.CASES[3], bad_ids=True)), "table"
    elif case == "bf16-dy_a":
        c, kind = R.build_case(**dict(R.CASES[8], dy_a=True)), "dy_a"
    else:
        c, kind = R.build_case(**R.CASES[9]), "drop"
    names = []
    for name, got in _mutants(c, kind):
        bad, _ = R.check_slabs(got, c["ref"], c["ref32"], drop=c["drop_p"] > 0)
        names.append(name)
        if name == "honest":
            assert not bad, bad
        else:
            assert bad, f"{name}: not rejected"
    assert len(names) == 6 and names[0] == "honest"
