"""CPU tests of tests/gru_ref.py, the float64 reference the GRU step-kernel tests (test_gpu_gru_kernels.py) compare against: the stack
against torch.nn.GRU in float64 with autograd, inter-layer dropout against hand-written arithmetic, the 4-slot translation, and the
storage form against the oracle form."""
import numpy as np
import pytest
import torch

import gru_ref as R


def _params(rs, NL, in0, H, with_x0=True):
    a = 1.0 / np.sqrt(H)
    ps = []
    for l in range(NL):
        n_in = in0 if l == 0 else H
        ps.append(dict(w_ih=rs.uniform(-a, a, (3 * H, n_in)) if (l > 0 or with_x0) else None, w_hh=rs.uniform(-a, a, (3 * H, H)),
                       b_ih=rs.uniform(-a, a, 3 * H), b_hh=rs.uniform(-a, a, 3 * H)))
    return ps


def _relmax(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


@pytest.mark.parametrize("NL", [1, 2, 3])
@pytest.mark.parametrize("given_h0", [True, False])
@pytest.mark.parametrize("grad", ["output", "h_n", "both"])
def test_float64_stack_matches_torch_gru(NL, given_h0, grad):
    """Ragged descending lengths that include T and 1, through pack_padded_sequence; every output and gradient within 1e-12 of torch's, relative
    to the tensor's largest element."""
    T, B, in0, H = 7, 6, 5, 9
    rs = np.random.RandomState(10 * NL + given_h0)
    lengths = np.array([7, 7, 5, 3, 1, 1])
    ps = _params(rs, NL, in0, H)
    x = rs.standard_normal((T, B, in0))
    h0 = [rs.standard_normal((B, H)) for _ in range(NL)] if given_h0 else None
    dy = rs.standard_normal((T, B, H)) if grad in ("output", "both") else None
    dhl = [rs.standard_normal((B, H)) for _ in range(NL)] if grad in ("h_n", "both") else None
    ref = R.gru_stack(ps, lengths, T, B, x0=x, h0=h0, dy=dy, dh_last=dhl)

    g = torch.nn.GRU(in0, H, NL).double()
    with torch.no_grad():
        for l in range(NL):
            for k in ("w_ih", "w_hh", "b_ih", "b_hh"):
                getattr(g, k.replace("w_", "weight_").replace("b_", "bias_") + f"_l{l}").copy_(torch.from_numpy(ps[l][k]))
    xt = torch.from_numpy(x).requires_grad_(True)
    h0t = (torch.from_numpy(np.stack(h0)) if given_h0 else torch.zeros(NL, B, H, dtype=torch.float64)).requires_grad_(True)
    packed = torch.nn.utils.rnn.pack_padded_sequence(xt, torch.from_numpy(lengths))
    yp, hn = g(packed, h0t)
    y, _ = torch.nn.utils.rnn.pad_packed_sequence(yp, total_length=T)
    loss = torch.zeros((), dtype=torch.float64)
    if dy is not None:
        loss = loss + (y * torch.from_numpy(dy)).sum()
    if dhl is not None:
        loss = loss + (hn * torch.from_numpy(np.stack(dhl))).sum()
    loss.backward()
    errs = {"y": _relmax(ref[-1]["y"], y.detach().numpy()), "dx": _relmax(ref[0]["dx"], xt.grad.numpy())}
    for l in range(NL):
        errs[f"h_n{l}"] = _relmax(ref[l]["h_last"], hn[l].detach().numpy())
        errs[f"dh0_{l}"] = _relmax(ref[l]["dh0"], h0t.grad[l].numpy())
        for k, name in (("dW_ih", "weight_ih"), ("dW_hh", "weight_hh"), ("db_ih", "bias_ih"), ("db_hh", "bias_hh")):
            errs[f"{k}{l}"] = _relmax(ref[l][k], getattr(g, f"{name}_l{l}").grad.numpy())
    bad = {k: v for k, v in errs.items() if not v <= 1e-12}
    assert not bad, bad
    # the saved tensors are consistent with the gradients: db = column sums of dG, dW = dG^T . operand, in the 4-slot layout
    for l in range(NL):
        dG = ref[l]["dG"].reshape(T * B, 4 * H)
        assert _relmax(R.unslot_ih(dG.sum(0)), ref[l]["db_ih"]) <= 1e-12 and _relmax(R.unslot_hh(dG.sum(0)), ref[l]["db_hh"]) <= 1e-12
        assert _relmax(R.unslot_hh(dG.T @ ref[l]["h_prev"].reshape(T * B, H)), ref[l]["dW_hh"]) <= 1e-12
        assert _relmax(R.unslot_ih(dG.T @ ref[l]["x_in"].reshape(T * B, -1)), ref[l]["dW_ih"]) <= 1e-12
        for t in range(T):
            assert not ref[l]["y"][t, lengths <= t].any() and not ref[l]["dG"][t, lengths <= t].any()


def test_layer0_addends_equal_an_input_sequence():
    """A table row + a time-invariant addend + a per-step addend is the same stack as the real sequence whose projection they are."""
    T, B, in0, H, NL, V = 5, 4, 6, 7, 2, 11
    rs = np.random.RandomState(3)
    lengths = np.array([5, 4, 2, 1])
    ps = _params(rs, NL, in0, H)
    emb, idx = rs.standard_normal((V, 2)), rs.randint(0, V, (B, T + 2))
    zc, xs = rs.standard_normal((B, 3)), rs.standard_normal((T, B, 1))
    x = np.concatenate([emb[idx[:, :T].T], np.broadcast_to(zc[None], (T, B, 3)), xs], 2)
    W = ps[0]["w_ih"]
    dy, dhl = rs.standard_normal((T, B, H)), [rs.standard_normal((B, H)) for _ in range(NL)]
    a = R.gru_stack(ps, lengths, T, B, x0=x, dy=dy, dh_last=dhl)
    ps_b = [dict(ps[0], w_ih=None)] + ps[1:]
    b = R.gru_stack(ps_b, lengths, T, B, table=emb @ W[:, :2].T, index=idx, add_const=zc @ W[:, 2:5].T, add_step=xs @ W[:, 5:].T, dy=dy, dh_last=dhl)
    for l in range(NL):
        for k in ("y", "h_last", "gates", "dG", "dh0", "dW_hh", "db_ih", "db_hh"):
            assert _relmax(b[l][k], a[l][k]) <= 1e-12, (l, k)
    assert b[0]["dW_ih"] is None and b[0]["x_in"] is None
    # and the two kinds of layer-0 input add: half the projection as a sequence, half as an addend
    c = R.gru_stack([dict(ps[0], w_ih=W[:, :3])] + ps[1:], lengths, T, B, x0=x[:, :, :3], add_step=x[:, :, 3:] @ W[:, 3:].T, dy=dy, dh_last=dhl)
    assert _relmax(c[1]["dG"], a[1]["dG"]) <= 1e-12 and _relmax(c[0]["dW_ih"], a[0]["dW_ih"][:, :3]) <= 1e-12


def test_inter_layer_dropout_by_hand():
    """torch's own mask cannot be injected: the same arithmetic with torch.nn.functional cells written out -- layer l+1 reads
    y_l * keep / (1 - p), and autograd returns the factor on the way back."""
    T, B, in0, H, NL, p = 4, 3, 4, 5, 3, 0.3
    rs = np.random.RandomState(5)
    lengths = np.array([4, 2, 1])
    ps = _params(rs, NL, in0, H)
    x, dy = rs.standard_normal((T, B, in0)), rs.standard_normal((T, B, H))
    h0 = [rs.standard_normal((B, H)) for _ in range(NL)]
    mask = (rs.uniform(size=(NL - 1, T, B, H)) >= p).astype(np.uint8)
    ref = R.gru_stack(ps, lengths, T, B, x0=x, h0=h0, dy=dy, drop_mask=mask, drop_p=p)
    tp = [{k: torch.from_numpy(v).requires_grad_(True) for k, v in q.items()} for q in ps]
    h0t = [torch.from_numpy(h).requires_grad_(True) for h in h0]
    seq = [torch.from_numpy(x[t]) for t in range(T)]
    tl = torch.from_numpy(lengths)
    for l in range(NL):
        h, outs = h0t[l], []
        for t in range(T):
            gi = torch.nn.functional.linear(seq[t], tp[l]["w_ih"], tp[l]["b_ih"]); gh = torch.nn.functional.linear(h, tp[l]["w_hh"], tp[l]["b_hh"])
            r = torch.sigmoid(gi[:, :H] + gh[:, :H]); z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
            n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
            m = (t < tl)[:, None]
            hn = (1 - z) * n + z * h
            h = torch.where(m, hn, h)
            outs.append(torch.where(m, hn, torch.zeros_like(hn)))
        if l + 1 < NL:
            got_hd = np.stack([o.detach().numpy() for o in outs]) * mask[l] / (1.0 - p)
            assert _relmax(ref[l]["hdrop"], got_hd) <= 1e-12
            seq = [o * torch.from_numpy(mask[l][t].astype(np.float64)) / (1.0 - p) for t, o in enumerate(outs)]
        assert _relmax(ref[l]["h_last"], h.detach().numpy()) <= 1e-12
    (torch.stack(outs) * torch.from_numpy(dy)).sum().backward()
    assert ref[-1]["hdrop"] is None
    for l in range(NL):
        assert _relmax(ref[l]["dh0"], h0t[l].grad.numpy()) <= 1e-12
        for k in ("w_ih", "w_hh", "b_ih", "b_hh"):
            assert _relmax(ref[l]["d" + k.replace("w_", "W_")], tp[l][k].grad.numpy()) <= 1e-12, (l, k)
    # the factor is really there: without the mask the lower layers' gradients differ
    plain = R.gru_stack(ps, lengths, T, B, x0=x, h0=h0, dy=dy)
    assert _relmax(plain[0]["dW_hh"], ref[0]["dW_hh"]) > 1e-2


def test_slot_translation_round_trip_and_one_unit_by_hand():
    rs = np.random.RandomState(0)
    H, n_in = 4, 3
    w_ih, w_hh, b_ih, b_hh = rs.standard_normal((3 * H, n_in)), rs.standard_normal((3 * H, H)), rs.standard_normal(3 * H), rs.standard_normal(3 * H)
    assert np.array_equal(R.unslot_ih(R.pack_w_ih(w_ih)), w_ih) and np.array_equal(R.unslot_hh(R.pack_w_hh(w_hh)), w_hh)
    assert not R.pack_w_ih(w_ih)[3 * H:].any() and not R.pack_w_hh(w_hh)[2 * H:3 * H].any()
    b4 = R.pack_bias(b_ih, b_hh)
    assert np.array_equal(R.unslot_ih(b4)[2 * H:], b_ih[2 * H:]) and np.array_equal(R.unslot_hh(b4)[2 * H:], b_hh[2 * H:])
    assert np.array_equal(b4[:2 * H], (b_ih + b_hh)[:2 * H])
    assert np.array_equal(R.pack_addend(b_ih)[:3 * H], b_ih) and not R.pack_addend(b_ih)[3 * H:].any()
    # one unit, one input, one step, numbers chosen by hand: the four pre-activation slots of the kernel's contraction
    #   slot k = W_ih4[k] x + W_hh4[k] h + bias4[k]      ->  r = s(slot0), z = s(slot1), n = tanh(slot2 + r * slot3)
    wi, wh = np.array([[0.5], [-1.0], [2.0]]), np.array([[0.25], [0.75], [-0.5]])
    bi, bh = np.array([0.1, 0.2, 0.3]), np.array([0.01, 0.02, 0.03])
    assert R.pack_w_ih(wi)[:, 0].tolist() == [0.5, -1.0, 2.0, 0.0] and R.pack_w_hh(wh)[:, 0].tolist() == [0.25, 0.75, 0.0, -0.5]
    assert np.allclose(R.pack_bias(bi, bh), [0.11, 0.22, 0.3, 0.03], rtol=0, atol=1e-16)
    x, h = 0.4, -0.6
    pre = R.pack_w_ih(wi)[:, 0] * x + R.pack_w_hh(wh)[:, 0] * h + R.pack_bias(bi, bh)
    assert np.allclose(pre, [0.5 * 0.4 - 0.25 * 0.6 + 0.11, -0.4 - 0.45 + 0.22, 0.8 + 0.3, 0.3 + 0.03], rtol=0, atol=1e-15)
    s = lambda v: 1.0 / (1.0 + np.exp(-v))
    r, z = s(pre[0]), s(pre[1]); n = np.tanh(pre[2] + r * pre[3]); hn = (1 - z) * n + z * h
    ref = R.gru_stack([dict(w_ih=wi, w_hh=wh, b_ih=bi, b_hh=bh)], None, 1, 1, x0=np.array([[[x]]]), h0=[np.array([[h]])], dy=np.ones((1, 1, 1)))[0]
    assert np.allclose(ref["gates"][0, 0], [r, z, n, pre[3]], rtol=0, atol=1e-15) and abs(ref["y"][0, 0, 0] - hn) < 1e-15
    dn = (1 - z) * (1 - n * n); dpr = dn * pre[3] * r * (1 - r); dpz = (h - n) * z * (1 - z)
    assert np.allclose(ref["dG"][0, 0], [dpr, dpz, dn, dn * r], rtol=0, atol=1e-15)
    assert abs(ref["dh0"][0, 0] - (z + dpr * 0.25 + dpz * 0.75 + dn * r * -0.5)) < 1e-15
    assert np.array_equal(R.dG_to_slots(np.array([1., 2., 3.]), np.array([1., 2., 4.])), [1., 2., 3., 4.])
    assert np.array_equal(R.gates_to_slots(*[np.array([v]) for v in (1., 2., 3., 4.)]), [1., 2., 3., 4.])


@pytest.mark.parametrize("drop", [False, True])
def test_storage_form_without_rounding_is_the_oracle_form_bit_for_bit(drop):
    T, B, in0, H, NL, V = 6, 5, 4, 8, 3, 9
    rs = np.random.RandomState(8)
    lengths = np.array([6, 6, 4, 2, 1])
    ps = _params(rs, NL, in0, H)
    kw = dict(x0=rs.standard_normal((T, B, in0)), add_step=rs.standard_normal((T, B, 3 * H)), add_const=rs.standard_normal((B, 3 * H)),
              table=rs.standard_normal((V, 3 * H)), index=rs.randint(0, V, (B, T)), h0=[rs.standard_normal((B, H)) for _ in range(NL)],
              dy=rs.standard_normal((T, B, H)), dh_last=[rs.standard_normal((B, H)) for _ in range(NL)])
    if drop:
        kw.update(drop_mask=(rs.uniform(size=(NL - 1, T, B, H)) >= 0.25).astype(np.uint8), drop_p=0.25)
    a = R.gru_stack(ps, lengths, T, B, **kw)
    b = R.gru_stack(ps, lengths, T, B, storage_round=lambda v: v, **kw)
    for l in range(NL):
        for k in a[l]:
            if isinstance(a[l][k], np.ndarray):
                assert np.array_equal(a[l][k], b[l][k]), (l, k)
    # ... and rounding changes it by about the storage type's precision, not more (and not nothing)
    c = R.gru_stack(ps, lengths, T, B, storage_round=R.bf16_round, **kw)
    e = _relmax(c[NL - 1]["y"], a[NL - 1]["y"])
    assert 1e-4 < e < 3e-2, e
    assert np.array_equal(R.bf16_round(c[0]["dG"]), c[0]["dG"]) and np.array_equal(R.bf16_round(c[0]["gates"]), c[0]["gates"])
    f32 = R.gru_stack(ps, lengths, T, B, storage_round=R.bf16_round, math_dtype=np.float32, **kw)
    assert f32[0]["dG"].dtype == np.float32 and _relmax(f32[NL - 1]["y"], c[NL - 1]["y"]) < 1e-2


def test_bf16_round_and_ulp():
    assert R.bf16_round(np.array([1.0 + 2.0 ** -9, 1.0 + 2.0 ** -8 + 2.0 ** -12, 3.0])).tolist() == [1.0, 1.0 + 2.0 ** -7, 3.0]
    assert R.bf16_ulp(1.0) == 2.0 ** -7 and R.bf16_ulp(0.99) == 2.0 ** -8 and R.bf16_ulp(-3.0) == 2.0 ** -6 and R.bf16_ulp(0.0) == 0.0
