"""CPU tests of the packed weight shadows: every module's pack job table (ops.PackList, recorded by `_build_pack` on CPU buffers) is replayed
in torch and each shadow the kernels read is compared element for element with its layout restated here -- LSTM stacks straight, GRU
stacks in the 4-slot gate layout (W_ih rows (r, z, n, 0), W_hh rows (r, z, 0, n), bias slots (b_ir + b_hr, b_iz + b_hz, b_in, b_hn)),
zero padding everywhere else (models2d: hidden size 501 -> 512).  No kernel runs."""
import pytest
import torch

import molecular_vae_amd as mv
from molecular_vae_amd import _lib as L
from molecular_vae_amd import vocab as V

CPU = torch.device("cpu")
DTYPES = {L.MVAE_F32: torch.float32, L.MVAE_BF16: torch.bfloat16}


def _owner(pl, addr):
    """The storage of a tensor in the job table's keep list that holds byte address `addr`: (storage, its base address)."""
    for t in pl.keep:
        s = t.untyped_storage()
        if s.data_ptr() <= addr < s.data_ptr() + s.nbytes():
            return s, s.data_ptr()
    raise AssertionError(f"address {addr:#x} is in no tensor the job table keeps")


def _view(pl, addr, dtype, shape, ld, written=None):
    """[rows, cols] view with leading dimension `ld` at byte address `addr`; `written`: mark its elements, refusing a second write."""
    s, base = _owner(pl, addr)
    item = torch.empty((), dtype=dtype).element_size()
    assert (addr - base) % item == 0
    off, (R, C) = (addr - base) // item, shape
    assert off + (R - 1) * ld + C <= s.nbytes() // item, "job reaches past the end of its buffer"
    v = torch.empty(0, dtype=dtype).set_(s, off, (R, C), (ld, 1))
    if written is not None:
        m = written.setdefault((s.data_ptr(), dtype), torch.zeros(s.nbytes() // item, dtype=torch.bool)).as_strided((R, C), (ld, 1), off)
        assert not m.any(), "two jobs write the same element"
        m.fill_(True)
    return v


def replay(pl):
    """Run the job table in torch: kind 0 cast and / or transpose, kind 1 add, kind 2 copy (mvae_pack_multi's semantics, include/mvae.h)."""
    written = {}
    for j in pl.jobs:
        sd, dd = DTYPES[j.src_dtype], DTYPES[j.dst_dtype]
        if j.kind == 1:
            n = j.R * j.C
            a, b = _view(pl, j.src, torch.float32, (1, n), n), _view(pl, j.src2, torch.float32, (1, n), n)
            _view(pl, j.dst, torch.float32, (1, n), n, written).copy_(a + b)
            continue
        src = _view(pl, j.src, sd, (j.R, j.C), j.lds).float()
        if j.kind == 2:
            assert sd == dd == torch.float32 and not j.dstT
            _view(pl, j.dst, dd, (j.R, j.C), j.ldd, written).copy_(src)
            continue
        assert j.kind == 0 and (j.dst or j.dstT)
        if j.dst:
            _view(pl, j.dst, dd, (j.R, j.C), j.ldd, written).copy_(src.to(dd))
        if j.dstT:
            _view(pl, j.dstT, dd, (j.C, j.R), j.ldt, written).copy_(src.t().to(dd))


def _randomise(mod, seed=7):
    """Distinct, non-bf16-representable values in every parameter (so a swapped slot or a missed rounding shows)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(torch.randn(p.shape, generator=g))


def _packed(mod):
    _randomise(mod)
    with torch.no_grad():
        mod._build_pack(CPU)
    pl = mod._pack_list
    replay(pl)
    return mod._packed


def check(buf, shape, dtype, *blocks):
    """buf == a zero [shape] tensor of `dtype` with each (index, value) of `blocks` written in (value rounded to dtype)."""
    want = torch.zeros(shape, dtype=dtype)
    for idx, val in blocks:
        want[idx] = val.detach().to(dtype)
    assert buf.dtype == dtype and tuple(buf.shape) == tuple(shape)
    assert torch.equal(buf, want), (buf.float() - want.float()).abs().max()


def gru_slots(w3, H, Hp, Kp, n_slot):
    """torch's [3H, K] gate rows (r, z, n) -> [4Hp, Kp] slot rows, n in slot `n_slot`, zero elsewhere."""
    out = torch.zeros(4 * Hp, Kp)
    for g, s in ((0, 0), (1, 1), (2, n_slot)):
        out[s * Hp:s * Hp + H, :w3.shape[1]] = w3[g * H:(g + 1) * H]
    return out


def check_gru_stack(P, rnn, dt, Hp, ldw, ldwT):
    """Whh / WhhT (every layer), Wih / WihT (layers >= 1) and the 4-slot bias of a GRU stack from `P` (dict with those lists)."""
    H = rnn.hidden_size
    for l in range(rnn.num_layers):
        w = gru_slots(getattr(rnn, f"weight_hh_l{l}"), H, Hp, Hp, 3)
        check(P["Whh"][l], (4 * Hp, ldw), dt, ((slice(None), slice(0, Hp)), w))
        check(P["WhhT"][l], (Hp, ldwT), dt, ((slice(None), slice(0, 4 * Hp)), w.t()))
        if l > 0:
            w = gru_slots(getattr(rnn, f"weight_ih_l{l}"), H, Hp, Hp, 2)
            check(P["Wih"][l], (4 * Hp, ldw), dt, ((slice(None), slice(0, Hp)), w))
            check(P["WihT"][l], (Hp, ldwT), dt, ((slice(None), slice(0, 4 * Hp)), w.t()))
        else:
            assert P["Wih"][0] is None and P["WihT"][0] is None
        bi, bh = getattr(rnn, f"bias_ih_l{l}"), getattr(rnn, f"bias_hh_l{l}")
        check(P["bias"][l], (4 * Hp,), torch.float32, (slice(0, H), bi[:H] + bh[:H]), (slice(Hp, Hp + H), bi[H:2 * H] + bh[H:2 * H]),
              (slice(2 * Hp, 2 * Hp + H), bi[2 * H:]), (slice(3 * Hp, 3 * Hp + H), bh[2 * H:]))


def check_lstm_stack(P, rnn, dt, ldw, ldwT):
    """LSTM stacks are straight copies: W [4H, H] in [4H, ldw], W^T in [H, ldwT], bias = b_ih + b_hh."""
    H = rnn.hidden_size
    for l in range(rnn.num_layers):
        for k in ("hh", "ih") if l > 0 else ("hh",):
            w = getattr(rnn, f"weight_{k}_l{l}")
            check(P[f"W{k}"][l], (4 * H, ldw), dt, ((slice(None), slice(0, H)), w))
            check(P[f"W{k}T"][l], (H, ldwT), dt, ((slice(None), slice(0, 4 * H)), w.t()))
        check(P["bias"][l], (4 * H,), torch.float32, (slice(None), getattr(rnn, f"bias_ih_l{l}") + getattr(rnn, f"bias_hh_l{l}")))


def pad(n, m):
    return (n + m - 1) // m * m


def test_mol_encoder_pack_layout():
    m = mv.MolEncoder(i=24, o=16, c=12, h_size=56, num_lstm=3)
    P = _packed(m)
    g, H, E, Cv = m.gru, m.gru.hidden_size, m.gru.input_size, 12
    Hp, f32 = pad(H, 32), torch.float32
    emb = m.embedding.weight
    check(P["E_p"], (Cv, pad(E, 4)), f32, ((slice(None), slice(0, E)), emb))
    check(P["ET"], (E, pad(Cv, 4)), f32, ((slice(None), slice(0, Cv)), emb.t()))
    check(P["Wih0_p"], (4 * H, pad(E, 4)), f32, ((slice(None), slice(0, E)), g.weight_ih_l0))
    check(P["Wih0T"], (E, 4 * H), f32, (slice(None), g.weight_ih_l0.t()))
    check_lstm_stack(P, g, f32, Hp, 4 * H)
    d1 = m.dense_1[0]
    check(P["W1T"], (d1.in_features, d1.out_features), f32, (slice(None), d1.weight.t()))
    zm, zv = m.lmbd.z_mean, m.lmbd.z_log_var
    wml = torch.cat([zm.weight, zv.weight])
    check(P["Wml"], (32, 512), f32, (slice(None), wml))
    check(P["WmlT"], (512, 32), f32, (slice(None), wml.t()))
    check(P["bml"], (32,), f32, (slice(None), torch.cat([zm.bias, zv.bias])))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_mol_decoder_pack_layout(dt):
    m = mv.MolDecoder(i=16, o=24, c=12, num_gru=3, h_size=64, dtype=dt)
    P = _packed(m)
    g, H, o, C, f32 = m.gru, 64, 16, 12, torch.float32
    li = m.latent_input[0]
    check(P["WliT"], (o, pad(o, 4)), f32, ((slice(None), slice(0, o)), li.weight.t()))
    check(P["Wih0T"], (o, 4 * H), f32, (slice(None), g.weight_ih_l0.t()))
    check_lstm_stack(P, g, dt, P["ldw"], P["ldwT"])
    assert (P["ldw"], P["ldwT"]) == (H + 64, 4 * H + 64)
    w = m.decoded_mean.module[0].weight
    check(P["Wout"], (C, H), dt, (slice(None), w))
    check(P["WoutT"], (H, 128 if dt == torch.bfloat16 else pad(C, 8)), dt, ((slice(None), slice(0, C)), w.t()))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_mosesvae_pack_layout(dt):
    m = mv.mosesvae.VAE(V.OneHotVocab(set("CNO()=c1")), dtype=dt)
    P = _packed(m)
    Vn, dz, f32 = len(m.vocabulary), m.d_z, torch.float32
    Vp = pad(Vn, 4)
    E = m.x_emb.weight
    check(P["E_p"], (Vn, Vp), f32, ((slice(None), slice(0, Vn)), E))
    check(P["ET_p"], (Vn, Vp), f32, ((slice(None), slice(0, Vn)), E.t()))
    for name, rnn in (("enc", m.encoder_rnn), ("dec", m.decoder_rnn)):
        Pn, H = P[name], rnn.hidden_size
        assert (Pn["H"], Pn["ldw"], Pn["ldwT"]) == (H, H + 64, 4 * H + 64)
        check_gru_stack(Pn, rnn, dt, H, H + 64, 4 * H + 64)
        w0 = rnn.weight_ih_l0[:, :Vn]
        check(Pn["Wx_p"], (3 * H, Vp), f32, ((slice(None), slice(0, Vn)), w0))
        check(Pn["WxT"], (Vn, 3 * H), f32, (slice(None), w0.t()))
    Hd = m.decoder_rnn.hidden_size
    wz = m.decoder_rnn.weight_ih_l0[:, Vn:]
    check(P["Wz"], (3 * Hd, dz), f32, (slice(None), wz))
    check(P["WzT"], (dz, 3 * Hd), f32, (slice(None), wz.t()))
    for n, seq in (("mu", m.q_mu), ("lv", m.q_logvar)):
        check(P[n + "_W0T"], tuple(seq[0].weight.t().shape), f32, (slice(None), seq[0].weight.t()))
        check(P[n + "_W2T"], tuple(seq[2].weight.t().shape), f32, (slice(None), seq[2].weight.t()))
    check(P["WlatT"], (dz, Hd), f32, (slice(None), m.decoder_lat.weight.t()))
    w = m.decoder_fc.weight
    check(P["Wfc"], (Vn, Hd + 64), dt, ((slice(None), slice(0, Hd)), w))
    check(P["WfcT"], (Hd, 128 if dt == torch.bfloat16 else pad(Vn, 8)), dt, ((slice(None), slice(0, Vn)), w.t()))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_models2d_pack_layout(dt):
    m = mv.models2d.VAE(dtype=dt)
    P = _packed(m)
    H, Hp, C, f32 = 501, 512, 35, torch.float32
    w0 = m.fc0.weight
    check(P["W0p"], (435, 92), f32, ((slice(None), slice(0, 90)), w0))
    check(P["W0T"], (92, 436), f32, ((slice(0, 90), slice(0, 435)), w0.t()))
    wml = torch.cat([m.fc11.weight, m.fc12.weight])
    check(P["Wml"], (4, 436), f32, ((slice(None), slice(0, 435)), wml))
    check(P["WmlT"], (436, 4), f32, ((slice(0, 435), slice(None)), wml.t()))
    check(P["bml"], (4,), f32, (slice(None), torch.cat([m.fc11.bias, m.fc12.bias])))
    check(P["W2p"], (2, 4), f32, ((slice(None), slice(0, 2)), m.fc2.weight))
    check(P["W2T"], (4, 4), f32, ((slice(0, 2), slice(0, 2)), m.fc2.weight.t()))
    assert (P["ldw"], P["ldwT"]) == (Hp + 64, 4 * Hp + 64)
    check_gru_stack(P, m.gru, dt, Hp, Hp + 64, 4 * Hp + 64)
    wx = gru_slots(m.gru.weight_ih_l0, H, Hp, 4, 2)
    check(P["Wx0"], (4 * Hp, 4), f32, (slice(None), wx))
    check(P["Wx0T"], (4, 4 * Hp), f32, (slice(None), wx.t()))
    w = m.fc3.weight
    check(P["Wfc"], (C, Hp + 64), dt, ((slice(None), slice(0, H)), w))
    check(P["WfcT"], (Hp, 128 if dt == torch.bfloat16 else 40), dt, ((slice(0, H), slice(0, C)), w.t()))


@pytest.mark.parametrize("make", [lambda: mv.models2d.VAE(), lambda: mv.mosesvae.VAE(V.OneHotVocab(set("CNO"))),
                                  lambda: mv.MolEncoder(i=24, o=16, c=12, h_size=56), lambda: mv.MolDecoder(i=16, o=24, c=12, num_gru=2, h_size=32)],
                         ids=["models2d", "moses", "encoder", "decoder"])
def test_apply_invalidates_the_packed_shadows(make):
    """Initialisation hooks write through `p.data`, which torch's version counters do not see: `apply` bumps the parameter epoch instead."""
    m = make()
    before = L.PARAM_EPOCH[0]

    def init(mod):
        if isinstance(mod, torch.nn.Linear):
            mod.bias.data.fill_(0.5)
    m.apply(init)
    assert L.PARAM_EPOCH[0] == before + 1
