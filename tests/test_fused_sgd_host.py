"""CPU tests of FusedSGD (clip_grad_norm_ + torch.optim.SGD of train_distributed.py:73,91 as mvae_sumsq + mvae_clip_sgd): the C entry's
argument checks, the constructor's refusals, the flat-buffer / sink / shared partial-sum layout, torch.optim.SGD's state-dict layout, and the
data-parallel bookkeeping at world 2 over gloo."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import molecular_vae_amd as mv
from molecular_vae_amd import _lib as L


def _call_clip_sgd(n=8, npartial=1, momentum=0.9, dampening=0.0, nesterov=0, parity=0, null_buf=False):
    lib = L.load()
    host = (ctypes.c_float * 64)()
    words = (ctypes.c_int32 * 2)()
    a = ctypes.cast(host, ctypes.c_void_p)
    buf = None if null_buf else a
    return lib.mvae_clip_sgd(n, a, a, buf, a, npartial, 1.0, 5.0, 1e-3, momentum, dampening, 0.0, nesterov,
                             ctypes.cast(words, ctypes.c_void_p), parity, a, 2, None, None)


def test_clip_sgd_is_exported_and_rejects_bad_arguments_without_a_device():
    lib = L.load()
    assert hasattr(lib, "mvae_clip_sgd") and "mvae_clip_sgd" in L.SIGNATURES and L.ABI_VERSION >= 11
    bad = dict(n_negative=dict(n=-1), no_partials=dict(npartial=0), negative_momentum=dict(momentum=-0.1),
               nesterov_without_momentum=dict(momentum=0.0, nesterov=1), nesterov_with_dampening=dict(nesterov=1, dampening=0.3),
               bad_parity=dict(parity=2), momentum_without_buffer=dict(null_buf=True))
    for what, kw in bad.items():
        assert _call_clip_sgd(**kw) == -1, what


@pytest.mark.parametrize("kw", [dict(lr=-1e-3), dict(momentum=-0.5), dict(weight_decay=-1e-4), dict(nesterov=True),
                                dict(nesterov=True, momentum=0.9, dampening=0.1)])
def test_construction_refuses_what_torch_sgd_refuses(kw):
    ps = [torch.nn.Parameter(torch.zeros(3))]
    args = dict(dict(lr=1e-3), **kw)
    with pytest.raises(ValueError):
        torch.optim.SGD(ps, **args)
    with pytest.raises(ValueError):
        mv.FusedSGD([torch.nn.Parameter(torch.zeros(3))], **args)


@pytest.mark.parametrize("kw", [dict(maximize=True), dict(foreach=True), dict(fused=True), dict(differentiable=True)])
def test_construction_refuses_non_inert_torch_options(kw):
    with pytest.raises(ValueError):
        mv.FusedSGD([torch.nn.Parameter(torch.zeros(3))], lr=1e-3, **kw)
    with pytest.raises(ValueError):                       # ... in a param group of its own as well
        mv.FusedSGD([{"params": [torch.nn.Parameter(torch.zeros(3))], **kw}], lr=1e-3)


def test_flat_buffers_sinks_poison_slot_and_the_shared_partial_array():
    torch.manual_seed(0)
    a = [torch.nn.Parameter(torch.randn(70000)), torch.nn.Parameter(torch.randn(5, 7))]
    b = [torch.nn.Parameter(torch.randn(65536 * 2 + 3)), torch.nn.Parameter(torch.randn(11), requires_grad=False)]
    before = [p.detach().clone() for p in a + b]
    opt = mv.FusedSGD([{"params": a}, {"params": b, "lr": 1e-2}], lr=1e-3, momentum=0.85, max_grad_norm=5.0)
    for p, x in zip(a + b, before):
        assert torch.equal(p.detach(), x)
    f0, f1 = opt._flat
    for f, ps in ((f0, a), (f1, b[:1])):
        n = sum(p.numel() for p in ps)
        assert f["n"] == n and f["g"].numel() == f["p"].numel() == f["buf"].numel() == n + 1
        assert f["poison"].data_ptr() == f["g"][n:].data_ptr()
        off = 0
        for p in ps:
            assert p.data.data_ptr() == f["p"].data_ptr() + 4 * off          # p.data is a view of the flat buffer
            sink = p._mvae_sink
            assert sink[0]() is opt and sink[1] is f["g"] and sink[2] == off and sink[4].data_ptr() == f["poison"].data_ptr()
            off += p.numel()
    assert not hasattr(b[1], "_mvae_sink")
    # one partial-sum array: group 0's chunks, then group 1's; every group's update reads all of it
    n0, n1 = (f0["n"] + 1 + 65535) >> 16, (f1["n"] + 1 + 65535) >> 16
    assert (n0, n1) == (2, 3) and opt._partial.numel() == n0 + n1
    assert f0["partial"].data_ptr() == opt._partial.data_ptr() and f1["partial"].data_ptr() == opt._partial[n0:].data_ptr()
    assert f0["norm"] is f1["norm"] is opt._norm
    assert opt.last_grad_norm.data_ptr() == opt._norm.data_ptr() and opt.skipped_steps.data_ptr() == opt._norm[1:].data_ptr()
    with pytest.raises(L.MvaeError):                      # no CPU fallback
        opt.step()


def test_state_dict_has_torch_sgd_layout_and_round_trips_through_torch_sgd():
    torch.manual_seed(1)
    ps = [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(3))]
    opt = mv.FusedSGD(ps, lr=1.2e-3, momentum=0.85, max_grad_norm=5.0)
    sd = opt.state_dict()
    ref = torch.optim.SGD([torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.zeros(3))], lr=1.2e-3, momentum=0.85).state_dict()
    assert sd["state"] == {} and set(ref["param_groups"][0]) <= set(sd["param_groups"][0])
    assert {k: sd["param_groups"][0][k] for k in ref["param_groups"][0]} == ref["param_groups"][0]
    # into torch.optim.SGD, a step there (buffers appear), and back
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    t = torch.optim.SGD(qs, lr=1.0, momentum=0.5, dampening=0.3)
    t.load_state_dict(sd)
    assert t.param_groups[0]["lr"] == 1.2e-3 and t.param_groups[0]["momentum"] == 0.85 and t.param_groups[0]["dampening"] == 0
    for q in qs:
        q.grad = torch.randn_like(q)
    t.step()
    tsd = t.state_dict()
    assert set(tsd["state"]) == {0, 1}
    rs = [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(3))]
    o2 = mv.FusedSGD(rs, lr=5.0, momentum=0.1)
    o2.load_state_dict(tsd)
    assert o2.param_groups[0]["lr"] == 1.2e-3 and o2.param_groups[0]["momentum"] == 0.85
    assert int(o2._flat[0]["init"][0]) == 1 and int(o2._flat[0]["init"][1]) == 1
    back = o2.state_dict()
    for k in (0, 1):
        assert torch.equal(back["state"][k]["momentum_buffer"], tsd["state"][k]["momentum_buffer"])
    # entries without a buffer (torch: a parameter that had no gradient) count as zero; a dict with none at all clears the flag
    part = {"state": {0: {"momentum_buffer": None}, 1: {"momentum_buffer": torch.full((3,), 2.0)}}, "param_groups": tsd["param_groups"]}
    o2.load_state_dict(part)
    assert int(o2._flat[0]["init"][0]) == 1
    assert torch.equal(o2.state_dict()["state"][0]["momentum_buffer"], torch.zeros(4, 3))
    o2.load_state_dict({"state": {}, "param_groups": tsd["param_groups"]})
    assert int(o2._flat[0]["init"].sum()) == 0 and o2.state_dict()["state"] == {}
    with pytest.raises(ValueError):
        o2.load_state_dict({"state": {}, "param_groups": [dict(tsd["param_groups"][0], nesterov=True, dampening=0.5)]})


def test_shard_form_takes_one_group_and_needs_a_world():
    ps = [torch.nn.Parameter(torch.zeros(5))]
    opt = mv.FusedSGD(ps, lr=1e-3, momentum=0.9, grad_sync=mv.GradSync(), shard_optimizer=True)
    assert not opt.shard                                 # one process: nothing to shard


# ------------------------------------------------------------------------------------------------ world 2 over gloo
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    tot = sum(r + 1 for r in range(world))
    # (a) a MolecularVAE-shaped parameter list under FusedSGD: the decoder's four per-layer early ranges, then step()'s complement; the poison
    # slot of one rank reaches every rank
    enc = mv.MolEncoder(i=24, o=16, c=12, h_size=56, num_lstm=3)
    dec = mv.MolDecoder(i=16, o=24, c=12, num_gru=4, h_size=64, dtype=torch.float32)
    params = list(enc.parameters()) + list(dec.parameters())
    n = sum(p.numel() for p in params)
    sync = mv.GradSync(bucket_bytes=4 * 5000)
    opt = mv.FusedSGD(params, lr=1.2e-3, momentum=0.85, max_grad_norm=5.0, grad_sync=sync)
    f = opt._flat[0]
    assert f["g"].numel() == n + 1 and f["poison"].data_ptr() == f["g"][n:].data_ptr()
    assert L.grad_sink_range(list(dec.parameters()))[0] is opt and opt.grad_sync is sync      # what the decoder's backward looks up
    names = [k for k, _ in enc.named_parameters()] + ["D." + k for k, _ in dec.named_parameters()]
    offs, off = {}, 0
    for k, p_ in zip(names, params):
        offs[k] = off; off += p_.numel()
    g = f["g"]
    g.copy_(torch.arange(n + 1, dtype=torch.float32).remainder(1000) * (rank + 1))
    for k, p_ in zip(names, params):                          # gradients handed over as views of the sink (the decoder's fork path)
        p_.grad = g[offs[k]:offs[k] + p_.numel()].view(p_.shape)
    first = lambda l: "D.gru.weight_ih_l%d" % l if l >= 1 else "D.gru.weight_hh_l0"
    hi = n
    for l in (3, 2, 1, 0):
        lo = offs[first(l)]
        sync.start_early(g, lo, hi); hi = lo
    if rank == 1:
        f["poison"].fill_(float("nan"))
    flats = opt.gather_grads()                                # the gradients live in the sink: nothing is copied over the reduced ranges
    assert len(flats) == 1 and flats[0] is g
    sync.start_rest(g); sync.wait()
    want = torch.arange(n + 1, dtype=torch.float32).remainder(1000) * tot
    assert torch.equal(g[:n], want[:n]) and bool(torch.isnan(g[n]))
    assert sync.stats["early_ranges"] == 4 and sync.stats["bytes_early"] + sync.stats["bytes_rest"] == 4 * (n + 1)
    for p_ in params:
        L.clear_grad_sink(p_)
    # (b) the sharded form: equal slices on 64K-element boundaries, partial-sum slices per rank, one group only
    sync2 = mv.GradSync()
    enc2 = mv.MolEncoder(i=24, o=16, c=12, h_size=56, num_lstm=3)
    dec2 = mv.MolDecoder(i=16, o=24, c=12, num_gru=4, h_size=64, dtype=torch.float32)
    p2 = list(enc2.parameters()) + list(dec2.parameters())
    opt2 = mv.FusedSGD(p2, lr=1.2e-3, momentum=0.85, grad_sync=sync2, shard_optimizer=True)
    f2 = opt2._flat[0]
    S = f2["shard_elems"]
    assert opt2.shard and S % 65536 == 0 and world * S >= n + 1 and (world * S - (n + 1)) < world * 65536
    assert f2["g"].numel() == f2["p"].numel() == f2["buf"].numel() == world * S and opt2._partial.numel() == world * (S >> 16)
    assert sync2.allow_early is False
    opt2._moments_stale = True                                # what step() leaves behind
    try:
        opt2.state_dict(); refused = False
    except L.MvaeError:
        refused = True
    assert refused
    f2["buf"].fill_(float(rank + 1))
    opt2.gather_state()
    assert torch.equal(f2["buf"][:S], torch.ones(S)) and torch.equal(f2["buf"][S:], torch.full((S,), 2.0)) and not opt2._moments_stale
    for p_ in p2:
        L.clear_grad_sink(p_)
    try:
        mv.FusedSGD([{"params": [torch.nn.Parameter(torch.zeros(3))]}, {"params": [torch.nn.Parameter(torch.zeros(3))]}], lr=1e-3,
                    grad_sync=mv.GradSync(), shard_optimizer=True)
        two_groups_refused = False
    except ValueError:
        two_groups_refused = True
    assert two_groups_refused
    if rank == 0:
        np.save(os.path.join(out_dir, "ok.npy"), np.array([1.0]))
    dist.all_reduce(torch.zeros(1))
    dist.destroy_process_group()


def test_fused_sgd_two_ranks_gloo_bookkeeping(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    assert os.path.exists(os.path.join(str(tmp_path), "ok.npy"))
