#!/usr/bin/env python3
"""Data-parallel runs of FusedSGD on ONE GPU box (the child processes of tests/test_gpu_fused_sgd.py): K training steps of the full model
with FusedSGD(momentum=0.85, max_grad_norm=5.0), either one process at global batch 2b or two ranks (gloo, sharing cuda:0) at b each.
  python tests/dp_sgd_equiv.py --out a.json
  python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 tests/dp_sgd_equiv.py --out b.json [--shard]
--poison-rank r: that rank writes a NaN into the optimiser's poison slot between backward and step() at --poison-step (what a persistent
launch that gives up leaves behind); every rank must skip that update."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
ap.add_argument("--b", type=int, default=32)
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
ap.add_argument("--lr", type=float, default=2e-2)
ap.add_argument("--shard", action="store_true", help="world > 1: FusedSGD(shard_optimizer=True)")
ap.add_argument("--poison-rank", type=int, default=-1)
ap.add_argument("--poison-step", type=int, default=1)
args = ap.parse_args()

import molecular_vae_amd as mv          # noqa: E402

rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
if world > 1:
    import torch.distributed as dist
    dist.init_process_group("gloo")
L_SEQ, VOCAB, LATENT = 120, 35, 292
torch.manual_seed(42)
model = mv.MolecularVAE(i=L_SEQ, o=LATENT, c=VOCAB, dtype=torch.float32 if args.dtype == "f32" else torch.bfloat16).to(dev)
sync = mv.GradSync() if world > 1 else None
opt = mv.FusedSGD(model.parameters(), lr=args.lr, momentum=0.85, max_grad_norm=5.0, grad_sync=sync, shard_optimizer=args.shard)
loss_fn = mv.make_loss_function(L_SEQ)
g = torch.Generator().manual_seed(7)
gb = 2 * args.b
data_all = torch.randint(0, VOCAB, (gb, L_SEQ), generator=g)
eps_all = 1e-2 * torch.randn(args.steps, gb, LATENT, generator=g)
per = gb // world
sl = slice(rank * per, (rank + 1) * per)
data = data_all[sl].to(dev)
ohe = torch.nn.functional.one_hot(data, VOCAB).float()
out = dict(loss=[], psum=[], gnorm=[], world=world)
for s in range(args.steps):
    opt.zero_grad(set_to_none=True)
    recon, mu, lv = model(data, eps=eps_all[s, sl].to(dev))
    loss = loss_fn(recon, ohe, mu, lv)
    loss.backward()
    if rank == args.poison_rank and s == args.poison_step:
        opt._flat[0]["poison"].fill_(float("nan"))
    opt.step()
    lt = loss.detach().clone()
    if world > 1:
        dist.all_reduce(lt); lt /= world
    out["loss"].append(float(lt))
    out["gnorm"].append(float(opt.last_grad_norm))
    out["psum"].append(float(sum(p.detach().double().abs().sum() for p in model.parameters())))
out["early_ranges"] = sync.stats["early_ranges"] if sync is not None else 0
out["skipped"] = float(opt.skipped_steps)
out["pcheck"] = [float(p.detach().double().sum()) for p in model.parameters()]
if args.shard and world > 1:
    try:
        opt.state_dict(); out["stale_state_dict_refused"] = False
    except mv._lib.MvaeError:
        out["stale_state_dict_refused"] = True
    opt.gather_state()
st = opt.state_dict()["state"]
out["bcheck"] = [float(st[i]["momentum_buffer"].double().sum()) for i in sorted(st)]
if world > 1:
    allr = [None] * world
    dist.all_gather_object(allr, dict(psum=out["psum"], skipped=out["skipped"], pcheck=out["pcheck"]))
    out["ranks"] = allr
if rank == 0:
    json.dump(out, open(args.out, "w"))
if world > 1:
    dist.destroy_process_group()
