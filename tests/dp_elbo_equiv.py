#!/usr/bin/env python3
"""Two-rank check of the index-target ELBO (MolecularVAE.elbo / elbo_train_step) against the existing path (model(x) -> bce_kl_loss on the
float one-hot, train_step) under data parallelism: every rank holds two copies of the same model, each with its own FusedAdam + GradSync
(early all-reduce ranges from the decoder's backward), and runs K steps of both paths on the same shard and noise.  Rank 0 writes the
all-reduced losses, global gradient norms and parameter sums of both paths.  Usage on a GPU box (two ranks sharing cuda:0, gloo):
  python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29541 tests/dp_elbo_equiv.py --out elbo2.json"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--b", type=int, default=32, help="per-rank batch")
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
args = ap.parse_args()

import torch.distributed as dist  # noqa: E402
import molecular_vae_amd as mv  # noqa: E402

rank = int(os.environ.get("RANK", 0)); world = int(os.environ.get("WORLD_SIZE", 1))
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
if world > 1:
    dist.init_process_group("gloo")
L_SEQ, VOCAB, LATENT = 120, 35, 292
torch.manual_seed(42)
dtype = torch.float32 if args.dtype == "f32" else torch.bfloat16
model_a = mv.MolecularVAE(i=L_SEQ, o=LATENT, c=VOCAB, dtype=dtype).to(dev)
model_b = mv.MolecularVAE(i=L_SEQ, o=LATENT, c=VOCAB, dtype=dtype).to(dev)      # not a deepcopy: each decoder pairs with its own encoder
model_b.load_state_dict(model_a.state_dict())
opts = [mv.FusedAdam(m.parameters(), lr=8e-4, max_grad_norm=3.0, grad_sync=(mv.GradSync() if world > 1 else None)) for m in (model_a, model_b)]
loss_fn = mv.make_loss_function(L_SEQ)
g = torch.Generator().manual_seed(7)
gb = world * args.b
data_all = torch.randint(0, VOCAB, (gb, L_SEQ), generator=g)
eps_all = 1e-2 * torch.randn(args.steps, gb, LATENT, generator=g)
sl = slice(rank * args.b, (rank + 1) * args.b)
data = data_all[sl].to(dev)
ohe = torch.nn.functional.one_hot(data, VOCAB).float()
out = {k: [] for k in ("loss_a", "loss_b", "gnorm_a", "gnorm_b", "psum_a", "psum_b")}
out["world"] = world
for s in range(args.steps):
    eps = eps_all[s, sl].to(dev)
    la = mv.train_step(model_a, opts[0], loss_fn, data, ohe, eps=eps)
    lb = mv.elbo_train_step(model_b, opts[1], data, eps=eps)
    for tag, l_, opt, m in (("a", la, opts[0], model_a), ("b", lb, opts[1], model_b)):
        lt = l_.clone()
        if world > 1:
            dist.all_reduce(lt); lt /= world
        out["loss_" + tag].append(float(lt))
        out["gnorm_" + tag].append(float(opt.last_grad_norm))
        out["psum_" + tag].append(float(sum(p.detach().double().abs().sum() for p in m.parameters())))
out["early_ranges"] = [o.grad_sync.stats["early_ranges"] if o.grad_sync is not None else 0 for o in opts]
if rank == 0 and args.out:
    json.dump(out, open(args.out, "w"))
    print(out)
if world > 1:
    dist.destroy_process_group()
