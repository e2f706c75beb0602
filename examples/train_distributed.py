#!/usr/bin/env python3
"""train_distributed.py of the reference, re-hosted on the MI355X path: one process per GPU under torch.distributed.run instead of
``nn.DataParallel`` (:72), each rank on its own shard of every global batch of 512 (:62-63), ``optim.SGD(lr=1.2e-3, momentum=0.85)`` (:73)
with the ``clip_grad_norm(5.0)`` of :91 as ONE fused optimiser (FusedSGD: the gradient all-reduce starts from inside backward),
``ReduceLROnPlateau('min', factor=0.8, patience=10, threshold=1e-3)`` on the validation loss (:74, :140), the exact-match accuracy of
:127-131, and rank 0 saving the reference's checkpoint dictionary (:145-151).

One deliberate difference: the reference trains AND tests on ``df[~msk]`` (:58-59), i.e. on the same 20 % of the data; here the split is a
real one (80 % train, the rest for validation).  The data set is a .smi/CSV file, or synthetic SMILES when none is given.

    python -m torch.distributed.run --nproc-per-node 8 examples/train_distributed.py --smi data/zinc_cleaned.smi --epochs 3000
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import molecular_vae_amd as mv                     # noqa: E402
from molecular_vae_amd import data as D            # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch_size", default=512, type=int, help="GLOBAL batch (train_distributed.py:62); every rank takes batch_size / world")
ap.add_argument("--smi", default=None)
ap.add_argument("--max_len", default=120, type=int)
ap.add_argument("--epochs", default=1, type=int)
ap.add_argument("--lr", default=3.0e-4 * 4, type=float)                                     # :73
ap.add_argument("--local_rank", default=int(os.environ.get("LOCAL_RANK", 0)), type=int)
ap.add_argument("--n_synth", default=4096, type=int, help="size of the synthetic corpus when no --smi is given")
ap.add_argument("--out_dir", default=".", help="where save.pt goes")
ap.add_argument("--report", default=None, help="write a JSON summary (per-epoch losses, accuracy, lr, molecules/s) here")
args = ap.parse_args()

rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
torch.cuda.set_device(args.local_rank)
dev = torch.device("cuda", args.local_rank)
if world > 1:
    torch.distributed.init_process_group("nccl", device_id=dev)
if args.batch_size % world:
    raise SystemExit(f"--batch_size {args.batch_size} is not a multiple of the world size {world}")
per_rank = args.batch_size // world

if args.smi:
    smiles = [s for s in D.load_smiles(args.smi) if len(s) < args.max_len]
else:
    smiles = D.synthetic_smiles(args.n_synth, seed=0)
max_len = args.max_len
vocab = D.build_vocab(smiles, max_len)
charset = {i: c for c, i in vocab.items()}
enc = D.encode_smiles(smiles, vocab, max_len)
msk = np.random.RandomState(1).rand(len(enc)) < 0.8                       # :57, but train on msk and validate on ~msk
train_ds, test_ds = D.DeviceDataset(enc[msk], len(vocab), dev), D.DeviceDataset(enc[~msk], len(vocab), dev)

torch.manual_seed(42)                                                     # :69
model = mv.MolecularVAE(i=max_len, c=len(vocab)).to(dev)                  # :71
sync = mv.GradSync() if world > 1 else None
optimizer = mv.FusedSGD(model.parameters(), lr=args.lr, momentum=0.85, max_grad_norm=5.0, grad_sync=sync)          # :73, :91
scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, "min", factor=0.8, patience=10, threshold=1e-3)  # :74
loss_function = mv.make_loss_function(max_len)
log_interval = 100

report = dict(batch_size=args.batch_size, world=world, n_train=len(train_ds), n_test=len(test_ds), vocab=len(vocab), epochs=[])
ckpt_path = os.path.join(args.out_dir, "save.pt")
for epoch in range(1, args.epochs + 1):
    model.train()
    total, n, nb = torch.zeros((), device=dev), 0, 0
    t_beg, t_end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t_beg.record()
    for batch_idx, (data, ohe) in enumerate(train_ds.batches(per_rank, epoch=epoch, seed=0, rank=rank, world=world)):
        loss = mv.train_step(model, optimizer, loss_function, data, ohe)          # :82-96
        total += loss; n += data.shape[0]; nb += 1
        if batch_idx % log_interval == 0 and rank == 0:
            print(f"train: {epoch} / {batch_idx}\t{float(loss):.4f}", flush=True)
    t_end.record(); torch.cuda.synchronize()
    epoch_ms = t_beg.elapsed_time(t_end)
    train_loss = float(total) / max(nb, 1)
    # test(epoch), :101-136: forward-only loss and exact-match accuracy over this rank's shard, averaged over the ranks
    val, acc = mv.evaluate(model, loss_function, test_ds.batches(per_rank, shuffle=False, rank=rank, world=world, drop_last=False))
    if world > 1:                                         # every rank must take the same ReduceLROnPlateau decision
        t = torch.tensor([val, acc, train_loss], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t); val, acc, train_loss = (t / world).tolist()
    scheduler.step(val)                                   # :140
    lr = optimizer.param_groups[-1]["lr"]                 # :141-143
    if rank == 0:
        print(f"epoch {epoch}: train {train_loss:.5f}  val {val:.5f}  acc {acc:.4f}  lr {lr:.2e}", flush=True)
        # :145-151 (no latent_size in this dictionary); the state dict has torch.optim.SGD's layout
        mv.save_checkpoint(ckpt_path, model, optimizer, epoch, charset, max_len)
        report["epochs"].append(dict(epoch=epoch, mean_batch_loss=train_loss, val_loss=val, val_acc=acc, lr=lr,
                                     skipped_steps=float(optimizer.skipped_steps),
                                     molecules_per_s=n * world / (epoch_ms * 1e-3)))
if rank == 0 and args.report:
    import json
    report["checkpoint"] = ckpt_path
    json.dump(report, open(args.report, "w"))
if world > 1:
    torch.distributed.destroy_process_group()
