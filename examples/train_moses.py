#!/usr/bin/env python3
"""The MOSES character-VAE trainer (moses_train_distrib.py:160-356 surface) on the MI355X path: char vocabulary from the corpus, sorted
collate, KL annealing, cosine LR with restarts, clip 50 + Adam(3e-4), rank-0 checkpoint + vocabulary pickle + samples per epoch.  One
process per GPU under torch.distributed.run (the reference's DistributedDataParallel / DistributedSampler lines are commented out there;
here the gradient all-reduce is FusedAdam's GradSync and the data shard is ShardedSampler).

    python examples/train_moses.py --smi data/moses_train.smi --epochs 2 -b 128
    python examples/train_moses.py --smi data/moses_train.smi --epochs 2 -b 1024 --device-data --bucket 8

--device-data keeps the tokenised corpus in HBM and collates every batch in one launch (data.MosesDeviceDataset: the same batches, no host
work in the step); --bucket K additionally groups rows of similar length within windows of K batches, which shortens the batches' T.
--augment (with --device-data) is SMILES enumeration: every molecule goes in under another randomised spelling of the same graph each
epoch (MosesDeviceDataset.batches(augment=True): one mvae_smiles_rewrite_corpus launch in front of the collate); rows that cannot be
respelled, or whose spelling does not fit the batch's width plus --augment-slack, go in unchanged and are counted.
"""
import argparse
import os
import pickle
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import molecular_vae_amd as mv                          # noqa: E402
from molecular_vae_amd import data as D, mosesvae as MV, vocab as VC, ops   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--local_rank", default=int(os.environ.get("LOCAL_RANK", 0)), type=int)     # moses_train_distrib.py:27
ap.add_argument("--smi", default=None)
ap.add_argument("-b", "--batch_size", default=128, type=int)                                # moses_train_distrib.py:177
ap.add_argument("--epochs", default=100, type=int)
ap.add_argument("--n_samples", default=1024, type=int)
ap.add_argument("--n_synth", default=8192, type=int, help="size of the synthetic corpus when no --smi is given")
ap.add_argument("--out_dir", default=".")
ap.add_argument("--word-dropout", default=0.0, type=float, help="probability that a decoder input token becomes <unk> (0 = off)")
ap.add_argument("--free-bits", default=0.0, type=float, help="nats per latent dimension that cost no KL (0 = off)")
ap.add_argument("--kl-cycle", default=0, type=int, help="cyclical KL weight with cycles of this many epochs (0: the linear KLAnnealer)")
ap.add_argument("--device-data", action="store_true", help="feed from a device-resident corpus (data.MosesDeviceDataset) instead of the DataLoader")
ap.add_argument("--bucket", default=0, type=int, help="with --device-data: group rows of similar length within windows of this many batches (0 = off)")
ap.add_argument("--augment", action="store_true", help="with --device-data: SMILES enumeration -- every molecule goes in under another randomised "
                                                       "spelling each epoch (one more launch per batch, no host work)")
ap.add_argument("--augment-slack", default=0, type=int, help="with --augment: extra columns per batch for spellings longer than the original")
ap.add_argument("--selfies", action="store_true", help="with --device-data: train on the corpus encoded as SELFIES on the device "
                                                       "(MosesDeviceDataset.selfies(): this library's own encoding, not the selfies package's)")
ap.add_argument("--report", default=None, help="write a JSON summary (the per-epoch postfix dictionaries + samples) here")
args = ap.parse_args()
if args.bucket and not args.device_data:
    ap.error("--bucket needs --device-data")
if args.augment and not args.device_data:
    ap.error("--augment needs --device-data")
if args.selfies and (not args.device_data or args.augment):
    ap.error("--selfies needs --device-data and excludes --augment (the rewrite respells SMILES rows)")

rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
torch.cuda.set_device(args.local_rank)
dev = torch.device("cuda", args.local_rank)
if world > 1:
    torch.distributed.init_process_group("nccl", device_id=dev)

if args.smi:
    smiles = D.load_smiles(args.smi)
else:                                                    # synthetic MOSES-like corpus (no data ships with the reference)
    rs = np.random.RandomState(0)
    lens = np.clip(rs.normal(38, 8, size=args.n_synth), 10, 57).astype(int)
    smiles = [D.synthetic_smiles(1, seed=1000 + i, lo=int(n), hi=int(n) + 1)[0] for i, n in enumerate(lens)]
vocab = VC.OneHotVocab.from_data(smiles)                 # moses_train_distrib.py:166
collate = VC.get_padded_collate_fn(vocab, pin_memory=True)
sampler = mv.ShardedSampler(len(smiles), rank=rank, world=world, seed=0)
loader = torch.utils.data.DataLoader(smiles, batch_size=args.batch_size, sampler=sampler, collate_fn=collate, drop_last=True)
device_data = D.MosesDeviceDataset(smiles, vocab, device=dev) if args.device_data else None
if args.selfies:                                         # one encode launch; the model is built on the SELFIES vocabulary
    device_data = device_data.selfies()
    print(f"--selfies: {len(device_data)} of {len(smiles)} rows encoded", flush=True)
    vocab = device_data.vocab
    sampler = mv.ShardedSampler(len(device_data), rank=rank, world=world, seed=0)

torch.manual_seed(42)
model = MV.VAE(vocab).to(dev)
sync = mv.GradSync() if world > 1 else None
optimizer = mv.FusedAdam(model.parameters(), lr=3e-4, max_grad_norm=50.0, grad_sync=sync)   # :188, :227
model.word_dropout, model.free_bits = args.word_dropout, args.free_bits                       # remedies for posterior collapse
kl_annealer = mv.CyclicalKLAnnealer(args.kl_cycle) if args.kl_cycle > 0 else mv.KLAnnealer(args.epochs)    # :47-58, :185
lr_annealer = mv.CosineAnnealingLRWithRestart(optimizer)                                     # :61-89, :195

report = dict(vocab=len(vocab), n=len(smiles), epochs=[], samples=[])
for epoch in range(args.epochs):
    sampler.set_epoch(epoch)
    kl_weight = kl_annealer(epoch)
    if device_data is not None:                          # the same shard of the same permutation as the sampler's (seed 0 + epoch)
        batches = device_data.batches(args.batch_size, epoch=epoch, seed=0, rank=rank, world=world, bucket=args.bucket, augment=args.augment,
                                      augment_seed=0, augment_slack=args.augment_slack)
    else:
        batches = (b.to(dev) for b in loader)
    post = mv.moses_train_epoch(model, epoch, batches, kl_weight, optimizer, log_every=100 if rank == 0 else 0)
    if rank == 0:                                        # :342-353
        print(post, flush=True)
        if args.augment:
            counts = device_data.augment_counts.tolist()
            print("augment: respelled", counts[0], "of", sum(counts), "rows so far; unchanged by reason:",
                  {ops.REWRITE_STATUS_NAMES[i]: c for i, c in enumerate(counts[:14]) if i and c}, flush=True)
        report["epochs"].append(post)
        torch.save(model.state_dict(), os.path.join(args.out_dir, "trained_save.pt"))
        with open(os.path.join(args.out_dir, "vocab.pkl"), "wb") as f:
            pickle.dump(vocab, f)
        model.eval()
        res, _ = model.sample(min(args.n_samples, 64), max_len=60)
        model.train()
        for s in res[:5]:
            print("sample:", s)
        report["samples"] = res[:16]
    lr_annealer.step()                                   # :355
if rank == 0 and args.report:
    import json
    json.dump(report, open(args.report, "w"))
if world > 1:
    torch.distributed.destroy_process_group()
