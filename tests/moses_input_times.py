"""What the input feed costs the MOSES train step (mosesvae.VAE, bf16, train mode, FusedAdam; the synthetic corpus of examples/train_moses.py:
lengths ~ N(38, 8) in [10, 57]): ms per step over whole epochs, wall clock around a device synchronisation, for
  (a) host0 / host8: the DataLoader + ShardedSampler + get_padded_collate_fn feed of examples/train_moses.py with 0 and with 8 worker
      processes (persistent; the workers collate without pinning -- a forked worker must not touch the device),
  (b) resident: one resident batch replayed -- what bench.py times, the floor,
  (c) device: data.MosesDeviceDataset.batches(bucket=0) -- the same batches as (a), collated by one launch each,
  (d) bucket8: data.MosesDeviceDataset.batches(bucket=8), with the mean T of its batches beside the mean T of (c),
alternated in one process after a warm-up epoch each, with the spread of the repeated rounds; and the collate launch by itself (device
events around back-to-back launches).  Not a pytest file.

    python tests/moses_input_times.py --B 1024 128 --out profiles/moses_input_times.json
"""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, nargs="+", default=[1024, 128])
ap.add_argument("--n", type=int, default=8192, help="corpus size")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--workers", type=int, default=8)
ap.add_argument("--bucket", type=int, default=8)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
sys.path.insert(0, ROOT)
import molecular_vae_amd as mv          # noqa: E402
from molecular_vae_amd import data as D, mosesvae as MV, vocab as VC   # noqa: E402

rs = np.random.RandomState(0)
lens = np.clip(rs.normal(38, 8, size=args.n), 10, 57).astype(int)
smiles = [D.synthetic_smiles(1, seed=1000 + i, lo=int(n), hi=int(n) + 1)[0] for i, n in enumerate(lens)]
vocab = VC.OneHotVocab.from_data(smiles)
dataset = D.MosesDeviceDataset(smiles, vocab, device=dev)


def report(per, steps):
    res = {}
    for k, v in per.items():
        med = statistics.median(v)
        res[k] = dict(ms_per_step=med, min=min(v), max=max(v), spread=(max(v) - min(v)) / med, steps_per_round=steps[k], all=v)
        print(f"{k:>10}: {med:8.4f} ms/step  (min {min(v):.4f}, max {max(v):.4f}, spread {100 * res[k]['spread']:.2f} %; {steps[k]} steps per round)",
              flush=True)
    return res


def run(B):
    torch.manual_seed(42)
    model = MV.VAE(vocab, dtype=torch.bfloat16).to(dev).train()
    optimizer = mv.FusedAdam(model.parameters(), lr=3e-4, max_grad_norm=50.0)
    sampler = mv.ShardedSampler(len(smiles), rank=0, world=1, seed=0)
    loaders = {"host0": torch.utils.data.DataLoader(smiles, batch_size=B, sampler=sampler, drop_last=True,
                                                    collate_fn=VC.get_padded_collate_fn(vocab, pin_memory=True))}
    if args.workers > 0:
        loaders[f"host{args.workers}"] = torch.utils.data.DataLoader(smiles, batch_size=B, sampler=sampler, drop_last=True, num_workers=args.workers,
                                                                     persistent_workers=True, collate_fn=VC.get_padded_collate_fn(vocab))
    n_steps = (len(smiles) // B)
    resident = next(iter(dataset.batches(B, epoch=0)))
    mean_T = {}

    def feed(kind, epoch):
        if kind in loaders:
            sampler.set_epoch(epoch)
            return (b.to(dev) for b in loaders[kind])
        if kind == "resident":
            return (resident for _ in range(n_steps))
        return dataset.batches(B, epoch=epoch, bucket=args.bucket if kind.startswith("bucket") else 0)

    def epoch_ms(kind, epoch):
        torch.cuda.synchronize()
        t0, steps, Ts = time.perf_counter(), 0, 0
        for batch in feed(kind, epoch):
            mv.moses_train_step(model, optimizer, 0.5, batch)
            steps += 1
            Ts += batch.x_pad.shape[1]
        torch.cuda.synchronize()
        mean_T.setdefault(kind, []).append(Ts / steps)
        return 1e3 * (time.perf_counter() - t0) / steps, steps

    kinds = list(loaders) + ["resident", "device", f"bucket{args.bucket}"]
    for k in kinds:                                            # warm-up: workspaces, the worker processes, the plan's code paths
        epoch_ms(k, 0)
    mean_T.clear()
    per, steps = {k: [] for k in kinds}, {}
    for r in range(args.rounds):
        for k in (kinds if r % 2 == 0 else kinds[::-1]):
            ms, steps[k] = epoch_ms(k, 1 + r)
            per[k].append(ms)
    print(f"mosesvae.VAE train step, B = {B}, bf16, corpus n = {len(smiles)}; {args.rounds} rounds of one epoch each, alternated", flush=True)
    res = report(per, steps)
    for k in kinds:
        res[k]["mean_T"] = statistics.mean(mean_T[k])
    print(f"mean T: device {res['device']['mean_T']:.2f}, bucket{args.bucket} {res[f'bucket{args.bucket}']['mean_T']:.2f}, "
          f"resident {res['resident']['mean_T']:.2f}", flush=True)
    # the collate launch by itself
    order = torch.randperm(len(smiles))[:B].to(dev)
    T = dataset.max_len + 2
    for _ in range(10):
        dataset.gather(order, T=T)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(200):
        dataset.gather(order, T=T)
    e.record(); torch.cuda.synchronize()
    res["collate_launch_us"] = 1e3 * s.elapsed_time(e) / 200
    print(f"mvae_moses_collate + its three output allocations, B = {B}, T = {T}, back to back: {res['collate_launch_us']:.2f} us each", flush=True)
    dataset.check_errors()
    return res


out = dict(n=len(smiles), rounds=args.rounds, workers=args.workers, bucket=args.bucket, device=torch.cuda.get_device_name(0), results={})
for B in args.B:
    out["results"][str(B)] = run(B)
if args.out:
    json.dump(out, open(args.out, "w"), indent=1)
