"""Step time of the full-size bf16 MolecularVAE with FusedSGD vs FusedAdam vs torch.optim.SGD + clip_grad_norm_, alternated in one process
--profile-only K: just K FusedSGD steps (for rocprofv3 --kernel-trace --stats)."""
import argparse, json, os, sys, statistics
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import molecular_vae_amd as mv

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="128,1024")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--min-ms", type=float, default=1000.0)
ap.add_argument("--profile-only", type=int, default=0)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
loss_fn = mv.make_loss_function(120)


def make(kind):
    torch.manual_seed(42)
    m = mv.MolecularVAE(dtype=torch.bfloat16).to(dev)
    if kind == "fused_sgd":
        o = mv.FusedSGD(m.parameters(), lr=1.2e-3, momentum=0.85, max_grad_norm=5.0)
    elif kind == "fused_adam":
        o = mv.FusedAdam(m.parameters(), lr=8e-4, max_grad_norm=5.0)
    else:
        o = torch.optim.SGD(m.parameters(), lr=1.2e-3, momentum=0.85)
    return m, o


def step(kind, m, o, data, ohe):
    if kind == "torch_sgd":
        o.zero_grad(set_to_none=True)
        r, mu, lv = m(data)
        loss = loss_fn(r, ohe, mu, lv)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 5.0)
        o.step()
        return loss.detach()
    return mv.train_step(m, o, loss_fn, data, ohe)


g = torch.Generator().manual_seed(0)
if args.profile_only:
    m, o = make("fused_sgd")
    data = torch.randint(0, 35, (1024, 120), generator=g).to(dev)
    ohe = torch.nn.functional.one_hot(data, 35).float()
    for _ in range(args.profile_only):
        step("fused_sgd", m, o, data, ohe)
    torch.cuda.synchronize()
    print("profiled", args.profile_only, "steps; skipped", float(o.skipped_steps))
    sys.exit(0)

res = {}
for B in [int(b) for b in args.batches.split(",")]:
    data = torch.randint(0, 35, (B, 120), generator=g).to(dev)
    ohe = torch.nn.functional.one_hot(data, 35).float()
    kinds = ["fused_sgd", "fused_adam", "torch_sgd"]
    runs = {k: make(k) for k in kinds}
    for k in kinds:                                   # warm-up + calibration
        for _ in range(5):
            step(k, *runs[k], data, ohe)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(5):
        step("fused_sgd", *runs["fused_sgd"], data, ohe)
    e.record(); torch.cuda.synchronize()
    K = max(20, int(args.min_ms / (s.elapsed_time(e) / 5)) + 1)
    per = {k: [] for k in kinds}
    for r in range(args.rounds):
        for k in (kinds if r % 2 == 0 else kinds[::-1]):
            s.record()
            for _ in range(K):
                loss = step(k, *runs[k], data, ohe)
            e.record(); torch.cuda.synchronize()
            per[k].append(s.elapsed_time(e) / K)
    res[B] = dict(steps_per_run=K, ms_per_step={k: dict(median=statistics.median(v), all=v) for k, v in per.items()},
                  skipped_fused_sgd=float(runs["fused_sgd"][1].skipped_steps))
    print(B, json.dumps(res[B]), flush=True)
    del runs
    torch.cuda.empty_cache()
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)
