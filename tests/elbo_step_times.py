"""Step time and peak memory of MolecularVAE training through the existing path (model(x) -> bce_kl_loss on the float one-hot, train_step)
vs the index-target ELBO (model.elbo, elbo_train_step), alternated in one process, FusedAdam, bf16.  Shapes "BxLxC".
--profile-only K --path existing|elbo: just K steps of one path at the first shape (for rocprofv3 --kernel-trace --stats and
tests/step_launches.py)."""
import argparse, json, os, sys, statistics
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import molecular_vae_amd as mv

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="1024x120x35,128x120x35,2048x256x64")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--min-ms", type=float, default=1000.0)
ap.add_argument("--profile-only", type=int, default=0)
ap.add_argument("--path", default="elbo", choices=["existing", "elbo"])
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)


def make(L, C):
    torch.manual_seed(42)
    m = mv.MolecularVAE(i=L, c=C, dtype=torch.bfloat16).to(dev)
    return m, mv.FusedAdam(m.parameters(), lr=8e-4, max_grad_norm=5.0)


def step(path, m, o, data, ohe, loss_fn):
    if path == "existing":
        return mv.train_step(m, o, loss_fn, data, ohe)
    return mv.elbo_train_step(m, o, data)


g = torch.Generator().manual_seed(0)
shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
if args.profile_only:
    B, L, C = shapes[0]
    m, o = make(L, C)
    data = torch.randint(0, C, (B, L), generator=g).to(dev)
    ohe = torch.nn.functional.one_hot(data, C).float() if args.path == "existing" else None
    for _ in range(args.profile_only):
        step(args.path, m, o, data, ohe, mv.make_loss_function(L))
    torch.cuda.synchronize()
    print("profiled", args.profile_only, args.path, "steps at", shapes[0])
    sys.exit(0)

res = {}
paths = ["existing", "elbo"]
for B, L, C in shapes:
    loss_fn = mv.make_loss_function(L)
    data = torch.randint(0, C, (B, L), generator=g).to(dev)
    ohe = torch.nn.functional.one_hot(data, C).float()
    runs = {p: make(L, C) for p in paths}
    peak = {}
    for p in paths:                                   # warm-up; then the peak of one steady step above what is allocated before it
        for _ in range(5):
            step(p, *runs[p], data, ohe, loss_fn)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(p, *runs[p], data, ohe, loss_fn)
        torch.cuda.synchronize()
        peak[p] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(5):
        step("existing", *runs["existing"], data, ohe, loss_fn)
    e.record(); torch.cuda.synchronize()
    K = max(20, int(args.min_ms / (s.elapsed_time(e) / 5)) + 1)
    per = {p: [] for p in paths}
    for r in range(args.rounds):
        for p in (paths if r % 2 == 0 else paths[::-1]):
            s.record()
            for _ in range(K):
                step(p, *runs[p], data, ohe, loss_fn)
            e.record(); torch.cuda.synchronize()
            per[p].append(s.elapsed_time(e) / K)
    key = f"{B}x{L}x{C}"
    res[key] = dict(steps_per_run=K, ms_per_step={p: dict(median=statistics.median(v), all=v) for p, v in per.items()},
                    peak_step_MiB=peak, onehot_MiB=ohe.numel() * 4 / 2 ** 20)
    print(key, json.dumps(res[key]), flush=True)
    del runs, ohe
    torch.cuda.empty_cache()
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)
