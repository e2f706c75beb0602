"""Time of mosesvae.VAE.sample on its default path vs with top-k / top-p truncation and return_logp (bf16, B = 1024, max_len = 100 by
default), alternated in one process: ms per call (device events) for the whole call and for the device loop alone (VAE._sample_tokens: no
copy to the host, no strings), whose time / (max_len - 1) is the token period.  Both run to max_len, so the weights do not matter: a
seeded random model is used.
  --profile-only N --path default|filtered: just N device loops of one path (for rocprofv3 --kernel-trace --stats).
  --generate N: moses_generate of N samples at --batch-size against the same number of sample() calls (wall clock, host work included), for a
    near-uniform model with N(0, I) latents (everything unique: every row goes to the host) and with top_k = 2, max_len = 6 on the zeros
    prior (almost nothing unique)."""
import argparse, json, os, sys, statistics, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import molecular_vae_amd as mv
from molecular_vae_amd import mosesvae as MV

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=1024)
ap.add_argument("--max-len", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--top-k", type=int, default=8)
ap.add_argument("--top-p", type=float, default=0.9)
ap.add_argument("--profile-only", type=int, default=0)
ap.add_argument("--path", default="filtered", choices=["default", "filtered"])
ap.add_argument("--generate", type=int, default=0)
ap.add_argument("--batch-size", type=int, default=4096)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)

torch.manual_seed(0)
model = MV.VAE(mv.OneHotVocab([chr(ord("a") + i) for i in range(26)])).to(dev).eval()
z = torch.randn(args.B, model.d_z, generator=torch.Generator().manual_seed(1)).to(dev)
K, P = model._check_filters(args.top_k, args.top_p)


def run(path):
    if path == "default":
        return model.sample(args.B, max_len=args.max_len, z=z, seed=7)
    if path == "filtered":
        return model.sample(args.B, max_len=args.max_len, z=z, seed=7, top_k=args.top_k, top_p=args.top_p, return_logp=True)
    if path == "loop_default":
        return model._sample_tokens(z, args.max_len, 1.0, 7, filtered=False)
    return model._sample_tokens(z, args.max_len, 1.0, 7, K, P)


if args.profile_only:
    run("loop_" + args.path)
    torch.cuda.synchronize()
    for _ in range(args.profile_only):
        run("loop_" + args.path)
    torch.cuda.synchronize()
    print("profiled", args.profile_only, args.path, "device loops at B =", args.B, "max_len =", args.max_len)
    sys.exit(0)

if args.generate:
    n, bs = args.generate, args.batch_size
    cases = {"all_unique": dict(prior="normal", kw=dict(max_len=args.max_len)), "few_unique": dict(prior="zeros", kw=dict(max_len=6, top_k=2))}
    res = {}
    for name, c in cases.items():
        model.prior = c["prior"]
        model.seed_noise(3)

        def by_sample():
            seen = set()
            for j, b0 in enumerate(range(0, n, bs)):
                s, _ = model.sample(min(bs, n - b0), seed=j, **c["kw"])
                seen.update(s)                                  # hugesample.py: hash the strings on the host
            return len(seen)

        def by_generate():
            return mv.moses_generate(model, n, batch_size=bs, seed=0, **c["kw"])["unique"]
        t = {"sample": [], "generate": []}
        uniq = {}
        by_sample(); by_generate()                              # warm-up
        for r in range(args.rounds):
            for p, f in ((("sample", by_sample), ("generate", by_generate)) if r % 2 == 0 else (("generate", by_generate), ("sample", by_sample))):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                uniq[p] = f()
                torch.cuda.synchronize(); t[p].append(time.perf_counter() - t0)
        res[name] = {p: dict(samples_per_s=n / statistics.median(v), s_per_call_all=v, unique=uniq[p]) for p, v in t.items()}
        print(name, json.dumps(res[name]), flush=True)
    if args.out:
        json.dump(dict(n=n, batch_size=bs, res=res), open(args.out, "w"), indent=1)
    sys.exit(0)

paths = ["default", "filtered", "loop_default", "loop_filtered"]
for p in paths:                                        # warm-up (workspaces, LDS attributes)
    run(p)
torch.cuda.synchronize()
s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
per = {p: [] for p in paths}
for r in range(args.rounds):
    for p in (paths if r % 2 == 0 else paths[::-1]):
        s.record()
        for _ in range(args.calls):
            run(p)
        e.record(); torch.cuda.synchronize()
        per[p].append(s.elapsed_time(e) / args.calls)
res = {}
for p, v in per.items():
    med = statistics.median(v)
    res[p] = dict(ms_per_call=med, all=v, spread=(max(v) - min(v)) / med)
    if p.startswith("loop_"):
        res[p]["token_period_us"] = med * 1e3 / (args.max_len - 1)
    else:
        res[p]["molecules_per_s"] = args.B / (med / 1e3)
    print(p, json.dumps(res[p]), flush=True)
for p in ("default", "filtered"):                       # the host's share of a whole call is the id-to-string conversion: it grows with the lengths
    res[p]["mean_string_length"] = statistics.mean(len(t) for t in run(p)[0])
    print(p, "mean string length", res[p]["mean_string_length"])
print("filtered / default, whole call:", res["filtered"]["ms_per_call"] / res["default"]["ms_per_call"])
print("filtered / default, token period:", res["loop_filtered"]["ms_per_call"] / res["loop_default"]["ms_per_call"])
if args.out:
    json.dump(dict(B=args.B, max_len=args.max_len, calls=args.calls, top_k=args.top_k, top_p=args.top_p, res=res), open(args.out, "w"), indent=1)
