"""Time of mosesvae.VAE.sample vs VAE.decode at beam widths 1, 4 and 8 (bf16, B = 1024, max_len = 100 by default), alternated in one
process: ms per call and molecules per second.  Both run to max_len (4 launches per token), so the weights do not matter: a seeded random
model is used.  --profile-only N --path sample|k1|k4|k8: just N calls of one path (for rocprofv3 --kernel-trace --stats)."""
import argparse, json, os, sys, statistics
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import molecular_vae_amd as mv
from molecular_vae_amd import mosesvae as MV

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=1024)
ap.add_argument("--max-len", type=int, default=100)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--profile-only", type=int, default=0)
ap.add_argument("--path", default="k1", choices=["sample", "k1", "k4", "k8"])
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)

torch.manual_seed(0)
model = MV.VAE(mv.OneHotVocab([chr(ord("a") + i) for i in range(26)])).to(dev).eval()
z = torch.randn(args.B, model.d_z, generator=torch.Generator().manual_seed(1)).to(dev)


def run(path):
    if path == "sample":
        return model.sample(args.B, max_len=args.max_len, z=z, seed=7)
    return model.decode(z, beam_width=int(path[1:]), max_len=args.max_len)


if args.profile_only:
    run(args.path)
    torch.cuda.synchronize()
    for _ in range(args.profile_only):
        run(args.path)
    torch.cuda.synchronize()
    print("profiled", args.profile_only, args.path, "calls at B =", args.B, "max_len =", args.max_len)
    sys.exit(0)

paths = ["sample", "k1", "k4", "k8"]
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
    res[p] = dict(ms_per_call=med, all=v, molecules_per_s=args.B / (med / 1e3))
    print(p, json.dumps(res[p]), flush=True)
print("k1 / sample:", res["k1"]["ms_per_call"] / res["sample"]["ms_per_call"])
if args.out:
    json.dump(dict(B=args.B, max_len=args.max_len, calls=args.calls, res=res), open(args.out, "w"), indent=1)
