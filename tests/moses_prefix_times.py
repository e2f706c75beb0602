"""Time of mosesvae.VAE.sample(return_logp=True) and VAE.decode(beam_width=4) with and without a prefix (bf16, B = 4096, max_len = 100,
a 30-token prefix by default), alternated in one process: ms per call (device events) of the device loops alone (VAE._sample_tokens,
VAE._beam_search: no copy to the host, no strings), whose time / (max_len - 1) is the token period.  Every path runs to max_len (4
launches per token), so the weights do not matter: a seeded random model is used.  A forced step skips the head and the draw (sampling) or
the per-row top-K (decoding), so a prefixed call should cost no more than a free one.
  --profile-only N --path sample|sample_prefix|decode|decode_prefix: just N device loops of one path (for rocprofv3 --kernel-trace --stats)."""
import argparse, json, os, sys, statistics
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import molecular_vae_amd as mv
from molecular_vae_amd import mosesvae as MV

PATHS = ["sample", "sample_prefix", "decode", "decode_prefix"]
ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=4096)
ap.add_argument("--max-len", type=int, default=100)
ap.add_argument("--prefix-len", type=int, default=30)
ap.add_argument("--beam-width", type=int, default=4)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--profile-only", type=int, default=0)
ap.add_argument("--path", default="sample_prefix", choices=PATHS)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)

torch.manual_seed(0)
model = MV.VAE(mv.OneHotVocab([chr(ord("a") + i) for i in range(26)])).to(dev).eval()
z = torch.randn(args.B, model.d_z, generator=torch.Generator().manual_seed(1)).to(dev)
prefix = torch.randint(0, 26, (args.prefix_len,), generator=torch.Generator().manual_seed(2))
forced = model._prefix_table(prefix, args.B, args.max_len, "times")


def run(path):
    if path == "sample":
        return model._sample_tokens(z, args.max_len, 1.0, 7)
    if path == "sample_prefix":
        return model._sample_tokens(z, args.max_len, 1.0, 7, forced=forced)
    return model._beam_search(z, args.beam_width, args.max_len, prefix=prefix if path == "decode_prefix" else None)


if args.profile_only:
    run(args.path)
    torch.cuda.synchronize()
    for _ in range(args.profile_only):
        run(args.path)
    torch.cuda.synchronize()
    print("profiled", args.profile_only, args.path, "device loops at B =", args.B, "max_len =", args.max_len)
    sys.exit(0)

for p in PATHS:                                        # warm-up (workspaces, LDS attributes)
    run(p)
torch.cuda.synchronize()
s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
per = {p: [] for p in PATHS}
for r in range(args.rounds):
    for p in (PATHS if r % 2 == 0 else PATHS[::-1]):
        s.record()
        for _ in range(args.calls):
            run(p)
        e.record(); torch.cuda.synchronize()
        per[p].append(s.elapsed_time(e) / args.calls)
res = {}
for p, v in per.items():
    med = statistics.median(v)
    res[p] = dict(ms_per_call=med, all=v, spread=(max(v) - min(v)) / med, token_period_us=med * 1e3 / (args.max_len - 1))
    print(p, json.dumps(res[p]), flush=True)
print("sample: prefix / free:", res["sample_prefix"]["ms_per_call"] / res["sample"]["ms_per_call"])
print("decode: prefix / free:", res["decode_prefix"]["ms_per_call"] / res["decode"]["ms_per_call"])
if args.out:
    json.dump(dict(B=args.B, max_len=args.max_len, prefix_len=args.prefix_len, beam_width=args.beam_width, calls=args.calls, res=res),
              open(args.out, "w"), indent=1)
