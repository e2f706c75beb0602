"""Time of mosesvae.VAE.decode with and without the syntax constraint (bf16, B = 1024, beam widths 1 and 4, max_len = 100 by default),
alternated in one process: ms per call of the whole decode (events around --calls calls, median of --rounds rounds) and us per launch of the
beam kernel (device time of the kernels named moses_beam_step in a torch profile of one call).  Both paths run to max_len (4 launches per
token), so the weights do not matter: a seeded random model over the synthetic_smiles alphabet is used.  On a tree whose decode() has no
`syntax` argument only the plain path is timed, so the same script measures an older commit for comparison.
--profile-only N --path k1|k4|k1s|k4s: just N calls of one path (for rocprofv3 --kernel-trace --stats)."""
import argparse, inspect, json, os, sys, statistics
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import molecular_vae_amd as mv
from molecular_vae_amd import mosesvae as MV

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=1024)
ap.add_argument("--max-len", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--profile-only", type=int, default=0)
ap.add_argument("--path", default="k1", choices=["k1", "k4", "k1s", "k4s"])
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)

torch.manual_seed(0)
model = MV.VAE(mv.OneHotVocab(set("CNOSFcnos()=#123[]@H+-lBr"))).to(dev).eval()
z = torch.randn(args.B, model.d_z, generator=torch.Generator().manual_seed(1)).to(dev)
has_syntax = "syntax" in inspect.signature(MV.VAE.decode).parameters


def run(path):
    kw = dict(syntax=True) if path.endswith("s") else {}
    return model.decode(z, beam_width=int(path[1]), max_len=args.max_len, **kw)


if args.profile_only:
    run(args.path)
    torch.cuda.synchronize()
    for _ in range(args.profile_only):
        run(args.path)
    torch.cuda.synchronize()
    print("profiled", args.profile_only, args.path, "calls at B =", args.B, "max_len =", args.max_len)
    sys.exit(0)

paths = ["k1", "k4"] + (["k1s", "k4s"] if has_syntax else [])
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
from torch.profiler import profile, ProfilerActivity
res = {}
for p in paths:
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        run(p)
        torch.cuda.synchronize()
    evs = [ev for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA]
    beam = [ev.device_time for ev in evs if "moses_beam_step" in ev.name]
    gru = [ev.device_time for ev in evs if "step_fwd" in ev.name or "gru_step" in ev.name or "lstm_step" in ev.name]
    med = statistics.median(per[p])
    res[p] = dict(ms_per_call=med, all=per[p], beam_us_per_launch=sum(beam) / max(len(beam), 1), beam_launches=len(beam),
                  gru_us_per_token=sum(gru) / max(len(beam), 1))
    print(p, json.dumps(res[p]), flush=True)
if has_syntax:
    for k in ("k1", "k4"):
        print(f"{k}: syntax on / off: decode {res[k + 's']['ms_per_call'] / res[k]['ms_per_call']:.3f}, beam launch "
              f"{res[k + 's']['beam_us_per_launch'] / res[k]['beam_us_per_launch']:.3f}")
if args.out:
    json.dump(dict(B=args.B, max_len=args.max_len, calls=args.calls, has_syntax=has_syntax, res=res), open(args.out, "w"), indent=1)
