"""Cost of the SMILES syntax mask in mosesvae.VAE.sample (bf16, B = 1024, max_len = 100 by default): ms per call (device events) of the
device loop (VAE._sample_tokens: no copy to the host, no strings) and of the whole call, for the filtered sampling path (return_logp: the
launch the syntax launch is a variant of) and for syntax=True, alternated in one process; medians over the rounds.  Every loop runs to
max_len whatever the rows do, so the weights do not matter: a seeded random model over the synthetic_smiles vocabulary is used.
  --profile-only N --path filtered|syntax: just N device loops of one path (for a kernel trace).
  --root DIR --filtered-only: time the filtered path alone with the package of another checkout (the previous commit's, built), to be
    alternated with `--filtered-only` runs of this one: the filtered path must cost what it cost before the flag was added."""
import argparse, json, os, sys, statistics
import torch
_ap = argparse.ArgumentParser(add_help=False)
_ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.abspath(_ap.parse_known_args()[0].root))
import molecular_vae_amd as mv
from molecular_vae_amd import data as D, mosesvae as MV

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=1024)
ap.add_argument("--max-len", type=int, default=100)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=40)          # a timed window of 0.3 - 0.7 s
ap.add_argument("--root", default=None)
ap.add_argument("--filtered-only", action="store_true")
ap.add_argument("--profile-only", type=int, default=0)
ap.add_argument("--path", default="syntax", choices=["filtered", "syntax"])
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)

torch.manual_seed(0)
model = MV.VAE(mv.OneHotVocab.from_data(D.synthetic_smiles(2048, seed=0))).to(dev).eval()
z = torch.randn(args.B, model.d_z, generator=torch.Generator().manual_seed(1)).to(dev)


def run(path):
    if path == "filtered":
        return model.sample(args.B, max_len=args.max_len, z=z, seed=7, return_logp=True)
    if path == "syntax":
        return model.sample(args.B, max_len=args.max_len, z=z, seed=7, return_logp=True, syntax=True)
    return model._sample_tokens(z, args.max_len, 1.0, 7, **(dict(syntax=True) if path == "loop_syntax" else {}))


if args.profile_only:
    run("loop_" + args.path)
    torch.cuda.synchronize()
    for _ in range(args.profile_only):
        run("loop_" + args.path)
    torch.cuda.synchronize()
    print("profiled", args.profile_only, args.path, "device loops at B =", args.B, "max_len =", args.max_len)
    sys.exit(0)

paths = ["filtered", "loop_filtered"] if args.filtered_only else ["filtered", "syntax", "loop_filtered", "loop_syntax"]
for p in paths:                                        # warm-up (workspaces, the token table)
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
    print(p, json.dumps(res[p]), flush=True)
if args.filtered_only:
    if args.out:
        json.dump(dict(B=args.B, max_len=args.max_len, calls=args.calls, rounds=args.rounds, root=args.root, res=res), open(args.out, "w"), indent=1)
    sys.exit(0)
for p in ("filtered", "syntax"):
    out = run(p)[0]
    res[p]["mean_string_length"] = statistics.mean(len(t) for t in out)
x = model._sample_tokens(z, args.max_len, 1.0, 7, syntax=True)[0]
res["syntax"]["well_formed"] = float(model.syntax_valid(x).float().mean())
x = model._sample_tokens(z, args.max_len, 1.0, 7)[0]
res["filtered"]["well_formed"] = float(model.syntax_valid(x).float().mean())
res["ratio_loop"] = res["loop_syntax"]["ms_per_call"] / res["loop_filtered"]["ms_per_call"]
res["ratio_call"] = res["syntax"]["ms_per_call"] / res["filtered"]["ms_per_call"]
print("syntax / filtered, device loop:", res["ratio_loop"], " whole call:", res["ratio_call"])
print("well-formed: filtered", res["filtered"]["well_formed"], "syntax", res["syntax"]["well_formed"])
if args.out:
    json.dump(dict(B=args.B, max_len=args.max_len, calls=args.calls, rounds=args.rounds, res=res), open(args.out, "w"), indent=1)
