"""Time of the latent diagnostics on one MI355X: mvae_gauss_pairwise_lse at Nz = Nx = 4096 and 16384 (d_z = 160) against the FP32
vector roof (3 lane-operations per pair and dimension at 78.6e12 lane-FMA/s), VAE.iw_log_likelihood for 1024 molecules at K = 100 and
K = 500, and train.moses_latent_diagnostics over 16384 molecules.  A bf16 VAE (26 symbols, V = 30) with seeded random weights; molecules
are random strings of 20 .. 50 symbols (MOSES-like lengths).  Device events around calls that end in a synchronise; medians of --rounds."""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import molecular_vae_amd as mv
from molecular_vae_amd import mosesvae as MV, ops

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--diag-n", type=int, default=16384)
ap.add_argument("--diag-k", type=int, default=500)
ap.add_argument("--skip", default="", help="comma list of pairwise,iw,diag")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
res = {}
ev = lambda: torch.cuda.Event(enable_timing=True)


def timed(fn, calls):
    fn(); torch.cuda.synchronize()
    out = []
    for _ in range(args.rounds):
        s, e = ev(), ev()
        s.record()
        for _ in range(calls):
            fn()
        e.record(); torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / calls)
    return statistics.median(out), out


if "pairwise" not in args.skip:
    g = torch.Generator(device="cpu").manual_seed(0)
    for N in (4096, 16384):
        dz = 160
        mu = torch.randn(N, dz, generator=g).to(dev)
        lv = (torch.rand(N, dz, generator=g) * 3 - 2).to(dev)
        z = (mu + torch.exp(0.5 * lv) * torch.randn(N, dz, generator=g).to(dev)).contiguous()
        out = torch.empty(N, device=dev)
        ms, allv = timed(lambda: ops.gauss_pairwise_lse(z, mu, lv, out, N, N, dz), 20 if N == 4096 else 5)
        roof_ms = 3.0 * N * N * dz / 78.6e12 * 1e3
        res[f"pairwise_N{N}"] = dict(ms=ms, all=allv, roof_ms=roof_ms, share_of_fp32_roof=roof_ms / ms,
                                     lane_ops_per_s=3.0 * N * N * dz / (ms / 1e3))
        print(f"pairwise_N{N}", json.dumps(res[f"pairwise_N{N}"]), flush=True)

torch.manual_seed(0)
model = MV.VAE(mv.OneHotVocab([chr(ord("a") + i) for i in range(26)])).to(dev).eval()
rs = np.random.RandomState(1)


def molecules(n):
    return ["".join(chr(ord("a") + c) for c in rs.randint(0, 26, L)) for L in rs.randint(20, 51, n)]


if "iw" not in args.skip:
    xs = [model.string2tensor(s, device="cpu") for s in molecules(1024)]
    for K in (100, 500):
        ms, allv = timed(lambda: model.iw_log_likelihood(xs, n_samples=K, seed=3), 1)
        res[f"iw_B1024_K{K}"] = dict(ms=ms, all=allv, decoder_rows=1024 * K, molecules_per_s=1024 / (ms / 1e3))
        print(f"iw_B1024_K{K}", json.dumps(res[f"iw_B1024_K{K}"]), flush=True)

if "diag" not in args.skip:
    mols = molecules(args.diag_n)
    batches = [[model.string2tensor(s, device="cpu") for s in mols[i:i + 1024]] for i in range(0, args.diag_n, 1024)]
    mv.moses_latent_diagnostics(model, batches[:1], n_samples=4, seed=5)          # warm-up (workspaces)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = mv.moses_latent_diagnostics(model, batches, n_samples=args.diag_k, seed=5)
    wall = time.perf_counter() - t0
    res["diag"] = dict(seconds=wall, n_molecules=args.diag_n, n_samples=args.diag_k, result=r)
    print("diag", json.dumps(res["diag"]), flush=True)

if args.out:
    json.dump(res, open(args.out, "w"), indent=1)
