"""What the latent k-NN costs (mvae_latent_knn, ops.latent_knn, MosesLatentIndex.search) on a synthetic N(0, I) latent table with MOSES-like
sizes -- N = 1.6 M rows, d_z = 160, k = 16 -- beside the route a user has without it, timed in the same run on the same box:
  (a) the search at Q = 1, 64, 1024 and 4096 random N(0, I) queries: device events around each of several launches (scan + merge), the
      first launch apart (it loads the code object), with the achieved flop/s (3 flop per pair and dimension: sub, mul, add) against the
      157 TF vector data-sheet rate and the bytes/s of one pass over the table against the 6.3 TB/s a streaming copy reaches here;
  (b) torch.cdist + topk over table chunks sized so that the [Q, chunk] distance block stays under 2 GB, the partial answers merged by one
      more topk: what has to be written by hand today (cdist's default may take the expanded GEMM form; it is timed, not checked);
  (c) MosesDeviceDataset.encode_latents for a whole synthetic corpus of the same N (lengths ~ N(38, 8) in [10, 57]) under a randomly
      initialised mosesvae.VAE, wall clock around the call and a synchronisation.
Medians, with min and max.  Not a pytest file.

    python tests/latent_knn_times.py --out profiles/latent_knn_times.json
"""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_600_000, help="table rows")
ap.add_argument("--dz", type=int, default=160)
ap.add_argument("--k", type=int, default=16)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--skip_encode", action="store_true")
ap.add_argument("--skip_torch", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
sys.path.insert(0, ROOT)
from molecular_vae_amd import _lib as L, data as D, mosesvae as MV, vocab as VC, ops   # noqa: E402

VEC_TF, HBM_TBS = 157.3, 6.3
N, dz, k = args.n, args.dz, args.k
g = torch.Generator(device=dev); g.manual_seed(0)
table = torch.randn(N, dz, device=dev, generator=g)
res = dict(n=N, dz=dz, k=k, device=torch.cuda.get_device_name(0), table_bytes=4 * N * dz, search={}, torch_cdist_topk={})


def med(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), all=v)


def events(fn, reps):
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record(); fn(); e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e))
    return out


def cdist_topk(q):
    chunk = max(1, min(N, (2 << 30) // (4 * q.shape[0])))
    best_d, best_j = None, None
    for lo in range(0, N, chunk):
        d = torch.cdist(q, table[lo:lo + chunk]).square_()
        dd, jj = torch.topk(d, min(k, d.shape[1]), dim=1, largest=False)
        jj += lo
        if best_d is None:
            best_d, best_j = dd, jj
        else:
            cd, cj = torch.cat([best_d, dd], 1), torch.cat([best_j, jj], 1)
            best_d, pick = torch.topk(cd, k, dim=1, largest=False)
            best_j = torch.gather(cj, 1, pick)
    return best_d, best_j


lib = L.load()
first_done = False
for Q in (1, 64, 1024, 4096):
    q = torch.randn(Q, dz, device=dev, generator=g)
    dist = torch.empty(Q, k, device=dev)
    idx = torch.empty(Q, k, dtype=torch.long, device=dev)
    run = lambda: ops.latent_knn(q, table, k, dist=dist, idx=idx)
    first = events(run, 1)[0]
    reps = args.rounds if Q >= 1024 else 3 * args.rounds
    times = events(run, reps)
    m = statistics.median(times)
    flops = 3.0 * Q * N * dz
    entry = dict(first_ms=first, first_loads_code=not first_done, ms=med(times), workspace_bytes=int(lib.mvae_latent_knn_workspace(Q, N, dz, k)),
                 tflops=flops / (m * 1e-3) / 1e12, of_vector_peak=flops / (m * 1e-3) / 1e12 / VEC_TF,
                 table_tbs=4.0 * N * dz / (m * 1e-3) / 1e12, of_hbm=4.0 * N * dz / (m * 1e-3) / 1e12 / HBM_TBS)
    first_done = True
    res["search"][str(Q)] = entry
    print(f"latent_knn Q = {Q}: first {first:.3f} ms, then median {m:.3f} ms (min {min(times):.3f}, max {max(times):.3f}); "
          f"{entry['tflops']:.2f} TF = {100 * entry['of_vector_peak']:.1f} % of {VEC_TF} TF; one table pass in that time is "
          f"{entry['table_tbs']:.3f} TB/s = {100 * entry['of_hbm']:.1f} % of {HBM_TBS} TB/s; workspace {entry['workspace_bytes']} B", flush=True)
    if not args.skip_torch:
        ref = lambda: cdist_topk(q)
        first_t = events(ref, 1)[0]
        times_t = events(ref, max(2, args.rounds // 2) if Q >= 1024 else args.rounds)
        td, tj = cdist_topk(q)
        agree = float((tj == idx).float().mean())
        res["torch_cdist_topk"][str(Q)] = dict(first_ms=first_t, ms=med(times_t), rows_agreeing=agree)
        print(f"  torch.cdist + topk in chunks: first {first_t:.3f} ms, then median {statistics.median(times_t):.3f} ms (min {min(times_t):.3f}, "
              f"max {max(times_t):.3f}); {100 * agree:.2f} % of its rows equal the kernel's", flush=True)
        del td, tj
    del q, dist, idx
    torch.cuda.empty_cache()

if not args.skip_encode:
    ALPHABET = "CNOSFcnos()=#123[]@H+-lBr"
    vocab = VC.OneHotVocab(set(ALPHABET))
    rs = np.random.RandomState(0)
    lens = np.clip(rs.normal(38, 8, size=N), 10, 57).astype(np.int64)
    offsets = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    tokens = rs.randint(0, len(ALPHABET), size=int(offsets[-1])).astype(np.uint8)
    dataset = D.MosesDeviceDataset((tokens, offsets), vocab, device=dev)
    torch.manual_seed(42)
    model = MV.VAE(vocab, dtype=torch.bfloat16).to(dev).eval()
    dataset.encode_latents(model, batch_size=4096) if N <= 65536 else D.MosesDeviceDataset(
        (tokens[:offsets[8192]], offsets[:8193]), vocab, device=dev).encode_latents(model)          # warm-up: workspaces, code objects
    per = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index = dataset.encode_latents(model, batch_size=4096)
        torch.cuda.synchronize()
        per.append(time.perf_counter() - t0)
    dataset.check_errors()
    res["encode_latents"] = dict(n=N, batch_size=4096, d_z=model.d_z, seconds=med(per), rows_per_second=N / statistics.median(per))
    print(f"encode_latents, {N} rows in batches of 4096: median {statistics.median(per):.2f} s (min {min(per):.2f}, max {max(per):.2f}) = "
          f"{N / statistics.median(per):.0f} rows per second", flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
