"""What the token-level Levenshtein kernels cost (mvae_edit_knn / MosesDeviceDataset.nearest_strings, mvae_edit_distance_rows,
moses_generate(nearest=True)) on the synthetic corpus of tests/latent_knn_times.py -- N = 1.6 M rows, lengths ~ N(38, 8) in [10, 57] over
the 25 characters of the MOSES alphabet:
  (a) the search at Q = 1, 64, 1024 and 4096 queries sampled from the corpus with 0 to 3 random edits, k = 1 and k = 16: device events
      around each of several launches (scan + merge), the first launch apart (it loads the code object), with the pairs per second and
      the VALU operation rate that implies -- 137 / 4 = 34.25 instructions per (pair, text token) of the one-word inner loop, read
      off the compiled code (the v_ instructions of one text token's block, which advances 4 queries; mostly 32-bit logic, a few
      64-bit shifts and adds counted once), a wave instruction being 64 lane operations -- against the 78.6 T lane operations per second of the data sheet's vector rate (157.3 TF of FMAs);
  (b) the pair kernel at B = 4096;
  (c) moses_generate with and without nearest=True at the example's batch size under a randomly initialised mosesvae.VAE.
Medians, with min and max.  Not a pytest file.

    python tests/edit_distance_times.py --out profiles/edit_distance_times.json
"""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_600_000, help="corpus rows")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--valu_per_token", type=float, default=137 / 4,
                help="VALU instructions per (pair, text token) in the compiled one-word inner loop: 137 v_ instructions per token and 4 queries")
ap.add_argument("--skip_generate", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
sys.path.insert(0, ROOT)
from molecular_vae_amd import _lib as L, data as D, mosesvae as MV, vocab as VC, ops, train as TR   # noqa: E402

LANE_OPS_PEAK = 157.3e12 / 2
ALPHABET = "CNOSFcnos()=#123[]@H+-lBr"
N = args.n
vocab = VC.OneHotVocab(set(ALPHABET))
rs = np.random.RandomState(0)
lens = np.clip(rs.normal(38, 8, size=N), 10, 57).astype(np.int64)
offsets = np.zeros(N + 1, dtype=np.int64)
np.cumsum(lens, out=offsets[1:])
ids = np.array(sorted(vocab.c2i[c] for c in ALPHABET), np.uint8)
tokens = ids[rs.randint(0, len(ALPHABET), size=int(offsets[-1]))]
dataset = D.MosesDeviceDataset((tokens, offsets), vocab, device=dev)
res = dict(n=N, device=torch.cuda.get_device_name(0), corpus_bytes=int(offsets[-1]), mean_len=float(lens.mean()),
           valu_per_token=args.valu_per_token, search={}, rows={}, generate={})


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


def make_queries(Q, T=60):
    x = np.full((Q, T), vocab.pad, np.int64)
    x[:, 0] = vocab.bos
    for i, r in enumerate(rs.randint(0, N, Q)):
        s = list(tokens[offsets[r]:offsets[r + 1]])
        for _ in range(rs.randint(4)):
            op, pos = rs.randint(3), rs.randint(len(s))
            if op == 0:
                s[pos] = ids[rs.randint(len(ids))]
            elif op == 1 and len(s) > 1:
                del s[pos]
            elif len(s) < T - 2:
                s.insert(pos, ids[rs.randint(len(ids))])
        x[i, 1:1 + len(s)] = s
        x[i, 1 + len(s)] = vocab.eos
    return torch.from_numpy(x).to(dev)


lib = L.load()
first_done = False
for k in (1, 16):
    for Q in (1, 64, 1024, 4096):
        x = make_queries(Q)
        dist = torch.empty(Q, k, dtype=torch.int32, device=dev)
        idx = torch.empty(Q, k, dtype=torch.long, device=dev)
        run = lambda: ops.edit_knn(x, dataset.tokens, dataset.offsets, N, k, vocab.eos, len(vocab), dist=dist, idx=idx)
        first = events(run, 1)[0]
        times = events(run, args.rounds if Q >= 1024 else 3 * args.rounds)
        m = statistics.median(times)
        pairs = float(Q) * N / (m * 1e-3)
        lane_ops = pairs * float(lens.mean()) * args.valu_per_token
        entry = dict(first_ms=first, first_loads_code=not first_done, ms=med(times), pairs_per_second=pairs,
                     workspace_bytes=int(lib.mvae_edit_knn_workspace(Q, N, k)), lane_ops_per_second=lane_ops,
                     of_vector_peak=lane_ops / LANE_OPS_PEAK, mean_nearest_dist=float(dist[:, 0].float().mean()))
        first_done = True
        res["search"][f"k{k}_Q{Q}"] = entry
        print(f"edit_knn k = {k} Q = {Q}: first {first:.3f} ms, then median {m:.3f} ms (min {min(times):.3f}, max {max(times):.3f}); "
              f"{pairs:.3e} pairs/s; {lane_ops / 1e12:.2f} T lane-ops/s = {100 * entry['of_vector_peak']:.1f} % of the vector rate; "
              f"mean nearest distance {entry['mean_nearest_dist']:.2f}; workspace {entry['workspace_bytes']} B", flush=True)
        del x, dist, idx

B = 4096
a, b = make_queries(B, 100), make_queries(B, 100)
out = torch.empty(B, dtype=torch.int32, device=dev)
run = lambda: ops.edit_distance_rows(a, b, vocab.eos, len(vocab), dist=out)
first = events(run, 1)[0]
times = events(run, 5 * args.rounds)
res["rows"] = dict(B=B, T=100, first_ms=first, ms=med(times))
print(f"edit_distance_rows B = {B}: first {first:.3f} ms, then median {statistics.median(times):.3f} ms "
      f"(min {min(times):.3f}, max {max(times):.3f})", flush=True)

if not args.skip_generate:
    torch.manual_seed(42)
    model = MV.VAE(vocab, dtype=torch.bfloat16).to(dev).eval()
    n, bs = 8192, 4096                                             # examples/sample_moses.py: --n_batch 4096
    for nearest in (False, True):
        TR.moses_generate(model, bs, batch_size=bs, novel_against=dataset, nearest=nearest, seed=9)        # warm-up
        per = []
        for r in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out_ = TR.moses_generate(model, n, batch_size=bs, novel_against=dataset, nearest=nearest, seed=r)
            torch.cuda.synchronize()
            per.append(time.perf_counter() - t0)
        res["generate"]["nearest" if nearest else "plain"] = dict(n=n, batch_size=bs, unique=out_["unique"], seconds=med(per))
        print(f"moses_generate n = {n}, batch {bs}, nearest={nearest}: median {statistics.median(per):.3f} s "
              f"(min {min(per):.3f}, max {max(per):.3f}), {out_['unique']} unique", flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
