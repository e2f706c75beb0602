"""What the fingerprint feature costs (mvae_smiles_fp_corpus / MosesDeviceDataset.fingerprints, mvae_tanimoto_knn, mvae_tanimoto_sum,
moses_generate(int_div=, snn=)) on the corpus of tests/smiles_graph_times.py (drug-like strings assembled from fragments, 50,000 draws
repeated to N = 1.6 M rows).  One step per process, so that each can run under a time limit of its own:
  --step corpus    the fingerprint pass over all N CSR rows beside the graph pass (mvae_smiles_graph_corpus), alternated;
  --step knn       mvae_tanimoto_knn at Q = 4096, N = 1.6 M, k = 1, beside the VALU bound of 64 integer operations per pair
                   (256 CUs x 64 lanes at 2.4 GHz);
  --step sum       mvae_tanimoto_sum at M = 30,000;
  --step generate  moses_generate with and without int_div / snn at the example's batch size under a randomly initialised mosesvae.VAE,
                   alternated.
Device events around each launch (a host clock around moses_generate), the first launch apart (it loads the code object); four rounds;
medians, with min and max.  No time is a pass criterion.  Not a pytest file.  Each step merges its section into --out.

    python tests/fingerprint_times.py --step corpus --out profiles/fingerprint_times.json
"""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--step", required=True, choices=("corpus", "knn", "sum", "generate"))
ap.add_argument("--n", type=int, default=1_600_000, help="corpus rows")
ap.add_argument("--q", type=int, default=4096)
ap.add_argument("--m", type=int, default=30_000)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
sys.path.insert(0, ROOT)
from molecular_vae_amd import data as D, mosesvae as MV, vocab as VC, ops, train as TR   # noqa: E402

DISTINCT = 50_000
LINKS = ["C", "CC", "O", "N", "C(=O)", "C(C)", "c1ccc(cc1)", "C1CCN(CC1)", "S(=O)(=O)", "c1cc(F)c(cn1)", "C(=O)N", "[C@H](C)", "C=C", "n1cc(nn1)"]
ENDS = ["C", "F", "Cl", "O", "N", "C(F)(F)F", "C#N", "c1ccccc1", "Br", "c1ccc2[nH]ccc2c1", "C1CC1", "[N+](=O)[O-]"]
rs = np.random.RandomState(0)
base = ["C" + "".join(LINKS[i] for i in rs.randint(len(LINKS), size=rs.randint(3, 10))) + ENDS[rs.randint(len(ENDS))] for _ in range(DISTINCT)]
vocab = VC.OneHotVocab.from_data(base)
n_rows = args.n if args.step in ("corpus", "knn") else DISTINCT
tok1, off1 = D.tokenize_corpus(base, vocab)
reps = -(-n_rows // DISTINCT)
lens = np.tile(np.diff(off1), reps)[:n_rows]
offsets = np.zeros(n_rows + 1, dtype=np.int64)
np.cumsum(lens, out=offsets[1:])
tokens = np.tile(tok1, reps)[:int(offsets[-1])]
dataset = D.MosesDeviceDataset((tokens, offsets), vocab, device=dev)
N = len(dataset)
tok_d, chem_d = VC.smiles_token_table(vocab).to(dev), VC.smiles_chem_table(vocab).to(dev)
res = dict(n=N, device=torch.cuda.get_device_name(0), rounds=args.rounds)


def med(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), all=v)


def event(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record(); fn(); e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def alternated(runs):
    """{name: fn} -> {name: (first_ms, [ms per round])}: every fn once (the first launch), then args.rounds rounds of every fn in turn."""
    first = {k: event(f) for k, f in runs.items()}
    times = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, f in runs.items():
            times[k].append(event(f))
    return {k: dict(first_ms=first[k], ms=med(times[k])) for k in runs}


if args.step == "corpus":
    gout = ops.smiles_graph_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d)
    fout = ops.smiles_fp_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d)
    r = alternated({"graph_corpus": lambda: ops.smiles_graph_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d, *gout),
                    "fp_corpus": lambda: ops.smiles_fp_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d, *fout)})
    assert torch.equal(gout[0], fout[0])
    bits = (fout[1].view(torch.uint8)[:DISTINCT, :, None] >> torch.arange(8, device=dev, dtype=torch.uint8) & 1).sum((1, 2))
    r.update(tokens=int(offsets[-1]), status0=int((fout[0] == 0).sum()), distinct_fp=int(torch.unique(fout[1][:DISTINCT], dim=0).shape[0]),
             mean_bits=float(bits.float().mean()), max_bits=int(bits.max()))
    res["corpus"] = r
    for k in ("graph_corpus", "fp_corpus"):
        m = r[k]["ms"]
        print(f"{k} N = {N}: first {r[k]['first_ms']:.3f} ms, then median {m['median']:.3f} ms (min {m['min']:.3f}, max {m['max']:.3f}); "
              f"{N / (m['median'] * 1e-3):.3e} rows/s", flush=True)
    print(f"status 0: {r['status0']}, distinct fingerprints among the {DISTINCT} draws: {r['distinct_fp']}, bits set: mean {r['mean_bits']:.1f}, "
          f"max {r['max_bits']}", flush=True)
elif args.step == "knn":
    table = dataset.fingerprints()["fp"]
    q = table[torch.from_numpy(np.random.RandomState(1).choice(DISTINCT, size=args.q)).to(dev)].contiguous()
    sim, idx = ops.tanimoto_knn(q, table, 1)
    r = alternated({"knn": lambda: ops.tanimoto_knn(q, table, 1, sim=sim, idx=idx)})["knn"]
    assert bool((sim == 1.0).all())                                 # every query is a corpus row
    pairs = args.q * N
    bound_ms = 64.0 * pairs / (256 * 64 * 2.4e9) * 1e3
    r.update(Q=args.q, k=1, pairs=pairs, valu_bound_ms=bound_ms, ratio_to_bound=r["ms"]["median"] / bound_ms,
             pairs_per_second=pairs / (r["ms"]["median"] * 1e-3))
    res["knn"] = r
    print(f"tanimoto_knn Q = {args.q}, N = {N}, k = 1: first {r['first_ms']:.3f} ms, then median {r['ms']['median']:.3f} ms (min "
          f"{r['ms']['min']:.3f}, max {r['ms']['max']:.3f}); {r['pairs_per_second']:.3e} pairs/s; VALU bound of 64 integer operations per "
          f"pair {bound_ms:.3f} ms, ratio {r['ratio_to_bound']:.2f}", flush=True)
elif args.step == "sum":
    a = dataset.fingerprints()["fp"][:args.m].contiguous()
    out = ops.tanimoto_sum(a, a)
    r = alternated({"sum": lambda: ops.tanimoto_sum(a, a, out=out)})["sum"]
    M = a.shape[0]
    r.update(M=M, pairs=M * M, pairs_per_second=M * M / (r["ms"]["median"] * 1e-3), int_div=1.0 - float(out) / (M * M))
    res["sum"] = r
    print(f"tanimoto_sum M = {M}: first {r['first_ms']:.3f} ms, then median {r['ms']['median']:.3f} ms (min {r['ms']['min']:.3f}, max "
          f"{r['ms']['max']:.3f}); {r['pairs_per_second']:.3e} pairs/s; IntDiv of those rows {r['int_div']:.4f}", flush=True)
else:
    torch.manual_seed(42)
    model = MV.VAE(vocab, dtype=torch.bfloat16).to(dev).eval()
    n, bs = 8192, 4096                                             # examples/sample_moses.py: --n_batch 4096
    dataset.build_index()
    dataset.fingerprints()
    kinds = {"plain": {}, "int_div": dict(int_div=True), "snn": dict(snn=True), "both": dict(int_div=True, snn=True)}
    per = {k: [] for k in kinds}
    last = {}
    for k, kw in kinds.items():
        TR.moses_generate(model, bs, batch_size=bs, syntax=True, novel_against=dataset, seed=9, **kw)      # warm-up
    for r_ in range(args.rounds):
        for k, kw in kinds.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = TR.moses_generate(model, n, batch_size=bs, syntax=True, novel_against=dataset, seed=r_, **kw)
            torch.cuda.synchronize()
            per[k].append(time.perf_counter() - t0)
    res["generate"] = {}
    for k in kinds:
        entry = dict(n=n, batch_size=bs, corpus_rows=N, unique=last[k]["unique"], seconds=med(per[k]))
        entry.update({key: last[k][key] for key in ("n_fingerprinted", "int_div", "snn") if key in last[k]})
        res["generate"][k] = entry
        print(f"moses_generate n = {n}, batch {bs}, corpus {N} rows, {k}: median {statistics.median(per[k]):.3f} s (min {min(per[k]):.3f}, max "
              f"{max(per[k]):.3f}), " + ", ".join(f"{key} {entry[key]}" for key in ("unique", "n_fingerprinted", "int_div", "snn") if key in entry),
              flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    merged = json.load(open(args.out)) if os.path.exists(args.out) else {}
    merged.update(res)
    json.dump(merged, open(args.out, "w"), indent=1)
