"""What the aromatic normal form costs against the canonical spelling (mvae_smiles_aromatize_corpus beside mvae_smiles_canon_corpus from
the same build, which share the walk, the ranks, the search and the emission: the difference is one matching and the bounded cycle
search) on the corpus of tests/smiles_canon_times.py (drug-like strings assembled from fragments, 50,000 draws repeated to N rows).  One
step per process, so that each can run under a time limit of its own:
  --step batch    one batch of B = 1024 rows of MOSES' lengths: the canon launch and the aromatize launch, alternated;
  --step corpus   one launch of each over all N rows, alternated, and MosesDeviceDataset.normal_form() (the launch, the compaction of
                  the gapped CSR and the host's wait for the lengths; a host clock).
Device events around each launch, the first launch apart; medians, with min and max.  No time is a pass criterion: aromatize is
reported against the canon of the same run.  Not a pytest file.  Each step merges its section into --out.

    python tests/smiles_aromatize_times.py --step batch --out profiles/aromatize_times.json
"""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--step", required=True, choices=("batch", "corpus"))
ap.add_argument("--n", type=int, default=1_600_000, help="corpus rows")
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
sys.path.insert(0, ROOT)
from molecular_vae_amd import data as D, vocab as VC, ops   # noqa: E402

DISTINCT, BATCH = 50_000, 1024
LINKS = ["C", "CC", "O", "N", "C(=O)", "C(C)", "c1ccc(cc1)", "C1CCN(CC1)", "S(=O)(=O)", "c1cc(F)c(cn1)", "C(=O)N", "C=C", "n1cc(nn1)"]
ENDS = ["C", "F", "Cl", "O", "N", "C(F)(F)F", "C#N", "c1ccccc1", "Br", "c1ccc2[nH]ccc2c1", "C1CC1", "[N+](=O)[O-]"]
rs = np.random.RandomState(0)
base = ["C" + "".join(LINKS[i] for i in rs.randint(len(LINKS), size=rs.randint(3, 10))) + ENDS[rs.randint(len(ENDS))] for _ in range(DISTINCT)]
vocab = VC.OneHotVocab.from_data(base + ["0123456789"])        # a respelling may need a ring digit the corpus never uses
tok1, off1 = D.tokenize_corpus(base, vocab)
reps = -(-args.n // DISTINCT)
lens = np.tile(np.diff(off1), reps)[:args.n]
offsets = np.zeros(args.n + 1, dtype=np.int64)
np.cumsum(lens, out=offsets[1:])
tokens = np.tile(tok1, reps)[:int(offsets[-1])]
dataset = D.MosesDeviceDataset((tokens, offsets), vocab, device=dev)
N = len(dataset)
res = dict(n=N, device=torch.cuda.get_device_name(0), rounds=args.rounds, mean_tokens=float(lens.mean()), max_tokens=int(lens.max()))


def med(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), all=v)


def event(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record(); fn(); e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternated(runs, timer=event, rounds=None):
    first = {k: timer(f) for k, f in runs.items()}
    times = {k: [] for k in runs}
    for _ in range(args.rounds if rounds is None else rounds):
        for k, f in runs.items():
            times[k].append(timer(f))
    return {k: dict(first_ms=first[k], ms=med(times[k])) for k in runs}


def show(section, r):
    for k, v in r.items():
        if isinstance(v, dict) and "ms" in v:
            m = v["ms"]
            print(f"{section} {k}: first {v['first_ms']:.3f} ms, then median {m['median']:.4f} ms (min {m['min']:.4f}, max {m['max']:.4f})", flush=True)


def pair(name, rows, mc, stride):
    """The canon and the aromatize launch over the same rows, alternated; the aromatize's info summed up."""
    a = (dataset.tokens, dataset.offsets, N, rows, tok_d, chem_d, emit_d, mc, stride)
    cn = ops.smiles_canon_corpus(*a)
    ar = ops.smiles_aromatize_corpus(*a)
    r = alternated({"canon_" + name: lambda: ops.smiles_canon_corpus(*a, *cn),
                    "aromatize_" + name: lambda: ops.smiles_aromatize_corpus(*a, *ar),
                    "aromatize_without_info_arom_" + name: lambda: ops.smiles_aromatize_corpus(*a, *ar[:3], info=False, arom=False)},
                   rounds=None if rows.numel() <= 4 * BATCH else 4)
    info = ar[3].double()
    r.update({"ratio_aromatize_to_canon_" + name: r["aromatize_" + name]["ms"]["median"] / r["canon_" + name]["ms"]["median"],
              "status_counts_" + name: torch.bincount(ar[2], minlength=32).tolist(),
              "mean_info_" + name: dict(zip(ops.AROMATIZE_INFO, info.mean(0).tolist()))})
    return r


tok_d, chem_d = dataset._fp_tables("normal_form")
emit_d = VC.smiles_emit_table(vocab).to(dev)
if args.step == "batch":
    rows = torch.from_numpy(np.random.RandomState(1).permutation(N)[:BATCH].astype(np.int64)).to(dev)
    T = int(dataset.lengths[rows.cpu().numpy()].max()) + 2
    r = pair("1024", rows, T - 2, T - 2)
    r["T"] = T
    res["batch"] = r
    show("batch", r)
    print(f"T = {T}; aromatize / canon = {r['ratio_aromatize_to_canon_1024']:.3f} at 1024 rows; mean info {r['mean_info_1024']}", flush=True)
else:
    r = pair("all_rows", torch.arange(N, device=dev), 127, max(dataset.max_len, 127))

    def normal_form():
        dataset._normal = None
        dataset.normal_form()
    r.update(alternated({"dataset_normal_form": normal_form}, timer=clock, rounds=2))
    r.update(rows_per_second=N / (r["aromatize_all_rows"]["ms"]["median"] * 1e-3), n_distinct=dataset.n_distinct,
             n_distinct_normal=dataset.normal_form().n_distinct)
    res["corpus"] = r
    show("corpus", r)
    print(f"N = {N}: aromatize / canon = {r['ratio_aromatize_to_canon_all_rows']:.3f}; {r['rows_per_second']:.3e} rows/s in one launch; "
          f"{r['n_distinct']} distinct rows, {r['n_distinct_normal']} distinct normal forms", flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    merged = json.load(open(args.out)) if os.path.exists(args.out) else {}
    merged.update(res)
    json.dump(merged, open(args.out, "w"), indent=1)
