"""What the scaffold SMILES costs against its two parts (mvae_smiles_scaffold_smiles_rows / _corpus beside mvae_smiles_canon_rows /
_corpus, whose ranks, search and emission it runs on a smaller graph, and mvae_smiles_scaffold_rows / _corpus, whose atom sets it
computes) on the corpus of tests/smiles_canon_times.py (drug-like strings assembled from fragments, 50,000 draws repeated to N rows).
One step per process, so that each can run under a time limit of its own:
  --step batch    one batch of B = 1024 padded rows of MOSES' lengths: the three _rows launches, alternated;
  --step corpus   one _corpus launch of each over all N rows, alternated, and MosesDeviceDataset.scaffold_smiles() (the launch, the
                  compaction of the gapped CSR and the host's waits; a host clock).
Device events around each launch, the first launch apart; medians, with min and max.  No time is a pass criterion: the entry is reported
against canon and scaffold of the same run; the expectation is about canon's time plus the set computation and a second, smaller
adjacency, and less than canon + scaffold.  Not a pytest file.  Each step merges its section into --out.

    python tests/scaffold_smiles_times.py --step batch --out profiles/scaffold_smiles_times.json
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


def summed(r, status, info):
    """The ratios the expectation is stated in, and what the launch found."""
    t = {k: r[k]["ms"]["median"] for k in ("scaffold_smiles", "canon", "scaffold")}
    inf = info.double()[status == 0]
    r.update(ratio_to_canon=t["scaffold_smiles"] / t["canon"], ratio_to_canon_plus_scaffold=t["scaffold_smiles"] / (t["canon"] + t["scaffold"]),
             status_counts=torch.bincount(status, minlength=16).tolist(), mean_info_written=dict(zip(ops.SCAFFOLD_SMILES_INFO, inf.mean(0).tolist())))
    return r


tok_d, chem_d = dataset._fp_tables("scaffold_smiles")
emit_d = VC.smiles_emit_table(vocab).to(dev)
if args.step == "batch":
    pick = np.random.RandomState(1).permutation(N)[:BATCH]
    ids = [vocab.string2ids(s, add_bos=True, add_eos=True) for s in dataset.smiles(pick)]
    x = torch.full((BATCH, max(map(len, ids))), vocab.pad, dtype=torch.long)
    for b, row in enumerate(ids):
        x[b, :len(row)] = torch.as_tensor(row)
    x = x.to(dev)
    T = x.shape[1]
    sp = ops.smiles_scaffold_smiles_rows(x, tok_d, chem_d, emit_d, vocab.bos, vocab.eos, vocab.pad, T - 2, T)
    cn = ops.smiles_canon_rows(x, tok_d, chem_d, emit_d, vocab.bos, vocab.eos, vocab.pad, T - 2, T)
    sc = ops.smiles_scaffold_rows(x, tok_d, chem_d, vocab.eos)
    r = alternated({"scaffold_smiles": lambda: ops.smiles_scaffold_smiles_rows(x, tok_d, chem_d, emit_d, vocab.bos, vocab.eos, vocab.pad, T - 2, T, *sp),
                    "canon": lambda: ops.smiles_canon_rows(x, tok_d, chem_d, emit_d, vocab.bos, vocab.eos, vocab.pad, T - 2, T, *cn),
                    "scaffold": lambda: ops.smiles_scaffold_rows(x, tok_d, chem_d, vocab.eos, *sc)})
    r = summed(r, sp[2], sp[3])
    r["T"] = T
    res["batch"] = r
    show("batch", r)
    print(f"T = {T}; scaffold_smiles / canon = {r['ratio_to_canon']:.3f}, / (canon + scaffold) = {r['ratio_to_canon_plus_scaffold']:.3f}; "
          f"statuses {r['status_counts']}; mean info of the written rows {r['mean_info_written']}", flush=True)
else:
    all_rows = torch.arange(N, device=dev)
    sp = ops.smiles_scaffold_smiles_corpus(dataset.tokens, dataset.offsets, N, all_rows, tok_d, chem_d, emit_d, 127, 127)
    cn = ops.smiles_canon_corpus(dataset.tokens, dataset.offsets, N, all_rows, tok_d, chem_d, emit_d, 127, 127, info=False, rank=False)
    sc = ops.smiles_scaffold_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d)
    r = alternated({"scaffold_smiles": lambda: ops.smiles_scaffold_smiles_corpus(dataset.tokens, dataset.offsets, N, all_rows, tok_d, chem_d, emit_d, 127,
                                                                                 127, *sp),
                    "canon": lambda: ops.smiles_canon_corpus(dataset.tokens, dataset.offsets, N, all_rows, tok_d, chem_d, emit_d, 127, 127, *cn[:3],
                                                             info=False, rank=False),
                    "scaffold": lambda: ops.smiles_scaffold_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d, *sc)}, rounds=4)
    r = summed(r, sp[2], sp[3])

    def scaffolds():
        dataset._scaffold_smiles = None
        dataset.scaffold_smiles()
    r.update(alternated({"dataset_scaffold_smiles": scaffolds}, timer=clock, rounds=2))
    ds_scaf, rows = dataset.scaffold_smiles()
    r.update(rows_per_second=N / (r["scaffold_smiles"]["ms"]["median"] * 1e-3), n_with_scaffold=int(rows.numel()), n_distinct_scaffolds=ds_scaf.n_distinct,
             n_scaffold_keys=int(dataset.scaffold_histogram()[0].numel()))
    res["corpus"] = r
    show("corpus", r)
    print(f"N = {N}: scaffold_smiles / canon = {r['ratio_to_canon']:.3f}, / (canon + scaffold) = {r['ratio_to_canon_plus_scaffold']:.3f}; "
          f"{r['rows_per_second']:.3e} rows/s in one launch; {r['n_with_scaffold']} rows with a scaffold, {r['n_distinct_scaffolds']} distinct "
          f"scaffold strings, {r['n_scaffold_keys']} scaffold keys", flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    merged = json.load(open(args.out)) if os.path.exists(args.out) else {}
    merged.update(res)
    json.dump(merged, open(args.out, "w"), indent=1)
