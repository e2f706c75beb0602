"""What the fragment entries cost beside the scaffold entries they are modelled on, in one run on one device: mvae_smiles_fragment_rows /
_corpus beside mvae_smiles_scaffold_rows / _corpus (the keys), and mvae_smiles_fragment_smiles_rows / _corpus with frag = 0 beside
mvae_smiles_scaffold_smiles_rows / _corpus (the strings), on the corpus of tests/smiles_canon_times.py (drug-like strings assembled from
fragments, 50,000 draws repeated to N rows).  One step per process, so that each can run under a time limit of its own:
  --step batch    one batch of B = 1024 padded rows of MOSES' lengths: the four _rows launches, alternated;
  --step corpus   one _corpus launch of each over all N rows, alternated.
Device events around each launch, the first launch apart; medians, with min and max.  No time is a pass criterion.  The design
expectation, unmeasured when it was written, is that the fragment keys entry costs no more than about 1.5 x the scaffold keys entry: one
set of refinement rounds where the scaffold entry runs two, plus the cut set, the labels and the atom lists.  Not a pytest file.  Each
step merges its section into --out.

    python tests/fragment_times.py --step batch --out profiles/fragment_times.json
"""
import argparse, json, os, statistics, sys
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


def alternated(runs, rounds=None):
    first = {k: event(f) for k, f in runs.items()}
    times = {k: [] for k in runs}
    for _ in range(args.rounds if rounds is None else rounds):
        for k, f in runs.items():
            times[k].append(event(f))
    return {k: dict(first_ms=first[k], ms=med(times[k])) for k in runs}


def show(section, r):
    for k, v in r.items():
        if isinstance(v, dict) and "ms" in v:
            m = v["ms"]
            print(f"{section} {k}: first {v['first_ms']:.3f} ms, then median {m['median']:.4f} ms (min {m['min']:.4f}, max {m['max']:.4f})", flush=True)


def summed(r, status, desc):
    """The ratios the expectation is stated in, and what the launch found."""
    t = {k: r[k]["ms"]["median"] for k in ("fragment", "scaffold", "fragment_smiles", "scaffold_smiles")}
    d = desc.double()[status == 0]
    r.update(fragment_to_scaffold=t["fragment"] / t["scaffold"], fragment_smiles_to_scaffold_smiles=t["fragment_smiles"] / t["scaffold_smiles"],
             status_counts=torch.bincount(status, minlength=16).tolist(), mean_desc_ok=dict(zip(ops.FRAGMENT_DESC, d.mean(0).tolist())))
    return r


def report(section, r):
    show(section, r)
    print(f"{section}: fragment / scaffold = {r['fragment_to_scaffold']:.3f}, fragment_smiles / scaffold_smiles = "
          f"{r['fragment_smiles_to_scaffold_smiles']:.3f}; statuses {r['status_counts']}; mean desc of the status-0 rows {r['mean_desc_ok']}", flush=True)


tok_d, chem_d = dataset._fp_tables("fragments")
emit_d = VC.smiles_emit_table(vocab).to(dev)
if args.step == "batch":
    pick = np.random.RandomState(1).permutation(N)[:BATCH]
    ids = [vocab.string2ids(s, add_bos=True, add_eos=True) for s in dataset.smiles(pick)]
    x = torch.full((BATCH, max(map(len, ids))), vocab.pad, dtype=torch.long)
    for b, row in enumerate(ids):
        x[b, :len(row)] = torch.as_tensor(row)
    x = x.to(dev)
    T = x.shape[1]
    fr = ops.smiles_fragment_rows(x, tok_d, chem_d, vocab.eos)
    sc = ops.smiles_scaffold_rows(x, tok_d, chem_d, vocab.eos)
    fs = ops.smiles_fragment_smiles_rows(x, tok_d, chem_d, emit_d, vocab.bos, vocab.eos, vocab.pad, 0, T - 2, T)
    sp = ops.smiles_scaffold_smiles_rows(x, tok_d, chem_d, emit_d, vocab.bos, vocab.eos, vocab.pad, T - 2, T)
    r = alternated({"fragment": lambda: ops.smiles_fragment_rows(x, tok_d, chem_d, vocab.eos, *fr),
                    "scaffold": lambda: ops.smiles_scaffold_rows(x, tok_d, chem_d, vocab.eos, *sc),
                    "fragment_smiles": lambda: ops.smiles_fragment_smiles_rows(x, tok_d, chem_d, emit_d, vocab.bos, vocab.eos, vocab.pad, 0, T - 2, T, *fs),
                    "scaffold_smiles": lambda: ops.smiles_scaffold_smiles_rows(x, tok_d, chem_d, emit_d, vocab.bos, vocab.eos, vocab.pad, T - 2, T, *sp)})
    r = summed(r, fr[0], fr[2])
    r["T"] = T
    res["batch"] = r
    report("batch", r)
else:
    all_rows = torch.arange(N, device=dev)
    fr = ops.smiles_fragment_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d)
    sc = ops.smiles_scaffold_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d)
    fs = ops.smiles_fragment_smiles_corpus(dataset.tokens, dataset.offsets, N, all_rows, tok_d, chem_d, emit_d, 0, 127, 127)
    sp = ops.smiles_scaffold_smiles_corpus(dataset.tokens, dataset.offsets, N, all_rows, tok_d, chem_d, emit_d, 127, 127)
    r = alternated({"fragment": lambda: ops.smiles_fragment_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d, *fr),
                    "scaffold": lambda: ops.smiles_scaffold_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d, *sc),
                    "fragment_smiles": lambda: ops.smiles_fragment_smiles_corpus(dataset.tokens, dataset.offsets, N, all_rows, tok_d, chem_d, emit_d, 0,
                                                                                 127, 127, *fs),
                    "scaffold_smiles": lambda: ops.smiles_scaffold_smiles_corpus(dataset.tokens, dataset.offsets, N, all_rows, tok_d, chem_d, emit_d, 127,
                                                                                 127, *sp)}, rounds=4)
    r = summed(r, fr[0], fr[2])
    r.update(rows_per_second=N / (r["fragment"]["ms"]["median"] * 1e-3), n_fragment_keys=int(ops.key_histogram(fr[3])[0].numel()))
    res["corpus"] = r
    report("corpus", r)
    print(f"N = {N}: {r['rows_per_second']:.3e} rows/s in one fragment launch; {r['n_fragment_keys']} distinct fragment keys", flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    merged = json.load(open(args.out)) if os.path.exists(args.out) else {}
    merged.update(res)
    json.dump(merged, open(args.out, "w"), indent=1)
