"""What the scaffold feature costs (mvae_smiles_scaffold_corpus / MosesDeviceDataset.scaffolds, moses_generate(scaffolds=)) on the corpus
of tests/fingerprint_times.py (drug-like strings assembled from fragments, 50,000 draws repeated to N = 1.6 M rows).  One step per
process, so that each can run under a time limit of its own:
  --step corpus    the scaffold pass over all N CSR rows beside the fingerprint pass (mvae_smiles_fp_corpus), the yardstick, alternated:
                   16 refinement rounds against the fingerprint's 2;
  --step generate  moses_generate with and without scaffolds=True at the example's batch size under a randomly initialised mosesvae.VAE,
                   alternated.
Device events around each launch (a host clock around moses_generate), the first launch apart (it loads the code object); four rounds;
medians, with min and max.  No time is a pass criterion.  Not a pytest file.  Each step merges its section into --out.

    python tests/scaffold_times.py --step corpus --out profiles/scaffold_times.json
"""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--step", required=True, choices=("corpus", "generate"))
ap.add_argument("--n", type=int, default=1_600_000, help="corpus rows")
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
n_rows = args.n if args.step == "corpus" else DISTINCT
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
    fout = ops.smiles_fp_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d)
    sout = ops.smiles_scaffold_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d)
    r = alternated({"fp_corpus": lambda: ops.smiles_fp_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d, *fout),
                    "scaffold_corpus": lambda: ops.smiles_scaffold_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d, *sout)})
    assert torch.equal(fout[0], sout[0])
    keys, counts = ops.key_histogram(sout[3][:DISTINCT, 1])
    r.update(tokens=int(offsets[-1]), status0=int((sout[0] == 0).sum()), with_scaffold=int((sout[3][:DISTINCT, 1] != 0).sum()),
             distinct_scaffolds=keys.numel(), distinct_graphs=ops.key_histogram(sout[3][:DISTINCT, 0])[0].numel(),
             distinct_strings=len(set(base)), mean_scaffold_atoms=float(sout[2][:DISTINCT, 0].float().mean()),
             ratio=r["scaffold_corpus"]["ms"]["median"] / r["fp_corpus"]["ms"]["median"])
    res["corpus"] = r
    for k in ("fp_corpus", "scaffold_corpus"):
        m = r[k]["ms"]
        print(f"{k} N = {N}: first {r[k]['first_ms']:.3f} ms, then median {m['median']:.3f} ms (min {m['min']:.3f}, max {m['max']:.3f}); "
              f"{N / (m['median'] * 1e-3):.3e} rows/s", flush=True)
    print(f"ratio scaffold / fingerprint {r['ratio']:.2f}; status 0: {r['status0']}; among the {DISTINCT} draws: {r['distinct_strings']} distinct "
          f"strings, {r['distinct_graphs']} distinct molecule keys, {r['with_scaffold']} with a scaffold, {r['distinct_scaffolds']} distinct "
          f"scaffold keys, {r['mean_scaffold_atoms']:.1f} scaffold atoms on average", flush=True)
else:
    torch.manual_seed(42)
    model = MV.VAE(vocab, dtype=torch.bfloat16).to(dev).eval()
    n, bs = 8192, 4096                                             # examples/sample_moses.py: --n_batch 4096
    dataset.build_index()
    dataset.scaffold_histogram()
    dataset.mol_keys_sorted()
    kinds = {"plain": {}, "scaffolds": dict(scaffolds=True)}
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
    shown = ("unique", "unique_graphs", "n_scaffolds", "scaf", "scaffold_novel", "graph_novel")
    for k in kinds:
        entry = dict(n=n, batch_size=bs, corpus_rows=N, seconds=med(per[k]))
        entry.update({key: last[k][key] for key in shown if key in last[k]})
        res["generate"][k] = entry
        print(f"moses_generate n = {n}, batch {bs}, corpus {N} rows, {k}: median {statistics.median(per[k]):.3f} s (min {min(per[k]):.3f}, max "
              f"{max(per[k]):.3f}), " + ", ".join(f"{key} {entry[key]}" for key in shown if key in entry), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    merged = json.load(open(args.out)) if os.path.exists(args.out) else {}
    merged.update(res)
    json.dump(merged, open(args.out, "w"), indent=1)
