"""What the substructure search costs (mvae_smiles_substruct_rows / _corpus) beside the graph walk alone (mvae_smiles_graph_corpus) and
the rewrite, which builds the same adjacency (mvae_smiles_rewrite_corpus), on the corpus of tests/smiles_canon_times.py (drug-like
strings assembled from fragments, 50,000 draws repeated to N rows).  One step per process, so that each can run under a time limit of
its own:
  --step batch    one batch of B = 1024 rows of MOSES' lengths as padded rows: the graph launch, the rewrite launch and the substructure
                  launch with 1, 16 and 64 queries, alternated; then the budget row -- 64 copies of 25 cyclopropanes against a 16-ring,
                  which uses up 65,536 steps and ends after 92,938 of 131,072;
  --step corpus   one launch of each over all N rows with 1 and 16 queries, alternated, and MosesDeviceDataset.substructure_counts.
Device events around each launch, the first launch apart; medians, with min and max.  No time is a pass criterion.  Not a pytest file.
Each step merges its section into --out.

    python tests/substruct_times.py --step batch --out profiles/substruct_times.json
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
QUERIES = ["C(=O)O", "c1ccccc1", "C(=O)N", "S(=O)(=O)", "C#N", "c1ccncc1", "C[N+](=O)[O-]", "C1CCNCC1", "CCCCCCCC", "c1ccc2[nH]ccc2c1", "C1CC1",
           "C(F)(F)F", "C(C)(C)C", "c1cc[nH]c1", "CCCCCCCN", "C1CCCCC1", "C=C", "Cl", "c1ccc(cc1)C(=O)", "Br", "n1ccnn1", "CC(C)CC(C)CC(C)C"]
QUERIES = list(dict.fromkeys(QUERIES + LINKS + ENDS + ["C" * k for k in range(3, 33)] + ["CO", "CN", "CCO", "CCN", "OCCO", "NCCN"]))[:64]
assert len(QUERIES) == 64
BUDGET_QUERY, BUDGET_ROW = "C1CCCCCCCCCCCCCCC1", "C1CC1" * 25 + "CC"
rs = np.random.RandomState(0)
base = ["C" + "".join(LINKS[i] for i in rs.randint(len(LINKS), size=rs.randint(3, 10))) + ENDS[rs.randint(len(ENDS))] for _ in range(DISTINCT)]
vocab = VC.OneHotVocab.from_data(base + ["0123456789"])
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


def tables(n):
    return D.compile_substructures(QUERIES[:n], vocab).on(dev)


tok_d, chem_d = dataset._fp_tables("substructure_counts")
emit_d = VC.smiles_emit_table(vocab).to(dev)
if args.step == "batch":
    ids = [vocab.string2ids(base[i % DISTINCT], add_bos=True, add_eos=True) for i in np.random.RandomState(1).permutation(N)[:BATCH]]
    T = max(map(len, ids))
    x = torch.full((BATCH, T), vocab.pad, dtype=torch.long)
    for b, row in enumerate(ids):
        x[b, :len(row)] = torch.as_tensor(row)
    x = x.to(dev)
    runs = {"graph_1024": lambda: ops.smiles_graph_rows(x, tok_d, chem_d, vocab.eos),
            "rewrite_1024": lambda: ops.smiles_rewrite_rows(x, tok_d, chem_d, emit_d, vocab.bos, vocab.eos, vocab.pad)}
    outs = {}
    for q in (1, 16, 64):
        t = tables(q)
        outs[q] = ops.smiles_substruct_rows(x, tok_d, chem_d, vocab.eos, t)
        runs[f"substruct_1024_q{q}"] = (lambda t=t, o=outs[q]: ops.smiles_substruct_rows(x, tok_d, chem_d, vocab.eos, t, 65536, None, o[0], o[1], o[2],
                                                                                         steps=o[4]))
    r = alternated(runs)
    for q in (1, 16, 64):
        steps = outs[q][4].double()
        r[f"steps_q{q}"] = dict(mean_per_pair=float(steps.mean()), max=int(steps.max()), hits=ops.substruct_bits(outs[q][1], q).sum(0).tolist(),
                                undecided=int(ops.substruct_bits(outs[q][2], q).sum()))
    r["per_query_ms_16_to_64"] = (r["substruct_1024_q64"]["ms"]["median"] - r["substruct_1024_q16"]["ms"]["median"]) / 48
    # the budget row
    ids = [vocab.string2ids(BUDGET_ROW, add_bos=True, add_eos=True)] * 64
    xb = torch.tensor(ids, dtype=torch.long, device=dev)
    tb = D.compile_substructures([BUDGET_QUERY], vocab).on(dev)
    r.update(alternated({f"budget_row_x64_{b}": (lambda b=b: ops.smiles_substruct_rows(xb, tok_d, chem_d, vocab.eos, tb, b)) for b in (65536, 131072)},
                        rounds=4))
    for b in (65536, 131072):
        o = ops.smiles_substruct_rows(xb, tok_d, chem_d, vocab.eos, tb, b)
        r[f"budget_row_{b}"] = dict(steps=int(o[4][0, 0]), undecided=int(o[2][0]), hit=int(o[1][0]))
    r["T"] = T
    res["batch"] = r
    show("batch", r)
    print({k: v for k, v in r.items() if k.startswith(("steps_", "budget_row_6", "budget_row_1", "per_query"))}, flush=True)
else:
    runs = {"graph_all_rows": lambda: ops.smiles_graph_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d),
            "rewrite_all_rows": lambda: ops.smiles_rewrite_corpus(dataset.tokens, dataset.offsets, N, torch.arange(N, device=dev), tok_d, chem_d, emit_d,
                                                                  0, None, 127, max(dataset.max_len, 127))}
    outs = {}
    for q in (1, 16):
        t = tables(q)
        outs[q] = ops.smiles_substruct_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d, t, steps=False)
        runs[f"substruct_all_rows_q{q}"] = (lambda t=t, o=outs[q]: ops.smiles_substruct_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d, t, 65536,
                                                                                               None, o[0], o[1], o[2], steps=False))
    r = alternated(runs, rounds=4)
    r["per_query_ms_1_to_16"] = (r["substruct_all_rows_q16"]["ms"]["median"] - r["substruct_all_rows_q1"]["ms"]["median"]) / 15
    counts = dataset.substructure_counts(QUERIES[:16])
    r["counts_q16"] = dict(zip(QUERIES[:16], counts.cpu().tolist()))
    r["rows_per_second_q16"] = N / (r["substruct_all_rows_q16"]["ms"]["median"] * 1e-3)
    res["corpus"] = r
    show("corpus", r)
    print(f"N = {N}: each further query adds {r['per_query_ms_1_to_16']:.3f} ms; counts {r['counts_q16']}", flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    merged = json.load(open(args.out)) if os.path.exists(args.out) else {}
    merged.update(res)
    json.dump(merged, open(args.out, "w"), indent=1)
