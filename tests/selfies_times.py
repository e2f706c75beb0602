"""What SELFIES costs against the canonical spelling: mvae_selfies_encode_corpus and mvae_selfies_decode_corpus beside
mvae_smiles_canon_corpus from the same build, on the corpus of tests/smiles_canon_times.py (drug-like strings assembled from fragments,
50,000 draws repeated to N rows).  The decode launch reads the SELFIES corpus the encode launch made of those rows, so the three launches
see the same molecules; decode shares the ranks, the search and the emission with canon, encode has none of them.  One step per process,
so that each can run under a time limit of its own:
  --step batch    one batch of B = 1024 rows of MOSES' lengths: the canon, the encode and the decode launch, alternated;
  --step corpus   one launch of each over all N rows, alternated, and MosesDeviceDataset.selfies() end to end (the launch, the compaction
                  of the gapped CSR and the host's wait for the lengths; a host clock).
Device events around each launch, the first launch apart; medians, with min and max.  No time is a pass criterion: both are reported
against the canon of the same run.  Not a pytest file.  Each step merges its section into --out.

    python tests/selfies_times.py --step batch --out profiles/selfies_times.json
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
svocab = VC.SelfiesVocab.default()
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


def trio(name, rows, stride):
    """The canon, the encode and the decode launch over the same molecules, alternated.  The decode launch reads the gapped CSR the encode
    launch wrote: row 2 b of it is batch member b."""
    a = (dataset.tokens, dataset.offsets, N, rows, tok_d, chem_d, emit_d)
    cn = ops.smiles_canon_corpus(*a, 127, stride)
    en = ops.selfies_encode_corpus(*a, semit_d, 127, 127)
    s_tokens, s_offsets, B = en[0].reshape(-1), en[1], rows.numel()
    s_rows = 2 * torch.arange(B, device=dev)
    d = (s_tokens, s_offsets, 2 * B, s_rows, sinfo_d, emit_d, 127, stride)
    de = ops.selfies_decode_corpus(*d)
    r = alternated({"canon_" + name: lambda: ops.smiles_canon_corpus(*a, 127, stride, *cn),
                    "encode_" + name: lambda: ops.selfies_encode_corpus(*a, semit_d, 127, 127, *en),
                    "decode_" + name: lambda: ops.selfies_decode_corpus(*d, *de)},
                   rounds=None if B <= 4 * BATCH else 4)
    both = (en[2] == 0) & (cn[2] == 0)
    same = (de[0][both] == cn[0][both]).all(1)           # canon of the corpus row against the decoded encoding of it, where canon has no lower case
    r.update({"ratio_encode_to_canon_" + name: r["encode_" + name]["ms"]["median"] / r["canon_" + name]["ms"]["median"],
              "ratio_decode_to_canon_" + name: r["decode_" + name]["ms"]["median"] / r["canon_" + name]["ms"]["median"],
              "encode_status_counts_" + name: torch.bincount(en[2], minlength=32).tolist(),
              "decode_status_counts_" + name: torch.bincount(de[2], minlength=32).tolist(),
              "mean_encode_info_" + name: dict(zip(ops.SELFIES_ENCODE_INFO, en[3].double().mean(0).tolist())),
              "mean_selfies_symbols_" + name: float((en[1][1::2] - en[1][0:-1:2]).double().mean()),
              "decoded_rows_equal_to_canon_" + name: int(same.sum()), "rows_compared_" + name: int(both.sum())})
    return r


tok_d, chem_d = dataset._fp_tables("selfies")
emit_d = VC.smiles_emit_table(vocab).to(dev)
semit_d, sinfo_d = VC.selfies_emit_table(svocab).to(dev), VC.selfies_info_table(svocab).to(dev)
if args.step == "batch":
    rows = torch.from_numpy(np.random.RandomState(1).permutation(N)[:BATCH].astype(np.int64)).to(dev)
    r = trio("1024", rows, 127)
    res["batch"] = r
    show("batch", r)
    print(f"encode / canon = {r['ratio_encode_to_canon_1024']:.3f}, decode / canon = {r['ratio_decode_to_canon_1024']:.3f} at 1024 rows; "
          f"mean encode info {r['mean_encode_info_1024']}", flush=True)
else:
    r = trio("all_rows", torch.arange(N, device=dev), max(dataset.max_len, 127))

    def selfies():
        dataset._selfies = None
        dataset.selfies(svocab)
    r.update(alternated({"dataset_selfies": selfies}, timer=clock, rounds=2))
    r.update(encode_rows_per_second=N / (r["encode_all_rows"]["ms"]["median"] * 1e-3),
             decode_rows_per_second=N / (r["decode_all_rows"]["ms"]["median"] * 1e-3), selfies_rows=len(dataset.selfies(svocab)))
    res["corpus"] = r
    show("corpus", r)
    print(f"N = {N}: encode / canon = {r['ratio_encode_to_canon_all_rows']:.3f}, decode / canon = {r['ratio_decode_to_canon_all_rows']:.3f}; "
          f"{r['encode_rows_per_second']:.3e} / {r['decode_rows_per_second']:.3e} rows/s; {r['selfies_rows']} rows in ds.selfies()", flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    merged = json.load(open(args.out)) if os.path.exists(args.out) else {}
    merged.update(res)
    json.dump(merged, open(args.out, "w"), indent=1)
