"""What SMILES enumeration costs in the input feed (mvae_smiles_rewrite_corpus in front of mvae_moses_collate:
MosesDeviceDataset.batches(augment=True)) on the corpus of tests/fingerprint_times.py without its one stereo fragment (drug-like strings
assembled from fragments, 50,000 draws repeated to N rows).  One step per process, so that each can run under a time limit of its own:
  --step batch    one batch of B = 1024 rows of MOSES' lengths: the plain collate, the rewrite launch alone, and rewrite + collate (what
                  an augmented batch costs, the draw arithmetic included), alternated;
  --step corpus   the same three over the whole corpus: one rewrite launch over all N rows, an epoch of plain batches of 1024 and an
                  epoch of augmented ones (a host clock around each epoch: the launches are asynchronous, the device is waited for once);
  --step plain    the plain collate alone, batch and epoch -- the step to run from a checkout of the parent commit in the same session
                  (--package names the package directory to import), so that the baseline is measured, not copied.
Device events around each launch, the first launch apart; medians, with min and max.  No time is a pass criterion; the 5.26 ms MOSES
training step of the README is quoted beside the figures.  Not a pytest file.  Each step merges its section into --out.

    python tests/smiles_rewrite_times.py --step batch --out profiles/smiles_rewrite_times.json
"""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--step", required=True, choices=("batch", "corpus", "plain"))
ap.add_argument("--n", type=int, default=1_600_000, help="corpus rows")
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--package", default=ROOT, help="the checkout whose molecular_vae_amd is imported")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
sys.path.insert(0, os.path.abspath(args.package))
from molecular_vae_amd import data as D, vocab as VC, ops   # noqa: E402

STEP_MS = 5.26                                                 # README: the MOSES training step at B = 1024 on one MI355X
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
res = dict(n=N, device=torch.cuda.get_device_name(0), rounds=args.rounds, mean_tokens=float(lens.mean()), max_tokens=int(lens.max()),
           training_step_ms=STEP_MS)


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
            print(f"{section} {k}: first {v['first_ms']:.3f} ms, then median {m['median']:.4f} ms (min {m['min']:.4f}, max {m['max']:.4f}); "
                  f"{m['median'] / STEP_MS:.4f} of the {STEP_MS} ms step", flush=True)


rows = torch.from_numpy(np.random.RandomState(1).permutation(N)[:BATCH].astype(np.int64)).to(dev)
T = int(dataset.lengths[rows.cpu().numpy()].max()) + 2


def epoch(**kw):
    for _ in dataset.batches(BATCH, epoch=1, seed=0, **kw):
        pass


if args.step == "plain":
    r = alternated({"collate_1024": lambda: dataset._collate(rows, T)})
    r.update(alternated({"epoch_plain": epoch}, timer=clock, rounds=2))
    r["batches_per_epoch"] = N // BATCH
    res = {"parent_plain": dict(res, **r)}
    show("parent", r)
else:
    tok_d, chem_d = dataset._fp_tables("augment")
    emit_d = VC.smiles_emit_table(vocab).to(dev)
    if args.step == "batch":
        draw = ops.draw_words(rows * 3 + 1)
        out = ops.smiles_rewrite_corpus(dataset.tokens, dataset.offsets, N, rows, tok_d, chem_d, emit_d, 0, draw, T - 2, T - 2)
        r = alternated({"collate_1024": lambda: dataset._collate(rows, T),
                        "rewrite_1024": lambda: ops.smiles_rewrite_corpus(dataset.tokens, dataset.offsets, N, rows, tok_d, chem_d, emit_d, 0, draw, T - 2,
                                                                          T - 2, *out),
                        "rewrite_and_collate_1024": lambda: dataset._collate_augmented(rows, T, 0, 1, 0),
                        "rewrite_and_collate_1024_slack4": lambda: dataset._collate_augmented(rows, T, 0, 1, 4)})
        counts = torch.bincount(out[2], minlength=16).tolist()
        r.update(T=T, status_counts=counts, ratio_to_step=r["rewrite_and_collate_1024"]["ms"]["median"] / STEP_MS,
                 extra_over_collate_ms=r["rewrite_and_collate_1024"]["ms"]["median"] - r["collate_1024"]["ms"]["median"])
        res["batch"] = r
        show("batch", r)
        print(f"T = {T}, status counts {counts}, augmentation / step = {r['ratio_to_step']:.4f}", flush=True)
    else:
        all_rows = torch.arange(N, device=dev)
        stride = dataset.max_len
        out = ops.smiles_rewrite_corpus(dataset.tokens, dataset.offsets, N, all_rows, tok_d, chem_d, emit_d, 0, None, min(stride, 127), stride)
        r = alternated({"rewrite_all_rows": lambda: ops.smiles_rewrite_corpus(dataset.tokens, dataset.offsets, N, all_rows, tok_d, chem_d, emit_d, 0, None,
                                                                              min(stride, 127), stride, *out)}, rounds=4)
        r.update(alternated({"epoch_plain": epoch, "epoch_augmented": lambda: epoch(augment=True)}, timer=clock, rounds=2))
        counts = torch.bincount(out[2], minlength=16).tolist()
        new_len = (out[1][1::2] - out[1][0:-1:2]).cpu().numpy()
        grew = np.bincount(np.clip(new_len - lens, -8, 8) + 8, minlength=17).tolist()
        nb = N // BATCH
        r.update(status_counts=counts, length_change_hist_minus8_to_8=grew, batches_per_epoch=nb,
                 per_batch_plain_ms=r["epoch_plain"]["ms"]["median"] / nb, per_batch_augmented_ms=r["epoch_augmented"]["ms"]["median"] / nb,
                 rows_per_second=N / (r["rewrite_all_rows"]["ms"]["median"] * 1e-3), augment_counts=dataset.augment_counts.tolist())
        res["corpus"] = r
        show("corpus", r)
        print(f"N = {N}: status counts {counts}; per batch plain {r['per_batch_plain_ms']:.4f} ms, augmented {r['per_batch_augmented_ms']:.4f} ms; "
              f"{r['rows_per_second']:.3e} rows/s in one launch; length change histogram (-8 .. +8) {grew}", flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    merged = json.load(open(args.out)) if os.path.exists(args.out) else {}
    merged.update(res)
    json.dump(merged, open(args.out, "w"), indent=1)
