"""What the SMILES graph walk costs (mvae_smiles_graph_corpus / MosesDeviceDataset.descriptors, mvae_smiles_graph_rows / VAE.descriptors,
moses_generate(valence=True)) on a corpus of drug-like strings assembled from fragments (50,000 draws, repeated to N = 1.6 M rows):
  (a) the corpus pass, one launch over all N CSR rows, with rows and tokens per second;
  (b) on a padded batch of B = 65,536 of those rows: the graph walk beside the syntax check (mvae_smiles_syntax_check), which reads the
      same tokens and runs the automaton alone -- the difference is what the graph costs;
  (c) moses_generate with and without valence=True at the example's batch size under a randomly initialised mosesvae.VAE.
Device events around each of several launches, the first launch apart (it loads the code object); medians, with min and max.  No time is
a pass criterion.  Not a pytest file.

    python tests/smiles_graph_times.py --out profiles/smiles_graph_times.json
"""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_600_000, help="corpus rows")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--skip_generate", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
sys.path.insert(0, ROOT)
from molecular_vae_amd import data as D, mosesvae as MV, vocab as VC, ops, train as TR   # noqa: E402

DISTINCT = 50_000
# drug-like strings from two-ended pieces closed by a one-ended one: well-formed and valence-consistent, so the walk runs to the end of the
# row as it does on MOSES (data.synthetic_smiles draws characters, and the automaton refuses such a row within a few tokens)
LINKS = ["C", "CC", "O", "N", "C(=O)", "C(C)", "c1ccc(cc1)", "C1CCN(CC1)", "S(=O)(=O)", "c1cc(F)c(cn1)", "C(=O)N", "[C@H](C)", "C=C", "n1cc(nn1)"]
ENDS = ["C", "F", "Cl", "O", "N", "C(F)(F)F", "C#N", "c1ccccc1", "Br", "c1ccc2[nH]ccc2c1", "C1CC1", "[N+](=O)[O-]"]
rs = np.random.RandomState(0)
base = ["C" + "".join(LINKS[i] for i in rs.randint(len(LINKS), size=rs.randint(3, 10))) + ENDS[rs.randint(len(ENDS))] for _ in range(DISTINCT)]
vocab = VC.OneHotVocab.from_data(base)
tok1, off1 = D.tokenize_corpus(base, vocab)
reps = -(-args.n // DISTINCT)
lens = np.tile(np.diff(off1), reps)[:args.n]
offsets = np.zeros(args.n + 1, dtype=np.int64)
np.cumsum(lens, out=offsets[1:])
tokens = np.tile(tok1, reps)[:int(offsets[-1])]
dataset = D.MosesDeviceDataset((tokens, offsets), vocab, device=dev)
N = len(dataset)
tok_d, chem_d = VC.smiles_token_table(vocab).to(dev), VC.smiles_chem_table(vocab).to(dev)
res = dict(n=N, device=torch.cuda.get_device_name(0), corpus_bytes=int(offsets[-1]), mean_len=float(lens.mean()), corpus={}, rows={}, generate={})


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


out = ops.smiles_graph_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d)
run = lambda: ops.smiles_graph_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d, *out)
first = events(run, 1)[0]
times = events(run, args.rounds)
m = statistics.median(times)
counts = torch.bincount(out[0], minlength=7).tolist()
res["corpus"] = dict(first_ms=first, ms=med(times), rows_per_second=N / (m * 1e-3), tokens_per_second=float(offsets[-1]) / (m * 1e-3),
                     status_counts=dict(zip(ops.SMILES_STATUS_NAMES, counts)))
print(f"smiles_graph_corpus N = {N} ({offsets[-1]} tokens): first {first:.3f} ms, then median {m:.3f} ms (min {min(times):.3f}, max "
      f"{max(times):.3f}); {N / (m * 1e-3):.3e} rows/s, {float(offsets[-1]) / (m * 1e-3):.3e} tokens/s; statuses {res['corpus']['status_counts']}",
      flush=True)

B = min(65536, N)
x = dataset.gather(torch.arange(B, device=dev)).x_pad
valid = torch.empty(B, dtype=torch.uint8, device=dev)
bad = torch.empty(B, dtype=torch.int32, device=dev)
gout = ops.smiles_graph_rows(x, tok_d, chem_d, vocab.eos)
for name, run in (("syntax_check", lambda: ops.smiles_syntax_check(x, tok_d, vocab.eos, valid, bad)),
                  ("graph_rows", lambda: ops.smiles_graph_rows(x, tok_d, chem_d, vocab.eos, *gout))):
    first = events(run, 1)[0]
    times = events(run, 3 * args.rounds)
    res["rows"][name] = dict(B=B, T=int(x.shape[1]), first_ms=first, ms=med(times))
    print(f"{name} B = {B}, T = {x.shape[1]}: first {first:.3f} ms, then median {statistics.median(times):.3f} ms "
          f"(min {min(times):.3f}, max {max(times):.3f})", flush=True)
assert bool(((gout[0] != 1) == valid.bool()).all())

if not args.skip_generate:
    torch.manual_seed(42)
    model = MV.VAE(vocab, dtype=torch.bfloat16).to(dev).eval()
    n, bs = 8192, 4096                                             # examples/sample_moses.py: --n_batch 4096
    for valence in (False, True):
        TR.moses_generate(model, bs, batch_size=bs, syntax=True, valence=valence, seed=9)        # warm-up
        per = []
        for r in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out_ = TR.moses_generate(model, n, batch_size=bs, syntax=True, valence=valence, seed=r)
            torch.cuda.synchronize()
            per.append(time.perf_counter() - t0)
        entry = dict(n=n, batch_size=bs, unique=out_["unique"], seconds=med(per))
        if valence:
            entry["chem_valid"] = out_["chem_valid"]
        res["generate"]["valence" if valence else "plain"] = entry
        print(f"moses_generate n = {n}, batch {bs}, syntax=True, valence={valence}: median {statistics.median(per):.3f} s "
              f"(min {min(per):.3f}, max {max(per):.3f}), {out_['unique']} unique" + (f", {out_['chem_valid']} valence-consistent" if valence else ""),
              flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
