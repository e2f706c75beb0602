"""What the corpus index costs (mvae_corpus_index_build / mvae_corpus_index_probe, MosesDeviceDataset.lookup, moses_generate(novel_against=))
on a synthetic corpus in (tokens, offsets) form with MOSES-like sizes -- 1.6 M distinct rows, lengths ~ N(38, 8) in [10, 57], i.i.d. tokens
over the 25 characters of data.synthetic_smiles -- beside the host route it replaces, timed in the same run on the same box:
  (a) build: the memsets and the one kernel, device events around each of several builds (the first one apart: it loads the code object
      and finds the corpus in HBM, the later ones find ~80 MB of it in the 256 MiB Infinity Cache), with the bytes the build must read
      (tokens + offsets) and write (the table) and the time those bytes take at the 6.3 TB/s a streaming copy reaches here;
  (b) probe: one launch for a 4096 x 100 batch of which about half the rows are corpus rows, device events around back-to-back launches;
  (c) one moses_generate batch (4096 samples, max_len 100, syntax=True so that rows end in <eos>) with and without novel_against,
      alternated, wall clock around the call (it ends in a device synchronisation);
  (d) the host route: a Python set of the 1.6 M corpus strings, and ``in`` over 4096 strings.
Medians, with min and max.  Not a pytest file.

    python tests/moses_novelty_times.py --out profiles/moses_novelty_times.json
"""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_600_000, help="corpus rows")
ap.add_argument("--B", type=int, default=4096)
ap.add_argument("--T", type=int, default=100)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
sys.path.insert(0, ROOT)
import molecular_vae_amd as mv          # noqa: E402
from molecular_vae_amd import data as D, mosesvae as MV, vocab as VC, ops   # noqa: E402

HBM_TBS = 6.3                            # what a float4 copy reaches on this part (8.0 is the data sheet's)
ALPHABET = "CNOSFcnos()=#123[]@H+-lBr"
vocab = VC.OneHotVocab(set(ALPHABET))
rs = np.random.RandomState(0)
lens = np.clip(rs.normal(38, 8, size=args.n), 10, 57).astype(np.int64)
offsets = np.zeros(args.n + 1, dtype=np.int64)
np.cumsum(lens, out=offsets[1:])
tokens = rs.randint(0, len(ALPHABET), size=int(offsets[-1])).astype(np.uint8)
dataset = D.MosesDeviceDataset((tokens, offsets), vocab, device=dev)
N = len(dataset)


def med(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), all=v)


def events(fn, reps):
    """Device time of each of `reps` calls of fn, ms."""
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record(); fn(); e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e))
    return out


res = dict(n=N, tokens_bytes=int(tokens.nbytes), device=torch.cuda.get_device_name(0))

# (a) the build
n_slots = 1 << (2 * N - 1).bit_length()
slots = torch.empty(n_slots, dtype=torch.long, device=dev)
nd = torch.empty(1, dtype=torch.long, device=dev)
build = lambda: ops.corpus_index_build(dataset.tokens, dataset.offsets, N, slots, nd)
first = events(build, 1)[0]
times = events(build, args.rounds)
read_b, write_b = int(tokens.nbytes) + 8 * (N + 1), 8 * n_slots
floor_ms = 1e3 * (read_b + write_b) / (HBM_TBS * 1e12)
res["build"] = dict(first_ms=first, ms=med(times), n_slots=n_slots, read_bytes=read_b, table_bytes=write_b, floor_ms=floor_ms,
                    n_distinct=int(nd.item()))
print(f"build, N = {N}, {n_slots} slots: first {first:.3f} ms, then median {res['build']['ms']['median']:.3f} ms (min {min(times):.3f}, max "
      f"{max(times):.3f}); reads {read_b / 1e6:.1f} MB (tokens + offsets), clears {write_b / 1e6:.1f} MB of table: {floor_ms:.3f} ms at "
      f"{HBM_TBS} TB/s; n_distinct {res['build']['n_distinct']}", flush=True)

# (b) the probe: half the rows from the corpus, half random
B, T = args.B, args.T
hit_rows = rs.randint(0, N, size=B // 2)
x = np.full((B, T), vocab.pad, dtype=np.int64)
x[:, 0] = vocab.bos
for b, r in enumerate(hit_rows):
    n = int(lens[r])
    x[b, 1:1 + n] = tokens[offsets[r]:offsets[r + 1]]
    x[b, 1 + n] = vocab.eos
for b in range(B // 2, B):
    n = int(rs.randint(10, 58))
    x[b, 1:1 + n] = rs.randint(0, len(ALPHABET), size=n)
    x[b, 1 + n] = vocab.eos
order = rs.permutation(B)
x_d = torch.from_numpy(x[order]).to(dev)
dataset._slots, dataset._n_distinct_d = slots, nd                  # the table built above
match = torch.empty(B, dtype=torch.long, device=dev)
probe = lambda: ops.corpus_index_probe(dataset.tokens, dataset.offsets, N, slots, x_d, vocab.eos, match)
for _ in range(10):
    probe()
hits = int((match >= 0).sum())
assert (match.cpu().numpy() >= 0).tolist() == (order < B // 2).tolist()
per = []
for _ in range(args.rounds):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(200):
        probe()
    e.record(); torch.cuda.synchronize()
    per.append(1e3 * s.elapsed_time(e) / 200)
res["probe"] = dict(B=B, T=T, hits=hits, us=med(per))
print(f"probe, {B} x {T}, {hits} hits: median {res['probe']['us']['median']:.2f} us per launch, 200 back to back (min {min(per):.2f}, max "
      f"{max(per):.2f})", flush=True)

# (c) one moses_generate batch with and without the lookup
torch.manual_seed(42)
model = MV.VAE(vocab, dtype=torch.bfloat16).to(dev).eval()
z = torch.from_numpy(np.random.RandomState(1).standard_normal((B, model.d_z)).astype(np.float32)).to(dev)


def gen(with_index):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = mv.moses_generate(model, B, batch_size=B, max_len=T, seed=0, z=z, syntax=True, novel_against=dataset if with_index else None)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


gen(False); gen(True)                                               # warm-up: workspaces, staging buffers
per = {False: [], True: []}
for r in range(args.rounds):
    for w in ((False, True) if r % 2 == 0 else (True, False)):
        ms, out = gen(w)
        per[w].append(ms)
res["generate"] = dict(B=B, max_len=T, plain_ms=med(per[False]), novel_ms=med(per[True]), unique=out["unique"])
d = res["generate"]["novel_ms"]["median"] - res["generate"]["plain_ms"]["median"]
print(f"moses_generate, one batch of {B}, max_len {T}, syntax=True: {res['generate']['plain_ms']['median']:.2f} ms without, "
      f"{res['generate']['novel_ms']['median']:.2f} ms with novel_against (difference {d:+.2f} ms; without: min {min(per[False]):.2f}, max "
      f"{max(per[False]):.2f}; with: min {min(per[True]):.2f}, max {max(per[True]):.2f}); the probe launch is "
      f"{100 * res['probe']['us']['median'] / 1e3 / res['generate']['plain_ms']['median']:.3f} % of the batch", flush=True)

# (d) the host route
table = np.array([ord(vocab.i2c[i]) for i in range(len(ALPHABET))], dtype=np.uint8)
raw = table[tokens].tobytes().decode("latin-1")
offs = offsets.tolist()
t0 = time.perf_counter()
strings = [raw[offs[i]:offs[i + 1]] for i in range(N)]
t_slice = time.perf_counter() - t0
t0 = time.perf_counter()
corpus_set = set(strings)
t_set = time.perf_counter() - t0
queries = [vocab.ids2string(r[1:list(r).index(vocab.eos)], rem_bos=False, rem_eos=False) for r in x[order].tolist()]
per = []
for _ in range(args.rounds):
    t0 = time.perf_counter()
    found = [q in corpus_set for q in queries]
    per.append(1e3 * (time.perf_counter() - t0))
assert found == (order < B // 2).tolist()
res["host"] = dict(set_build_s=t_set, slice_strings_s=t_slice, membership_ms=med(per))
print(f"host route: set() of {N} strings {t_set:.3f} s (the strings given; cutting them out of one buffer took {t_slice:.3f} s), `in` over {B} "
      f"strings median {res['host']['membership_ms']['median']:.3f} ms (min {min(per):.3f}, max {max(per):.3f})", flush=True)
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)
