"""What the kekulisation test costs (mvae_smiles_kekule_corpus / MosesDeviceDataset.kekule, moses_generate(kekule=)) on the corpus of
tests/fingerprint_times.py (drug-like strings assembled from fragments, 50,000 draws repeated to N = 1.6 M rows).  One step per process,
so that each can run under a time limit of its own:
  --step corpus    the kekule pass over all N CSR rows beside the graph pass (mvae_smiles_graph_corpus) and the scaffold pass
                   (mvae_smiles_scaffold_corpus), the two yardsticks, alternated, with and without the mate output;
  --step generate  moses_generate with and without kekule=True at the example's batch size under a randomly initialised mosesvae.VAE,
                   alternated;
  --step worst     one launch each over 4,096 copies of a row that is expensive for the matcher: the 125-atom odd ring (the largest graph
                   a row can hold; the greedy start leaves one atom, which needs no search), 25 three-rings in a chain (25 searches
                   that each contract a blossom and fail), and a 111-atom system on which the greedy start is one pair short and the
                   augmenting path runs through an odd ring.  Each launch runs once, after a launch on 64 of the rows that loads the
                   code object.
Device events around each launch (a host clock around moses_generate), the first launch apart; four rounds; medians, with min and max.
No time is a pass criterion.  Not a pytest file.  Each step merges its section into --out.

    python tests/kekule_times.py --step corpus --out profiles/kekule_times.json
"""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--step", required=True, choices=("corpus", "generate", "worst"))
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
n_rows = args.n if args.step == "corpus" else 64 if args.step == "worst" else DISTINCT
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
    sout = ops.smiles_scaffold_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d)
    kout = ops.smiles_kekule_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d)
    knom = ops.smiles_kekule_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d, mate=False)
    r = alternated({"graph_corpus": lambda: ops.smiles_graph_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d, *gout),
                    "scaffold_corpus": lambda: ops.smiles_scaffold_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d, *sout),
                    "kekule_corpus": lambda: ops.smiles_kekule_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d, *kout),
                    "kekule_corpus_no_mate": lambda: ops.smiles_kekule_corpus(dataset.tokens, dataset.offsets, N, tok_d, chem_d, knom[0], knom[1], False)})
    assert torch.equal(gout[0] == 0, (kout[0] == 0) | (kout[0] == 7)) and torch.equal(kout[0], knom[0]) and torch.equal(kout[1], knom[1])
    # what the matcher has to work on: rows with atoms in N, and how many atoms and bonds
    d = kout[1][:DISTINCT]
    r.update(tokens=int(offsets[-1]), status0=int((kout[0] == 0).sum()), status7=int((kout[0] == 7).sum()),
             rows_with_aromatic_atoms=int((d[:, 0] > 0).sum()), mean_aromatic_atoms=float(d[:, 0].float().mean()),
             mean_aromatic_bonds=float(d[:, 1].float().mean()), distinct_strings=len(set(base)),
             ratio_to_graph=r["kekule_corpus"]["ms"]["median"] / r["graph_corpus"]["ms"]["median"],
             ratio_to_scaffold=r["kekule_corpus"]["ms"]["median"] / r["scaffold_corpus"]["ms"]["median"])
    res["corpus"] = r
    for k in ("graph_corpus", "scaffold_corpus", "kekule_corpus", "kekule_corpus_no_mate"):
        m = r[k]["ms"]
        print(f"{k} N = {N}: first {r[k]['first_ms']:.3f} ms, then median {m['median']:.3f} ms (min {m['min']:.3f}, max {m['max']:.3f}); "
              f"{N / (m['median'] * 1e-3):.3e} rows/s", flush=True)
    print(f"kekule / graph {r['ratio_to_graph']:.2f}, kekule / scaffold {r['ratio_to_scaffold']:.2f}; status 0: {r['status0']}, status 7: "
          f"{r['status7']}; among the {DISTINCT} draws: {r['rows_with_aromatic_atoms']} rows with atoms in N, {r['mean_aromatic_atoms']:.1f} atoms "
          f"in N and {r['mean_aromatic_bonds']:.1f} bonds in E on average", flush=True)
elif args.step == "worst":
    chem = VC.OneHotVocab(set("c1[nH]()0123456789"))
    tok_w, chem_w = VC.smiles_token_table(chem).to(dev), VC.smiles_chem_table(chem).to(dev)
    rows = {"odd_ring_125": "c1" + "c" * 124 + "1", "three_rings_25": "c1cc1" * 25,
            "blossom_111": "c0cc1ccccccnccc(cccccccccc2cccccccccccc2c2cccccccccccccccc2c0)ccccccccccnc0cc(ccccccccccccccccccccc0)cccccccccccccccccnccccc1"}
    res["worst"] = {}
    for name, s in rows.items():
        ids = chem.string2ids(s, add_bos=True, add_eos=True)
        x = torch.tensor(ids, dtype=torch.long, device=dev).repeat(4096, 1)
        first = event(lambda: ops.smiles_kekule_rows(x[:64], tok_w, chem_w, chem.eos))
        out = [None]
        ms = event(lambda: out.__setitem__(0, ops.smiles_kekule_rows(x, tok_w, chem_w, chem.eos)))
        status, desc, _ = out[0]
        assert (status == status[0]).all() and (desc == desc[0]).all()
        res["worst"][name] = dict(rows=4096, tokens=len(s), first_64_rows_ms=first, ms=ms, status=int(status[0]), desc=desc[0].tolist())
        print(f"{name}: 4096 rows of {len(s)} tokens, one launch {ms:.3f} ms (a 64-row launch before it {first:.3f} ms), status {int(status[0])}, "
              f"desc {desc[0].tolist()}", flush=True)
else:
    torch.manual_seed(42)
    model = MV.VAE(vocab, dtype=torch.bfloat16).to(dev).eval()
    n, bs = 8192, 4096                                             # examples/sample_moses.py: --n_batch 4096
    kinds = {"plain": {}, "kekule": dict(kekule=True)}
    per = {k: [] for k in kinds}
    last = {}
    for k, kw in kinds.items():
        TR.moses_generate(model, bs, batch_size=bs, syntax=True, seed=9, **kw)      # warm-up
    for r_ in range(args.rounds):
        for k, kw in kinds.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = TR.moses_generate(model, n, batch_size=bs, syntax=True, seed=r_, **kw)
            torch.cuda.synchronize()
            per[k].append(time.perf_counter() - t0)
    res["generate"] = {}
    shown = ("unique", "kekule_valid", "kekule_valid_unique", "kekule_status_counts")
    for k in kinds:
        entry = dict(n=n, batch_size=bs, seconds=med(per[k]))
        entry.update({key: last[k][key] for key in shown if key in last[k]})
        res["generate"][k] = entry
        print(f"moses_generate n = {n}, batch {bs}, {k}: median {statistics.median(per[k]):.3f} s (min {min(per[k]):.3f}, max "
              f"{max(per[k]):.3f}), " + ", ".join(f"{key} {entry[key]}" for key in shown if key in entry), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    merged = json.load(open(args.out)) if os.path.exists(args.out) else {}
    merged.update(res)
    json.dump(merged, open(args.out, "w"), indent=1)
