"""Cost of the posterior-collapse remedies on the B = 1024 MOSES train step (bench.py's configs[3] workload: bf16, lengths ~ N(38, 8) in
[10, 57] + 2 specials, train mode with inter-layer dropout, FusedAdam): ms per step (device events) with the options off, with word dropout,
with free bits and with both, alternated in one process after a warm-up, with the spread of the repeated rounds.
  --parent-root DIR: a checkout of the parent commit with its library built.  Its package is loaded beside this one (under another module
    name, with its own library) and its step is alternated with this tree's options-off step in the same process: the default path must sit
    inside the parent's run-to-run spread."""
import argparse, importlib.util, json, os, statistics, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=1024)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--word-dropout", type=float, default=0.3)
ap.add_argument("--free-bits", type=float, default=0.1)
ap.add_argument("--parent-root", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)


def load_package(root, name):
    d = os.path.join(root, "molecular-vae_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class Workload:
    def __init__(self, pkg):
        self.mv = pkg
        v = pkg.vocab.OneHotVocab([chr(ord("a") + i) for i in range(26)])
        torch.manual_seed(42)
        self.model = pkg.mosesvae.VAE(v, dtype=torch.bfloat16).to(dev).train()
        self.optimizer = pkg.FusedAdam(self.model.parameters(), lr=3e-4, max_grad_norm=50.0)
        rs = np.random.RandomState(1234)
        lens = np.sort(np.clip(np.rint(rs.normal(38, 8, size=args.B)), 10, 57).astype(int))[::-1]
        seqs = [torch.tensor([v.bos] + rs.randint(0, 26, size=n).tolist() + [v.eos]) for n in lens]
        self.batch = pkg.vocab.pad_batch(seqs, v.pad).to(dev)

    def step(self, word_dropout=0.0, free_bits=0.0):
        if hasattr(self.model, "word_dropout"):                   # (the parent commit's model has neither attribute)
            self.model.word_dropout, self.model.free_bits = word_dropout, free_bits
        return self.mv.moses_train_step(self.model, self.optimizer, 0.5, self.batch)[0]


def alternate(variants):
    """variants: {name: callable}; rounds of `steps` calls each, the order reversed every other round -> {name: [ms per step]}."""
    for f in variants.values():
        for _ in range(args.warmup):
            f()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = {k: [] for k in variants}
    names = list(variants)
    for r in range(args.rounds):
        for k in (names if r % 2 == 0 else names[::-1]):
            s.record()
            for _ in range(args.steps):
                variants[k]()
            e.record(); torch.cuda.synchronize()
            per[k].append(s.elapsed_time(e) / args.steps)
    return per


def report(per):
    res = {}
    for k, v in per.items():
        med = statistics.median(v)
        res[k] = dict(ms_per_step=med, min=min(v), max=max(v), spread=(max(v) - min(v)) / med, all=v)
        print(f"{k:>12}: {med:.4f} ms/step  (min {min(v):.4f}, max {max(v):.4f}, spread {100 * res[k]['spread']:.2f} %)", flush=True)
    return res


sys.path.insert(0, ROOT)
import molecular_vae_amd as mv          # noqa: E402
wl = Workload(mv)
print(f"mosesvae.VAE train step, B = {args.B}, T = {wl.batch.x_pad.shape[1]}, bf16; {args.rounds} rounds of {args.steps} steps, alternated", flush=True)
p, fb = args.word_dropout, args.free_bits
out = dict(B=args.B, rounds=args.rounds, steps=args.steps, word_dropout=p, free_bits=fb)
out["options"] = report(alternate({"off": lambda: wl.step(), "word_dropout": lambda: wl.step(p, 0.0), "free_bits": lambda: wl.step(0.0, fb),
                                   "both": lambda: wl.step(p, fb)}))
off = out["options"]["off"]["ms_per_step"]
for k in ("word_dropout", "free_bits", "both"):
    d = out["options"][k]["ms_per_step"] - off
    print(f"{k:>12} - off: {1e3 * d:+.1f} us/step ({100 * d / off:+.2f} %)")
if args.parent_root:
    parent = Workload(load_package(args.parent_root, "mvae_parent"))
    assert not hasattr(parent.model, "word_dropout"), "--parent-root is not the parent commit: its VAE already has word_dropout"
    print(f"options-off step of this tree against the parent commit's step ({args.parent_root}), alternated:", flush=True)
    out["vs_parent"] = r = report(alternate({"parent": lambda: parent.step(), "this_off": lambda: wl.step()}))
    d = r["this_off"]["ms_per_step"] - r["parent"]["ms_per_step"]
    margin = r["parent"]["max"] - r["parent"]["min"]
    inside = r["parent"]["min"] <= r["this_off"]["ms_per_step"] <= r["parent"]["max"] or d <= 0
    print(f"this_off - parent: {1e3 * d:+.1f} us/step; the parent's own run-to-run spread is {1e3 * margin:.1f} us "
          f"({r['parent']['min']:.4f} .. {r['parent']['max']:.4f} ms): {'inside' if inside else 'OUTSIDE'}")
    out["vs_parent"]["inside_parent_spread"] = bool(inside)
if args.out:
    json.dump(out, open(args.out, "w"), indent=1)
