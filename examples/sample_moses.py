#!/usr/bin/env python3
"""The MOSES generation run (hugesample.py's surface: sample in batches of 8192, hash, count unique / valid / total, log a
``time,unique,valid,total`` CSV and samples per second) on the MI355X path.  The reference moves every sampled string to a hasher process;
here ``mv.moses_generate`` hashes the token rows inside the sampling launches and deduplicates them on the device, so only sequences not
seen before in their round reach the host; the rounds are merged in a dictionary.  Checkpoint and vocabulary as ``examples/train_moses.py``
writes them (without them: a seeded random model over a synthetic corpus' vocabulary, which exercises the path but generates noise).
``valid`` needs rdkit (``Chem.MolFromSmiles``); without it the column is left empty.  ``syntax_valid`` needs nothing: it is the number of
samples (duplicates included) that are well-formed SMILES strings -- balanced branches, closed rings and brackets, no dangling bond;
syntax, not chemistry -- counted on the device.  ``--syntax`` samples under that grammar, so that every sample is well-formed.
``--novel_against FILE`` loads the training strings (one per line) into a ``data.MosesDeviceDataset`` and counts ``novel``: the distinct
samples whose token row equals no row of that corpus, looked up on the device in its exact index (no set of strings on the host).
``--neighbors K`` (with ``--novel_against``) encodes that corpus once (``MosesDeviceDataset.encode_latents``) and prints, for the first few
unique samples, their K nearest training molecules in latent space with the squared distances (``MosesLatentIndex.neighbors``).
``--nearest`` (with ``--novel_against``) also asks for every unique sample's nearest training string by token-level Levenshtein distance
(``mv.moses_generate(nearest=True)``, ``MosesDeviceDataset.nearest_strings``) and prints the mean and the histogram of that distance and a
few sample / neighbour pairs.
``--valence`` runs the SMILES graph walk on every batch (``mv.moses_generate(valence=True)``): it prints how many samples are
valence-consistent -- well-formed, every atom within its allowed valence, sane ring bonds, aromatic atoms in rings; a necessary condition
for chemical validity, not rdkit's verdict -- and the others by reason, and the mean and standard deviation of molecular weight and heavy
atoms over the valence-consistent unique samples and, with ``--novel_against``, over the corpus (``MosesDeviceDataset.descriptors``).
``--int_div`` and ``--snn`` (the latter with ``--novel_against``) print the two MOSES figures defined on fingerprints for each round's
samples (``mv.moses_generate(int_div=True, snn=True)``): IntDiv, 1 - the mean pairwise Tanimoto similarity inside the round's distinct
valence-consistent samples (each with itself included, the MOSES form), and SNN, the mean over those samples of the largest similarity to
any training molecule.  The fingerprint is this library's own 1024-bit circular fingerprint (``VAE.fingerprints``), built like ECFP4 but
not rdkit's Morgan fingerprint: the figures compare runs of this script, not published tables.
``--scaffolds`` prints, for each round, the distinct molecular graphs and the distinct Murcko scaffolds among the samples
(``mv.moses_generate(scaffolds=True)``: 64-bit graph keys that do not depend on how a string spells its molecule, so ``OCC`` and ``C(O)C``
are one graph) and, with ``--novel_against``, the MOSES Scaf figure -- the cosine similarity of the generated and the training scaffold
histograms --, the scaffolds and the graphs absent from the corpus; at the end the five most frequent generated scaffolds, each with a
sample that has it and one training molecule that has it (``MosesDeviceDataset.rows_with_scaffold``).  The scaffold is the rings, the
linkers between them and the atoms double-bonded to either, on the graph of the SMILES graph walk: not rdkit's MurckoScaffold.
``--fragments`` prints, for each round, the distinct fragments among the samples (``mv.moses_generate(fragments=True)``: every molecule
cut at its ring substituent bonds and its acyl-heteroatom bonds -- this library's own rule, not BRICS and not RECAP) and, with
``--novel_against``, the MOSES Frag figure: the cosine similarity of the generated and the training fragment histograms.
``--top_scaffolds K`` (with ``--scaffolds``) also prints each round's K most frequent scaffolds as SMILES, with the samples drawn
(``mv.moses_generate(top_scaffolds=K)``: ``VAE.scaffold_smiles``, lost substituents turned into hydrogens, this library's canonical
spelling -- not rdkit's MurckoScaffoldSmiles: nothing is sanitised, no aromaticity perception, no stereo).
``--kekule`` prints, for each round, how many samples are kekulisable (``mv.moses_generate(kekule=True)``: valence-consistent, and every
aromatic atom that needs a ring double bond gets one -- an exact matching on the graph of the SMILES graph walk) and how many fail on
that alone, and with ``--novel_against`` audits the corpus once (``MosesDeviceDataset.kekule``).  A tighter necessary condition than
``--valence`` counts, still not rdkit's verdict: no aromaticity perception, not rdkit's Kekulize.
``--respell N`` prints, at the end, N randomised spellings of each of the first five unique samples (``VAE.respell``: the same graph
under the SMILES graph walk, written from a random root in a random neighbour order -- not canonical, not rdkit's doRandom).
``--canonical`` prints, for each round, the distinct canonical spellings among its samples (``mv.moses_generate(canonical=True)``:
this library's canonical SMILES -- two spellings of one graph count once, compared on tokens; no aromaticity perception, no stereo, not
rdkit's) and, with ``--novel_against``, how many of them are in no row of the canonicalised corpus (``MosesDeviceDataset.canonical``).  It has no
aromaticity perception: for a figure that counts ``C1=CC=CC=C1`` and ``c1ccccc1`` once, see ``--normal``.
``--normal`` prints, for each round, the distinct aromatic normal forms among its samples (``mv.moses_generate(normal=True)``:
aromaticity perceived by this library's own rule -- cycles of 5 - 7 candidate atoms with 4 k + 2 electrons --, then the canonical
spelling, so a Kekule spelling, an aromatic spelling and every respelling of one molecule count once, compared on tokens; no stereo, not
rdkit's aromaticity model) and, with ``--novel_against``, how many of them are in no row of the corpus in normal form
(``MosesDeviceDataset.normal_form``).  With ``--canonical`` both figures stand side by side.
``--filters FILE`` (one SMILES fragment per line, at most 64, each of at most 32 atoms) prints, for each round, the MOSES "Filters"
figure on them (``mv.moses_generate(filters=)``): the share of the valence-consistent samples that contain none of the fragments, and
the hits per fragment.  Fragments are matched as graphs (element, aromatic flag, charge, bond class) -- not SMARTS, so MOSES' own MCF
and PAINS lists cannot be given here, and not rdkit's HasSubstructMatch.
``--reconstruct FILE`` (strings, one per line) skips the generation: it encodes the strings (z = mu), decodes them deterministically
(``--beam_width``) without and with the syntax constraint (``mv.moses_reconstruction(..., syntax=)``) and prints the exact-match
reconstruction fraction of each, the mean log p(x | mu) and the mean token edit distance between input and decode.

    python examples/sample_moses.py --ckpt trained_save.pt --vocab vocab.pkl --rounds 10 --top_p 0.95 --syntax --novel_against train.smi
"""
import argparse
import os
import pickle
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import molecular_vae_amd as mv                          # noqa: E402
from molecular_vae_amd import data as D, mosesvae as MV, vocab as VC   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ckpt", default=None)
ap.add_argument("--vocab", default=None)
ap.add_argument("-b", "--batch_size", default=8192, type=int)                # hugesample.py:113
ap.add_argument("--batches_per_round", default=4, type=int)
ap.add_argument("--rounds", default=5, type=int)
ap.add_argument("--max_len", default=100, type=int)
ap.add_argument("--temp", default=1.0, type=float)
ap.add_argument("--top_k", default=None, type=int)
ap.add_argument("--top_p", default=None, type=float)
ap.add_argument("--syntax", action="store_true", help="constrain every step to the tokens that keep the string well-formed SMILES")
ap.add_argument("--prefix", default=None, metavar="STRING", help="every sample starts with this fragment; the model finishes the string")
ap.add_argument("--prior", default="normal", choices=["normal", "zeros"], help="zeros = sample_z_prior as the reference is written")
ap.add_argument("--seed", default=0, type=int)
ap.add_argument("--log", default="log_small.csv")
ap.add_argument("--novel_against", default=None, metavar="FILE", help="training strings, one per line: count the unique samples not among them")
ap.add_argument("--neighbors", default=0, type=int, metavar="K", help="with --novel_against: print the K nearest training molecules (latent "
                                                                    "space) of the first few unique samples")
ap.add_argument("--nearest", action="store_true", help="with --novel_against: the nearest training string of every unique sample by "
                                                       "token-level Levenshtein distance")
ap.add_argument("--valence", action="store_true", help="count the valence-consistent samples and the others by reason; print weight and "
                                                       "heavy-atom statistics")
ap.add_argument("--int_div", action="store_true", help="print each round's internal diversity (1 - mean pairwise Tanimoto similarity of the "
                                                       "library's circular fingerprints)")
ap.add_argument("--snn", action="store_true", help="with --novel_against: print each round's mean similarity to the nearest training molecule")
ap.add_argument("--scaffolds", action="store_true", help="print each round's distinct graphs and Murcko scaffolds and, with --novel_against, the "
                                                         "Scaf figure; at the end the most frequent generated scaffolds")
ap.add_argument("--kekule", action="store_true", help="count the kekulisable samples (valence-consistent, and the aromatic atoms can all take "
                                                      "their ring double bond)")
ap.add_argument("--respell", default=0, type=int, metavar="N", help="at the end print N randomised spellings (VAE.respell) of each of the first "
                                                                   "five unique samples the walk accepts")
ap.add_argument("--fragments", action="store_true", help="print each round's distinct fragments (this library's own cut rule, not BRICS) and, "
                                                         "with --novel_against, the Frag figure")
ap.add_argument("--top_scaffolds", type=int, default=0, help="with --scaffolds: print each round's K most frequent scaffolds as SMILES "
                                                             "(this library's scaffold SMILES, not rdkit's MurckoScaffoldSmiles)")
ap.add_argument("--canonical", action="store_true", help="print each round's distinct canonical spellings (unique@k on graphs) and, with "
                                                         "--novel_against, those absent from the canonicalised corpus")
ap.add_argument("--normal", action="store_true", help="print each round's distinct aromatic normal forms (unique@k on molecules: a Kekule and "
                                                      "an aromatic spelling count once) and, with --novel_against, those absent from the "
                                                      "corpus in normal form")
ap.add_argument("--selfies", action="store_true", help="the model's vocabulary is a vocab.SelfiesVocab (--vocab, else SelfiesVocab.default()): "
                                                       "every batch is decoded to SMILES on the device (this library's own SELFIES rules, not "
                                                       "the selfies package's) and every figure is computed on the decoded rows")
ap.add_argument("--filters", default=None, metavar="FILE", help="SMILES fragments, one per line: print each round's share of valence-consistent "
                                                                   "samples that contain none of them, and the hits per fragment")
ap.add_argument("--reconstruct", default=None, metavar="FILE", help="strings, one per line: report exact-match reconstruction at z = mu "
                                                                  "without and with the syntax constraint, then exit")
ap.add_argument("--beam_width", default=1, type=int, help="with --reconstruct: the beam width of the deterministic decode")
ap.add_argument("--out", default=None, help="write the unique strings with their counts (and, with --novel_against, 1 for novel / 0) here, "
                                            "tab separated")
args = ap.parse_args()

try:
    from rdkit import Chem, rdBase
    rdBase.DisableLog("rdApp.error")
except ImportError:
    Chem = None

dev = torch.device("cuda", 0)
if args.vocab:
    with open(args.vocab, "rb") as f:
        vocab = pickle.load(f)
else:
    vocab = VC.OneHotVocab.from_data(D.synthetic_smiles(2048, seed=0))
smiles_vocab = vocab                                      # the vocabulary of the molecules: the corpus, the filters, the figures
if args.selfies:                                          # ... and `vocab`, the model's, spells SELFIES symbols
    if args.reconstruct:
        sys.exit("--selfies excludes --reconstruct: the file holds SMILES and the model reads SELFIES (encode it with data.selfies_from_smiles)")
    if not isinstance(vocab, VC.SelfiesVocab):
        vocab = VC.SelfiesVocab.default()
    writes = set("BCNOPSFIHclrnos=#()[]+-0123456789")     # every character the decoder can write
    lines = D.load_smiles(args.novel_against) if args.novel_against else []
    foreign = sorted(set().union(*map(set, lines)) - writes) if lines else []
    if foreign:                                           # they get ids, so that the corpus rows stay what they are; no sample can equal such a row
        print(f"--selfies: the corpus uses characters no decoded row holds: {' '.join(foreign)}", flush=True)
    smiles_vocab = VC.OneHotVocab(writes | set(foreign))
torch.manual_seed(42)
model = MV.VAE(vocab)
if args.ckpt:
    model.load_state_dict(mv.strip_module_prefix(torch.load(args.ckpt, map_location="cpu")))
model = model.to(dev).eval()
model.prior = args.prior
model.seed_noise(args.seed)
corpus = mv.MosesDeviceDataset(D.load_smiles(args.novel_against), smiles_vocab, device=dev) if args.novel_against else None

if args.reconstruct:
    collate = VC.get_collate_fn(vocab)
    strings = D.load_smiles(args.reconstruct)
    batches = [collate(strings[i:i + args.batch_size]) for i in range(0, len(strings), args.batch_size)]
    for syntax in (False, True):
        t0 = time.time()
        frac, mean_lp, mean_ed = mv.moses_reconstruction(model, batches, beam_width=args.beam_width, max_len=args.max_len, syntax=syntax,
                                                         edit_distance=True)
        print(f"reconstruction of {len(strings)} strings, beam width {args.beam_width}, syntax={syntax}: exact match {frac:.4f}, "
              f"mean log p(x | mu) {mean_lp:.3f}, mean token edit distance {mean_ed:.3f}, {time.time() - t0:.2f} s", flush=True)
    sys.exit(0)


def is_valid(s):
    try:
        return Chem.MolFromSmiles(s) is not None
    except Exception:
        return False


if args.nearest and corpus is None:
    sys.exit("--nearest needs --novel_against (the training strings to search)")
if args.snn and corpus is None:
    sys.exit("--snn needs --novel_against (the training strings to search)")
filters = None
if args.filters:
    with open(args.filters) as ff:
        filters = mv.compile_substructures([line.strip() for line in ff if line.strip()], smiles_vocab)
seen, total, valid, syntax_valid = {}, 0, 0, 0
chem_valid, reasons, props = 0, [0] * 7, {}               # unique valence-consistent string -> (weight, heavy atoms)
near = {}                                                 # unique string -> (distance, corpus row) of its nearest training string
novel = set()                                             # the unique strings that are not in the corpus
kekule_valid, kekule_failed = 0, 0                        # samples with status 0 / 7 under the kekule entry, duplicates included
scaffold_count, scaffold_sample = {}, {}                  # scaffold key -> samples drawn with it (duplicates included), one such string
per_round = args.batch_size * args.batches_per_round
start = time.time()
with open(args.log, "w", buffering=1) as f:
    f.write("time,unique,valid,total,syntax_valid" + (",novel\n" if corpus is not None else "\n"))
    for r in range(args.rounds):
        res = mv.moses_generate(model, per_round, batch_size=args.batch_size, max_len=args.max_len, temp=args.temp, top_k=args.top_k,
                                top_p=args.top_p, seed=args.seed + r * args.batches_per_round, syntax=args.syntax, count_valid=True,
                                novel_against=corpus, prefix=args.prefix, nearest=args.nearest, valence=args.valence,
                                int_div=args.int_div, snn=args.snn, scaffolds=args.scaffolds, kekule=args.kekule, canonical=args.canonical,
                                filters=filters, top_scaffolds=args.top_scaffolds if args.scaffolds else 0, fragments=args.fragments, normal=args.normal,
                                selfies=smiles_vocab if args.selfies else None)
        total += res["total"]
        if args.selfies:
            print(f"round {r}: {res['decoded']} of {res['total']} SELFIES samples decoded to a SMILES row", flush=True)
        if args.kekule:
            kekule_valid += res["kekule_valid"]
            kekule_failed += res["kekule_status_counts"][7]
        if args.scaffolds:
            for s, c, key in zip(res["strings"], res["counts"], res["scaffold_key"]):
                if key:
                    scaffold_count[key] = scaffold_count.get(key, 0) + c
                    scaffold_sample.setdefault(key, s)
        if args.valence:
            chem_valid += res["chem_valid"]
            reasons = [a + res["status_counts"][k] for k, a in enumerate(reasons)]
            props.update((s, (w, h)) for s, st, w, h in zip(res["strings"], res["status"], res["weight"], res["heavy_atoms"]) if st == 0)
        syntax_valid += res["valid"]
        for i, (s, c) in enumerate(zip(res["strings"], res["counts"])):
            if s not in seen:
                seen[s] = 0
                if corpus is not None and res["is_novel"][i]:
                    novel.add(s)
                if args.nearest:
                    near[s] = (res["nearest_dist"][i], res["nearest_row"][i])
                if Chem is not None and is_valid(s):
                    valid += 1
            seen[s] += c
        now = time.time()
        f.write("{0},{1},{2},{3},{4}".format(now, len(seen), valid if Chem is not None else "", total, syntax_valid)
                + (f",{len(novel)}\n" if corpus is not None else "\n"))
        print(f"round {r}: unique {len(seen)} ({len(seen) / total:.3f}), sampled {total}, samples per second {total / (now - start):.0f}, "
              f"unique per second {len(seen) / (now - start):.0f}, well-formed {syntax_valid} ({syntax_valid / total:.3f})"
              + (f", valence-consistent {chem_valid} ({chem_valid / total:.3f})" if args.valence else "")
              + (f", kekulisable {kekule_valid} ({kekule_valid / total:.3f}), valence-consistent but not kekulisable {kekule_failed}"
                 if args.kekule else "")
              + (f", IntDiv of this round's {res['n_fingerprinted']} valence-consistent unique samples {res['int_div']:.4f}" if args.int_div else "")
              + (f", SNN {res['snn']:.4f}" if args.snn else "")
              + (f", this round's distinct graphs {res['unique_graphs']} and scaffolds {res['n_scaffolds']}" if args.scaffolds else "")
              + (f", this round's distinct fragments {res['n_fragments']} (samples of more than 16 fragments: {res['fragment_many']})"
                 if args.fragments else "")
              + (f", Frag {res['frag']:.4f}" if args.fragments and corpus is not None else "")
              + (f", Scaf {res['scaf']:.4f}, scaffolds not in the corpus {res['scaffold_novel']}, graphs not in the corpus {res['graph_novel']}"
                 if args.scaffolds and corpus is not None else "")
              + (f", this round's distinct canonical spellings {res['unique_canonical']} of {res['canonical_status_counts'][0]} written"
                 if args.canonical else "")
              + (f", of which in no corpus row {res['novel_canonical']}" if args.canonical and corpus is not None else "")
              + (f", this round's distinct aromatic normal forms {res['unique_normal']} of {res['normal_status_counts'][0]} written"
                 if args.normal else "")
              + (f", of which in no corpus row {res['novel_normal']}" if args.normal and corpus is not None else "")
              + (f", Filters {res['filters']:.4f} (hits " + ", ".join(f"{p} {h}" for p, h in zip(filters.patterns, res["filter_hits"]))
                 + f"; undecided {sum(res['filter_undecided'])})" if filters is not None else "")
              + (f", valid unique {valid}" if Chem is not None else "")
              + (f", novel {len(novel)} ({len(novel) / len(seen):.3f} of unique)" if corpus is not None else ""), flush=True)
        if args.scaffolds and args.top_scaffolds > 0:
            print(f"round {r}: the most frequent scaffolds (samples drawn): " + ", ".join(f"{s} {c}" for s, c in res["top_scaffolds"]), flush=True)
if args.respell > 0 and seen:
    picked = [s for s in list(seen)[:256] if s][:64]
    ok = model.chem_valid(picked).tolist() if picked else []
    for s in [s for s, good in zip(picked, ok) if good][:5]:
        rows, status = model.respell([s] * args.respell, seed=args.seed, draw=torch.arange(args.respell))
        texts = set()
        for ids, st in zip(rows.tolist(), status.tolist()):
            if st == 0:
                texts.add("".join(vocab.i2c[i] for i in ids[1:ids.index(vocab.eos)]))
        print(f"respell {s}: " + " ".join(sorted(texts)), flush=True)
if args.kekule and corpus is not None:
    st = corpus.kekule()["status"]
    print(f"corpus: {int((st == 0).sum())} of {corpus.n} rows kekulisable, {int((st == 7).sum())} valence-consistent but not kekulisable",
          flush=True)
if args.scaffolds and scaffold_count:
    top = sorted(scaffold_count, key=lambda k: (-scaffold_count[k], k))[:5]
    shown = [scaffold_sample[k] for k in top]
    names = [None] * len(top)
    if corpus is not None:
        offsets, rows = corpus.rows_with_scaffold(shown)
        offsets, rows = offsets.tolist(), rows.tolist()
        first = [rows[offsets[i]] if offsets[i + 1] > offsets[i] else -1 for i in range(len(top))]
        names = corpus.smiles(first)
        shared = [offsets[i + 1] - offsets[i] for i in range(len(top))]
    print(f"{len(scaffold_count)} distinct scaffolds among {total} samples; the most frequent (samples drawn, a sample that has it"
          + (", training molecules that have it, one of them" if corpus is not None else "") + "):", flush=True)
    for i, k in enumerate(top):
        print(f"    {scaffold_count[k]:8d}  {shown[i]}" + (f"  {shared[i]:8d}  {names[i] if names[i] is not None else '-'}" if corpus is not None else ""))
if args.valence:
    from molecular_vae_amd import ops

    def mean_std(t):
        t = torch.as_tensor(t, dtype=torch.float64)
        return f"{float(t.mean()):.2f} +- {float(t.std(unbiased=False)):.2f}" if t.numel() else "n/a"
    print(f"valence check of {total} samples: " + ", ".join(f"{ops.SMILES_STATUS_NAMES[k]} {n}" for k, n in enumerate(reasons)), flush=True)
    print(f"    {len(props)} valence-consistent unique samples: weight {mean_std([w for w, _ in props.values()])}, heavy atoms "
          f"{mean_std([h for _, h in props.values()])}", flush=True)
    if corpus is not None:
        d = corpus.descriptors()
        ok = d["status"] == 0
        print(f"    {int(ok.sum())} of {len(corpus)} corpus rows valence-consistent: weight {mean_std(d['weight'][ok].cpu())}, heavy atoms "
              f"{mean_std(d['heavy_atoms'][ok].cpu())}", flush=True)
if near:
    dists = sorted(d for d, _ in near.values())
    hist = {}
    for d in dists:
        hist[min(d, 10)] = hist.get(min(d, 10), 0) + 1
    print(f"nearest training string of {len(near)} unique samples: mean token edit distance {sum(dists) / len(dists):.2f}, median "
          f"{dists[len(dists) // 2]}; histogram " + ", ".join(f"{'10+' if d == 10 else d}: {hist[d]}" for d in sorted(hist)), flush=True)
    shown = [s for s in list(near)[:8]]
    for s, name in zip(shown, corpus.smiles([near[s][1] for s in shown])):
        print(f"    {near[s][0]:4d}  {s}  <-  {name}")
if args.neighbors > 0 and corpus is None:
    print("--neighbors needs --novel_against (the training strings to search)", flush=True)
elif args.neighbors > 0:
    t0 = time.time()
    index = corpus.encode_latents(model)
    shown = [s for s in list(seen)[:8] if s]
    if shown:
        dist, rows = index.neighbors(shown, args.neighbors, model)
        names = corpus.smiles(rows)                                 # waits for the search; one copy
        print(f"latent table of {len(corpus)} molecules and {len(shown)} searches: {time.time() - t0:.2f} s")
        for i, (s, d) in enumerate(zip(shown, dist.tolist())):
            print(f"{s}  ({'novel' if s in novel else 'in the corpus'})")
            for j in range(args.neighbors):
                if names[i * args.neighbors + j] is not None:
                    print(f"    {d[j]:10.4f}  {names[i * args.neighbors + j]}")
if args.out:
    with open(args.out, "w") as f:
        for s, c in sorted(seen.items(), key=lambda kv: -kv[1]):
            f.write(f"{s}\t{c}" + (f"\t{int(s in novel)}\n" if corpus is not None else "\n"))
