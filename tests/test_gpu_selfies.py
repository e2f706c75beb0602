"""GPU tests of SELFIES on the device: mvae_selfies_decode_rows / _corpus and mvae_selfies_encode_rows / _corpus against the host entries
(the same source compiled for the CPU, which tests/test_selfies_host.py holds against the reference), bit for bit in tokens, lengths,
statuses and info at the block edges; the round trip encode -> decode -> aromatize entirely on the device; MosesDeviceDataset.selfies()
and VAE.to_smiles against the host entries; moses_generate(selfies=) against values recomputed from its own samples."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from molecular_vae_amd import data as D, mosesvae as MV, train as TR, vocab as VC, ops   # noqa: E402
import chem_ref as CR                                                 # noqa: E402
import fp_ref as FR                                                   # noqa: E402
import rewrite_ref as RR                                              # noqa: E402
import selfies_ref as SF                                              # noqa: E402
from test_smiles_aromatize_host import TABLE, STAY_KEKULE, NOT_AROMATIC, NOT_KEKULE, EIGHT_RING       # noqa: E402  (plain data)
from test_selfies_host import EXTRA, HAND, selfies_rows               # noqa: E402  (plain data and the row builder)

DEV = torch.device("cuda")
FILL = 0x7f7f7f7f
NAMES = ("out", "out_len", "status", "info")
T_IN, LD, T_OUT = 131, 134, 131


def _differing(got, want):
    return [(name, torch.nonzero((g.cpu() != w).reshape(w.shape[0], -1).any(1)).flatten()[:5].tolist())
            for g, w, name in zip(got, want, NAMES) if not torch.equal(g.cpu(), w)]


@pytest.fixture(scope="module")
def env():
    """260 SMILES rows (the aromatic hand tables, one refused row of every kind, 100 molecules of MOSES' lengths, a slice of the mutation
    corpus) and 260 SELFIES rows (the hand table of the host test, the encodings of the SMILES rows, random symbol rows of lengths 1 ..
    127), with the host entries' outputs for both, computed once and left unchanged."""
    v, sv = CR.vocabulary(), VC.SelfiesVocab.default()
    tok, chem, emit = VC.smiles_token_table(v), VC.smiles_chem_table(v), VC.smiles_emit_table(v)
    sinfo, semit = VC.selfies_info_table(sv), VC.selfies_emit_table(sv)
    smiles = [s for _, ks, a, _ in TABLE for s in ks + [a]] + STAY_KEKULE + NOT_AROMATIC + NOT_KEKULE + [EIGHT_RING] + EXTRA
    smiles += ["F/C=C/F", "C(", "C=F", "C1=S(C)=CCC1", "c1" + "c" * 123 + "1"] + RR.fragment_corpus(100, seed=1)
    smiles += CR.mutation_corpus()[1000:1000 + 260 - len(smiles)]
    xs = torch.from_numpy(CR.token_rows(smiles, v, LD))
    enc = ops.selfies_encode_host(xs[:, :T_IN], tok, chem, emit, v.eos, semit, sv.bos, sv.eos, sv.pad, 127, T_OUT)
    st = enc[2].tolist()
    assert len(smiles) == 260 and set(st) >= {0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 18} and st.count(0) >= 120
    texts = [r[0] for r in HAND if all(s in sv.sym2char or s.startswith("<") for s in SF.split(r[0]))]
    texts += [sv.ids2string(enc[0][b, :enc[1][b]].tolist()) for b in range(260) if st[b] == 0][:110]
    rs = np.random.RandomState(9)
    while len(texts) < 260:
        texts.append("".join(sv.symbols[i] for i in rs.randint(len(sv.symbols), size=int(rs.randint(1, 128)))))
    xf = torch.from_numpy(selfies_rows(texts, sv, T=LD))
    dec = ops.selfies_decode_host(xf[:, :T_IN], sinfo, emit, v.bos, v.eos, v.pad, 127, T_OUT)
    assert len(texts) == 260 and set(dec[2].tolist()) >= {0, 1} and (dec[2] == 0).sum() >= 200 and (dec[3][:, 2] > 0).sum() >= 3
    return {"v": v, "sv": sv, "smiles": smiles, "texts": texts, "xs": xs, "xf": xf, "enc": enc, "dec": dec,
            "host": (tok, chem, emit, sinfo, semit), "dev": tuple(t.to(DEV) for t in (tok, chem, emit, sinfo, semit))}


def _pre(B, T_out, fill):
    if not fill:
        return (None,) * 4
    return (torch.full((B, T_out), FILL, dtype=torch.int64, device=DEV), torch.full((B,), FILL, dtype=torch.int32, device=DEV),
            torch.full((B,), FILL, dtype=torch.int32, device=DEV), torch.full((B, 4), FILL, dtype=torch.int32, device=DEV))


def _decode(env, x, max_content=127, T_out=T_OUT, counts=None, fill=True, tabs="dev", entry=None):
    v = env["v"]
    tok, chem, emit, sinfo, semit = env[tabs]
    entry = entry or ops.selfies_decode_rows
    kw = {} if entry is ops.selfies_decode_host else {"counts": counts}
    return entry(x, sinfo, emit, v.bos, v.eos, v.pad, max_content, T_out, *_pre(x.shape[0], T_out, fill and tabs == "dev"), **kw)


def _encode(env, x, max_content=127, T_out=T_OUT, counts=None, fill=True, tabs="dev", entry=None):
    v, sv = env["v"], env["sv"]
    tok, chem, emit, sinfo, semit = env[tabs]
    entry = entry or ops.selfies_encode_rows
    kw = {} if entry is ops.selfies_encode_host else {"counts": counts}
    return entry(x, tok, chem, emit, v.eos, semit, sv.bos, sv.eos, sv.pad, max_content, T_out, *_pre(x.shape[0], T_out, fill and tabs == "dev"), **kw)


@pytest.mark.parametrize("B", [1, 63, 65, 130, 260])
@pytest.mark.parametrize("way", ["decode", "encode"])
def test_rows_entries_equal_the_host_entries(env, way, B):
    """B around the block size of 64; a strided input (x_ld = 134 > T = 131); outputs garbage-filled beforehand, so every element must be
    written; a second run is bit-identical; counts is the histogram of status."""
    x = env["xf" if way == "decode" else "xs"].to(DEV)[:B, :T_IN]
    assert x.stride(0) == LD or B == 1
    run = _decode if way == "decode" else _encode
    counts = torch.zeros(32, dtype=torch.int32, device=DEV)
    out = run(env, x, counts=counts)
    want = tuple(t[:B] for t in env["dec" if way == "decode" else "enc"])
    assert not _differing(out, want), _differing(out, want)
    assert torch.equal(counts.cpu(), torch.bincount(want[2], minlength=32).int())
    again = run(env, x, fill=False)
    assert all(torch.equal(a, o) for a, o in zip(again, out))


@pytest.mark.parametrize("way", ["decode", "encode"])
def test_rows_entries_cut_at_t_out_and_honour_max_content(env, way):
    """T_out smaller than needed: the rows are the first columns of the uncut ones and out_len stays; a small max_content gives LONG as
    on the host; info may be left out."""
    name, run = ("xf", _decode) if way == "decode" else ("xs", _encode)
    x = env[name].to(DEV)[:, :T_IN]
    full = run(env, x)
    cut = run(env, x, T_out=9)
    assert torch.equal(cut[0], full[0][:, :9]) and all(torch.equal(c, f) for c, f in zip(cut[1:], full[1:]))
    assert (full[1] > 9).sum() > 50
    host_entry = ops.selfies_decode_host if way == "decode" else ops.selfies_encode_host
    for mc in (1, 12):
        got = run(env, x, max_content=mc)
        want = run(env, env[name][:, :T_IN], max_content=mc, tabs="host", entry=host_entry)
        assert not _differing(got, want) and (want[2] == RR.LONG).sum() >= 10
    v, sv = env["v"], env["sv"]
    tok, chem, emit, sinfo, semit = env["dev"]
    if way == "decode":
        bare = ops.selfies_decode_rows(x, sinfo, emit, v.bos, v.eos, v.pad, 127, T_OUT, info=False)
    else:
        bare = ops.selfies_encode_rows(x, tok, chem, emit, v.eos, semit, sv.bos, sv.eos, sv.pad, 127, T_OUT, info=False)
    assert bare[3] is None and all(torch.equal(b, f) for b, f in zip(bare[:3], full[:3]))


def _corpus_case(strings, tokens, offsets, B):
    """B row ids into a CSR corpus whose row 0 is empty, with a repeat and two ids outside [0, N)."""
    rs = np.random.RandomState(B)
    rows = rs.randint(0, len(strings), size=B)
    rows[0] = 0 if B > 1 else 2
    if B >= 4:
        rows[1], rows[2], rows[3] = rows[B - 1], -1, len(strings)
    return rows


@pytest.mark.parametrize("B", [1, 63, 65, 130])
@pytest.mark.parametrize("way", ["decode", "encode"])
def test_corpus_entries_equal_the_host_entries(env, way, B):
    """One launch over selected CSR rows: tokens_out, offsets_out, status and info equal what the host entry gives for the same rows; an
    id outside the corpus is an empty row with status 1, info 0 0 0 -1 and err 2; counts is the histogram; a second run is identical."""
    v, sv = env["v"], env["sv"]
    tok, chem, emit, sinfo, semit = env["dev"]
    if way == "decode":
        strings = [""] + [t for t in env["texts"] if "<" not in t]
        tokens, offsets = D.tokenize_corpus([sv.encode_chars(t) for t in strings], sv)
    else:
        strings = [""] + [s for s in env["smiles"] if len(s) <= 127]
        tokens, offsets = D.tokenize_corpus(strings, v)
    N, stride = len(strings), 127
    rows = _corpus_case(strings, tokens, offsets, B)
    inside = (rows >= 0) & (rows < N)
    picked = [strings[r] if ok else "" for r, ok in zip(rows, inside)]
    if way == "decode":
        want = _decode(env, torch.from_numpy(selfies_rows(picked, sv, T=129)), T_out=129, tabs="host", entry=ops.selfies_decode_host)
    else:
        want = _encode(env, torch.from_numpy(CR.token_rows(picked, v, 129)), T_out=129, tabs="host", entry=ops.selfies_encode_host)
    tokens_d = torch.from_numpy(np.concatenate([tokens, np.zeros(1, np.uint8)])).to(DEV)
    offsets_d, rows_d = torch.from_numpy(offsets).to(DEV), torch.from_numpy(rows).to(DEV)
    counts = torch.zeros(32, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    pre = (torch.full((B, stride), 0x7f, dtype=torch.uint8, device=DEV), torch.full((2 * B + 1,), FILL, dtype=torch.int64, device=DEV),
           torch.full((B,), FILL, dtype=torch.int32, device=DEV), torch.full((B, 4), FILL, dtype=torch.int32, device=DEV))
    if way == "decode":
        call = lambda *out, **kw: ops.selfies_decode_corpus(tokens_d, offsets_d, N, rows_d, sinfo, emit, 127, stride, *out, **kw)   # noqa: E731
    else:
        call = lambda *out, **kw: ops.selfies_encode_corpus(tokens_d, offsets_d, N, rows_d, tok, chem, emit, semit, 127, stride, *out, **kw)   # noqa: E731
    tokens_out, offsets_out, status, info = call(*pre, counts=counts, err=err)
    lens = want[1].numpy() - 2
    assert int(err.item()) == (2 if not inside.all() else 0)
    assert status.cpu().tolist() == [int(s) if ok else 1 for s, ok in zip(want[2], inside)]
    off = offsets_out.cpu().numpy()
    assert off[0::2].tolist() == [b * stride for b in range(B + 1)] and (off[1::2] - off[0:-1:2]).tolist() == lens.tolist()
    content = np.zeros((B, stride), np.int64)
    for b in range(B):
        content[b, :lens[b]] = want[0][b, 1:1 + lens[b]].numpy()
    assert (tokens_out.cpu().numpy() == content).all()
    # the column of a refused token counts from <bos> in a padded row and from 0 in a CSR row
    want_info = want[3].clone()
    shift = (want[2] == 1) & (want_info[:, 3] >= 0) & torch.from_numpy(inside) if way == "decode" else torch.zeros(B, dtype=torch.bool)
    want_info[shift, 3] -= 1
    want_info[~torch.from_numpy(inside)] = torch.tensor([0, 0, 0, -1], dtype=torch.int32)
    assert torch.equal(info.cpu(), want_info), torch.nonzero((info.cpu() != want_info).any(1)).flatten()[:5]
    assert torch.equal(counts.cpu(), torch.bincount(status.cpu(), minlength=32).int())
    again = call()
    assert all(torch.equal(a, o) for a, o in zip(again, (tokens_out, offsets_out, status, info)))


def test_round_trip_on_the_device(env):
    """encode launch -> decode launch -> aromatize launch: for every row with encode status 0 and aromatize status 0 the result is the
    aromatize launch's row of the original, token for token, and the decode launch refuses none of them."""
    v = env["v"]
    tok, chem, emit, sinfo, semit = env["dev"]
    x = env["xs"].to(DEV)[:, :T_IN]
    a_out, a_len, a_st, _, _ = ops.smiles_aromatize_rows(x, tok, chem, emit, v.bos, v.eos, v.pad, 127, T_OUT, info=False, arom=False)
    e_out, _, e_st, e_info = _encode(env, x)
    d_out, _, d_st, d_info = _decode(env, e_out)
    b_out, b_len, b_st, _, _ = ops.smiles_aromatize_rows(d_out, tok, chem, emit, v.bos, v.eos, v.pad, 127, T_OUT, info=False, arom=False)
    both = (e_st == 0) & (a_st == 0)
    assert int(both.sum()) >= 100 and 2 * int(both.sum()) >= int((a_st == 0).sum())
    assert not d_st[both].any() and not b_st[both].any()
    assert torch.equal(b_out[both], a_out[both]) and torch.equal(b_len[both], a_len[both])
    assert torch.equal(d_info[both][:, 0], e_info[both][:, 0])


@pytest.fixture(scope="module")
def small():
    """A SMILES corpus of 100 molecules of MOSES' lengths, the aromatic hand table and 20 rows the encoder refuses."""
    vocab = CR.vocabulary()
    refused = ["C[C@H](N)O", "CI(C)C", "C(", "c1cccc1", "C[C]C"] * 4
    smiles = RR.fragment_corpus(100, seed=5) + [s for _, ks, a, _ in TABLE for s in ks + [a]] + refused
    return smiles, vocab, D.MosesDeviceDataset(smiles, vocab, device=DEV)


def test_python_surface_equals_the_host_entries(small):
    smiles, vocab, ds = small
    sv = VC.SelfiesVocab.default()
    want, want_st = D.selfies_from_smiles(smiles, vocab, sv, return_status=True)
    fine = [i for i, st in enumerate(want_st.tolist()) if st == 0]
    assert len(fine) >= 120 and set(want_st.tolist()) >= {0, 1, 7, 8, 13, 18}
    sf = ds.selfies()
    assert sf is ds.selfies() and sf.vocab.symbols == sv.symbols and sf.device == ds.device and len(sf) == len(fine)
    assert torch.equal(ds.selfies_status().cpu(), torch.from_numpy(want_st))
    assert sf.source_rows.dtype == torch.int64 and sf.source_rows.cpu().tolist() == fine
    tokens, offsets = sf.tokens.cpu().numpy(), sf.offsets.cpu().numpy()
    got = [sf.vocab.ids2string(tokens[offsets[i]:offsets[i + 1]].tolist()) for i in range(len(sf))]
    assert got == [want[i] for i in fine]
    mine = ds.selfies(sv)
    assert mine is not sf and mine is ds.selfies(sv) and torch.equal(mine.tokens, sf.tokens)
    # VAE.to_smiles on a SELFIES model, against the host decode and the host aromatize behind it
    texts = [want[i] for i in fine] + ["[nop]", "[C][F][C]", "[C][C][C][=Ring1][Ring1]"]
    model = MV.VAE(sv, dtype=torch.float32).to(DEV)
    tabs = (VC.smiles_token_table(vocab), VC.smiles_chem_table(vocab), VC.smiles_emit_table(vocab))
    x = torch.from_numpy(selfies_rows(texts, sv))
    h_out, _, h_st, h_info = ops.selfies_decode_host(x, VC.selfies_info_table(sv), tabs[2], vocab.bos, vocab.eos, vocab.pad, 127, 129)
    rows, status = model.to_smiles(texts, vocab)
    assert rows.shape[1] == max(129, x.shape[1]) and torch.equal(rows.cpu()[:, :129], h_out) and torch.equal(status.cpu(), h_st)
    rows, status, extra = model.to_smiles(x.to(DEV), vocab, info=True)
    assert torch.equal(rows.cpu()[:, :129], h_out) and all(torch.equal(extra[n].cpu(), h_info[:, i]) for i, n in enumerate(ops.SELFIES_DECODE_INFO))
    n_out, _, n_st, _, _ = ops.smiles_aromatize_host(h_out, *tabs, vocab.bos, vocab.eos, vocab.pad, 127, 129, info=False, arom=False)
    rows, status = model.to_smiles(texts, vocab, normal=True)
    assert torch.equal(rows.cpu()[:, :129], n_out) and torch.equal(status.cpu(), torch.where(h_st == 0, n_st, h_st))
    assert (n_out != h_out).any(1).sum() >= 30                          # aromatic rings came back in lower case
    with pytest.raises(ValueError, match="to_smiles"):
        model.sample(2, max_len=10, syntax=True)
    with pytest.raises(ValueError, match="to_smiles"):
        model.sample(2, max_len=10, syntax=True, prefix="[C]")
    with pytest.raises(ValueError, match="SelfiesVocab"):
        MV.VAE(vocab, dtype=torch.float32).to_smiles(["C"], vocab)
    assert D.smiles_from_selfies(texts[:5], sv, vocab) == ["".join(vocab.i2c[int(i)] for i in r[1:list(r).index(vocab.eos)]) for r in h_out[:5].numpy()]


def _host_strings(out, out_len, v):
    return ["".join(v.i2c[int(i)] for i in row[1:k - 1]) for row, k in zip(out.numpy(), out_len.numpy())]


def test_moses_generate_selfies_equals_values_recomputed_from_its_samples():
    """Two batches of 128 of a small randomly initialised SELFIES-vocabulary model: every figure is recomputed from the returned SELFIES
    strings through the host entries; "decoded" is the status-0 count, and the valence-consistent count equals it -- every decoded row
    is a molecule under the walk.  Without selfies= a SMILES model returns exactly the keys it returned."""
    sv, vocab = VC.SelfiesVocab.default(), CR.vocabulary()
    torch.manual_seed(0)
    model = MV.VAE(sv, dtype=torch.float32).to(DEV)
    n, kw = 256, dict(batch_size=128, max_len=24, seed=3)
    first = TR.moses_generate(model, n, selfies=vocab, **kw)
    tabs = (VC.smiles_token_table(vocab), VC.smiles_chem_table(vocab), VC.smiles_emit_table(vocab))
    ids = (vocab.bos, vocab.eos, vocab.pad)
    x = torch.from_numpy(selfies_rows(first["strings"], sv))
    h_out, h_len, h_st, _ = ops.selfies_decode_host(x, VC.selfies_info_table(sv), tabs[2], *ids, 127, 129)
    decoded = _host_strings(h_out, h_len, vocab)
    fine = [i for i, st in enumerate(h_st.tolist()) if st == 0]
    assert len(fine) >= 100
    # a corpus that holds every other decoded molecule, some of them respelled
    respelled = _host_strings(*ops.smiles_rewrite_host(h_out, *tabs, *ids, 5)[:2], vocab)
    corpus = ["CCCCCCCCO"] + [respelled[i] if k % 4 == 0 else decoded[i] for k, i in enumerate(fine[::2])]
    ds = D.MosesDeviceDataset(corpus, vocab, device=DEV)
    flags = dict(count_valid=True, valence=True, kekule=True, canonical=True, normal=True, scaffolds=True, fragments=True, int_div=True,
                 snn=True, nearest=True, novel_against=ds, filters=["C=O", "N"])
    res = TR.moses_generate(model, n, selfies=vocab, **flags, **kw)
    counts = np.array(res["counts"])
    assert res["strings"] == first["strings"] and res["unique"] == len(decoded) and counts.sum() == n == res["total"]
    assert {k: res[k] for k in first} == first and set(first) == {"total", "unique", "strings", "counts", "logq", "decoded", "decode_status"}
    # decode
    assert res["decode_status"] == h_st.tolist() and res["decoded"] == int(counts[fine].sum())
    print("unique", res["unique"], "decoded", res["decoded"], "status", np.bincount(h_st.numpy()).tolist())
    # syntax, valence, kekule: every decoded row is a molecule
    g_st, _, desc, formula = ops.smiles_graph_host(h_out, tabs[0], tabs[1], vocab.eos)
    assert g_st[fine].tolist() == [0] * len(fine)
    assert res["status"] == g_st.tolist() and res["chem_valid"] == res["decoded"] == res["valid"] and res["chem_valid_unique"] == len(fine) == res["valid_unique"]
    assert res["heavy_atoms"] == [int(d) if st == 0 else 0 for d, st in zip(desc[:, 0], g_st)]
    k_st = ops.smiles_kekule_host(h_out, tabs[0], tabs[1], vocab.eos)[0]
    assert res["kekule_status"] == k_st.tolist() and res["kekule_valid"] == int(counts[(k_st == 0).numpy()].sum())
    # canonical and normal form: the decoder writes the canonical spelling already
    c_out, c_len, c_st, _, _ = ops.smiles_canon_host(h_out, *tabs, *ids, 127, 129, info=False, rank=False)
    assert torch.equal(c_out[fine], h_out[fine]) and res["canonical_status"] == c_st.tolist()
    canon = _host_strings(c_out, c_len, vocab)
    assert [res["canonical_strings"][i] for i in fine] == [canon[i] for i in fine] and res["unique_canonical"] == len({canon[i] for i in fine})
    assert res["unique_canonical"] <= len(fine)
    a_out, a_len, a_st, _, _ = ops.smiles_aromatize_host(h_out, *tabs, *ids, 127, 129, info=False, arom=False)
    normal = _host_strings(a_out, a_len, vocab)
    a_fine = [i for i, st in enumerate(a_st.tolist()) if st == 0]
    assert res["normal_status"] == a_st.tolist() and res["unique_normal"] == len({normal[i] for i in a_fine})
    # the corpus: exact rows, canonical rows, the nearest row
    rows = [corpus.index(s) if st == 0 and s in corpus else -1 for s, st in zip(decoded, h_st.tolist())]
    assert res["corpus_row"] == rows and res["novel"] == rows.count(-1) and 0 < res["novel"] < len(rows)
    cc = _host_strings(*ops.smiles_canon_host(torch.from_numpy(CR.token_rows(corpus, vocab)), *tabs, *ids, info=False, rank=False)[:2], vocab)
    c_rows = [cc.index(canon[i]) if c_st[i] == 0 and canon[i] in cc else -1 for i in range(len(canon))]
    assert res["canonical_corpus_row"] == c_rows and sum(c >= 0 and r < 0 for c, r in zip(c_rows, rows)) >= 5
    assert res["novel_canonical"] == len({canon[i] for i in fine if c_rows[i] < 0})
    assert [d == 0 for d in res["nearest_dist"]] == [r >= 0 for r in rows]
    # scaffolds, fragments, fingerprints
    s_st, _, _, s_key = ops.smiles_scaffold_host(h_out, tabs[0], tabs[1], vocab.eos, mask=False)
    assert res["mol_key"] == s_key[:, 0].tolist() and res["scaffold_key"] == s_key[:, 1].tolist()
    assert res["unique_graphs"] == len(set(s_key[:, 0].tolist()) - {0}) and res["n_scaffolds"] == len(set(s_key[:, 1].tolist()) - {0})
    f_st, _, _, f_key = ops.smiles_fragment_host(h_out, tabs[0], tabs[1], vocab.eos, mask=False)
    assert res["n_fragments"] == len(set(f_key.flatten().tolist()) - {0})
    p_st, fp = ops.smiles_fp_host(h_out, tabs[0], tabs[1], vocab.eos)
    p_fine = (p_st == 0).numpy()
    assert res["n_fingerprinted"] == int(p_fine.sum()) == len(fine)
    sim = FR.similarity(fp.numpy()[p_fine], fp.numpy()[p_fine]).astype(np.float64)
    assert abs(res["int_div"] - (1.0 - sim.sum() / p_fine.sum() ** 2)) < 1e-9
    c_fp = ops.smiles_fp_host(torch.from_numpy(CR.token_rows(corpus, vocab)), tabs[0], tabs[1], vocab.eos)[1].numpy()
    best = FR.similarity(fp.numpy()[p_fine], c_fp).max(1).astype(np.float64)
    assert abs(res["snn"] - best.mean()) < 1e-9 and 0.0 <= res["filters"] <= 1.0 and len(res["filter_hits"]) == 2
    assert all(0 <= h <= res["chem_valid"] for h in res["filter_hits"]) and res["filter_hits"][1] > 0
    # without selfies= nothing changes: a SMILES model's keys are what they were, and a SELFIES model without it decodes nothing
    plain = MV.VAE(vocab, dtype=torch.float32).to(DEV)
    assert set(TR.moses_generate(plain, 64, batch_size=64, max_len=12, seed=1)) == {"total", "unique", "strings", "counts", "logq"}
    assert set(TR.moses_generate(model, 64, batch_size=64, max_len=12, seed=1)) == {"total", "unique", "strings", "counts", "logq"}
    with pytest.raises(ValueError, match="SelfiesVocab"):
        TR.moses_generate(plain, 8, selfies=vocab)
    with pytest.raises(ValueError, match="to_smiles"):
        TR.moses_generate(model, 8, selfies=vocab, syntax=True)
