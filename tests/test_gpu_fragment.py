"""GPU tests of the fragment feature: mvae_smiles_fragment_rows / _corpus and mvae_smiles_fragment_smiles_rows / _corpus against the host
entries (the same source compiled for the CPU, which tests/test_fragment_host.py holds against the reference of tests/frag_ref.py), bit
for bit at the block edges; the edge rows against the reference as well; VAE.fragments / fragment_smiles, MosesDeviceDataset.fragments /
fragment_histogram / rows_with_fragment and moses_generate(fragments=True) against the reference on the strings."""
import collections
import inspect
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import molecular_vae_amd as mv                                        # noqa: E402
from molecular_vae_amd import data as D, mosesvae as MV, vocab as VC, ops   # noqa: E402
import chem_ref as CR                                                 # noqa: E402
import frag_ref as FG                                                 # noqa: E402
import scaffold_ref as SR                                             # noqa: E402

DEV = torch.device("cuda")
FILL = 0x7f7f7f7f
KEYS = {"total", "unique", "strings", "counts", "logq"}
KEYS_NOVEL = {"corpus_row", "is_novel", "novel"}
NEW = {"n_fragments", "fragment_many"}
NEW_NOVEL = {"frag"}
RINGS16, RINGS17 = "C1CC1" * 16, "C1CC1" * 17


@pytest.fixture(scope="module")
def env():
    """The mutation corpus with the host entries' outputs for it, computed once and left unchanged: the keys entry, and the string entry
    for frag = 0, 1 and 15 (T_out = 131).  The two ring rows stand in front of the string entry's rows, so that frag = 15 writes something."""
    v = CR.vocabulary()
    tok, chem, emit = VC.smiles_token_table(v), VC.smiles_chem_table(v), VC.smiles_emit_table(v)
    strings = CR.mutation_corpus()
    x = torch.from_numpy(CR.token_rows(strings, v))
    host = tuple(t.numpy() for t in ops.smiles_fragment_host(x, tok, chem, v.eos))
    srows = [RINGS16, RINGS17] + strings[:-2]
    sx = torch.from_numpy(CR.token_rows(srows, v, 134))
    shost = {f: ops.smiles_fragment_smiles_host(sx, tok, chem, emit, v.bos, v.eos, v.pad, f, 127, 131) for f in (0, 1, 15)}
    assert (shost[15][2] == 0).sum() == 2 and (shost[1][2] == 0).sum() >= 200 and (shost[1][2] == FG.NO_FRAGMENT).sum() >= 200
    return {"v": v, "tok": tok, "chem": chem, "emit": emit, "tabs": (tok.to(DEV), chem.to(DEV)), "emit_d": emit.to(DEV), "strings": strings,
            "x": x, "host": host, "srows": srows, "sx": sx, "shost": shost}


def _filled(n):
    return (torch.full((n,), FILL, dtype=torch.int32, device=DEV), torch.full((n, 16, 2), 0x7f7f7f7f7f7f7f7f, dtype=torch.int64, device=DEV),
            torch.full((n, 4), FILL, dtype=torch.int32, device=DEV), torch.full((n, 16), 0x7f7f7f7f7f7f7f7f, dtype=torch.int64, device=DEV))


def _same(got, want):
    for g, w, name in zip(got, want, ("status", "mask", "desc", "key")):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        w = w.cpu().numpy() if torch.is_tensor(w) else w
        wrong = np.nonzero((g != w).reshape(g.shape[0], -1).any(1))[0]
        assert g.shape == w.shape and wrong.size == 0, (name, wrong[:5].tolist(), g[wrong[:3]].tolist(), w[wrong[:3]].tolist())


@pytest.mark.parametrize("B", [1, 63, 64, 65, 4250])
def test_rows_entry_equals_the_host_entry(env, B):
    """B around the block size of 64, and the whole corpus; the outputs are garbage-filled beforehand, so every element must be written
    and a row that is not ok must come back zeroed; a second run is bit-identical; the mask may be left out."""
    lo = 0 if B == 4250 else 1000                                    # a stretch of the sorted corpus with several statuses
    x = env["x"][lo:lo + B].to(DEV)
    want = tuple(w[lo:lo + B] for w in env["host"])
    assert B < 60 or len(set(want[0].tolist())) >= 3
    out = _filled(B)
    ops.smiles_fragment_rows(x, *env["tabs"], env["v"].eos, *out)
    _same(out, want)
    bad = out[0] != 0
    assert not out[1][bad].any() and not out[2][bad].any() and not out[3][bad].any()     # this corpus has no FRAG_MANY row
    again = ops.smiles_fragment_rows(x, *env["tabs"], env["v"].eos)
    assert all(torch.equal(a, o) for a, o in zip(again, out))
    status, _, desc, key = _filled(B)
    got = ops.smiles_fragment_rows(x, *env["tabs"], env["v"].eos, status, False, desc, key)
    assert got[1] is None and torch.equal(status, out[0]) and torch.equal(desc, out[2]) and torch.equal(key, out[3])


@pytest.mark.parametrize("N", [1, 63, 64, 65, 4250])
def test_corpus_entry_equals_the_host_entry(env, N):
    """The CSR entry in one launch, with an empty row, a 127-token row and a 128-token row in front (3 < N < 4250)."""
    v = env["v"]
    first = ["", "C1CC1" + "C" * 117 + "C1CC1", "C" * 128]
    strings = [first[1]] if N == 1 else first + env["strings"][1000:1000 + N - 3] if N < 4250 else env["strings"]
    assert len(strings) == N
    tokens, offsets = D.tokenize_corpus(strings, v)
    tokens = torch.from_numpy(np.concatenate([tokens, np.zeros(1, np.uint8)])).to(DEV)
    offsets = torch.from_numpy(offsets).to(DEV)
    out = _filled(N)
    ops.smiles_fragment_corpus(tokens, offsets, N, *env["tabs"], *out)
    if N == 4250:
        want = env["host"]
    else:
        want = tuple(t.numpy() for t in ops.smiles_fragment_host(torch.from_numpy(CR.token_rows(strings, v)), env["tok"], env["chem"], v.eos))
    _same(out, want)
    again = ops.smiles_fragment_corpus(tokens, offsets, N, *env["tabs"])
    assert all(torch.equal(a, o) for a, o in zip(again, out))
    without = ops.smiles_fragment_corpus(tokens, offsets, N, *env["tabs"], mask=False)
    assert without[1] is None and torch.equal(without[3], out[3])
    if 3 < N < 4250:
        assert out[0][:3].tolist() == [CR.SYNTAX, 0, CR.TOO_LONG] and out[2][1].tolist() == [3, 2, 0, 117]


def test_rows_entry_edge_rows(env):
    """Two cuts at the two ends of a 117-atom chain in a 127-token row; a fragment that straddles atom 64, so that both mask words are in
    use; the 16- and 17-ring rows (the last status 0, the first FRAG_MANY with zero mask and keys and its true counts); a cage; 128
    content tokens (TOO_LONG, zeros); a strided view with x_ld > T: against the reference and the host entry."""
    v = env["v"]
    strings = ["C1CC1" + "C" * 117 + "C1CC1", "C1CC1" + "C" * 58 + "C1CCCCCCC1", RINGS16, RINGS17, "C12C3C4C1C5C2C3C45" + "C" * 100, "C" * 128,
               "c1ccccc1" + "C" * 62 + "c1ccccc1", "CC(=O)Oc1ccccc1C(=O)O"]
    x_h = torch.from_numpy(CR.token_rows(strings, v))
    out = _filled(len(strings))
    ops.smiles_fragment_rows(x_h.to(DEV), *env["tabs"], v.eos, *out)
    assert out[0].tolist() == [0, 0, 0, FG.FRAG_MANY, 0, CR.TOO_LONG, 0, 0]
    _same(out, FG.expected(strings))
    _same(out, ops.smiles_fragment_host(x_h, env["tok"], env["chem"], v.eos))
    assert out[2].tolist() == [[3, 2, 0, 117], [3, 2, 0, 58], [16, 15, 0, 3], [17, 16, 0, 3], [2, 1, 0, 100], [0] * 4, [3, 2, 0, 62], [4, 3, 1, 6]]
    assert (out[1][0, 1] != 0).all() and (out[1][1, 2] != 0).all()          # both mask words in use: a chain, a ring
    assert not out[1][3].any() and not out[3][3].any() and (out[3][2] != 0).all()
    wide = torch.full((len(strings), 200), v.eos, dtype=torch.long)
    wide[:, :x_h.shape[1]] = x_h
    view = wide.to(DEV)[:, :x_h.shape[1]]
    assert view.stride(0) == 200
    got = ops.smiles_fragment_rows(view, *env["tabs"], v.eos)
    assert all(torch.equal(g, o) for g, o in zip(got, out))


def _differing(got, want):
    return [(name, torch.nonzero((g.cpu() != w).reshape(w.shape[0], -1).any(1)).flatten()[:5].tolist())
            for g, w, name in zip(got, want, ("out", "out_len", "status", "info")) if not torch.equal(g.cpu(), w)]


@pytest.mark.parametrize("B", [1, 65, 4250])
@pytest.mark.parametrize("frag", [0, 1, 15])
def test_string_rows_entry_equals_the_host_entry(env, frag, B):
    """A strided input (x_ld = 134 > T = 131); outputs garbage-filled beforehand, so every element must be written; a second run is
    bit-identical; counts (32 slots) is the histogram of status, NO_FRAGMENT in slot 16."""
    v = env["v"]
    x = env["sx"].to(DEV)[:B, :131]
    assert B == 1 or x.stride(0) == 134
    counts = torch.zeros(32, dtype=torch.int32, device=DEV)
    pre = (torch.full((B, 131), FILL, dtype=torch.int64, device=DEV), torch.full((B,), FILL, dtype=torch.int32, device=DEV),
           torch.full((B,), FILL, dtype=torch.int32, device=DEV), torch.full((B, 4), FILL, dtype=torch.int32, device=DEV))
    out = ops.smiles_fragment_smiles_rows(x, *env["tabs"], env["emit_d"], v.bos, v.eos, v.pad, frag, 127, 131, *pre, counts=counts)
    want = tuple(t[:B] for t in env["shost"][frag])
    assert not _differing(out, want), _differing(out, want)
    assert torch.equal(counts.cpu(), torch.bincount(want[2], minlength=32).int())
    again = ops.smiles_fragment_smiles_rows(x, *env["tabs"], env["emit_d"], v.bos, v.eos, v.pad, frag, 127, 131)
    assert all(torch.equal(a, o) for a, o in zip(again, out))


@pytest.mark.parametrize("B", [1, 65, 4250])
@pytest.mark.parametrize("frag", [0, 1, 15])
def test_string_corpus_entry_equals_the_host_entry(env, frag, B):
    """One launch over selected CSR rows (in order, one id outside the corpus at B > 1): tokens_out, offsets_out (the gapped CSR),
    status and info equal what the host entry gives for the same strings; a row without the fragment is a slice of length 0."""
    v = env["v"]
    keep = [i for i, s in enumerate(env["srows"]) if len(s) <= 127]
    strings = [env["srows"][i] for i in keep]
    tokens, offsets = D.tokenize_corpus(strings, v)
    N, stride = len(strings), 127
    rows = np.arange(B, dtype=np.int64) % N
    if B > 1:
        rows[B - 1] = N
    want = [t[torch.as_tensor([keep[r] for r in rows if r < N])] for t in env["shost"][frag]]
    tokens_d = torch.from_numpy(np.concatenate([tokens, np.zeros(1, np.uint8)])).to(DEV)
    offsets_d, rows_d = torch.from_numpy(offsets).to(DEV), torch.from_numpy(rows).to(DEV)
    counts = torch.zeros(32, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    pre = (torch.full((B, stride), 0x7f, dtype=torch.uint8, device=DEV), torch.full((2 * B + 1,), FILL, dtype=torch.int64, device=DEV),
           torch.full((B,), FILL, dtype=torch.int32, device=DEV), torch.full((B, 4), FILL, dtype=torch.int32, device=DEV))
    tokens_out, offsets_out, status, info = ops.smiles_fragment_smiles_corpus(tokens_d, offsets_d, N, rows_d, *env["tabs"], env["emit_d"], frag, 127,
                                                                              stride, *pre, counts=counts, err=err)
    n_in = len(want[0])
    lens = np.concatenate([want[1].numpy() - 2, np.zeros(B - n_in, np.int64)])
    st = np.concatenate([want[2].numpy(), np.ones(B - n_in, np.int32)])
    assert int(err.item()) == (2 if n_in < B else 0) and status.cpu().tolist() == st.tolist()
    off = offsets_out.cpu().numpy()
    assert off[0::2].tolist() == [b * stride for b in range(B + 1)] and (off[1::2] - off[0:-1:2]).tolist() == lens.tolist()
    assert (lens[st != 0] == 0).all()
    content = np.zeros((B, stride), np.int64)
    for b in range(n_in):
        content[b, :lens[b]] = want[0][b, 1:1 + lens[b]].numpy()
    assert (tokens_out.cpu().numpy() == content).all()
    assert torch.equal(info.cpu()[:n_in], want[3]) and not info.cpu()[n_in:].any()
    assert torch.equal(counts.cpu(), torch.bincount(status.cpu(), minlength=32).int())
    again = ops.smiles_fragment_smiles_corpus(tokens_d, offsets_d, N, rows_d, *env["tabs"], env["emit_d"], frag, 127, stride)
    assert all(torch.equal(a, o) for a, o in zip(again, (tokens_out, offsets_out, status, info)))


# ---------------------------------------------------------------------------------------------------------------- the Python surface
@pytest.fixture(scope="module")
def setup(env):
    vocab = env["v"]
    pick = np.random.RandomState(9).choice(len(env["strings"]), size=300, replace=False)
    smiles = [env["strings"][i] for i in pick]
    torch.manual_seed(5)
    model = MV.VAE(vocab, dtype=torch.float32).to(DEV).eval()
    return smiles, D.MosesDeviceDataset(smiles, vocab, device=DEV), model, FG.expected(smiles)


def _check_dict(d, want, n):
    assert set(d) == {"status", "mask", "fragments", "cuts", "acyl_cuts", "largest", "keys"}
    assert all(t.is_cuda and t.shape[0] == n for t in d.values())
    assert d["status"].dtype == torch.int32 and d["status"].cpu().tolist() == want[0][:n].tolist()
    assert d["mask"].dtype == torch.int64 and d["mask"].shape == (n, 16, 2) and (d["mask"].cpu().numpy() == want[1][:n]).all()
    for i, name in enumerate(("fragments", "cuts", "acyl_cuts", "largest")):
        assert d[name].dtype == torch.int32 and d[name].cpu().tolist() == want[2][:n, i].tolist(), name
    assert d["keys"].dtype == torch.int64 and d["keys"].shape == (n, 16) and (d["keys"].cpu().numpy() == want[3][:n]).all()


def test_vae_and_dataset_methods(setup):
    smiles, ds, model, want = setup
    v = model.vocabulary
    _check_dict(model.fragments(smiles[:70]), want, 70)
    seqs = [model.string2tensor(s, device="cpu") for s in smiles[:70]]
    assert torch.equal(model.fragments(seqs)["keys"], model.fragments(smiles[:70])["keys"])
    for f in (0, 1):
        out, out_len, status = model.fragment_smiles(smiles[:70], f)
        assert out.is_cuda and out.dtype == torch.int64 and out_len.dtype == status.dtype == torch.int32 and out.shape[0] == 70
        refs = [FG.fragment_smiles(s, f) for s in smiles[:70]]
        assert status.cpu().tolist() == [r[0] for r in refs]
        got = [v.ids2string(r[:n], rem_bos=True, rem_eos=True) for r, n in zip(out.cpu().tolist(), out_len.cpu().tolist())]
        assert got == [r[1] for r in refs]
    assert D.fragment_smiles(smiles[:40], v, device=DEV) == [FG.all_fragment_smiles(s) for s in smiles[:40]]
    d = ds.fragments()
    assert ds.fragments() is d
    _check_dict(d, want, len(smiles))
    counter = collections.Counter(k for k in want[3].reshape(-1).tolist() if k)
    keys, counts = ds.fragment_histogram()
    assert ds.fragment_histogram()[0] is keys and keys.is_cuda and keys.dtype == counts.dtype == torch.int64 and keys.tolist() == sorted(counter)
    assert counts.tolist() == [counter[k] for k in sorted(counter)] and len(counter) >= 20 and max(counter.values()) >= 5
    # the corpus rows that hold a query's first fragment: benzene (biphenyl asks with its first ring), an acetyl, none for a bad row
    queries = ["c1ccccc1", "c1ccccc1c1ccccc1", "C(", "CC=O", smiles[0]]
    qk = FG.expected(queries)[3][:, 0]
    offsets, rows = ds.rows_with_fragment(queries)
    assert offsets.is_cuda and rows.is_cuda and offsets.dtype == rows.dtype == torch.int64 and offsets[0] == 0 and offsets.numel() == 6
    offsets, rows = offsets.tolist(), rows.tolist()
    for i, k in enumerate(qk.tolist()):
        assert rows[offsets[i]:offsets[i + 1]] == ([j for j in range(len(smiles)) if k in want[3][j].tolist()] if k else []), queries[i]
    assert offsets[1] - offsets[0] >= 5 and rows[offsets[0]:offsets[1]] == rows[offsets[1]:offsets[2]] and offsets[3] == offsets[2]
    assert 0 in rows[offsets[4]:offsets[5]] or want[0][0] != 0


def _generated(res):
    """The reference's fragment Counter of a result's strings, every drawn sample counting, and its FRAG_MANY rows."""
    gen, many = collections.Counter(), 0
    for s, c in zip(res["strings"], res["counts"]):
        st, _, _, keys = FG.fragments(s)
        many += st == FG.FRAG_MANY
        for k in keys:
            gen[k] += c
    return gen, many


def test_moses_generate_fragments(setup):
    """Three batches, the last one short.  "n_fragments" and "fragment_many" equal the reference computed from the returned strings,
    "frag" is within 8 x 2^-53 relative of the Counter cosine (three roundings on each side); without the flag the result has the keys
    it had, and the values the run with the flag reports for them; the ValueError comes before device work.  A second run with a benzene
    prefix, whose fragments the corpus has, gives the cosine a value strictly between 0 and 1."""
    smiles, ds, model, want = setup
    assert inspect.signature(mv.moses_generate).parameters["fragments"].default is False
    n, kw = 200, dict(batch_size=96, max_len=20, top_k=4, seed=2, syntax=True)
    z = torch.from_numpy(np.random.RandomState(4).standard_normal((n, model.d_z)).astype(np.float32)).to(DEV)
    plain = mv.moses_generate(model, n, z=z, novel_against=ds, **kw)
    assert set(plain) == KEYS | KEYS_NOVEL
    res = mv.moses_generate(model, n, z=z, novel_against=ds, fragments=True, **kw)
    assert set(res) == set(plain) | NEW | NEW_NOVEL
    assert {key: res[key] for key in plain} == plain
    only = mv.moses_generate(model, n, z=z, fragments=True, **kw)
    assert set(only) == KEYS | NEW and all(only[key] == res[key] for key in NEW)
    big = MV.VAE(VC.OneHotVocab([chr(65 + i) for i in range(61)]), dtype=torch.float32)
    with pytest.raises(ValueError, match="fragments=True supports at most 64 ids"):
        mv.moses_generate(big, 4, max_len=8, fragments=True)
    corpus = collections.Counter(k for k in want[3].reshape(-1).tolist() if k)
    for run in (res, mv.moses_generate(model, n, z=z, novel_against=ds, fragments=True, prefix="c1ccccc1", **kw)):
        # syntax=True: every sample ends in <eos>, so a string's status is its row's
        gen, many = _generated(run)
        cos = SR.cosine(gen, corpus)
        print("unique", run["unique"], "fragments", len(gen), "drawn", sum(gen.values()), "frag", run["frag"], "Counter", cos)
        assert isinstance(run["n_fragments"], int) and run["n_fragments"] == len(gen) and run["fragment_many"] == many and sum(run["counts"]) == n
        if math.isnan(cos):
            assert math.isnan(run["frag"]) and not gen
        else:
            assert isinstance(run["frag"], float) and abs(run["frag"] - cos) <= 8 * 2.0 ** -53 * cos
    assert len(gen) >= 2 and set(gen) & set(corpus) and 0 < cos < 1                   # the run with the prefix
