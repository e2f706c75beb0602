"""GPU tests of the kekulisation feature: mvae_smiles_kekule_rows / _corpus against the host entry (the same source compiled for the CPU),
bit for bit in status, desc and mate, over the mutation corpus and the ring-system corpus of tests/kekule_ref.py; VAE.kekule,
VAE.chem_valid(kekule=True), MosesDeviceDataset.kekule and moses_generate(kekule=True) against the reference on the strings."""
import inspect

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import molecular_vae_amd as mv                                        # noqa: E402
from molecular_vae_amd import data as D, mosesvae as MV, vocab as VC, ops   # noqa: E402
import chem_ref as CR                                                 # noqa: E402
import kekule_ref as KR                                               # noqa: E402

DEV = torch.device("cuda")
KEYS = {"total", "unique", "strings", "counts", "logq"}
KEYS_NOVEL = {"corpus_row", "is_novel", "novel"}
NEW = {"kekule_valid", "kekule_valid_unique", "kekule_status_counts", "kekule_status", "kekule_deficiency"}
NEW_NOVEL = {"kekule_valid_unique_novel"}


@pytest.fixture(scope="module")
def env():
    """Both corpora in one list (4 250 + 3 000 rows), the host entry's outputs for them, checked against the reference once."""
    v = CR.vocabulary()
    tok, chem = VC.smiles_token_table(v), VC.smiles_chem_table(v)
    mutation, m_status, m_desc = KR.mutation_expected()
    rings, r_status, r_desc, _ = KR.ring_system_expected()
    strings = list(mutation) + list(rings)
    x = torch.from_numpy(CR.token_rows(strings, v))
    host = tuple(t.numpy() for t in ops.smiles_kekule_host(x, tok, chem, v.eos))
    assert (host[0] == np.concatenate([m_status, r_status])).all() and (host[1] == np.concatenate([m_desc, r_desc])).all()
    return {"v": v, "tok": tok, "chem": chem, "tok_d": tok.to(DEV), "chem_d": chem.to(DEV), "strings": strings, "x": x, "host": host,
            "n_mutation": len(mutation)}


def _filled(n):
    return (torch.full((n,), 0x7f7f7f7f, dtype=torch.int32, device=DEV), torch.full((n, 4), 0x7f7f7f7f, dtype=torch.int32, device=DEV),
            torch.full((n, 128), 0x7f, dtype=torch.uint8, device=DEV))


def _same(got, want):
    for g, w, name in zip(got, want, ("status", "desc", "mate")):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        w = w.cpu().numpy() if torch.is_tensor(w) else w
        wrong = np.nonzero((g != w).reshape(g.shape[0], -1).any(1))[0]
        assert g.shape == w.shape and wrong.size == 0, (name, wrong[:5].tolist(), g[wrong[:3]].tolist(), w[wrong[:3]].tolist())


@pytest.mark.parametrize("B", [1, 63, 64, 65, 7250])
def test_rows_entry_equals_the_host_entry(env, B):
    """B around the block size of 64, and both whole corpora; the outputs are garbage-filled beforehand, so every element must be
    written; a second run is bit-identical; mate may be left out."""
    lo = 0 if B == 7250 else env["n_mutation"] - 30                  # a stretch across the seam of the two corpora
    x = env["x"][lo:lo + B].to(DEV)
    want = tuple(w[lo:lo + B] for w in env["host"])
    assert B < 60 or len(set(want[0].tolist())) >= 3
    out = _filled(B)
    ops.smiles_kekule_rows(x, env["tok_d"], env["chem_d"], env["v"].eos, *out)
    _same(out, want)
    other = (out[0] != 0) & (out[0] != 7)
    assert not out[1][other].any() and (out[2][other] == 255).all()
    again = ops.smiles_kekule_rows(x, env["tok_d"], env["chem_d"], env["v"].eos)
    assert all(torch.equal(a, o) for a, o in zip(again, out))
    status, desc, _ = _filled(B)
    got = ops.smiles_kekule_rows(x, env["tok_d"], env["chem_d"], env["v"].eos, status, desc, False)
    assert got[2] is None and torch.equal(status, out[0]) and torch.equal(desc, out[1])


@pytest.mark.parametrize("N", [1, 63, 64, 65, 7250])
def test_corpus_entry_equals_the_host_entry(env, N):
    """The CSR entry in one launch, with an empty row (SYNTAX at 0), the 127-token ring and a 128-token row in front (3 < N < 7250)."""
    v = env["v"]
    first = ["", "c1" + "c" * 124 + "1", "c" * 128]
    lo = env["n_mutation"] - 30
    strings = [first[1]] if N == 1 else first + env["strings"][lo:lo + N - 3] if N < 7250 else env["strings"]
    assert len(strings) == N
    tokens, offsets = D.tokenize_corpus(strings, v)
    tokens = torch.from_numpy(np.concatenate([tokens, np.zeros(1, np.uint8)])).to(DEV)
    offsets = torch.from_numpy(offsets).to(DEV)
    out = _filled(N)
    ops.smiles_kekule_corpus(tokens, offsets, N, env["tok_d"], env["chem_d"], *out)
    if N == 7250:
        want = env["host"]
    else:
        want = tuple(t.numpy() for t in ops.smiles_kekule_host(torch.from_numpy(CR.token_rows(strings, v)), env["tok"], env["chem"], v.eos))
    _same(out, want)
    again = ops.smiles_kekule_corpus(tokens, offsets, N, env["tok_d"], env["chem_d"])
    assert all(torch.equal(a, o) for a, o in zip(again, out))
    without = ops.smiles_kekule_corpus(tokens, offsets, N, env["tok_d"], env["chem_d"], mate=False)
    assert without[2] is None and torch.equal(without[0], out[0]) and torch.equal(without[1], out[1])
    if 3 < N < 7250:
        assert out[0][:3].tolist() == [CR.SYNTAX, 7, CR.TOO_LONG] and out[1][1].tolist() == [125, 125, 62, 1]
    if N == 1:
        assert out[0].tolist() == [7]


def test_rows_entry_edge_rows(env):
    """kekule_ref.edge_rows (the 125-atom odd ring, the 124-atom ring, 128 tokens, a closure between atoms 3 and 69, 25 three-rings
    chained and fused, ten digits open at once, two systems of more than 100 atoms that need a blossom), and a strided view with
    x_ld > T: against the stated figures, the reference and the host entry."""
    v = env["v"]
    rows = KR.edge_rows()
    strings = [r[0] for r in rows]
    x_h = torch.from_numpy(CR.token_rows(strings, v))
    out = _filled(len(strings))
    ops.smiles_kekule_rows(x_h.to(DEV), env["tok_d"], env["chem_d"], v.eos, *out)
    assert out[0].tolist() == [r[1] for r in rows] and out[1].tolist() == [r[2] for r in rows]
    ref = KR.expected(strings)
    assert (out[0].cpu().numpy() == ref[0]).all() and (out[1].cpu().numpy() == ref[1]).all()
    _same(out, ops.smiles_kekule_host(x_h, env["tok"], env["chem"], v.eos))
    mate = out[2].cpu().numpy()
    for i, s in enumerate(strings):
        if ref[0][i] in (0, 7):
            N, E = KR.graph(s)
            KR.check_mate(mate[i], N, E, int(ref[1][i, 2]))
    wide = torch.full((len(strings), 200), v.eos, dtype=torch.long)
    wide[:, :x_h.shape[1]] = x_h
    view = wide.to(DEV)[:, :x_h.shape[1]]
    assert view.stride(0) == 200
    got = ops.smiles_kekule_rows(view, env["tok_d"], env["chem_d"], v.eos)
    assert all(torch.equal(g, o) for g, o in zip(got, out))


# ---------------------------------------------------------------------------------------------------------------- the Python surface
@pytest.fixture(scope="module")
def setup(env):
    vocab = env["v"]
    rs = np.random.RandomState(9)
    pick = np.concatenate([rs.choice(env["n_mutation"], size=200, replace=False),
                           env["n_mutation"] + rs.choice(3000, size=100, replace=False)])
    smiles = [env["strings"][i] for i in pick] + [s for s, _ in CR.FORMULAS]
    torch.manual_seed(5)
    model = MV.VAE(vocab, dtype=torch.float32).to(DEV).eval()
    return smiles, D.MosesDeviceDataset(smiles, vocab, device=DEV), model, KR.expected(smiles)


def _check_dict(d, want, n, mate):
    assert set(d) == {"status", "n_atoms", "n_bonds", "pairs", "deficiency"} | ({"mate"} if mate is not None else set())
    assert d["status"].is_cuda and d["status"].cpu().tolist() == want[0][:n].tolist()
    for i, name in enumerate(("n_atoms", "n_bonds", "pairs", "deficiency")):
        assert d[name].dtype == torch.int32 and d[name].cpu().tolist() == want[1][:n, i].tolist(), name
    if mate:
        assert d["mate"].dtype == torch.uint8 and tuple(d["mate"].shape) == (n, 128)


def test_vae_and_dataset_methods(setup):
    """VAE.kekule and chem_valid(kekule=True) on strings, lists of id tensors and padded tensors; MosesDeviceDataset.kekule (one
    corpus launch) against VAE.kekule batch by batch."""
    smiles, ds, model, want = setup
    assert len(set(want[0].tolist())) >= 4 and (want[0] == 0).sum() >= 30 and (want[0] == 7).sum() >= 30
    d = model.kekule(smiles[:70])
    _check_dict(d, want, 70, True)
    seqs = [model.string2tensor(s, device="cpu") for s in smiles[:70]]
    from_seqs = model.kekule(seqs)
    padded = torch.from_numpy(CR.token_rows(smiles[:70], model.vocabulary)).to(DEV)
    from_rows = model.kekule(padded, mate=False)
    assert from_rows["mate"] is None
    for name in ("status", "n_atoms", "n_bonds", "pairs", "deficiency"):
        assert torch.equal(from_seqs[name], d[name]) and torch.equal(from_rows[name], d[name])
    assert torch.equal(from_seqs["mate"], d["mate"])
    for x in (smiles[:70], seqs, padded):
        ok = model.chem_valid(x, kekule=True)
        assert ok.dtype == torch.bool and ok.cpu().tolist() == (want[0][:70] == 0).tolist()
        ok2, status = model.chem_valid(x, return_status=True, kekule=True)
        assert torch.equal(ok2, ok) and status.cpu().tolist() == want[0][:70].tolist()
    plain, plain_status, _ = model.chem_valid(smiles[:70], return_status=True)              # the default is what it was
    assert plain.cpu().tolist() == [s in (0, 7) for s in want[0][:70].tolist()] and 7 not in plain_status.cpu().tolist()
    whole = ds.kekule()
    assert ds.kekule() is whole
    _check_dict(whole, want, len(smiles), None)
    for lo in range(0, len(smiles), 128):
        part = model.kekule(smiles[lo:lo + 128], mate=False)
        for name in ("status", "n_atoms", "n_bonds", "pairs", "deficiency"):
            assert torch.equal(part[name], whole[name][lo:lo + 128]), (name, lo)


def test_moses_generate_kekule(setup):
    """Three batches, the last one short, of a small randomly initialised model sampling under the syntax automaton after four prefixes (a
    benzene ring, a five-ring that does not kekulise as it stands, an open fused system, a carbon).  Every new key equals the reference computed from the returned strings; without the flag the result has the keys it had,
    and the values the run with the flag reports for them; it is independent of valence=."""
    smiles, ds, model, want = setup
    assert inspect.signature(mv.moses_generate).parameters["kekule"].default is False
    n, kw = 200, dict(batch_size=96, max_len=24, top_k=4, seed=2, syntax=True)
    z = torch.from_numpy(np.random.RandomState(4).standard_normal((n, model.d_z)).astype(np.float32)).to(DEV)
    prefix = ["c1ccccc1", "c1cccn1", "c1ccc2c", "C"] * (n // 4)
    plain = mv.moses_generate(model, n, z=z, novel_against=ds, prefix=prefix, **kw)
    assert set(plain) == KEYS | KEYS_NOVEL
    res = mv.moses_generate(model, n, z=z, novel_against=ds, prefix=prefix, kekule=True, **kw)
    assert set(res) == set(plain) | NEW | NEW_NOVEL
    assert {key: res[key] for key in plain} == plain
    assert set(mv.moses_generate(model, n, z=z, prefix=prefix, **kw)) == KEYS
    only = mv.moses_generate(model, n, z=z, prefix=prefix, kekule=True, **kw)
    assert set(only) == KEYS | NEW and all(only[key] == res[key] for key in NEW)
    both = mv.moses_generate(model, n, z=z, prefix=prefix, kekule=True, valence=True, **kw)
    assert all(both[key] == res[key] for key in NEW) and both["chem_valid"] == res["kekule_valid"] + res["kekule_status_counts"][7]
    # syntax=True: every sample ends in <eos>, so a string's status is its row's
    strings, counts = res["strings"], res["counts"]
    status, desc = KR.expected(strings)
    print("unique", len(strings), "kekulisable", int((status == 0).sum()), "status 7:", int((status == 7).sum()), "counts", res["kekule_status_counts"])
    assert res["kekule_status"] == status.tolist() and res["kekule_deficiency"] == desc[:, 3].tolist()
    assert (status == 0).sum() >= 1 and (status == 7).sum() >= 1
    assert res["kekule_valid_unique"] == int((status == 0).sum())
    assert res["kekule_valid"] == sum(c for c, s in zip(counts, status.tolist()) if s == 0)
    assert res["kekule_status_counts"] == {k: sum(c for c, s in zip(counts, status.tolist()) if s == k) for k in range(8)}
    assert sum(res["kekule_status_counts"].values()) == n == sum(counts)
    assert res["kekule_valid_unique_novel"] == sum(1 for s, nov in zip(status.tolist(), res["is_novel"]) if s == 0 and nov)
