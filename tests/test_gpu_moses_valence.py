"""GPU tests of the SMILES graph feature above the kernels: VAE.chem_valid / VAE.descriptors, MosesDeviceDataset.descriptors and
moses_generate(valence=True), against tests/chem_ref.py on the strings."""
import inspect

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import molecular_vae_amd as mv                                   # noqa: E402
from molecular_vae_amd import data as D, mosesvae as MV, ops    # noqa: E402
import chem_ref as CR                                            # noqa: E402

DEV = torch.device("cuda")
# the keys of moses_generate's result before valence= existed, by the arguments that ask for them
KEYS = {"total", "unique", "strings", "counts", "logq"}
KEYS_VALID = {"valid", "valid_unique"}
KEYS_NOVEL = {"corpus_row", "is_novel", "novel"}
KEYS_VALENCE = {"chem_valid", "chem_valid_unique", "status_counts", "status", "weight", "heavy_atoms", "rings"}


@pytest.fixture(scope="module")
def setup():
    vocab = CR.vocabulary()
    strings, want = CR.corpus_and_expected()
    pick = np.random.RandomState(9).choice(len(strings), size=150, replace=False)
    smiles = [strings[i] for i in pick] + [s for s, _ in CR.FORMULAS]
    torch.manual_seed(5)
    model = MV.VAE(vocab, dtype=torch.float32).to(DEV).eval()
    return smiles, vocab, D.MosesDeviceDataset(smiles, vocab, device=DEV), model


def _check(d, strings, first_col=1):
    st, bad, desc, formula = CR.expected(strings, first_col)
    assert d["status"].cpu().tolist() == st.tolist() and d["bad_pos"].cpu().tolist() == bad.tolist()
    for i, name in enumerate(ops.SMILES_DESC_NAMES):
        assert d[name].dtype == torch.int32 and d[name].cpu().tolist() == desc[:, i].tolist(), name
    assert (d["formula"].cpu().numpy() == formula).all()
    ref = formula.astype(np.float64) @ np.array(CR.WEIGHTS)
    assert d["weight"].dtype == torch.float32 and (np.abs(d["weight"].cpu().numpy() - ref) <= 2e-6 * ref).all()
    assert (ref[st != 0] == 0).all()


def test_chem_valid_and_descriptors_take_strings_lists_and_tensors(setup):
    smiles, vocab, ds, model = setup
    strings = sorted(smiles[:40], key=len, reverse=True)
    want = CR.expected(strings)[0]
    ok = model.chem_valid(strings)
    assert ok.dtype == torch.bool and ok.is_cuda and ok.cpu().tolist() == (want == 0).tolist()
    seqs = [model.string2tensor(s, device="cpu") for s in strings]
    ok2, status, bad = model.chem_valid(seqs, return_status=True)
    assert torch.equal(ok2, ok) and status.cpu().tolist() == want.tolist() and bad.cpu().tolist() == CR.expected(strings)[1].tolist()
    x = torch.nn.utils.rnn.pad_sequence(seqs, batch_first=True, padding_value=model.pad)
    assert torch.equal(model.chem_valid(x.to(DEV)), ok) and torch.equal(model.chem_valid(x), ok)
    assert (model.syntax_valid(strings) | ~ok).all()                               # valence-consistent implies well-formed
    for arg in (strings, seqs, x.to(DEV)):
        _check(model.descriptors(arg), strings)
    assert D.formula_strings(*(lambda d: (d["formula"], d["charge"]))(model.descriptors([s for s, _ in CR.FORMULAS]))) == \
        [f for _, f in CR.FORMULAS]
    with pytest.raises(ValueError, match="at least one row"):
        model.chem_valid([])


def test_dataset_descriptors_equal_per_batch_vae_descriptors(setup):
    smiles, vocab, ds, model = setup
    d = ds.descriptors()
    assert ds.descriptors() is d                                                   # cached
    _check(d, smiles, first_col=0)
    for lo in range(0, len(smiles), 64):
        part = model.descriptors(smiles[lo:lo + 64])
        for k in d:
            a, b = d[k][lo:lo + 64], part[k]
            if k == "bad_pos":
                b = torch.where(b >= 0, b - 1, b)
            if k == "weight":                                  # a float32 dot product of 11 terms: the order of its sum may depend on the batch
                assert (torch.abs(a - b) <= 2e-6 * b).all(), lo
            else:
                assert torch.equal(a, b), (k, lo)


def test_moses_generate_valence(setup):
    """Two batches, the second one short.  The lists align with "strings" and every entry equals the reference on its string;
    status_counts sums to total; chem_valid <= valid; the counts equal a recount over all samples; without valence= the result has the
    keys it had and the values the run with valence= reports for them.
    That last comparison stands in for "what the parent commit returns for the same seed": a test cannot run the parent's code, and a
    recorded result would pin the random initialisation of a torch version and not this project.  What is checked is that the key set
    without valence= is the parent's, written out above by hand, and that asking for valence changes no value under those keys -- the
    shared launches are the same ones; that the default path itself is untouched is a matter of the diff (every added line of
    moses_generate sits behind `if valence`).
    valence=True adds no host wait per batch: under torch's sync debug mode the synchronisation warnings it adds are the same number for
    two batches and for four (the copies of its counts and lists after the loop)."""
    smiles, vocab, ds, model = setup
    assert inspect.signature(mv.moses_generate).parameters["valence"].default is False
    n, kw = 104, dict(batch_size=96, max_len=14, top_k=4, seed=2, syntax=True)
    z = torch.from_numpy(np.random.RandomState(4).standard_normal((n, model.d_z)).astype(np.float32)).to(DEV)
    plain = mv.moses_generate(model, n, z=z, count_valid=True, novel_against=ds, **kw)
    assert set(plain) == KEYS | KEYS_VALID | KEYS_NOVEL | {"valid_unique_novel"}
    res = mv.moses_generate(model, n, z=z, count_valid=True, novel_against=ds, valence=True, **kw)
    assert set(res) == set(plain) | KEYS_VALENCE | {"chem_valid_unique_novel"}
    assert {k: res[k] for k in plain} == plain
    assert set(mv.moses_generate(model, n, z=z, **kw)) == KEYS
    assert set(mv.moses_generate(model, n, z=z, valence=True, **kw)) == KEYS | KEYS_VALENCE
    # host waits (the runs above have loaded every kernel and uploaded every table): what valence=True adds does not grow with the number
    # of batches -- it is the copies of its counts and lists after the loop
    def waits(batch_size, **extra):
        import warnings
        args = dict(kw, batch_size=batch_size)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                mv.moses_generate(model, n, z=z, count_valid=True, novel_against=ds, **extra, **args)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        return sum("synchroniz" in str(w.message).lower() for w in seen)
    two = (waits(96), waits(96, valence=True))                   # 2 batches
    four = (waits(26), waits(26, valence=True))                  # 4 batches
    print("synchronisation warnings without / with valence: 2 batches", two, "4 batches", four)
    assert four[0] - two[0] >= 2                                  # the mode sees the one wait per batch
    assert two[1] - two[0] == four[1] - four[0] <= 6             # the two count vectors and the four lists, once
    m = res["unique"]
    assert m == len(res["strings"]) > 10 and all(len(res[k]) == m for k in ("status", "weight", "heavy_atoms", "rings"))
    assert sorted(res["status_counts"]) == list(range(7)) and sum(res["status_counts"].values()) == res["total"] == n
    assert res["chem_valid"] <= res["valid"] and res["chem_valid_unique"] <= res["valid_unique"]
    assert res["chem_valid_unique_novel"] <= min(res["chem_valid_unique"], res["valid_unique_novel"])
    st, _, desc, formula = CR.expected(res["strings"])
    assert res["status"] == st.tolist() and res["heavy_atoms"] == desc[:, 0].tolist() and res["rings"] == desc[:, 2].tolist()
    ref = formula.astype(np.float64) @ np.array(CR.WEIGHTS)
    assert (np.abs(np.array(res["weight"]) - ref) <= 2e-6 * ref).all()
    print("status counts:", res["status_counts"], "chem_valid", res["chem_valid"], "of", n)
    # syntax=True: every sample ends in <eos>, so a string's status is its row's, and the totals can be recounted from the unique ones
    count = np.zeros(7, np.int64)
    np.add.at(count, st, np.array(res["counts"]))
    assert count.tolist() == [res["status_counts"][k] for k in range(7)] and res["chem_valid"] == count[0]
    assert res["chem_valid_unique"] == int((st == 0).sum()) and count[1] == 0
    assert res["chem_valid_unique_novel"] == sum(s == 0 and nov for s, nov in zip(st.tolist(), res["is_novel"]))
