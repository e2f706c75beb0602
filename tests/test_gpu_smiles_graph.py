"""GPU tests of the SMILES graph kernels (mvae_smiles_graph_rows, mvae_smiles_graph_corpus) against tests/chem_ref.py -- a reference in
plain Python on strings, written from the rules and not from the kernel's method -- and against the host entry, which is the same walk
compiled for the CPU.  Every output is an integer and compared for equality."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from molecular_vae_amd import vocab as VC, ops   # noqa: E402
import chem_ref as CR                            # noqa: E402

dev = torch.device("cuda")
FILL = 0x7f7f7f7f


@pytest.fixture(scope="module")
def env():
    v = CR.vocabulary()
    tok, chem = VC.smiles_token_table(v), VC.smiles_chem_table(v)
    strings, want = CR.corpus_and_expected()
    pick = np.random.RandomState(5).choice(len(strings), size=300, replace=False)
    for k in range(6):                                            # the slice keeps every status
        assert (want[0][pick] == k).sum() >= 2, k
    return {"v": v, "tok": tok, "chem": chem, "tok_d": tok.to(dev), "chem_d": chem.to(dev),
            "slice": ([strings[i] for i in pick], tuple(w[pick] for w in want))}


def _filled(n):
    return [torch.full(shape, FILL, dtype=torch.int32, device=dev) for shape in ((n,), (n,), (n, 8), (n, 11))]


def _rows(env, x, **kw):
    return tuple(t.cpu().numpy() for t in ops.smiles_graph_rows(x, env["tok_d"], env["chem_d"], env["v"].eos, **kw))


def _same(got, want, what=""):
    for name, g, w in zip(("status", "bad_pos", "desc", "formula"), got, want):
        assert g.shape == w.shape and (g == w).all(), (what, name, np.nonzero(g != w)[0][:5])


def test_tables_on_the_device(env):
    strings = [s for s, _ in CR.FORMULAS] + [s for s, _, _ in CR.REJECTED]
    x = torch.from_numpy(CR.token_rows(strings, env["v"])).to(dev)
    got = _rows(env, x)
    _same(got, CR.expected(strings))
    n = len(CR.FORMULAS)
    assert (got[0][:n] == 0).all() and got[0][n:].tolist() == [st for _, st, _ in CR.REJECTED]
    assert got[1][n:].tolist() == [p + 1 if p >= 0 else -1 for _, _, p in CR.REJECTED]


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_mutation_slice_equals_the_reference_and_the_host_entry(env, B):
    """B around the block size of 64 and more than two blocks; the buffers are 0x7f-filled beforehand, so every element must be written
    and a row that is not ok must come back zeroed; a second run is bit-identical; the host entry gives the same on the same rows."""
    strings, want = env["slice"]
    strings, want = strings[:B], tuple(w[:B] for w in want)
    x_h = torch.from_numpy(CR.token_rows(strings, env["v"]))
    x = x_h.to(dev)
    out = _filled(B)
    ops.smiles_graph_rows(x, env["tok_d"], env["chem_d"], env["v"].eos, *out)
    got = tuple(t.cpu().numpy() for t in out)
    _same(got, want, B)
    assert (got[2][got[0] != 0] == 0).all() and (got[3][got[0] != 0] == 0).all()
    _same(_rows(env, x), got, "second run")
    host = ops.smiles_graph_host(x_h, env["tok"], env["chem"], env["v"].eos)
    _same(got, tuple(t.numpy() for t in host), "host entry")


def test_edge_rows(env):
    """T = 2; T = 129 with a 127-atom chain; 128 content tokens; a ring between atom 3 and atom 69 (both mask words); a 15-deep nest; a
    strided view with x_ld > T; rows without <eos>; ids -1 and V."""
    v = env["v"]
    x = torch.tensor([[v.bos, v.eos]] * 3, device=dev)
    st, bad, desc, formula = _rows(env, x)
    assert st.tolist() == [CR.SYNTAX] * 3 and bad.tolist() == [1] * 3 and not desc.any() and not formula.any()
    chain = ["C" * 127, "C" * 126 + "c", "C" * 125 + "=O", "C" * 122 + "C1CC1"]
    x = torch.from_numpy(CR.token_rows(chain, v)).to(dev)
    assert x.shape[1] == 129
    got = _rows(env, x)
    _same(got, CR.expected(chain))
    assert got[0].tolist() == [0, CR.AROMATIC, 0, 0] and got[2][0].tolist() == [127, 126, 0, 0, 0, 256, 0, 0]
    ring = "CCC1" + "C" * 66 + "1"
    strings = ["C" * 128, ring, "C" + "(C" * 15 + ")" * 15, "c1ccccc1" * 15 + "C" * 6 + "c", "C" * 200, "C" * 130 + "("]
    x = torch.from_numpy(CR.token_rows(strings, v)).to(dev)
    got = _rows(env, x)
    _same(got, CR.expected(strings))
    assert got[0].tolist() == [CR.TOO_LONG, 0, 0, CR.AROMATIC, CR.TOO_LONG, CR.SYNTAX] and got[2][1].tolist() == [69, 69, 1, 67, 0, 138, 0, 0]
    assert got[1].tolist() == [129, -1, -1, 128, 201, 132]
    # a strided view, rows without <eos>, ids outside the vocabulary
    strings = ["CCO", "CC(=O)O", "C=F", "CCN", "c1ccccc1"]
    x_h = torch.from_numpy(CR.token_rows(strings, v, T=12))
    x_h[0, 4] = v.pad
    x_h[1, 3] = -1
    x_h[3, 2] = len(v)
    wide = torch.full((5, 40), v.eos, dtype=torch.long)
    wide[:, :12] = x_h
    wide = wide.to(dev)
    view = wide[:, :12]
    assert view.stride(0) == 40
    got = _rows(env, view)
    assert got[0].tolist() == [1, 1, 2, 1, 0] and got[1].tolist() == [4, 3, 3, 2, -1]
    assert got[3][4].tolist() == [6, 0, 6] + [0] * 8 and not got[2][:4].any()
    cut = _rows(env, wide[:, :4])                                  # T = 4: every row runs out without <eos>, or fails before
    assert cut[0].tolist() == [1] * 5 and cut[1].tolist() == [4, 3, 4, 2, 4]
    _same(_rows(env, view), tuple(t.numpy() for t in ops.smiles_graph_host(view.cpu(), env["tok"], env["chem"], v.eos)))


@pytest.mark.parametrize("N", [1, 130])
def test_csr_entry_equals_the_padded_entry(env, N):
    """The CSR entry on N rows that include an empty row and a 127-token row, against the padded entry on the same rows (bad_pos moves by
    the <bos> column) and against the reference."""
    from molecular_vae_amd import data as D
    v = env["v"]
    strings = (["C" * 127] if N == 1 else ["", "C" * 127, "C" * 128] + env["slice"][0][:N - 3])
    assert len(strings) == N
    tokens, offsets = D.tokenize_corpus(strings, v)
    tokens = torch.from_numpy(np.concatenate([tokens, np.zeros(1, np.uint8)])).to(dev)
    offsets = torch.from_numpy(offsets).to(dev)
    out = _filled(N)
    ops.smiles_graph_corpus(tokens, offsets, N, env["tok_d"], env["chem_d"], *out)
    got = tuple(t.cpu().numpy() for t in out)
    _same(got, CR.expected(strings, first_col=0))
    padded = _rows(env, torch.from_numpy(CR.token_rows(strings, v)).to(dev))
    _same((got[0], np.where(got[1] >= 0, got[1] + 1, -1), got[2], got[3]), padded)
    again = tuple(t.cpu().numpy() for t in ops.smiles_graph_corpus(tokens, offsets, N, env["tok_d"], env["chem_d"]))
    _same(again, got, "second run")
    if N > 1:
        assert got[0][:3].tolist() == [CR.SYNTAX, 0, CR.TOO_LONG] and got[1][:3].tolist() == [0, -1, 128]
