"""GPU tests of the SMILES rewrite: mvae_smiles_rewrite_rows / _corpus against the host entry (the same source compiled for the CPU,
which tests/test_smiles_rewrite_host.py holds against the reference), bit for bit in tokens, lengths and statuses at the block edges;
the gapped CSR through the unchanged mvae_moses_collate; MosesDeviceDataset(augment=True), VAE.respell and data.randomized_smiles."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import molecular_vae_amd as mv                                        # noqa: E402
from molecular_vae_amd import data as D, mosesvae as MV, vocab as VC, ops   # noqa: E402
import chem_ref as CR                                                 # noqa: E402
import rewrite_ref as RR                                              # noqa: E402

DEV = torch.device("cuda")
SEED = 99
FILL = 0x7f7f7f7f


@pytest.fixture(scope="module")
def env():
    """260 rows: the hand rows (1 atom to 127 atoms, 127 tokens), refused rows of every kind, 100 molecules of MOSES' lengths and a
    slice of the mutation corpus; the
    host entry's outputs for them with T_out = 131, computed once and left unchanged."""
    v = CR.vocabulary()
    tok, chem, emit = VC.smiles_token_table(v), VC.smiles_chem_table(v), VC.smiles_emit_table(v)
    corpus = CR.mutation_corpus()
    strings = ["C"] + RR.HAND_ROWS + ["C[C@H](N)O", "F/C=C/F", "C" * 128, "C(", "C=F", "cc"]
    strings += RR.fragment_corpus(100, seed=1)
    strings += corpus[1000:1000 + 260 - len(strings)]
    draws = ops.draw_words(torch.arange(len(strings)) * 2654435761 + 17)
    x = torch.from_numpy(CR.token_rows(strings, v, 134))
    host = ops.smiles_rewrite_host(x, tok, chem, emit, v.bos, v.eos, v.pad, SEED, draws, 127, 131)
    assert len(set(host[2].tolist())) >= 6 and (host[2] == 0).sum() >= 60
    return {"v": v, "tabs": (tok.to(DEV), chem.to(DEV), emit.to(DEV)), "host_tabs": (tok, chem, emit), "strings": strings, "x": x,
            "draws": draws, "host": host}


def _rows(env, x, draws, max_content=127, T_out=131, counts=None, fill=True):
    v, B = env["v"], x.shape[0]
    pre = ((torch.full((B, T_out), FILL, dtype=torch.int64, device=DEV), torch.full((B,), FILL, dtype=torch.int32, device=DEV),
            torch.full((B,), FILL, dtype=torch.int32, device=DEV)) if fill else (None, None, None))
    return ops.smiles_rewrite_rows(x, *env["tabs"], v.bos, v.eos, v.pad, SEED, draws, max_content, T_out, *pre, counts=counts)


@pytest.mark.parametrize("B", [1, 63, 65, 130, 260])
def test_rows_entry_equals_the_host_entry(env, B):
    """B around the block size of 64; a strided input (x_ld = 134 > T = 131); outputs garbage-filled beforehand, so every element must be
    written; a second run is bit-identical; counts is the histogram of status."""
    x = env["x"].to(DEV)[:B, :131]
    assert x.stride(0) == 134
    draws = env["draws"][:B].to(DEV)
    counts = torch.zeros(16, dtype=torch.int32, device=DEV)
    out = _rows(env, x, draws, counts=counts)
    want = ops.smiles_rewrite_host(env["x"][:B, :131], *env["host_tabs"], env["v"].bos, env["v"].eos, env["v"].pad, SEED, env["draws"][:B], 127, 131)
    for g, w, name in zip(out, want, ("out", "out_len", "status")):
        assert torch.equal(g.cpu(), w), (name, torch.nonzero((g.cpu() != w).reshape(B, -1).any(1)).flatten()[:5].tolist())
    assert torch.equal(counts.cpu(), torch.bincount(want[2], minlength=16).int())
    again = _rows(env, x, draws, fill=False)
    assert all(torch.equal(a, o) for a, o in zip(again, out))


def test_rows_entry_cuts_at_t_out_and_honours_max_content(env):
    """T_out smaller than needed: the rows are the first columns of the uncut ones and out_len stays; a small max_content turns long
    spellings into LONG; draw NULL is the row number."""
    v = env["v"]
    x = env["x"].to(DEV)
    draws = env["draws"].to(DEV)
    full = _rows(env, x, draws)
    cut = _rows(env, x, draws, T_out=9)
    assert torch.equal(cut[0], full[0][:, :9]) and torch.equal(cut[1], full[1]) and torch.equal(cut[2], full[2])
    assert (full[1] > 9).sum() > 50
    for mc in (1, 20):
        got = _rows(env, x, draws, max_content=mc)
        want = ops.smiles_rewrite_host(env["x"], *env["host_tabs"], v.bos, v.eos, v.pad, SEED, env["draws"], mc, 131)
        assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want)) and (want[2] == RR.LONG).sum() >= 10
    got = _rows(env, x, None)
    want = ops.smiles_rewrite_host(env["x"], *env["host_tabs"], v.bos, v.eos, v.pad, SEED, None, 127, 131)
    assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want))


def _corpus_case(env, B):
    """A CSR corpus of the fixture's rows with an empty row in front, and B row ids with a repeat and two ids outside [0, N)."""
    v = env["v"]
    strings = [""] + [s for s in env["strings"] if len(s) <= 127]
    tokens, offsets = D.tokenize_corpus(strings, v)
    rs = np.random.RandomState(B)
    rows = rs.randint(0, len(strings), size=B)
    rows[0] = 0 if B > 1 else 2
    if B >= 4:
        rows[1], rows[2], rows[3] = rows[B - 1], -1, len(strings)
    return strings, tokens, offsets, rows


@pytest.mark.parametrize("B", [1, 63, 65, 130])
def test_corpus_entry_equals_the_host_entry_and_collates_unchanged(env, B):
    """One launch over selected CSR rows: tokens_out, offsets_out and status equal what the host entry gives for the same strings and
    draws; an id outside the corpus is an empty row with status 1 and err 2; counts is the histogram.  Then the gapped CSR goes through
    mvae_moses_collate as it is: lengths descending, rows_sorted // 2 the batch member, the tokens the kernel's."""
    v = env["v"]
    strings, tokens, offsets, rows = _corpus_case(env, B)
    N, stride = len(strings), 127
    inside = (rows >= 0) & (rows < N)
    picked = [strings[r] if ok else "" for r, ok in zip(rows, inside)]
    draws = ops.draw_words(torch.from_numpy(rows * 7 + 3))
    want = ops.smiles_rewrite_host(torch.from_numpy(CR.token_rows(picked, v, 129)), *env["host_tabs"], v.bos, v.eos, v.pad, SEED, draws, 127, 129)
    tokens_d = torch.from_numpy(np.concatenate([tokens, np.zeros(1, np.uint8)])).to(DEV)
    offsets_d, rows_d = torch.from_numpy(offsets).to(DEV), torch.from_numpy(rows).to(DEV)
    counts = torch.zeros(16, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    pre = (torch.full((B, stride), 0x7f, dtype=torch.uint8, device=DEV), torch.full((2 * B + 1,), FILL, dtype=torch.int64, device=DEV),
           torch.full((B,), FILL, dtype=torch.int32, device=DEV))
    tokens_out, offsets_out, status = ops.smiles_rewrite_corpus(tokens_d, offsets_d, N, rows_d, *env["tabs"], SEED, draws.to(DEV), 127, stride,
                                                                *pre, counts=counts, err=err)
    lens = want[1].numpy() - 2
    assert int(err.item()) == (2 if not inside.all() else 0)
    assert status.cpu().tolist() == [int(s) if ok else 1 for s, ok in zip(want[2], inside)]
    off = offsets_out.cpu().numpy()
    assert off[0::2].tolist() == [b * stride for b in range(B + 1)] and (off[1::2] - off[0:-1:2]).tolist() == lens.tolist()
    content = np.zeros((B, stride), np.int64)
    for b in range(B):
        content[b, :lens[b]] = want[0][b, 1:1 + lens[b]].numpy()
    assert (tokens_out.cpu().numpy() == content).all()
    assert torch.equal(counts.cpu(), torch.bincount(status.cpu(), minlength=16).int())
    again = ops.smiles_rewrite_corpus(tokens_d, offsets_d, N, rows_d, *env["tabs"], SEED, draws.to(DEV), 127, stride)
    assert all(torch.equal(a, o) for a, o in zip(again, (tokens_out, offsets_out, status)))
    # the gapped CSR through the unchanged collate
    T = int(lens.max()) + 2
    x_pad = torch.full((B, T), FILL, dtype=torch.long, device=DEV)
    lengths = torch.empty(B, dtype=torch.int32, device=DEV)
    member = torch.empty(B, dtype=torch.long, device=DEV)
    err.zero_()
    ops.moses_collate(tokens_out.view(-1), offsets_out, torch.arange(0, 2 * B, 2, device=DEV), x_pad, lengths, T, 2 * B, v.bos, v.eos, v.pad, member, err)
    lengths, member, x_pad = lengths.cpu().numpy(), member.cpu().numpy(), x_pad.cpu().numpy()
    assert int(err.item()) == 0 and (np.diff(lengths) <= 0).all() and (member % 2 == 0).all()
    assert sorted((member // 2).tolist()) == list(range(B)) and (lengths == lens[member // 2] + 2).all()
    assert (x_pad == want[0].numpy()[member // 2, :T]).all()


def test_corpus_entry_cuts_a_copied_row_longer_than_stride(env):
    v = env["v"]
    strings = ["C(", "C" * 40 + "(", "CC"]                       # refused rows are copied: the second is longer than the stride
    tokens, offsets = D.tokenize_corpus(strings, v)
    tokens_d = torch.from_numpy(np.concatenate([tokens, np.zeros(1, np.uint8)])).to(DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = ops.smiles_rewrite_corpus(tokens_d, torch.from_numpy(offsets).to(DEV), 3, torch.arange(3, device=DEV), *env["tabs"], SEED, None, 8, 8, err=err)
    assert int(err.item()) == 1 and out[2].tolist() == [1, 1, 0] and out[1].tolist() == [0, 2, 8, 16, 16, 18, 24]
    assert out[0][1].tolist() == tokens[2:10].tolist()


@pytest.fixture(scope="module")
def small():
    smiles = RR.fragment_corpus(200, seed=5)                     # 200 molecules of MOSES' lengths that the walk accepts
    vocab = CR.vocabulary()
    return smiles, vocab, D.MosesDeviceDataset(smiles, vocab, device=DEV)


def test_dataset_without_augment_is_what_it_was(small):
    smiles, vocab, ds = small
    for batch in ds.batches(32, epoch=1, seed=3):
        ref = ds.gather(batch.rows, T=batch.x_pad.shape[1])
        assert torch.equal(ref.x_pad, batch.x_pad) and torch.equal(ref.lengths, batch.lengths) and torch.equal(ref.rows, batch.rows)
    assert ds.augment_counts is None


def test_dataset_augmented_batches_are_the_same_molecules(small):
    """Every augmented batch row's molecule key equals its corpus row's; the spelling of a corpus row depends on (seed, epoch, row)
    alone: the same at batch sizes 32 and 64, different in another epoch for at least one row; most rows are respelled."""
    smiles, vocab, ds = small
    keys = ds.scaffolds()["mol_key"]
    status = ds.scaffolds()["status"]
    assert int((status == 0).sum()) == 200
    model = MV.VAE(vocab, dtype=torch.float32).to(DEV)
    spelled = {}
    for name, bs, epoch in (("a", 32, 2), ("b", 64, 2), ("c", 32, 3)):
        rows_seen = {}
        for batch in ds.batches(bs, epoch=epoch, seed=3, augment=True, augment_seed=11, augment_slack=2):
            got = model.scaffolds(batch.x_pad)
            assert torch.equal(got["mol_key"], keys[batch.rows]) and torch.equal(got["status"], status[batch.rows])
            assert (batch.lengths[:-1] >= batch.lengths[1:]).all()
            x, n, r = batch.x_pad.cpu().numpy(), batch.lengths.cpu().numpy(), batch.rows.cpu().numpy()
            for i in range(len(r)):
                rows_seen[int(r[i])] = tuple(x[i, :n[i]].tolist())
        spelled[name] = rows_seen
    common = set(spelled["a"]) & set(spelled["b"])
    assert len(common) >= 128 and all(spelled["a"][r] == spelled["b"][r] for r in common)
    assert any(spelled["a"][r] != spelled["c"][r] for r in set(spelled["a"]) & set(spelled["c"]))
    plain = {r: tuple(vocab.string2ids(smiles[r], add_bos=True, add_eos=True)) for r in spelled["a"]}
    assert sum(spelled["a"][r] != plain[r] for r in plain) >= len(plain) // 2
    ds.check_errors()
    counts = ds.augment_counts.cpu()
    assert int(counts.sum()) == sum(len(s) for s in spelled.values()) and int(counts[0]) >= int(counts.sum()) // 2
    # gather(augment=True) with the epoch's draw gives the same spelling
    some = sorted(common)[:16]
    g = ds.gather(some, augment=True, augment_seed=11, augment_epoch=2, augment_slack=6)
    x, n, r = g.x_pad.cpu().numpy(), g.lengths.cpu().numpy(), g.rows.cpu().numpy()
    for i in range(16):                                             # equal, unless one side fell back to the original for length
        got, before = tuple(x[i, :n[i]].tolist()), spelled["a"][int(r[i])]
        assert got == before or plain[int(r[i])] in (got, before), (i, got, before)
    assert sum(tuple(x[i, :n[i]].tolist()) == spelled["a"][int(r[i])] for i in range(16)) >= 8


def test_one_training_step_on_an_augmented_batch_and_respell(small):
    smiles, vocab, ds = small
    torch.manual_seed(0)
    model = MV.VAE(vocab, dtype=torch.float32).to(DEV)
    opt = mv.FusedAdam(model.parameters(), lr=3e-4, max_grad_norm=50.0)
    post = mv.moses_train_epoch(model, 0, list(ds.batches(64, augment=True))[:1], 0.1, opt)
    assert all(np.isfinite(post[k]) for k in ("loss", "kl_loss", "recon_loss")), post
    some = smiles[:40] + ["C[C@H](N)O", "C("]
    draw = torch.arange(len(some)) * 5 + 1
    rows, status = model.respell(some, seed=7, draw=draw)
    x = model._rows(some, "test", DEV)
    tok, chem, emit = (t.to(DEV) for t in (VC.smiles_token_table(vocab), VC.smiles_chem_table(vocab), VC.smiles_emit_table(vocab)))
    want = ops.smiles_rewrite_rows(x, tok, chem, emit, vocab.bos, vocab.eos, vocab.pad, 7, ops.draw_words(draw).to(DEV))
    assert torch.equal(rows, want[0]) and torch.equal(status, want[2]) and status[-2:].tolist() == [RR.STEREO, 1]
    assert model.syntax_valid(rows)[:-1].all() and torch.equal(model.scaffolds(rows)["mol_key"], model.scaffolds(x)["mol_key"])
    spell, st = D.randomized_smiles(smiles[:5], vocab, 6, seed=1, return_status=True)
    host = D.randomized_smiles(smiles[:5], vocab, 6, seed=1, device="cpu")
    assert spell == host and len(spell) == 5 and all(len(s) == 6 for s in spell) and not st.any()
    assert sum(len(set(s)) > 1 for s in spell) >= 4
