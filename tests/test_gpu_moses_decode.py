"""GPU tests of mosesvae.VAE.decode (greedy / beam search on the GRU step kernels + mvae_moses_beam_step), VAE.score (mvae_ce_rows_fwd)
and train.moses_reconstruction, against the float64 reference decoder of tests/beam_ref.py on the g3 parameters.

Comparisons with float64 are made where the decision is numerically meaningful: a token or a beam order is checked only where every
margin of the float64 search exceeds 1e-4 (the f32 path's log-probabilities are good to ~1e-6 per token, summed over <= 12 tokens)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import molecular_vae_amd as mv                  # noqa: E402
from molecular_vae_amd import _lib as L, mosesvae as MV, vocab as VC   # noqa: E402
from oracle import initparams as ip             # noqa: E402
import beam_ref as BR                           # noqa: E402

dev = torch.device("cuda")
MARGIN = 1e-4


def _moses_base(k):
    for a, b in (("vae.0.", "x_emb."), ("vae.1.0.", "x_emb."), ("encoder.0.", "x_emb."), ("encoder.1.", "encoder_rnn."),
                 ("encoder.2.", "q_mu."), ("encoder.3.", "q_logvar."), ("decoder.0.", "decoder_rnn."), ("decoder.1.", "decoder_lat."),
                 ("decoder.2.", "decoder_fc."), ("vae.1.1.", "encoder_rnn."), ("vae.1.2.", "q_mu."), ("vae.1.3.", "q_logvar."),
                 ("vae.2.0.", "decoder_rnn."), ("vae.2.1.", "decoder_lat."), ("vae.2.2.", "decoder_fc.")):
        if k.startswith(a):
            return b + k[len(a):]
    return k


def _g3_model(golden_dir, dtype):
    """The g3 model as test_gpu_parity's _moses_setup loads it (eval mode), and its parameters in float64."""
    g = np.load(os.path.join(golden_dir, "g3_moses.npz"))
    v = VC.OneHotVocab([chr(ord("a") + i) for i in range(26)])
    assert len(v) == int(g["V"]) and v.pad == int(g["pad"]) and v.bos == int(g["bos"])
    model = MV.VAE(v, dtype=dtype)
    params = ip.init_params(ip.moses_shapes(len(v)), 303, 1.5, np.float32)
    sd = {k: torch.from_numpy(params[k]) for k in params}
    model.load_state_dict({k: sd[_moses_base(k)] for k in model.state_dict()})
    return model.to(dev).eval(), {k: p.astype(np.float64) for k, p in params.items()}


def _latents(B, seed=0, scale=1.0):
    rs = np.random.RandomState(seed)
    return torch.from_numpy((rs.standard_normal((B, 160)) * scale).astype(np.float32)).to(dev)


def _check_invariants(model, ids, ends, scores, max_len):
    ids, ends, scores = ids.cpu(), ends.cpu(), scores.cpu()
    B, K, Lm = ids.shape
    assert Lm == max_len
    assert (ids[:, :, 0] == model.bos).all()
    assert ((ends >= 1) & (ends <= max_len)).all()
    pos = torch.arange(max_len)[None, None, :]
    assert (ids[pos.expand(B, K, -1) >= ends[:, :, None]] == model.pad).all()          # pad follows every end
    ended = ends < max_len                                                              # an end before max_len is an <eos>
    last = ids.gather(2, (ends - 1).clamp(min=0)[:, :, None])[:, :, 0]
    assert (last[ended] == model.eos).all()
    s = scores.double()
    s = torch.where(torch.isfinite(s), s, torch.full_like(s, -1e300))
    assert (s[:, 1:] <= s[:, :-1]).all()                                               # best first


def test_greedy_tokens_match_float64_argmax(golden_dir):
    """f32, beam_width = 1: every generated token is the float64 arg-max of its teacher-forced log p wherever the top-2 margin exceeds
    1e-4, and the reported score is the float64 log p of the decoded sequence."""
    model, p64 = _g3_model(golden_dir, torch.float32)
    z = _latents(9, seed=1)
    toks, scores = model.decode(z, beam_width=1, max_len=24, return_tokens=True)
    strings, best = model.decode(z, max_len=24)
    assert len(toks) == 9 and all(len(t) == 1 for t in toks) and scores.shape == (9, 1)
    assert torch.equal(best, scores[:, 0]) and strings == [model.tensor2string(t[0]) for t in toks]
    checked = 0
    for b in range(9):
        ids = toks[b][0].numpy()
        assert ids[0] == model.bos
        lp, arg, gap = BR.teacher_forced(p64, z[b].double().cpu().numpy(), ids)
        for i in range(len(ids) - 1):
            if gap[i] > MARGIN:
                assert arg[i] == ids[i + 1], (b, i)
                checked += 1
        assert abs(float(scores[b, 0]) - lp.sum()) < 1e-4, b
    assert checked >= 20


@pytest.mark.parametrize("K", [1, 3, 4])
@pytest.mark.parametrize("max_len", [1, 2, 12])
def test_beam_search_matches_float64_reference(golden_dir, K, max_len):
    """f32, B = 7 (not a multiple of 4): hypotheses, ends and scores equal the float64 beam search (same candidate, tie and finished-beam
    rules) on every molecule whose decision margins all exceed 1e-4; scores to 1e-4 absolute."""
    model, p64 = _g3_model(golden_dir, torch.float32)
    B = 7
    z = _latents(B, seed=2, scale=0.7)
    ids, ends, scores = model._beam_search(z, K, max_len)
    _check_invariants(model, ids, ends, scores, max_len)
    toks, sc = model.decode(z, beam_width=K, max_len=max_len, return_tokens=True)
    assert torch.equal(sc, scores)
    compared = 0
    for b in range(B):
        rid, rend, rsc, margin = BR.beam_search(p64, z[b].double().cpu().numpy(), K, max_len, model.bos, model.eos, model.pad)
        if margin <= MARGIN:
            continue
        compared += 1
        for k in range(K):
            if not np.isfinite(rsc[k]):
                assert not np.isfinite(float(scores[b, k])), (b, k)
                continue
            assert int(ends[b, k]) == rend[k], (b, k)
            assert np.array_equal(ids[b, k].cpu().numpy(), rid[k]), (b, k)
            assert torch.equal(toks[b][k], torch.from_numpy(rid[k][:rend[k]])), (b, k)
            assert abs(float(scores[b, k]) - rsc[k]) < 1e-4, (b, k, float(scores[b, k]), rsc[k])
    assert compared >= 4, compared


def test_bf16_scores_equal_float64_scores_of_the_chosen_sequences(golden_dir):
    """bf16: the decisions may differ from float64 (bf16 GRU state and weights), but the score reported for each hypothesis must be the
    float64 log p of the sequence the GPU chose.  Tolerance 2e-2 per counted token: bf16 keeps 8 significant bits (relative error 2^-9) on
    the weights and on the hidden state the head reads; with |logits| of a few units that moves each log-softmax by ~1e-2 at most, and the
    errors of successive tokens add up."""
    model, p64 = _g3_model(golden_dir, torch.bfloat16)
    z = _latents(7, seed=3, scale=0.7)
    toks, scores = model.decode(z, beam_width=4, max_len=12, return_tokens=True)
    worst = 0.0
    for b in range(7):
        for k in range(4):
            s = float(scores[b, k])
            assert np.isfinite(s)
            ids = toks[b][k].numpy()
            lp, _, _ = BR.teacher_forced(p64, z[b].double().cpu().numpy(), ids)
            err = abs(s - lp.sum()) / (len(ids) - 1)
            worst = max(worst, err)
    assert worst < 2e-2, worst


def test_decode_scores_agree_with_score_and_the_mean_reconstruction_loss(golden_dir):
    """f32: decode's score of each returned hypothesis equals VAE.score(that sequence, z) (1e-4), and -sum(score) / (counted tokens)
    equals forward_decoder's mean reconstruction loss (the existing mean-CE kernel) in eval mode."""
    model, _ = _g3_model(golden_dir, torch.float32)
    B, K = 6, 3
    z = _latents(B, seed=4, scale=0.7)
    toks, scores = model.decode(z, beam_width=K, max_len=14, return_tokens=True)
    # score() ignores pad targets as the loss does; a hypothesis that chose the pad token itself before its end is left out here
    keep = [(b, k) for b in range(B) for k in range(K) if not (toks[b][k][1:] == model.pad).any()]
    assert len(keep) >= B * K // 2
    seqs = [toks[b][k] for b, k in keep]
    zz = z[[b for b, _ in keep]]
    got = model.score(seqs, zz)
    assert got.dtype == torch.float32 and got.shape == (len(keep),) and got.is_cuda
    assert float((got.cpu() - torch.stack([scores[b, k] for b, k in keep]).cpu()).abs().max()) < 1e-4
    assert torch.equal(model.score(seqs, zz), got)                                    # bitwise deterministic
    order = sorted(range(len(seqs)), key=lambda i: -len(seqs[i]))
    with torch.no_grad():
        recon, _, _ = model.forward_decoder([seqs[i].to(dev) for i in order], zz[order])
    ntok = sum(len(s) - 1 for s in seqs)
    assert abs(-float(got.double().sum()) / ntok - float(recon)) < 1e-5 * abs(float(recon))
    # strings in any order, as forward takes them
    strs = ["hello", "abc", "zz", "molecule"]
    want = model.score([model.string2tensor(s, device="cpu") for s in strs], zz[:4])
    assert torch.equal(model.score(strs, zz[:4]), want)


def test_decode_invariants_and_determinism(golden_dir):
    model, _ = _g3_model(golden_dir, torch.bfloat16)
    z = _latents(37, seed=5)
    a = model._beam_search(z, 5, 20)
    b = model._beam_search(z, 5, 20)
    _check_invariants(model, *a, 20)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    s1, sc1 = model.decode(z, beam_width=5, max_len=20)
    s2, sc2 = model.decode(z, beam_width=5, max_len=20)
    assert s1 == s2 and torch.equal(sc1, sc2) and torch.equal(sc1, a[2][:, 0])


def test_decode_launches_four_kernels_per_token(golden_dir):
    """Per generated token ONE GRU wavefront pass (3 launches) + ONE beam launch, counted with a torch profiler as the sampler's test does."""
    model, _ = _g3_model(golden_dir, torch.bfloat16)
    z = _latents(64, seed=6)
    model.decode(z, beam_width=4, max_len=6)                                          # warm
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        model.decode(z, beam_width=4, max_len=26)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert sum(1 for n_ in names if "moses_beam_step" in n_) == 25
    steps = sum(1 for n_ in names if "gru_step" in n_ or "lstm_step" in n_ or "step_fwd" in n_)
    assert steps == 3 * 25, (steps, sorted(set(names)))
    assert sum(1 for n_ in names if "moses_beam_finalize" in n_) == 1


def _vocab_model(V, seed):
    import string
    chars = list(string.ascii_letters + string.digits)[:V - 4]
    v = VC.OneHotVocab(chars)
    assert len(v) == V
    torch.manual_seed(seed)
    model = MV.VAE(v, dtype=torch.float32).to(dev).eval()
    p64 = {n: p.detach().double().cpu().numpy() for n, p in model.named_parameters()}
    return model, p64


@pytest.mark.parametrize("V", [40, 64])
def test_f32_vocabularies_up_to_64(V):
    """The fp32 head of V = 40 / 64 tokens needs more than the default 64 KB of LDS (the launcher opts in): greedy decoding follows the
    float64 arg-max and the beam search keeps its invariants."""
    model, p64 = _vocab_model(V, seed=V)
    z = _latents(5, seed=V, scale=2.0)
    _check_invariants(model, *model._beam_search(z, 4, 10), 10)
    toks, scores = model.decode(z, beam_width=1, max_len=10, return_tokens=True)
    checked = 0
    for b in range(5):
        ids = toks[b][0].numpy()
        lp, arg, gap = BR.teacher_forced(p64, z[b].double().cpu().numpy(), ids)
        for i in range(len(ids) - 1):
            if gap[i] > MARGIN:
                assert arg[i] == ids[i + 1], (b, i)
                checked += 1
        assert abs(float(scores[b, 0]) - lp.sum()) < 1e-4
    assert checked >= 5


def test_vocabulary_above_64_is_refused():
    model, _ = _vocab_model(65, seed=1)
    with pytest.raises(L.MvaeError, match="mvae_moses_beam_step"):
        model.decode(_latents(2), beam_width=2, max_len=4)


def test_decode_at_scale():
    """B = 1024, K = 8, max_len = 100 (bf16, random weights) completes with every invariant holding."""
    v = VC.OneHotVocab([chr(ord("a") + i) for i in range(26)])
    torch.manual_seed(3)
    model = MV.VAE(v).to(dev).eval()
    z = _latents(1024, seed=7)
    ids, ends, scores = model._beam_search(z, 8, 100)
    torch.cuda.synchronize()
    assert ids.shape == (1024, 8, 100) and torch.isfinite(scores).all()
    _check_invariants(model, ids, ends, scores, 100)


def test_moses_reconstruction_equals_decode_and_score_by_hand(golden_dir):
    model, _ = _g3_model(golden_dir, torch.float32)
    rs = np.random.RandomState(8)
    collate = VC.get_collate_fn(model.vocabulary)
    batches = []
    for n in (5, 6):
        strs = ["".join(chr(ord("a") + int(c)) for c in rs.randint(0, 26, rs.randint(2, 9))) for _ in range(n)]
        batches.append(collate(strs))
    # one batch of what the model itself decodes from some latents: those can come back exactly
    dec, _ = model.decode(_latents(4, seed=9), max_len=20)
    dec = [s for s in dec if s and all("a" <= c <= "z" for c in s)]
    if dec:
        batches.append(collate(dec))
    frac, mean_lp = mv.moses_reconstruction(model, batches, beam_width=2, max_len=30)
    hits, lps, n = 0, [], 0
    for batch in batches:
        with torch.no_grad():
            mu, _, _ = model.forward_encoder(batch, eps=torch.zeros(len(batch), model.d_z, device=dev))
        strings, _ = model.decode(mu, beam_width=2, max_len=30)
        hits += sum(s == model.tensor2string(x) for s, x in zip(strings, batch))
        lps.append(model.score(batch, mu).double())
        n += len(batch)
    assert frac == hits / n
    assert abs(mean_lp - float(torch.cat(lps).sum()) / n) < 1e-9 * abs(mean_lp)
    assert mean_lp < 0
