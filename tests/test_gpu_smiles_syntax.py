"""GPU tests of syntax-constrained sampling (mvae_moses_sample_syntax_step, VAE.sample(syntax=True)) and of the SMILES syntax check
(mvae_smiles_syntax_check, VAE.syntax_valid, moses_generate(count_valid=True)) against tests/syntax_ref.py: the automaton of the
specification in plain Python (allowed sets, next states, first refusals) and an independently written validator (well-formedness of whole
strings), plus the float64 decoder of tests/sample_ref.py for the numbers.  The mask is integer logic: those assertions have no tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import molecular_vae_amd as mv                  # noqa: E402
from molecular_vae_amd import mosesvae as MV, vocab as VC, ops   # noqa: E402
from oracle import initparams as ip             # noqa: E402
import sample_ref as SR                         # noqa: E402
import syntax_ref as SY                         # noqa: E402

dev = torch.device("cuda")
ALPHABET = "CNOSFcnos()=#123[]@H+-lBr"          # data.synthetic_smiles' alphabet: V = 29 with the four specials
GOOD = ["CCO", "c1ccccc1", "CC(=O)Oc1ccccc1C(=O)O", "CN1CCC[C@H]1c2cccnc2", "O=C(O)c1ccccc1", "C1CC1", "N#Cc1ccc(Br)cc1",
        "CC(C)Cc1ccc(cc1)[C@@H](C)C(=O)O", "C[N+](C)(C)C", "[O-]C", "ClC(Cl)Cl"]
BAD = ["C(", "C)", "C1CC", "C11", "C()", "C(=)", "=C", "C=", "C[", "[]C", "C(C)1CC1", "Cr", "Bl", "CH", ""]


def _vocab():
    return VC.OneHotVocab(set(ALPHABET))


def _moses_base(k):
    for a, b in (("vae.0.", "x_emb."), ("vae.1.0.", "x_emb."), ("encoder.0.", "x_emb."), ("encoder.1.", "encoder_rnn."),
                 ("encoder.2.", "q_mu."), ("encoder.3.", "q_logvar."), ("decoder.0.", "decoder_rnn."), ("decoder.1.", "decoder_lat."),
                 ("decoder.2.", "decoder_fc."), ("vae.1.1.", "encoder_rnn."), ("vae.1.2.", "q_mu."), ("vae.1.3.", "q_logvar."),
                 ("vae.2.0.", "decoder_rnn."), ("vae.2.1.", "decoder_lat."), ("vae.2.2.", "decoder_fc.")):
        if k.startswith(a):
            return b + k[len(a):]
    return k


_PARAMS = {}


def _model(dtype, seed=303):
    """A mosesvae.VAE over the synthetic_smiles vocabulary with seeded random weights (eval mode), and the weights in float64."""
    v = _vocab()
    if seed not in _PARAMS:
        _PARAMS[seed] = ip.init_params(ip.moses_shapes(len(v)), seed, 1.5, np.float32)
    params = _PARAMS[seed]
    model = MV.VAE(v, dtype=dtype)
    sd = {k: torch.from_numpy(params[k]) for k in params}
    model.load_state_dict({k: sd[_moses_base(k)] for k in model.state_dict()})
    return model.to(dev).eval(), {k: p.astype(np.float64) for k, p in params.items()}


def _latents(B, seed=0):
    rs = np.random.RandomState(seed)
    return torch.from_numpy(rs.standard_normal((B, 160)).astype(np.float32)).to(dev)


# ---------------------------------------------------------------------------------------------- 1. the step on a fixed logit row
def _step_case(B, logits, seed=0):
    V, H, W = len(logits), 64, 128
    rs = np.random.RandomState(seed)
    h = torch.zeros(B, H, device=dev); h[:, 0] = 1.0
    wfc = torch.zeros(V, H, device=dev); wfc[:, 0] = torch.from_numpy(logits.astype(np.float32)).to(dev)
    table = torch.from_numpy(rs.standard_normal((V, W)).astype(np.float32)).to(dev)
    base = torch.from_numpy(rs.standard_normal((B, W)).astype(np.float32)).to(dev)
    return V, H, W, h, wfc, table, base


def _prefix_state(chars, n, left, rs):
    """A state n random legal tokens away from START from which the string can still be finished in left + 1 tokens."""
    st = SY.S0
    for i in range(1, n + 1):
        al = [t for t in SY.allowed_ids(st, chars, (n - i) + left + 1) if chars[t] != "$"]
        assert al, (st, n, left)
        st = SY.step(st, chars[al[rs.randint(len(al))]])
    assert SY.need(st) <= left + 1
    return st


# (max_len, step) of the launches: 50, 6, 3, 1 and 0 tokens left after the one being drawn, each at a step (so a column of x and a set of
# uniforms) of its own
LAUNCHES = ((64, 13), (18, 11), (13, 9), (9, 7), (15, 14))


@pytest.mark.parametrize("top_k,top_p", [(None, None), (5, 0.9)])
def test_syntax_step_on_a_fixed_logit_row(top_k, top_p):
    """B = 1027 rows, each with its own automaton state (a random legal prefix of 0-12 tokens: bracket modes, depth > 0, open rings and
    cur bits all occur, asserted) and, through five launches with different (max_len, step), its own number of tokens left; a launch sees
    the rows of the other launches as finished.  (1) no row draws a token outside its reference allowed set and (2) gstate after the
    launch is step(state, token) -- integer logic, every row; (3) finished rows keep gstate, logq, hash and x; (4) the draw is the host
    inverse CDF of the row's masked (and filtered) distribution at ops.sample_uniform for >= 99.9 % of the rows compared (the fixed-row
    bound of test_gpu_moses_sampling.py); with a filter a row is compared where its float64 filter margins exceed 1e-4 / 1e-5 (those of
    that file's loop test), at least 90 % of the rows; (5) logq within 1e-5; (6) add_out == table[w] + base for every row."""
    v = _vocab()
    chars, info = SY.token_chars(v), VC.smiles_token_table(v)
    B = 1027
    rs = np.random.RandomState(5)
    logits = rs.standard_normal(len(v)) * 2.0
    V, H, W, h, wfc, table, base = _step_case(B, logits)
    temp, seed = 0.7, 4321
    group = np.arange(B) % len(LAUNCHES)
    states = []
    for b in range(B):
        left = LAUNCHES[group[b]][0] - 1 - LAUNCHES[group[b]][1]
        n = int(rs.randint(0, 13))
        states.append(_prefix_state(chars, max(n, 1) if left == 0 else n, left, rs))
    modes = {s[0] for s in states}
    assert modes >= {SY.START, SY.ATOM, SY.RING, SY.BOND, SY.OPEN, SY.CLOSE, SY.KOPEN, SY.KSYM, SY.KH, SY.KCHG}, modes
    assert any(s[1] > 1 for s in states) and any(bin(s[2]).count("1") > 1 for s in states) and any(s[3] for s in states)
    gs0 = torch.from_numpy(SY.np_states(states, v)).to(dev)
    tok_info = info.to(dev)
    p_full = np.exp((logits - logits.max()) / temp)
    logq0 = rs.standard_normal(B).astype(np.float32)
    hash0 = rs.randint(-2 ** 62, 2 ** 62, B, dtype=np.int64)
    n_cmp = n_agree = n_live = 0
    worst = 0.0
    for g, (max_len, step) in enumerate(LAUNCHES):
        live = group == g
        gstate = gs0.clone()
        add = torch.empty(B, W, device=dev)
        x = torch.full((B, 16), 99, dtype=torch.long, device=dev)
        end_pads = torch.full((B,), 16, dtype=torch.long, device=dev)
        eos_mask = torch.from_numpy((~live).astype(np.uint8)).to(dev)
        w = torch.empty(B, dtype=torch.long, device=dev)
        logq, hsh = torch.from_numpy(logq0).to(dev), torch.from_numpy(hash0).to(dev)
        ops.moses_sample_syntax_step(h, H, wfc, None, temp, top_k or 0, top_p or 1.0, seed, step, v.eos, table, base, add, x, end_pads, eos_mask,
                                     w, B, V, H, tok_info, gstate, max_len, logq=logq, hash=hsh)
        torch.cuda.synchronize()
        wn, gn, lq, hs, xs = w.cpu().numpy(), gstate.cpu().numpy(), logq.cpu().numpy(), hsh.cpu().numpy(), x.cpu().numpy()
        assert ((wn >= 0) & (wn < V)).all()
        assert torch.equal(add, table[w] + base)                                                     # (6)
        assert (gn[~live] == gs0.cpu().numpy()[~live]).all() and (lq[~live] == logq0[~live]).all()   # (3)
        assert (hs[~live] == hash0[~live]).all() and (xs[~live] == 99).all() and (np.delete(xs, step, 1) == 99).all()
        u = ops.sample_uniform(seed, step, B)
        left = max_len - 1 - step
        for b in np.nonzero(live)[0]:
            al = SY.allowed_ids(states[b], chars, left)
            assert al and wn[b] in al, (b, states[b], left, wn[b], al)                               # (1)
            nxt = SY.step(states[b], chars[wn[b]])
            assert tuple(gn[b]) == SY.pack_state(nxt, v), (b, states[b], wn[b], gn[b])               # (2)
            assert xs[b, step] == wn[b]
            n_live += 1
            p = np.zeros(V); p[al] = p_full[al]
            with np.errstate(invalid="ignore"):
                a_m, b_m = SR.filter_margins(p, top_k, top_p)
            if a_m[0] <= 1e-4 or b_m[0] <= 1e-5:
                continue
            keep = SR.filter_keep(p, top_k, top_p) & (p > 0)
            q = p * keep; qn = q / q.sum()
            n_cmp += 1
            assert keep[wn[b]], (b, wn[b])
            n_agree += int(SR.draw(p, keep, u[b:b + 1])[0] == wn[b])                                 # (4)
            worst = max(worst, abs(float(lq[b]) - (float(logq0[b]) + np.log(qn[wn[b]]))))            # (5)
        ends, em = end_pads.cpu().numpy(), eos_mask.cpu().numpy()
        new_eos = live & (wn == v.eos)
        assert (ends[new_eos] == step + 1).all() and (ends[~new_eos] == 16).all() and (em.astype(bool) == (~live | new_eos)).all()
        if left == 0:
            assert new_eos[live].all()                                                               # the last step: <eos> and nothing else
    print(f"top_k={top_k} top_p={top_p}: live rows {n_live}, compared {n_cmp}, equal to the host inverse CDF {n_agree / n_cmp:.5f}, "
          f"max logq error {worst:.2e}")
    assert n_live == B and n_cmp >= 0.9 * B
    assert n_agree / n_cmp >= 0.999, n_cmp - n_agree
    assert worst < 1e-5, worst


# ---------------------------------------------------------------------------------------------- 2. a dominant illegal token
def test_dominant_illegal_logits_do_not_underflow_the_legal_tokens():
    """START state, logits +100 on ')' and <pad>, 0 on the other illegal tokens and -100 .. -98 on the legal ones (the atoms and '['):
    with the stabilising max over ALL classes every legal e would underflow to 0.  Every draw is legal, the frequencies over the legal
    tokens are within 4 sigma of their renormalised softmax, and logq is finite (and equals log of that softmax within 1e-5)."""
    v = _vocab()
    chars, info = SY.token_chars(v), VC.smiles_token_table(v)
    B, max_len, step = 4099, 40, 1
    legal = SY.allowed_ids(SY.S0, chars, max_len - 1 - step)
    assert sorted(chars[t] for t in legal) == sorted("CNOSFcnosB[")
    logits = np.zeros(len(v))
    logits[[v.c2i[")"], v.pad]] = 100.0
    logits[legal] = np.linspace(-100.0, -98.0, len(legal))
    V, H, W, h, wfc, table, base = _step_case(B, logits)
    gstate = torch.from_numpy(SY.np_states([SY.S0] * B, v)).to(dev)
    add = torch.empty(B, W, device=dev)
    x = torch.full((B, 8), 99, dtype=torch.long, device=dev)
    end_pads = torch.full((B,), 8, dtype=torch.long, device=dev)
    eos_mask = torch.zeros(B, dtype=torch.uint8, device=dev)
    w = torch.empty(B, dtype=torch.long, device=dev)
    logq = torch.zeros(B, device=dev)
    ops.moses_sample_syntax_step(h, H, wfc, None, 1.0, 0, 1.0, 9, step, v.eos, table, base, add, x, end_pads, eos_mask, w, B, V, H,
                                 info.to(dev), gstate, max_len, logq=logq)
    torch.cuda.synchronize()
    wn, lq = w.cpu().numpy(), logq.cpu().numpy().astype(np.float64)
    assert np.isin(wn, legal).all(), np.unique(wn)
    q = np.zeros(V); q[legal] = np.exp(logits[legal] - logits[legal].max()); q /= q.sum()
    freq = np.bincount(wn, minlength=V) / B
    assert (np.abs(freq[legal] - q[legal]) < 4 * np.sqrt(q[legal] * (1 - q[legal]) / B)).all(), np.abs(freq - q).max()
    assert np.isfinite(lq).all() and np.abs(lq - np.log(q[wn])).max() < 1e-5
    assert not eos_mask.any() and (gstate[:, 0].cpu().numpy() & 0xFF != SY.ERROR).all()


# ---------------------------------------------------------------------------------------------- 3. syntax=False changes nothing
def _kernel_names(fn):
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    evs = sorted((e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA), key=lambda e: e.time_range.start)
    return [e.name for e in evs]


def test_syntax_false_changes_nothing_and_both_modes_launch_four_kernels_per_token():
    model, _ = _model(torch.bfloat16)
    z = _latents(200, seed=2)
    a = model.sample(200, max_len=20, z=z, temp=0.9, seed=5, return_tokens=True, return_logp=True, top_k=9)
    b = model.sample(200, max_len=20, z=z, temp=0.9, seed=5, return_tokens=True, return_logp=True, top_k=9, syntax=False)
    assert all(torch.equal(s, t) for s, t in zip(a[0], b[0])) and torch.equal(a[2], b[2])
    c, _ = model.sample(200, max_len=20, z=z, seed=5, return_tokens=True)
    d, _ = model.sample(200, max_len=20, z=z, seed=5, return_tokens=True, syntax=False)
    assert all(torch.equal(s, t) for s, t in zip(c, d))
    p = model._sample_tokens(z, 20, 1.0, 6, 8, 0.9)
    q = model._sample_tokens(z, 20, 1.0, 6, 8, 0.9, syntax=False)
    assert all(torch.equal(s, t) for s, t in zip(p, q))                       # tokens, ends, logq, hash
    for kw, name, n_other in ((dict(), "moses_sample_step", "sample_filtered_step"), (dict(top_k=8), "sample_filtered_step", "moses_sample_step_kernel"),
                              (dict(syntax=True), "sample_filtered_step", "moses_sample_step_kernel")):
        model.sample(64, max_len=6, seed=1, **kw)                             # warm
        names = _kernel_names(lambda: model.sample(64, max_len=26, seed=1, **kw))
        is_smp = [name in n_ for n_ in names]
        is_gru = ["gru_step" in n_ or "lstm_step" in n_ or "step_fwd" in n_ for n_ in names]
        assert sum(is_smp) == 25 and sum(is_gru) == 3 * 25, (kw, sum(is_smp), sum(is_gru), sorted(set(names)))
        assert not any(n_other in n_ for n_ in names), (kw, sorted(set(names)))
        first, last = is_smp.index(True), len(names) - 1 - is_smp[::-1].index(True)
        between = [n_ for n_, s, g in zip(names[first:last + 1], is_smp[first:last + 1], is_gru[first:last + 1]) if not (s or g)]
        assert not between, (kw, sorted(set(between)))


# ---------------------------------------------------------------------------------------------- 4. end to end, by construction
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_constrained_samples_are_well_formed_by_construction(dtype):
    """B = 256 N(0, I) latents, temp 1, max_len 3 / 4 / 12 / 40 and one run with top_k = 5, top_p = 0.9: every row ends in <eos> within
    max_len, every string passes the independent validator and syntax_valid says so too.  The same model without the constraint at
    max_len = 40 is mostly ill-formed (printed; < 0.5 asserted: the untrained head is near-uniform, and uniform strings over this
    alphabet are well-formed at about 2 %)."""
    model, _ = _model(dtype)
    B = 256
    z = _latents(B, seed=4)
    for max_len, kw in ((3, {}), (4, {}), (12, {}), (40, {}), (40, dict(top_k=5, top_p=0.9))):
        x, ends, logq, _ = model._sample_tokens(z, max_len, 1.0, 17, *model._check_filters(kw.get("top_k"), kw.get("top_p")), syntax=True)
        xs, es = x.cpu().numpy(), ends.cpu().numpy()
        assert ((es >= 3) & (es <= max_len)).all() and (xs[np.arange(B), es - 1] == model.eos).all(), (max_len, kw)
        assert all((xs[b, es[b]:] == model.pad).all() for b in range(B))
        strings = [SY.row_string(xs[b], model.vocabulary) for b in range(B)]
        bad = [s for s in strings if s is None or not SY.valid_smiles(s)]
        assert not bad, (max_len, kw, bad[:5])
        assert bool(model.syntax_valid(x).all()) and bool(torch.isfinite(logq).all())
        toks, _ = model.sample(B, max_len=max_len, z=z, seed=17, syntax=True, **kw)     # the public call returns the same strings
        assert toks == strings
        if max_len == 40 and not kw:
            assert len(set(strings)) > 10                                       # a sample, not one string
    x_free = model._sample_tokens(z, 40, 1.0, 17, filtered=False)[0]
    ok = model.syntax_valid(x_free).cpu().numpy()
    want = np.array([SY.row_valid(r, model.vocabulary) for r in x_free.cpu().numpy()])
    assert (ok == want).all()
    print(f"{dtype}: unconstrained validity at max_len = 40: {ok.mean():.3f}")
    assert ok.mean() < 0.5, ok.mean()


# ---------------------------------------------------------------------------------------------- 5. the loop against float64
def _masked_reference(p64, vocab, z, x, ends, u_of_step, free_run=False):
    """The float64 decoder (sample_ref.BatchDecoder) plus the mask of the python automaton.  Teacher-forced on the rows x [B, max_len]
    (free_run: on its own draws instead): per step the reference draw, its draw margin and log(q_w / sum q) of the token that was fed."""
    B, T = x.shape
    chars = SY.token_chars(vocab)
    dec = SR.BatchDecoder(p64, z)
    hs = dec.h0()
    states = [SY.S0] * B
    prev = np.full(B, vocab.bos)
    tok, marg, logq = np.zeros((B, T - 1), np.int64), np.full((B, T - 1), np.inf), np.zeros((B, T - 1))
    done = np.zeros(B, bool)
    for i in range(1, T):
        logp, hs = dec.step(prev, hs)
        p = SR.softmax_temp(logp, 1.0)
        keep = np.zeros(p.shape, bool)
        for b in range(B):
            if not done[b]:
                keep[b, SY.allowed_ids(states[b], chars, T - 1 - i)] = True
            else:
                keep[b] = True
        assert keep.any(1).all()
        u = u_of_step(i)
        tok[:, i - 1] = SR.draw(p, keep, u)
        marg[:, i - 1] = SR.draw_margin(p, keep, u)
        fed = tok[:, i - 1] if free_run else x[:, i]
        q = p * keep
        with np.errstate(divide="ignore"):
            logq[:, i - 1] = np.log(np.take_along_axis(q, fed[:, None], 1)[:, 0] / q.sum(1))
        for b in range(B):
            if not done[b]:
                nxt = SY.step(states[b], chars[fed[b]]) if chars[fed[b]] is not None else None
                if nxt is None or nxt[0] == SY.END:
                    done[b] = True
                else:
                    states[b] = nxt
        prev = fed
        if free_run:
            x[:, i] = fed
    return dict(tok=tok, c=marg, logq=logq)


LOOP = dict(B=512, max_len=14, seed=77, zseed=12)


def reference_alone_skip_rate():
    """The float64 reference sampling on its own (no GPU): the share of its decisions whose draw margin is below 1e-5."""
    v = _vocab()
    params = ip.init_params(ip.moses_shapes(len(v)), 303, 1.5, np.float32)
    p64 = {k: p.astype(np.float64) for k, p in params.items()}
    B, T = LOOP["B"], LOOP["max_len"]
    z = np.random.RandomState(LOOP["zseed"]).standard_normal((B, 160)).astype(np.float32).astype(np.float64)
    x = np.full((B, T), v.pad, np.int64); x[:, 0] = v.bos
    ref = _masked_reference(p64, v, z, x, None, lambda i: ops.sample_uniform(LOOP["seed"], i, B), free_run=True)
    ends = np.array([list(r).index(v.eos) + 1 for r in x])
    valid = np.arange(1, T)[None] < ends[:, None]
    return float((valid & (ref["c"] <= 1e-5)).sum() / valid.sum()), int(valid.sum())


def test_constrained_sampling_loop_matches_float64_decisions():
    """f32, B = 512, max_len = 14, one N(0, I) latent per row, filters off: the float64 decoder with the python automaton's mask is
    teacher-forced on the GPU's own tokens; at every (row, step) whose draw margin exceeds 1e-5 the GPU token is the reference draw, at
    most 3 % of the decisions being skipped for a small margin (the float64 reference alone, sampling these latents with these uniforms,
    skips 0.07 % of its 5,838 decisions: reference_alone_skip_rate()); for the rows none of whose decisions was skipped logq equals the
    float64 sum of log(q_w / sum q) within 1e-4, and at least half of the rows are compared -- the margins and caps of
    test_filtered_sampling_loop_matches_float64_decisions."""
    model, p64 = _model(torch.float32)
    B, max_len, seed = LOOP["B"], LOOP["max_len"], LOOP["seed"]
    z = _latents(B, seed=LOOP["zseed"])
    x, ends, logq, _ = model._sample_tokens(z, max_len, 1.0, seed, syntax=True)
    x, ends = x.cpu().numpy(), ends.cpu().numpy()
    assert (x[:, 0] == model.bos).all() and (x[np.arange(B), ends - 1] == model.eos).all()
    ref = _masked_reference(p64, model.vocabulary, z.double().cpu().numpy(), x, ends, lambda i: ops.sample_uniform(seed, i, B))
    valid = np.arange(1, max_len)[None] < ends[:, None]                        # the decisions the row made before it ended
    ok = ref["c"] > 1e-5
    skipped = (valid & ~ok).sum() / valid.sum()
    wrong = valid & ok & (ref["tok"] != x[:, 1:])
    print(f"decisions {int(valid.sum())}, skipped for a small margin {skipped:.4f}, wrong {int(wrong.sum())}")
    assert skipped <= 0.03, skipped
    assert not wrong.any(), np.argwhere(wrong)[:10]
    clean = ~(valid & ~ok).any(1)
    want = np.where(valid, ref["logq"], 0.0).sum(1)
    err = np.abs(logq.cpu().numpy().astype(np.float64) - want)[clean]
    print(f"rows compared {int(clean.sum())} / {B}, max logq error {err.max():.2e}")
    assert clean.sum() >= B // 2, clean.sum()
    assert err.max() < 1e-4, err.max()


# ---------------------------------------------------------------------------------------------- 6. the check kernel
def test_syntax_check_kernel_equals_the_validator_and_the_automaton():
    """mvae_smiles_syntax_check on hand-made rows (the accepted and the rejected strings of the host tests, rows without <eos>, rows with
    an id outside the vocabulary) and 2,000 random ones (1,000 of uniform tokens, 1,000 constrained walks with one token replaced):
    valid equals the independent validator, bad_pos the plain-Python automaton's first refusal.  B = 2,032 rows, T = 40."""
    v = _vocab()
    chars, info = SY.token_chars(v), VC.smiles_token_table(v).to(dev)
    T = 40
    rows = [v.string2ids(s, add_bos=True, add_eos=True) for s in GOOD + BAD]
    rows += [v.string2ids("CCO", add_bos=True), v.string2ids("C" * (T - 1), add_bos=True), [v.bos], [v.bos, v.c2i["C"], v.pad, v.eos],
             [v.bos, v.c2i["C"], v.unk, v.eos], [v.bos, v.c2i["C"], v.eos, v.c2i[")"], v.eos]]
    n_hand = len(rows)
    rs = np.random.RandomState(3)
    for _ in range(1000):
        rows.append([v.bos] + list(rs.randint(0, len(v), rs.randint(1, T))))
    for _ in range(1000):
        ids, _ = SY.random_walk(chars, int(rs.randint(4, T + 1)), rs)
        ids[rs.randint(len(ids))] = int(rs.randint(0, len(v)))
        rows.append([v.bos] + ids)
    B = len(rows)
    assert B % 64 != 0 and B == n_hand + 2000
    x = np.full((B, T), v.pad, np.int64)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    x[n_hand - 1, 2] = len(v) + 5; x[n_hand - 2, 2] = -1                       # ids outside [0, V) are refused, not looked up
    xt = torch.from_numpy(x).to(dev)
    valid = torch.empty(B, dtype=torch.uint8, device=dev)
    bad = torch.empty(B, dtype=torch.int32, device=dev)
    ops.smiles_syntax_check(xt, info, v.eos, valid, bad)
    want_valid = np.array([SY.row_valid(r, v) for r in x])
    want_bad = np.array([SY.first_refusal(r, chars) for r in x])
    got_valid, got_bad = valid.cpu().numpy().astype(bool), bad.cpu().numpy()
    assert (got_valid == want_valid).all(), np.nonzero(got_valid != want_valid)[0][:10]
    assert (got_bad == want_bad).all(), np.nonzero(got_bad != want_bad)[0][:10]
    assert got_valid[:len(GOOD)].all() and not got_valid[len(GOOD):n_hand].any() and (got_bad[got_valid] == -1).all()
    assert got_bad[len(GOOD) + len(BAD)] == 4 and got_bad[len(GOOD) + len(BAD) + 1] == T        # no <eos>: <pad> refused / ran out
    assert 50 < got_valid[n_hand:].sum() < 900                                 # the random rows exercise both verdicts
    # eos_id alone ends a row: it is EOS whatever the table says of it, and another id the table calls EOS is refused
    t2 = info.clone(); t2[v.c2i["N"]] = VC.SMI_EOS; t2[v.eos] = VC.SMI_OTHER
    x2 = torch.tensor([[v.bos, v.c2i["C"], v.eos, v.pad], [v.bos, v.c2i["C"], v.c2i["N"], v.eos]], device=dev)
    ops.smiles_syntax_check(x2, t2, v.eos, valid[:2], bad[:2])
    assert valid[:2].tolist() == [1, 0] and bad[:2].tolist() == [-1, 2]
    # without bad_pos, through the model: strings, id tensors and padded ids give the same flags
    model, _ = _model(torch.bfloat16)
    f1 = model.syntax_valid(GOOD + BAD)
    f2, bp = model.syntax_valid([torch.tensor(r) for r in rows[:len(GOOD + BAD)]], bad_pos=True)
    assert f1.dtype == torch.bool and f1.tolist() == [True] * len(GOOD) + [False] * len(BAD) == f2.tolist()
    assert bp.tolist() == want_bad[:len(GOOD + BAD)].tolist()
    assert torch.equal(model.syntax_valid(xt[:, :T]), torch.from_numpy(want_valid).to(dev))


# ---------------------------------------------------------------------------------------------- 7. moses_generate
def test_moses_generate_counts_well_formed_samples():
    model, _ = _model(torch.bfloat16)
    n, bs = 700, 256
    z = _latents(n, seed=8)
    res = mv.moses_generate(model, n, batch_size=bs, max_len=24, seed=3, z=z, syntax=True, count_valid=True)
    assert res["total"] == n == res["valid"] and res["valid_unique"] == res["unique"] == len(res["strings"])
    assert all(SY.valid_smiles(s) for s in res["strings"])
    plain = mv.moses_generate(model, n, batch_size=bs, max_len=24, seed=3, z=z)
    assert "valid" not in plain and "valid_unique" not in plain
    free = mv.moses_generate(model, n, batch_size=bs, max_len=24, seed=3, z=z, count_valid=True)
    assert {k: free[k] for k in plain} == plain                                 # counting changes nothing else
    seen, valid, valid_unique = set(), 0, 0
    for j, b0 in enumerate(range(0, n, bs)):
        toks, _ = model.sample(min(bs, n - b0), max_len=24, z=z[b0:b0 + bs], seed=3 + j, return_tokens=True)
        for t in toks:
            ok = SY.row_valid(t.tolist(), model.vocabulary)
            valid += ok
            if tuple(t.tolist()) not in seen:
                seen.add(tuple(t.tolist()))
                valid_unique += ok
    print(f"unconstrained: {valid} of {n} well-formed, {valid_unique} of {len(seen)} distinct ones")
    assert free["valid"] == valid and free["valid_unique"] == valid_unique and free["unique"] == len(seen)
    assert valid < n
