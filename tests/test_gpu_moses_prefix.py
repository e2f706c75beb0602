"""GPU tests of prefix-constrained sampling and decoding: the forced launches alone (mvae_moses_sample_forced_step,
mvae_moses_beam_forced_step) against their siblings and against numpy, mvae_smiles_prefix_state against the plain-Python walk, and
VAE.sample / decode / moses_generate with prefix= against the unconstrained runs (the replay property), the float64 references of
tests/prefix_ref.py, sample_ref.py and beam_ref.py, and the independently written validator of syntax_ref.py.  Forced tokens, hashes,
automaton states and the bookkeeping are integer logic: those assertions have no tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import molecular_vae_amd as mv                  # noqa: E402
from molecular_vae_amd import vocab as VC, ops  # noqa: E402
import beam_ref as BR                           # noqa: E402
import prefix_ref as PR                         # noqa: E402
import sample_ref as SR                         # noqa: E402
import syntax_ref as SY                         # noqa: E402

dev = torch.device("cuda")
MARGIN = 1e-4
PREFIXES = ["", "C", "CC(", "c1cc", "CC(=O)O", "C[N+](C)", "N#Cc1ccc"]
BEAM_SETS = {4: ["", "C", "CC", "CO", "N", "O", "CN"], 12: PREFIXES}

_MODELS = {}


def _model(dtype):
    if dtype not in _MODELS:
        _MODELS[dtype] = PR.model(dtype, dev)
    return _MODELS[dtype]


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _fold(h, t):
    return SR.as_int64(((int(h) & SR.M64) ^ int(t)) * SR.FNV_PRIME & SR.M64)


# ---------------------------------------------------------------------------------------------- 1. the sampling launch alone, fixed logits
@pytest.mark.parametrize("syntax", [False, True])
def test_forced_step_on_a_fixed_logit_row(syntax):
    """B = 5 rows in one launch (two workgroups, the second with one row) over the same logits, top_k = 5 and top_p = 0.9 on: rows 0 and 3
    are forced, 1 and 4 free, 2 has ended.  Row 0's forced token '(' has the smallest logit of all, far outside the top 5; row 3's ')'
    is refused by the automaton (syntax: its state goes to ERROR, the token is written all the same).  A forced row gets its token,
    logq bit-unchanged, the hash folded, end_pads / eos_mask untouched, w_out and add_out = table[w] + base[b]; the free and the ended
    rows are bitwise what the sibling launch (filtered, or syntax with tok_info / gstate given) writes for the same inputs."""
    v = PR.vocab()
    V, H, W, B = len(v), 64, 128, 5
    temp, seed, step, max_len, top_k, top_p = 0.7, 12345, 3, 12, 5, 0.9
    rs = np.random.RandomState(0)
    logits = rs.standard_normal(V).astype(np.float32) * 2.0
    lpar, rpar = v.c2i["("], v.c2i[")"]
    logits[lpar] = logits.min() - 3.0
    assert np.argsort(-logits).tolist().index(lpar) == V - 1
    h = torch.zeros(B, H, device=dev); h[:, 0] = 1.0
    wfc = torch.zeros(V, H, device=dev); wfc[:, 0] = torch.from_numpy(logits).to(dev)
    table = torch.from_numpy(rs.standard_normal((V, W)).astype(np.float32)).to(dev)
    base = torch.from_numpy(rs.standard_normal((B, W)).astype(np.float32)).to(dev)
    forced = torch.full((B, max_len), -1, dtype=torch.int32, device=dev)
    forced[0, step], forced[3, step] = lpar, rpar
    forced[1, step - 1], forced[1, step + 1] = lpar, rpar                       # other steps' entries are not this launch's business
    logq0 = rs.standard_normal(B).astype(np.float32)
    hash0 = rs.randint(-2 ** 62, 2 ** 62, B, dtype=np.int64)
    st = SY.step(SY.S0, "C")
    g0 = np.array([SY.pack_state(st, v)] * B, np.int32)
    info = VC.smiles_token_table(v).to(dev)

    def fresh():
        em = torch.zeros(B, dtype=torch.uint8, device=dev); em[2] = 1
        ep = torch.full((B,), 8, dtype=torch.long, device=dev); ep[2] = 2
        return dict(add=torch.full((B, W), float("nan"), device=dev), x=torch.full((B, 8), 99, dtype=torch.long, device=dev), ep=ep, em=em,
                    w=torch.full((B,), -7, dtype=torch.long, device=dev), logq=torch.from_numpy(logq0).to(dev),
                    hsh=torch.from_numpy(hash0).to(dev), gs=torch.from_numpy(g0).to(dev))
    a, b = fresh(), fresh()
    common = (h, H, wfc, None, temp, top_k, top_p, seed, step, v.eos, table, base)
    if syntax:
        ops.moses_sample_syntax_step(*common, a["add"], a["x"], a["ep"], a["em"], a["w"], B, V, H, info, a["gs"], max_len, logq=a["logq"],
                                     hash=a["hsh"])
        ops.moses_sample_forced_step(*common, b["add"], b["x"], b["ep"], b["em"], b["w"], B, V, H, forced, tok_info=info, gstate=b["gs"],
                                     max_len=max_len, logq=b["logq"], hash=b["hsh"])
    else:
        ops.moses_sample_filtered_step(*common, a["add"], a["x"], a["ep"], a["em"], a["w"], B, V, H, logq=a["logq"], hash=a["hsh"])
        ops.moses_sample_forced_step(*common, b["add"], b["x"], b["ep"], b["em"], b["w"], B, V, H, forced, logq=b["logq"], hash=b["hsh"])
    torch.cuda.synchronize()
    free = torch.tensor([1, 2, 4], device=dev)
    for k in a:
        assert _same(a[k][free], b[k][free]), k
    assert int(a["x"][2, step]) == 99 and float(a["logq"][2]) == logq0[2]         # the ended row: as the sibling leaves it
    xs, ep, em, w, lq, hs, gs = (b[k].cpu().numpy() for k in ("x", "ep", "em", "w", "logq", "hsh", "gs"))
    for r, tok in ((0, lpar), (3, rpar)):
        assert xs[r, step] == tok and w[r] == tok and (np.delete(xs[r], step) == 99).all()
        assert lq[r] == logq0[r] and hs[r] == _fold(hash0[r], tok)
        assert ep[r] == 8 and em[r] == 0
        assert torch.equal(b["add"][r], table[tok] + base[r])
    if syntax:
        assert tuple(gs[0]) == SY.pack_state(SY.step(st, "("), v)
        assert SY.step(st, ")") is None and tuple(gs[3]) == ((int(g0[3, 0]) & ~0xFF) | SY.ERROR, int(g0[3, 1]))
    else:
        assert (gs == g0).all()
    assert int(a["w"][0]) != lpar                                                # the sibling never draws the token outside the top 5


# ---------------------------------------------------------------------------------------------- 2. an all-free table is the sibling launch
def _random_states(v, n, rs, max_len):
    chars = SY.token_chars(v)
    return np.array([SY.pack_state(SY.random_prefix(chars, int(rs.randint(0, 9)), rs, max_len=max_len)[0], v) for _ in range(n)], np.int32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_all_free_table_is_bitwise_the_sampling_siblings(dtype):
    """forced all -1, B = 131 (33 workgroups, the last with 3 rows), filters on and off: every written tensor equals, bit for bit, what
    mvae_moses_sample_filtered_step (tok_info / gstate NULL) and mvae_moses_sample_syntax_step (given) write."""
    v = PR.vocab()
    B, V, H, W, max_len, step = 131, len(v), 128, 256, 40, 9
    g = torch.Generator(device="cuda").manual_seed(5)
    h = (torch.randn(B, H + 8, device=dev, generator=g) * 0.5).to(dtype)
    wfc = (torch.randn(V, H + 8, device=dev, generator=g) * 0.4).to(dtype)
    bias = torch.randn(V, device=dev, generator=g) * 0.1
    table = torch.randn(V, W, device=dev, generator=g)
    base = torch.randn(B, W, device=dev, generator=g)
    info = VC.smiles_token_table(v).to(dev)
    g0 = torch.from_numpy(_random_states(v, B, np.random.RandomState(2), max_len - step)).to(dev)
    forced = torch.full((B, max_len), -1, dtype=torch.int32, device=dev)

    def state():
        em = torch.zeros(B, dtype=torch.uint8, device=dev); em[::5] = 1
        return [torch.full((B, W), float("nan"), device=dev), torch.full((B, max_len), 99, dtype=torch.long, device=dev),
                torch.full((B,), max_len, dtype=torch.long, device=dev), em, torch.full((B,), -7, dtype=torch.long, device=dev),
                torch.zeros(B, device=dev), torch.full((B,), 17, dtype=torch.long, device=dev), g0.clone()]
    for temp, top_k, top_p in ((1.0, 0, 1.0), (0.8, 5, 0.9)):
        head = (h, H + 8, wfc, bias, temp, top_k, top_p, 99, step, v.eos, table, base)
        a, b, c, d = state(), state(), state(), state()
        ops.moses_sample_filtered_step(*head, *a[:5], B, V, H, logq=a[5], hash=a[6])
        ops.moses_sample_forced_step(*head, *b[:5], B, V, H, forced, logq=b[5], hash=b[6])
        ops.moses_sample_syntax_step(*head, *c[:5], B, V, H, info, c[7], max_len, logq=c[5], hash=c[6])
        ops.moses_sample_forced_step(*head, *d[:5], B, V, H, forced, tok_info=info, gstate=d[7], max_len=max_len, logq=d[5], hash=d[6])
        torch.cuda.synchronize()
        for s, t in zip(a + c, b + d):
            assert _same(s, t)
        assert not torch.equal(a[4], c[4]) and not torch.equal(c[7], g0)        # the two siblings differ: the comparison can tell them apart


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_all_free_table_is_bitwise_the_beam_siblings(dtype):
    """forced all -1, B = 5 molecules, K in {1, 3, 4} (K = 1: a short last pass), rows finished, dead and active: every written tensor
    equals, bit for bit, what mvae_moses_beam_step and mvae_moses_beam_syntax_step write."""
    v = PR.vocab()
    V, H, ldh, W, B, max_len, step = len(v), 64, 72, 128, 5, 30, 7
    info = VC.smiles_token_table(v).to(dev)
    rs = np.random.RandomState(4)
    forced = torch.full((B, max_len), -1, dtype=torch.int32, device=dev)
    for K in (1, 3, 4):
        R = B * K
        g = torch.Generator(device="cuda").manual_seed(K)
        st0 = (torch.randn(2, 2, R, ldh, device=dev, generator=g)).to(dtype)
        wfc = (torch.randn(V, H, device=dev, generator=g) * 0.5).to(dtype)
        table = torch.randn(V, W, device=dev, generator=g)
        base = torch.randn(R, W, device=dev, generator=g)
        sc0 = torch.from_numpy(np.where(rs.rand(R) < 0.2, -np.inf, -5 * rs.rand(R)).astype(np.float32)).to(dev)
        fin0 = torch.from_numpy((rs.rand(R) < 0.2).astype(np.uint8)).to(dev)
        g0 = torch.from_numpy(_random_states(v, R, rs, max_len - step)).to(dev)

        def state():
            return [st0.clone(), torch.full((R, W), float("nan"), device=dev), sc0.clone(), fin0.clone(),
                    torch.full((R,), max_len, dtype=torch.long, device=dev), torch.full((max_len, R), -7, dtype=torch.int32, device=dev),
                    torch.full((max_len, R), -7, dtype=torch.int32, device=dev), g0.clone()]
        a, b, c, d = state(), state(), state(), state()
        head = lambda s: (s[0], ldh, wfc, None, step, v.eos, v.pad, table, base, s[1], s[2], s[3], s[4], s[5], s[6], B, K, V, H)
        ops.moses_beam_step(*head(a))
        ops.moses_beam_forced_step(*head(b), forced)
        ops.moses_beam_syntax_step(*head(c), info, c[7], max_len)
        ops.moses_beam_forced_step(*head(d), forced, tok_info=info, gstate=d[7], max_len=max_len)
        torch.cuda.synchronize()
        for s, t in zip(a + c, b + d):
            assert _same(s, t)
        assert not torch.equal(c[7], g0) and (K == 1 or not torch.equal(a[5], c[5]))


def test_forced_beam_launch_proposes_the_forced_token_alone():
    """K = 3, one layer, B = 5 molecules: molecules 0, 2 and 4 forced (to a token of small probability), 1 and 3 free.  A forced molecule's
    active beams each survive once, in beam order, with the forced token at score + log_softmax[token] (1e-5 against float64), dead beams
    stay -inf, a finished beam proposes itself; the free molecules are bitwise what mvae_moses_beam_step writes."""
    v = PR.vocab()
    V, H, ldh, W, B, K, max_len, step = len(v), 64, 72, 128, 5, 3, 12, 2
    R = B * K
    rs = np.random.RandomState(8)
    h1 = rs.standard_normal((R, ldh)).astype(np.float32); h1[:, :V] *= 2.0
    tok = v.c2i["#"]
    h1[:, tok] -= 6.0
    logits = h1[:, :V].astype(np.float64)
    mx = logits.max(1, keepdims=True)
    logp = logits - (mx + np.log(np.exp(logits - mx).sum(1, keepdims=True)))
    wfc = torch.eye(H, device=dev)[:V].contiguous()
    table = torch.from_numpy(rs.standard_normal((V, W)).astype(np.float32)).to(dev)
    base = torch.from_numpy(rs.standard_normal((R, W)).astype(np.float32)).to(dev)
    sc0 = np.sort(-5 * rs.rand(B, K), 1)[:, ::-1].astype(np.float32).copy()
    sc0[0, 1:] = -np.inf                                                         # molecule 0: beams 1, 2 dead, as during a prefix
    fin0 = np.zeros((B, K), np.uint8); fin0[2, 0] = 1                            # molecule 2: its best beam has finished
    end0 = np.full((B, K), max_len, np.int64); end0[2, 0] = 2
    forced = torch.full((B, max_len), -1, dtype=torch.int32, device=dev)
    forced[0, step] = forced[2, step] = forced[4, step] = tok

    def state():
        s = torch.zeros((1, 2, R, ldh), device=dev); s[0, 1] = torch.from_numpy(h1).to(dev)
        return [s, torch.full((R, W), float("nan"), device=dev), torch.from_numpy(sc0.reshape(R)).to(dev), torch.from_numpy(fin0.reshape(R)).to(dev),
                torch.from_numpy(end0.reshape(R)).to(dev), torch.full((max_len, R), -7, dtype=torch.int32, device=dev),
                torch.full((max_len, R), -7, dtype=torch.int32, device=dev)]
    a, b = state(), state()
    head = lambda s: (s[0], ldh, wfc, None, step, v.eos, v.pad, table, base, s[1], s[2], s[3], s[4], s[5], s[6], B, K, V, H)
    ops.moses_beam_step(*head(a))
    ops.moses_beam_forced_step(*head(b), forced)
    torch.cuda.synchronize()
    rows = torch.tensor([3, 4, 5, 9, 10, 11], device=dev)                        # molecules 1 and 3
    for s, t in zip(a, b):
        s, t = (s[0, 0], t[0, 0]) if s.dim() == 4 else (s[step], t[step]) if s.shape[0] == max_len else (s, t)
        assert _same(s[rows], t[rows])
    sc, fin, ends, ht, hp = b[2].cpu().numpy().reshape(B, K), b[3].cpu().numpy().reshape(B, K), b[4].cpu().numpy().reshape(B, K), \
        b[5][step].cpu().numpy().reshape(B, K), b[6][step].cpu().numpy().reshape(B, K)
    want = sc0.astype(np.float64) + logp[:, tok].reshape(B, K)
    # molecule 0: one live beam, then the dead ones in beam order; molecule 4: three live beams keep their order (equal increments would
    # not: the candidates are re-sorted by score)
    assert hp[0].tolist() == [0, 1, 2] and ht[0].tolist() == [tok] * 3 and np.isfinite(sc[0, 0]) and (sc[0, 1:] == -np.inf).all()
    assert abs(sc[0, 0] - want[0, 0]) < 1e-5
    order = sorted(range(K), key=lambda k: (-want[4, k], k))
    assert hp[4].tolist() == order and ht[4].tolist() == [tok] * 3 and np.abs(sc[4] - want[4, order]).max() < 1e-5
    assert (fin[[0, 4]] == 0).all() and (ends[[0, 4]] == max_len).all()
    # molecule 2: the finished beam proposes itself (pad, score unchanged), the others the forced token
    cand = sorted([(float(sc0[2, 0]), 0, v.pad)] + [(want[2, k], k, tok) for k in (1, 2)], key=lambda t: (-t[0], t[1]))
    assert hp[2].tolist() == [c[1] for c in cand] and ht[2].tolist() == [c[2] for c in cand]
    assert np.abs(sc[2] - np.array([c[0] for c in cand])).max() < 1e-5
    assert fin[2].tolist() == [1 if c[1] == 0 else 0 for c in cand] and ends[2].tolist() == [2 if c[1] == 0 else max_len for c in cand]
    par = (np.arange(R) // K) * K + hp.reshape(R)
    assert torch.equal(b[1], table[torch.from_numpy(ht.reshape(R).astype(np.int64)).to(dev)] + base)
    assert torch.equal(b[0][0, 0, :, :H], b[0][0, 1, torch.from_numpy(par).to(dev), :H])


# ---------------------------------------------------------------------------------------------- 3. the prefix walk
def test_prefix_state_equals_the_plain_python_walk():
    """B = 65 (one 64-thread workgroup and a tail row), lengths 0 .. 20 from syntax_ref.random_prefix, every fourth row with one token
    replaced; ids in a buffer wider than P, garbage behind each length.  State words, need and bad_pos equal the plain-Python walk."""
    v = PR.vocab()
    V, B, P = len(v), 65, 20
    chars = SY.token_chars(v)
    rs = np.random.RandomState(6)
    ids = rs.randint(0, V, (B, P + 4)).astype(np.int32)                          # what lies behind a row's length is never read as a token
    lens, rows = [], []
    for b in range(B):
        _, p = SY.random_prefix(chars, b % 21, rs)
        p = list(p)
        if b % 4 == 3 and p:
            p[rs.randint(len(p))] = [v.bos, v.pad, v.c2i[")"], v.c2i["]"], V + 3, -2][rs.randint(6)]
        ids[b, :len(p)] = p
        lens.append(len(p)); rows.append(p)
    assert max(lens) == 20 and min(lens) == 0
    buf = torch.from_numpy(ids).to(dev)
    state = torch.full((B, 2), -7, dtype=torch.int32, device=dev)
    need = torch.full((B,), -7, dtype=torch.int32, device=dev)
    bad = torch.full((B,), -7, dtype=torch.int32, device=dev)
    ops.smiles_prefix_state(buf[:, :P], torch.tensor(lens, dtype=torch.int32, device=dev), VC.smiles_token_table(v).to(dev), state, need, bad)
    st, nd, bp = state.cpu().numpy(), need.cpu().numpy(), bad.cpu().numpy()
    n_bad = 0
    for b in range(B):
        words, n, pos = PR.prefix_walk(rows[b], v)
        assert (tuple(int(t) for t in st[b]), int(nd[b]), int(bp[b])) == (words, n, pos), (b, rows[b])
        n_bad += pos >= 0
    assert n_bad >= 8 and (bp == -1).sum() >= 40, n_bad


# ---------------------------------------------------------------------------------------------- 4. the replay property
_REPLAY = {}
B_R, LEN_R, SEED_R = 7, 12, 77


def _replay_case(dtype, syntax, top_k, top_p):
    """Sample B = 7 rows at max_len = 12, then again with prefix[b] = x[b, 1 : 1 + P_b], P_b in 0 .. min(end_b, 12) - 2: row 0 at 0, row 1
    and the first row that ended in <eos> at the maximum, the rest drawn.  A prefix may not hold <bos> or <pad> (ValueError), which this
    random model does draw when no automaton stops it: P_b then ends in front of the first one."""
    key = (dtype, syntax, top_k, top_p)
    if key not in _REPLAY:
        model, p64 = _model(dtype)
        temp = 1.0 if top_k is None else 0.9
        k, p = model._check_filters(top_k, top_p)
        z = PR.latents(B_R, seed=3, scale=0.7, device=dev)
        free = model._sample_tokens(z, LEN_R, temp, SEED_R, k, p, syntax=syntax)
        xs, es = free[0].cpu().numpy(), free[1].cpu().numpy()
        rs = np.random.RandomState(1)
        full = np.minimum(es, LEN_R) - 2
        special = np.isin(xs[:, 1:], [model.bos, model.pad])
        top = np.minimum(full, np.where(special.any(1), special.argmax(1), LEN_R))
        P = np.array([int(rs.randint(0, t + 1)) for t in top])
        P[0], P[1] = 0, top[1]
        ended = [b for b in range(1, B_R) if xs[b, es[b] - 1] == model.eos and top[b] == full[b]]    # (row 0 stays at P = 0)
        if ended:
            P[ended[0]] = top[ended[0]]
        prefix = [free[0][b, 1:1 + P[b]].cpu() for b in range(B_R)]
        forced = model._prefix_table(prefix, B_R, LEN_R, "test")
        again = model._sample_tokens(z, LEN_R, temp, SEED_R, k, p, syntax=syntax, forced=forced)
        _REPLAY[key] = dict(model=model, p64=p64, z=z, temp=temp, free=free, again=again, P=P, prefix=prefix, ended=ended, full=full)
    return _REPLAY[key]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("syntax", [False, True])
@pytest.mark.parametrize("top_k,top_p", [(None, None), (5, 0.9)])
def test_replay_with_own_prefix_is_bit_identical(dtype, syntax, top_k, top_p):
    c = _replay_case(dtype, syntax, top_k, top_p)
    model, P = c["model"], c["P"]
    (x, ends, _, hsh), (x2, ends2, _, hsh2) = c["free"], c["again"]
    print(f"{dtype} syntax={syntax} top_k={top_k} top_p={top_p}: ends {ends.tolist()}, P {P.tolist()}")
    assert P[0] == 0 and (P <= c["full"]).all() and ((P == c["full"]) & (P > 0)).any()      # a row at 0 and a row at the maximum
    assert torch.equal(x, x2) and torch.equal(ends, ends2) and torch.equal(hsh, hsh2)
    xs, es, hs = x2.cpu().numpy(), ends2.cpu().numpy(), hsh2.cpu().numpy()
    for b in range(B_R):
        assert hs[b] == SR.as_int64(SR.fnv1a64(xs[b, 1:es[b]])), b
        assert (xs[b, 1:1 + P[b]] == c["prefix"][b].numpy()).all()
    if top_k is None:                                          # the default path (mvae_moses_sample_step without, the forced launch with)
        kw = dict(max_len=LEN_R, z=c["z"], temp=c["temp"], seed=SEED_R, return_tokens=True, syntax=syntax)
        a, _ = model.sample(B_R, **kw)
        b_, _ = model.sample(B_R, prefix=c["prefix"], **kw)
        for b in range(B_R):
            assert torch.equal(a[b], b_[b]) and torch.equal(a[b], x[b, :es[b]].cpu()), b


# ---------------------------------------------------------------------------------------------- 5. logq covers the free tokens only
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.bfloat16, 2e-2)])
def test_logq_is_the_float64_log_p_of_the_free_tokens(dtype, tol):
    """Filters off, temp = 1, the rows of the replay test: logq[b] is the float64 teacher-forced log p summed over the steps behind the
    prefix, within the bounds of test_unfiltered_logq_is_the_float64_log_p_of_the_sampled_tokens (1e-4 in f32, 2e-2 in bf16 for the sum
    of <= 11 tokens); a row whose prefix is its whole content gets the log p of <eos> alone; the unconstrained run's logq exceeds it by
    the prefix's own log p."""
    c = _replay_case(dtype, False, None, None)
    x, ends, logq_free, _ = c["free"]
    logq = c["again"][2].cpu().numpy().astype(np.float64)
    xs, es, P = x.cpu().numpy(), ends.cpu().numpy(), c["P"]
    ref = SR.teacher_forced_sampling(c["p64"], c["z"].double().cpu().numpy(), xs, 1.0, None, None,
                                     lambda i: ops.sample_uniform(SEED_R, i, B_R))["logq"]
    steps = np.arange(1, LEN_R)[None]
    counted = (steps > P[:, None]) & (steps < es[:, None])
    want = np.where(counted, ref, 0.0).sum(1)
    whole = np.where(steps < es[:, None], ref, 0.0).sum(1)
    err = np.abs(logq - want)
    print(f"{dtype}: P {P.tolist()}, ends {es.tolist()}, worst logq error {err.max():.2e}")
    assert err.max() < tol, err
    assert np.abs(logq_free.cpu().numpy() - whole).max() < tol
    assert (want[P > 0] > whole[P > 0]).all()                  # the prefix's own log p is missing from logq
    assert c["ended"], "no row ended in <eos>: pick other latents"
    b = c["ended"][0]
    assert P[b] == es[b] - 2 and counted[b].sum() == 1 and xs[b, es[b] - 1] == c["model"].eos
    assert abs(logq[b] - ref[b, es[b] - 2]) < tol


# ---------------------------------------------------------------------------------------------- 6. syntax guarantees
def test_prefixed_sampling_under_syntax_is_well_formed():
    """B = 37, bf16, max_len = 20, the seven prefixes in turn: every row starts with its prefix, passes syntax_valid and the independent
    validator and ends in <eos>; the same latents and prefixes with syntax=False give an ill-formed row (the test can fail)."""
    model, _ = _model(torch.bfloat16)
    v = model.vocabulary
    B, max_len = 37, 20
    z = PR.latents(B, seed=5, device=dev)
    prefix = [PREFIXES[b % 7] for b in range(B)]
    forced = model._prefix_table(prefix, B, max_len, "test")
    x, ends, _, _ = model._sample_tokens(z, max_len, 1.0, 11, syntax=True, forced=forced)
    assert bool(model.syntax_valid(x).all())
    xs, es = x.cpu().numpy(), ends.cpu().numpy()
    for b in range(B):
        pre = PR.string_ids(prefix[b], v)
        assert xs[b, 1:1 + len(pre)].tolist() == pre, b
        assert SY.row_valid(xs[b], v), (b, xs[b])
        assert len(pre) + 2 <= es[b] <= max_len and xs[b, es[b] - 1] == v.eos and (xs[b, es[b]:] == v.pad).all(), (b, xs[b])
    strings, _ = model.sample(B, max_len=max_len, z=z, seed=11, syntax=True, prefix=prefix)
    assert all(s.startswith(p) and SY.valid_smiles(s) for s, p in zip(strings, prefix))
    assert strings == [v.ids2string(xs[b, :es[b]]) for b in range(B)]
    y, _, _, _ = model._sample_tokens(z, max_len, 1.0, 11, syntax=False, forced=forced)
    assert not bool(model.syntax_valid(y).all()) and not all(SY.row_valid(r, v) for r in y.cpu().numpy())


def test_a_prefix_that_leaves_no_slack_gets_the_shortest_completion():
    """max_len = 7: "CC(" needs atom ) <eos> and "c1cc" needs 1 <eos> -- exactly the max_len - 1 - P tokens left -- so the completion is
    forced: "CC(" + atom + ")" and "c1cc1", for every latent and with filters on."""
    model, _ = _model(torch.float32)
    v = model.vocabulary
    for pre, need in (("CC(", 3), ("c1cc", 2)):
        assert PR.prefix_walk(PR.string_ids(pre, v), v)[1] == need == 7 - 1 - len(pre)
    B = 8
    prefix = ["CC(", "c1cc"] * 4
    strings, _ = model.sample(B, max_len=7, z=PR.latents(B, seed=8, device=dev), seed=2, syntax=True, prefix=prefix, top_k=6, top_p=0.95)
    for s, p in zip(strings, prefix):
        if p == "CC(":
            assert len(s) == 5 and s[:3] == p and s[3] in "CNOSFcnosB" and s[4] == ")", s
        else:
            assert s == "c1cc1", s
    toks, sc = model.decode(PR.latents(2, seed=8, device=dev), beam_width=2, max_len=7, syntax=True, prefix=["CC(", "c1cc"], return_tokens=True)
    assert model.tensor2string(toks[1][0]) == "c1cc1" and float(sc[1, 1]) == float("-inf")      # one completion exists, the second slot is dead
    assert model.tensor2string(toks[0][0])[:3] == "CC(" and model.tensor2string(toks[0][1])[:3] == "CC(" and bool(torch.isfinite(sc[0]).all())


def test_refused_prefixes_raise_and_name_row_and_position():
    model, _ = _model(torch.float32)
    z = PR.latents(3, seed=1, device=dev)
    calls = [lambda p, n: model.sample(3, max_len=n, z=z, syntax=True, prefix=p),
             lambda p, n: model.decode(z, beam_width=2, max_len=n, syntax=True, prefix=p),
             lambda p, n: mv.moses_generate(model, 3, batch_size=3, max_len=n, z=z, syntax=True, prefix=p)]
    for call in calls:
        with pytest.raises(ValueError, match=r"row 1, position 1: token '\)' is refused"):
            call(["C", "C)", "CC"], 10)
        with pytest.raises(ValueError, match=r"row 2, position 2: token '\(' is refused"):
            call(["C", "", "C(("], 6)
        with pytest.raises(ValueError, match=r"row 0, position 1: token '\)' is refused"):
            call("C)", 10)
        with pytest.raises(ValueError, match=r"row 1, position 2: the string needs 2 more tokens \(<eos> included\), max_len = 4 leaves 1"):
            call(["C", "C=", "CC"], 4)
        with pytest.raises(ValueError, match=r"row 2, position 2: the string needs 3 more tokens"):
            call(["C", "C=", "C("], 5)
    strings, _ = model.sample(3, max_len=5, z=z, syntax=True, prefix=["C", "C=", "CC"])         # one more token of room: fine
    assert [s[:2] for s in strings][1] == "C=" and all(SY.valid_smiles(s) for s in strings)
    model.sample(3, max_len=10, z=z, prefix=["C", "C)", "C(("])                                # without syntax nothing is checked


# ---------------------------------------------------------------------------------------------- 7. the beam search against float64
_REF = {}


def _beam_reference(p64, v, z, K, max_len, syntax):
    key = (K, max_len, syntax)
    if key not in _REF:
        _REF[key] = [PR.beam_search(p64, zb, K, max_len, v, prefix=PR.string_ids(s, v), syntax=syntax)
                     for zb, s in zip(z, BEAM_SETS[max_len])]
    return _REF[key]


@pytest.mark.parametrize("K", [1, 3, 4])
@pytest.mark.parametrize("syntax", [False, True])
@pytest.mark.parametrize("max_len", [4, 12])
def test_prefixed_beam_search_matches_float64_reference(K, syntax, max_len):
    """f32, B = 7: ids, ends and scores (1e-4) equal the float64 forced beam search on every molecule whose decision margins all exceed
    1e-4; at least 6 of the 7 molecules are compared (the reference alone gives 7 of 7, and 6 of 7 for syntax=False with K in {3, 4},
    where molecule 0 -- the empty prefix -- has a margin of 9.7e-5).  Dead slots agree; with syntax at max_len = 4 the "CC", "CO" and
    "CN" molecules have exactly one finite hypothesis."""
    model, p64 = _model(torch.float32)
    v = model.vocabulary
    B = 7
    z = PR.latents(B, seed=2, scale=0.7, device=dev)
    prefix = BEAM_SETS[max_len]
    ids, ends, scores = model._beam_search(z, K, max_len, syntax=syntax, prefix=prefix)
    toks, sc = model.decode(z, beam_width=K, max_len=max_len, return_tokens=True, syntax=syntax, prefix=prefix)
    strings, best = model.decode(z, beam_width=K, max_len=max_len, syntax=syntax, prefix=prefix)
    assert torch.equal(sc, scores) and torch.equal(best, scores[:, 0])
    assert strings == [model.tensor2string(t[0]) for t in toks] and all(s.startswith(p) for s, p in zip(strings, prefix))
    finite = np.isfinite(scores.cpu().numpy())
    assert finite[:, 0].all() and not bool(torch.isnan(scores).any())
    ref = _beam_reference(p64, v, z.double().cpu().numpy(), K, max_len, syntax)
    compared = 0
    for b in range(B):
        rid, rend, rsc, margin = ref[b]
        print(f"K={K} syntax={syntax} max_len={max_len} molecule {b}: margin {margin:.3e}")
        if margin <= MARGIN:
            continue
        compared += 1
        for k in range(K):
            assert bool(finite[b, k]) == bool(np.isfinite(rsc[k])), (b, k)
            if not finite[b, k]:
                continue
            assert int(ends[b, k]) == rend[k], (b, k)
            assert np.array_equal(ids[b, k].cpu().numpy(), rid[k]), (b, k)
            assert torch.equal(toks[b][k], torch.from_numpy(rid[k][:rend[k]])), (b, k)
            assert abs(float(scores[b, k]) - rsc[k]) < 1e-4, (b, k, float(scores[b, k]), rsc[k])
    assert compared >= 6, compared
    if syntax:
        ok = model.syntax_valid(ids.view(B * K, max_len)).view(B, K).cpu().numpy()
        assert ok[finite].all()
        if max_len == 4:
            assert finite.sum(1).tolist() == [K, K, 1, 1, K, K, 1]


# ---------------------------------------------------------------------------------------------- 8. beam replay and scores
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("syntax", [False, True])
def test_greedy_decode_replayed_with_its_own_prefix_is_bit_identical(dtype, syntax):
    model, _ = _model(dtype)
    B, max_len = 7, 12
    z = PR.latents(B, seed=2, scale=0.7, device=dev)
    ids, ends, scores = model._beam_search(z, 1, max_len, syntax=syntax)
    es, xs = ends[:, 0].cpu().numpy(), ids[:, 0].cpu().numpy()
    rs = np.random.RandomState(2)
    special = np.isin(xs[:, 1:], [model.bos, model.pad])                          # a prefix may hold neither: stop in front of the first
    top = np.minimum(np.minimum(es, max_len) - 2, np.where(special.any(1), special.argmax(1), max_len))
    P = [int(rs.randint(0, t + 1)) for t in top]
    P[0], P[1] = 0, int(top[1])
    prefix = [ids[b, 0, 1:1 + P[b]].cpu() for b in range(B)]
    ids2, ends2, scores2 = model._beam_search(z, 1, max_len, syntax=syntax, prefix=prefix)
    assert torch.equal(ids, ids2) and torch.equal(ends, ends2) and _same(scores, scores2)
    assert max(P) >= 3


@pytest.mark.parametrize("syntax", [False, True])
def test_f32_prefixed_scores_agree_with_score(syntax):
    """The prefix is part of the score: log p(tokens | z) of the whole string as VAE.score reports it (1e-4)."""
    model, _ = _model(torch.float32)
    B, K = 7, 3
    z = PR.latents(B, seed=4, scale=0.7, device=dev)
    toks, scores = model.decode(z, beam_width=K, max_len=12, return_tokens=True, syntax=syntax, prefix=PREFIXES)
    keep = [(b, k) for b in range(B) for k in range(K) if np.isfinite(float(scores[b, k]))]
    assert len(keep) == B * K
    got = model.score([toks[b][k] for b, k in keep], z[[b for b, _ in keep]])
    want = torch.stack([scores[b, k] for b, k in keep])
    assert float((got - want).abs().max()) < 1e-4


def test_bf16_prefixed_scores_equal_float64_scores_of_the_chosen_sequences():
    """bf16: each score is the float64 teacher-forced log p of the whole sequence, prefix included, within 2e-2 per counted token (the
    bound of test_gpu_moses_decode.py)."""
    model, p64 = _model(torch.bfloat16)
    z = PR.latents(7, seed=3, scale=0.7, device=dev)
    toks, scores = model.decode(z, beam_width=3, max_len=12, return_tokens=True, prefix=PREFIXES)
    worst = 0.0
    for b in range(7):
        for k in range(3):
            s = float(scores[b, k])
            assert np.isfinite(s)
            ids = toks[b][k].numpy()
            assert ids[1:1 + len(PREFIXES[b])].tolist() == PR.string_ids(PREFIXES[b], model.vocabulary)
            lp, _, _ = BR.teacher_forced(p64, z[b].double().cpu().numpy(), ids)
            worst = max(worst, abs(s - lp.sum()) / (len(ids) - 1))
    print(f"worst per-token score error {worst:.3e}")
    assert worst < 2e-2, worst


# ---------------------------------------------------------------------------------------------- 9. launch count
def _device_kernels(fn):
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_prefixed_sample_and_decode_launch_four_kernels_per_token():
    """A 10-token prefix at max_len = 26: a forced step is a step like another -- 25 sampling (beam) launches, 75 GRU step launches, one
    finalize; none of the other sampling / beam kernels runs."""
    model, _ = _model(torch.bfloat16)
    z = PR.latents(64, seed=6, device=dev)
    pre = "CCCCCCCCCC"
    model.sample(64, max_len=6, z=z, seed=1, prefix="C"); model.decode(z, beam_width=4, max_len=6, prefix="C")          # warm
    names = _device_kernels(lambda: model.sample(64, max_len=26, z=z, seed=1, prefix=pre))
    assert sum(1 for n_ in names if "moses_sample_filtered_step" in n_) == 25, sorted(set(names))
    assert not any("moses_sample_step" in n_ for n_ in names)
    assert sum(1 for n_ in names if "gru_step" in n_ or "lstm_step" in n_ or "step_fwd" in n_) == 75, sorted(set(names))
    names = _device_kernels(lambda: model.decode(z, beam_width=4, max_len=26, prefix=pre))
    assert sum(1 for n_ in names if "moses_beam_step" in n_) == 25, sorted(set(names))
    assert sum(1 for n_ in names if "gru_step" in n_ or "lstm_step" in n_ or "step_fwd" in n_) == 75, sorted(set(names))
    assert sum(1 for n_ in names if "moses_beam_finalize" in n_) == 1
    names = _device_kernels(lambda: model.sample(64, max_len=26, z=z, seed=1, prefix=pre, syntax=True))
    assert sum(1 for n_ in names if "moses_sample_filtered_step" in n_) == 25 and sum(1 for n_ in names if "smiles_prefix_state" in n_) == 1


# ---------------------------------------------------------------------------------------------- 10. moses_generate
def _host_dedup(model, n, bs, seed, prefix_of_batch, z=None, **kw):
    index, strings, counts, logqs = {}, [], [], []
    for j, b0 in enumerate(range(0, n, bs)):
        m = min(bs, n - b0)
        toks, _, lq = model.sample(m, seed=seed + j, return_tokens=True, return_logp=True, prefix=prefix_of_batch(b0, m),
                                   z=None if z is None else z[b0:b0 + m], **kw)
        lq = lq.tolist()
        pre = prefix_of_batch(b0, m)
        for b, t in enumerate(toks):
            assert model.tensor2string(t).startswith(pre if isinstance(pre, str) else pre[b]), (b0 + b, t)    # every row, before the dedup
            key = tuple(t.tolist())
            if key not in index:
                index[key] = len(strings)
                strings.append(model.tensor2string(t)); counts.append(0); logqs.append(lq[b])
            counts[index[key]] += 1
    return strings, counts, logqs


def test_moses_generate_with_a_prefix_equals_a_host_side_dedup_of_sample():
    """Zeros prior, top_k = 2, max_len = 8 with the prefix "CC(": at most 2^4 completions, so duplicates are certain and whole strings are
    what is deduplicated.  Then a list of n prefixes with given latents, consumed batch by batch."""
    model, _ = _model(torch.bfloat16)
    assert model.prior == "zeros"
    n, bs, seed = 300, 128, 40
    res = mv.moses_generate(model, n, batch_size=bs, max_len=8, top_k=2, seed=seed, prefix="CC(")
    strings, counts, logqs = _host_dedup(model, n, bs, seed, lambda b0, m: "CC(", max_len=8, top_k=2)
    assert 2 <= len(strings) <= 16 and all(s.startswith("CC(") for s in strings)
    assert res["total"] == n == sum(res["counts"]) and res["unique"] == len(strings)
    assert res["strings"] == strings and res["counts"] == counts and res["logq"] == logqs
    plain = mv.moses_generate(model, n, batch_size=bs, max_len=8, top_k=2, seed=seed)
    assert plain["strings"] != res["strings"] and plain == mv.moses_generate(model, n, batch_size=bs, max_len=8, top_k=2, seed=seed, prefix=None)
    z = PR.latents(n, seed=14, device=dev)
    prefix = [PREFIXES[b % 7] for b in range(n)]
    r2 = mv.moses_generate(model, n, batch_size=bs, max_len=20, seed=3, z=z, syntax=True, top_k=3, prefix=prefix, count_valid=True)
    strings, counts, logqs = _host_dedup(model, n, bs, 3, lambda b0, m: prefix[b0:b0 + m], z=z, max_len=20, syntax=True, top_k=3)
    assert r2["strings"] == strings and r2["counts"] == counts and r2["logq"] == logqs and r2["valid"] == n
    assert {s[:2] for s in strings} >= {"CC", "c1", "N#", "C["}
    # all prefixes are walked before the first batch: a refusal in a later batch names the sample index and nothing has been sampled
    bad = list(prefix); bad[2 * bs + 5] = "C)"
    with pytest.raises(ValueError, match=rf"row {2 * bs + 5}, position 1: token '\)' is refused"):
        mv.moses_generate(model, n, batch_size=bs, max_len=20, seed=3, z=z, syntax=True, prefix=bad)
