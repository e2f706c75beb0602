"""GPU tests of syntax-constrained decoding (mvae_moses_beam_syntax_step, VAE.decode(syntax=True), moses_reconstruction(syntax=True))
against tests/beam_syntax_ref.py (the float64 decoder of beam_ref under the plain-Python automaton of syntax_ref) and the independently
written validator of syntax_ref.  The mask, the automaton states and the bookkeeping are integer logic: those assertions have no
tolerance.  Decisions are compared with float64 where the float64 margin exceeds 1e-4, as in test_gpu_moses_decode.py."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import molecular_vae_amd as mv                  # noqa: E402
from molecular_vae_amd import _lib as L, mosesvae as MV, vocab as VC, ops   # noqa: E402
from oracle import initparams as ip             # noqa: E402
import beam_ref as BR                           # noqa: E402
import beam_syntax_ref as BS                    # noqa: E402
import syntax_ref as SY                         # noqa: E402

dev = torch.device("cuda")
ALPHABET = "CNOSFcnos()=#123[]@H+-lBr"          # data.synthetic_smiles' alphabet: V = 29 with the four specials
N_ATOMS = 10                                     # C N O S F c n o s B
MARGIN = 1e-4
GOOD = ["CCO", "c1ccccc1", "CC(=O)Oc1ccccc1C(=O)O", "CN1CCC[C@H]1c2cccnc2", "O=C(O)c1ccccc1", "C1CC1", "N#Cc1ccc(Br)cc1",
        "CC(C)Cc1ccc(cc1)[C@@H](C)C(=O)O", "C[N+](C)(C)C", "[O-]C", "ClC(Cl)Cl"]


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


def _model(dtype):
    """The model of test_gpu_smiles_syntax.py: a mosesvae.VAE over the synthetic_smiles vocabulary with seeded random weights (eval mode),
    and the weights in float64."""
    v = _vocab()
    if "p" not in _PARAMS:
        _PARAMS["p"] = ip.init_params(ip.moses_shapes(len(v)), 303, 1.5, np.float32)
    params = _PARAMS["p"]
    model = MV.VAE(v, dtype=dtype)
    sd = {k: torch.from_numpy(params[k]) for k in params}
    model.load_state_dict({k: sd[_moses_base(k)] for k in model.state_dict()})
    return model.to(dev).eval(), {k: p.astype(np.float64) for k, p in params.items()}


def _latents(B, seed=0, scale=1.0):
    rs = np.random.RandomState(seed)
    return torch.from_numpy((rs.standard_normal((B, 160)) * scale).astype(np.float32)).to(dev)


def _finite_rows_check(model, ids, ends, scores, max_len):
    """Every hypothesis with a finite score is well-formed (device check and independent validator), has <eos> at end - 1 and pad after
    its end; beam 0 is finite; scores are non-increasing with -inf last.  Returns the finite mask [B, K] (numpy)."""
    B, K, Lm = ids.shape
    assert Lm == max_len
    ok_dev = model.syntax_valid(ids.view(B * K, max_len)).view(B, K).cpu().numpy()
    xs, es, sc = ids.cpu().numpy(), ends.cpu().numpy(), scores.cpu().numpy().astype(np.float64)
    finite = np.isfinite(sc)
    assert not np.isnan(sc).any() and (sc[~finite] == -np.inf).all()
    assert finite[:, 0].all()
    s = np.where(finite, sc, -1e300)
    assert (s[:, 1:] <= s[:, :-1]).all()
    assert (xs[:, :, 0] == model.bos).all()
    for b in range(B):
        for k in range(K):
            if not finite[b, k]:
                continue
            e = es[b, k]
            assert ok_dev[b, k] and SY.row_valid(xs[b, k], model.vocabulary), (b, k, xs[b, k])
            assert 3 <= e <= max_len and xs[b, k, e - 1] == model.eos and (xs[b, k, e:] == model.pad).all(), (b, k, xs[b, k])
    return finite


# ---------------------------------------------------------------------------------------------- 1. the launch alone on fixed logits
# (max_len, step) of the launches: 0, 1, 3 and 50 tokens left after the one being chosen
LAUNCHES = ((15, 14), (9, 7), (13, 9), (64, 13))
END_STATE = (SY.END, 0, 0, 0, "$")
ERROR_WORDS = (SY.ERROR | 0xFF << 16, 0)


def _prefix_state(chars, n, left, rs):
    """A state n random legal tokens away from START from which the string can still be finished in left + 1 tokens."""
    st = SY.S0
    for i in range(1, n + 1):
        al = [t for t in SY.allowed_ids(st, chars, (n - i) + left + 1) if chars[t] != "$"]
        assert al, (st, n, left)
        st = SY.step(st, chars[al[rs.randint(len(al))]])
    assert SY.need(st) <= left + 1
    return st


def _launch_rows(B, K, max_len, step, chars, rs):
    """Per row: (automaton state or None for ERROR, fin, score, end).  About 15 % finished rows (state END, an end before this step),
    15 % dead rows (score -inf; half of them in ERROR), the rest active on a random legal prefix of 0-12 tokens."""
    left = max_len - 1 - step
    rows = []
    for _ in range(B * K):
        u = rs.rand()
        if u < 0.15:
            rows.append((END_STATE, 1, -5.0 * rs.rand(), int(rs.randint(3, step + 1))))
            continue
        n = int(rs.randint(0, 13))
        st = _prefix_state(chars, max(n, 1) if left == 0 else n, left, rs)
        if u < 0.30:
            rows.append((None if rs.rand() < 0.5 else st, 0, -np.inf, max_len))
        else:
            rows.append((st, 0, -5.0 * rs.rand(), max_len))
    return rows


def _pack(st, v):
    return ERROR_WORDS if st is None else SY.pack_state(st, v)


def _launch_reference(rows, logp, B, K, left, chars, v):
    """Per molecule: the K selected (score, parent, token) in the kernel's order, dead slots (-inf, 0, pad) last, and the margin."""
    out = []
    for m in range(B):
        cands, full = [], []
        for k in range(K):
            st, fin, sc, _ = rows[m * K + k]
            if fin:
                cands.append((sc, k, v.pad)); full.append(sc)
                continue
            al = [] if st is None else SY.allowed_ids(st, chars, left)
            c = sc + logp[m * K + k]
            full.extend(c[al].tolist())
            for t in sorted(al, key=lambda t: (-c[t], t))[:K]:
                cands.append((c[t], k, t))
        cands.sort(key=lambda t: (-t[0], t[1], t[2]))
        top = [t for t in sorted(full, reverse=True)[:K + 1] if np.isfinite(t)]
        margin = float(np.min(-np.diff(top))) if len(top) > 1 else np.inf
        n_real = min(K, len(cands))
        out.append((cands[:K] + [(-np.inf, 0, v.pad)] * (K - n_real), n_real, margin))
    return out


def test_beam_syntax_launch_on_fixed_logits():
    """One layer, H = 64, w_fc = the first V rows of the identity: row r's logits are h[r, :V].  B = 5 molecules, K in {1, 3, 16}, every row
    with its own automaton state, some finished and some dead, at launches leaving 0, 1, 3 and 50 tokens.  Against numpy: the surviving
    (parent, token) pairs and their order where the float64 margin exceeds 1e-4, scores to 1e-5; with no tolerance gstate, add_out,
    hist_tok, hist_par, fin, ends and the reordered recurrent state; two runs bit-identical; outputs NaN-filled first."""
    v = _vocab()
    chars, info = SY.token_chars(v), VC.smiles_token_table(v).to(dev)
    V, H, ldh, W, B = len(v), 64, 72, 128, 5
    rs = np.random.RandomState(11)
    wfc = torch.eye(H, device=dev)[:V].contiguous()
    table = torch.from_numpy(rs.standard_normal((V, W)).astype(np.float32)).to(dev)
    seen_states, n_cmp, n_mol, n_fin, n_dead, n_deadslot, worst = [], 0, 0, 0, 0, 0, 0.0
    for K in (1, 3, 16):
        R = B * K
        assert K == 16 or R % 4 != 0                                         # K = 1: 4 molecules per pass and a short last pass
        base = torch.from_numpy(rs.standard_normal((R, W)).astype(np.float32)).to(dev)
        for max_len, step in LAUNCHES:
            left = max_len - 1 - step
            rows = _launch_rows(B, K, max_len, step, chars, rs)
            seen_states += [r[0] for r in rows if r[0] is not None and r[0] != END_STATE]
            n_fin += sum(r[1] for r in rows); n_dead += sum(1 for r in rows if r[2] == -np.inf)
            h1 = rs.standard_normal((R, ldh)).astype(np.float32)
            h1[:, :V] *= 2.0
            logits = h1[:, :V].astype(np.float64)
            mx = logits.max(1, keepdims=True)
            logp = logits - (mx + np.log(np.exp(logits - mx).sum(1, keepdims=True)))
            ref = _launch_reference(rows, logp, B, K, left, chars, v)
            g_old = np.array([_pack(r[0], v) for r in rows], np.int32).reshape(R, 2)
            fin_old = np.array([r[1] for r in rows], np.uint8)
            sc_old = np.array([r[2] for r in rows], np.float32)
            end_old = np.array([r[3] for r in rows], np.int64)
            runs = []
            for _ in range(2):
                state = torch.full((1, 2, R, ldh), float("nan"), device=dev)
                state[0, 1] = torch.from_numpy(h1).to(dev)
                add = torch.full((R, W), float("nan"), device=dev)
                score, fin, ends = torch.from_numpy(sc_old).to(dev), torch.from_numpy(fin_old).to(dev), torch.from_numpy(end_old).to(dev)
                hist_tok = torch.full((max_len, R), -7, dtype=torch.int32, device=dev)
                hist_par = torch.full((max_len, R), -7, dtype=torch.int32, device=dev)
                gstate = torch.from_numpy(g_old).to(dev)
                ops.moses_beam_syntax_step(state, ldh, wfc, None, step, v.eos, v.pad, table, base, add, score, fin, ends, hist_tok, hist_par,
                                           B, K, V, H, info, gstate, max_len)
                torch.cuda.synchronize()
                runs.append((state, add, score, fin, ends, hist_tok, hist_par, gstate))
            for x, y in zip(*runs):
                assert torch.equal(x.view(torch.int32) if x.is_floating_point() else x, y.view(torch.int32) if y.is_floating_point() else y)
            state, add, score, fin, ends, hist_tok, hist_par, gstate = runs[0]
            ht, hp = hist_tok.cpu().numpy(), hist_par.cpu().numpy()
            assert (np.delete(ht, step, 0) == -7).all() and (np.delete(hp, step, 0) == -7).all()
            tok, par = ht[step].astype(np.int64), hp[step].astype(np.int64)
            sc, fn, en, gn = score.cpu().numpy(), fin.cpu().numpy(), ends.cpu().numpy(), gstate.cpu().numpy()
            assert ((tok >= 0) & (tok < V) & (par >= 0) & (par < K)).all() and not np.isnan(sc).any()
            assert torch.equal(add, table[torch.from_numpy(tok).to(dev)] + base)
            src = (np.arange(R) // K) * K + par                                   # the parent's row
            assert torch.equal(state[0, 0, :, :H], state[0, 1, torch.from_numpy(src).to(dev), :H])
            assert torch.equal(state[0, 1], torch.from_numpy(h1).to(dev))
            for r in range(R):
                m, p = r // K, int(par[r])
                pst, pfin, _, pend = rows[src[r]]
                sel, n_real, margin = ref[m]
                live = np.isfinite(sc[r])
                if pfin:
                    assert tok[r] == v.pad and fn[r] == 1 and en[r] == pend and tuple(gn[r]) == tuple(g_old[src[r]]), r
                else:
                    if live:
                        assert pst is not None and tok[r] in SY.allowed_ids(pst, chars, left), (r, pst, tok[r])
                    nxt = SY.step(pst, chars[tok[r]]) if (pst is not None and chars[tok[r]] is not None) else None
                    if nxt is None:
                        assert not live and (gn[r, 0] & 0xFF) == SY.ERROR, (r, gn[r])
                    else:
                        assert tuple(gn[r]) == SY.pack_state(nxt, v), (r, pst, tok[r], gn[r])
                    assert fn[r] == (1 if tok[r] == v.eos else 0) and en[r] == (step + 1 if tok[r] == v.eos else pend), r
                    if left == 0 and live:
                        assert tok[r] == v.eos
            for m in range(B):
                sel, n_real, margin = ref[m]
                n_mol += 1
                n_deadslot += K - n_real
                got = sc[m * K:(m + 1) * K]
                assert (got[n_real:] == -np.inf).all()                            # a slot without a candidate is dead
                if margin <= MARGIN:
                    continue
                n_cmp += 1
                for k in range(n_real):
                    s, p, t = sel[k]
                    t = v.pad if rows[m * K + p][1] else t
                    assert (par[m * K + k], tok[m * K + k]) == (p, t), (K, max_len, step, m, k)
                    if np.isfinite(s):
                        worst = max(worst, abs(float(got[k]) - s))
                    else:
                        assert got[k] == -np.inf
    modes = {s[0] for s in seen_states}
    assert modes >= {SY.START, SY.ATOM, SY.RING, SY.BOND, SY.OPEN, SY.CLOSE, SY.KOPEN, SY.KSYM}, modes
    assert any(s[1] > 1 for s in seen_states) and any(bin(s[2]).count("1") > 1 for s in seen_states) and any(s[3] for s in seen_states)
    print(f"molecules {n_mol}, compared {n_cmp}, finished rows {n_fin}, dead rows {n_dead}, dead slots {n_deadslot}, max score error {worst:.2e}")
    assert n_fin >= 10 and n_dead >= 10 and n_deadslot >= 1
    assert n_cmp >= 0.8 * n_mol, (n_cmp, n_mol)
    assert worst < 1e-5, worst


# ---------------------------------------------------------------------------------------------- 2. refusals
def test_beam_syntax_step_refusals_leave_the_outputs_untouched():
    """Each refusal returns its code before anything is enqueued: the outputs stay NaN-filled / as they were."""
    v = _vocab()
    V, H, ldh, W, B, K, max_len = len(v), 64, 72, 128, 3, 2, 10
    R = B * K
    lib = L.load()
    t = dict(state=torch.full((1, 2, R, ldh), float("nan"), device=dev), wfc=torch.eye(H, device=dev)[:V].contiguous(),
             table=torch.zeros(V, W, device=dev), base=torch.zeros(R, W, device=dev), add=torch.full((R, W), float("nan"), device=dev),
             score=torch.full((R,), float("nan"), device=dev), fin=torch.zeros(R, dtype=torch.uint8, device=dev),
             ends=torch.full((R,), max_len, dtype=torch.long, device=dev), ht=torch.full((max_len, R), -7, dtype=torch.int32, device=dev),
             hp=torch.full((max_len, R), -7, dtype=torch.int32, device=dev), info=VC.smiles_token_table(v).to(dev),
             gs=torch.full((R, 2), -7, dtype=torch.int32, device=dev))
    before = {k: x.clone() for k, x in t.items()}
    torch.cuda.synchronize()

    def call(dtype=L.MVAE_F32, B=B, K=K, V=V, H=H, layers=1, ldh=ldh, ldw=H, step=1, eos=v.eos, pad=v.pad, W=W, max_len=max_len, **null):
        p = {k: (None if k in null else L.ptr(x)) for k, x in t.items()}
        return lib.mvae_moses_beam_syntax_step(dtype, B, K, V, H, layers, p["state"], 2 * R * ldh, R * ldh, ldh, p["wfc"], ldw, None, step, eos, pad,
                                               p["table"], W, p["base"], p["add"], p["score"], p["fin"], p["ends"], p["ht"], p["hp"], p["info"],
                                               p["gs"], max_len, L.stream_ptr())
    INV, UNS = -1, -3
    # what mvae_moses_beam_step refuses
    for name in ("state", "wfc", "table", "base", "add", "score", "fin", "ends", "ht", "hp"):
        assert call(**{name: True}) == INV, name
    assert call(dtype=7) == INV and call(B=0) == INV and call(V=0) == INV and call(H=0) == INV and call(layers=0) == INV
    assert call(ldh=H - 1) == INV and call(ldw=H - 1) == INV and call(W=6) == INV and call(W=0) == INV and call(step=0) == INV
    assert call(K=0) == INV and call(K=17) == INV and call(K=5, V=4) == INV
    assert call(eos=V) == INV and call(eos=-1) == INV and call(pad=V) == INV and call(pad=-1) == INV
    # its own
    assert call(info=True) == INV and call(gs=True) == INV
    assert call(max_len=2) == INV and call(max_len=0) == INV
    assert call(step=-1) == INV and call(step=max_len) == INV and call(step=max_len + 1) == INV
    assert call(V=65, K=1, eos=1, pad=2) == UNS and call(V=64, H=1024, ldh=1024, ldw=1024) == UNS
    torch.cuda.synchronize()
    for k, x in t.items():
        a, b = (x.view(torch.int32), before[k].view(torch.int32)) if x.is_floating_point() else (x, before[k])
        assert torch.equal(a, b), k


# ---------------------------------------------------------------------------------------------- 3. end to end against float64
_REF = {}


def _reference(p64, v, z, K, max_len):
    key = (K, max_len)
    if key not in _REF:
        _REF[key] = [BS.beam_search(p64, zb, K, max_len, v) for zb in z]
    return _REF[key]


@pytest.mark.parametrize("K", [1, 3, 4])
@pytest.mark.parametrize("max_len", [3, 4, 12])
def test_constrained_beam_search_matches_float64_reference(K, max_len):
    """f32, B = 7: ids, ends and scores (1e-4) equal the float64 constrained beam search on every molecule whose decision margins all
    exceed 1e-4; at least 5 of the 7 molecules are compared (the reference alone gives 7 of 7, 6 of 7 at (3, 12) and (4, 12))."""
    model, p64 = _model(torch.float32)
    B = 7
    z = _latents(B, seed=2, scale=0.7)
    ids, ends, scores = model._beam_search(z, K, max_len, syntax=True)
    finite = _finite_rows_check(model, ids, ends, scores, max_len)
    toks, sc = model.decode(z, beam_width=K, max_len=max_len, return_tokens=True, syntax=True)
    strings, best = model.decode(z, beam_width=K, max_len=max_len, syntax=True)
    assert torch.equal(sc, scores) and torch.equal(best, scores[:, 0])
    assert strings == [model.tensor2string(t[0]) for t in toks] and all(SY.valid_smiles(s) for s in strings)
    ref = _reference(p64, model.vocabulary, z.double().cpu().numpy(), K, max_len)
    compared = 0
    for b in range(B):
        rid, rend, rsc, margin = ref[b]
        print(f"K={K} max_len={max_len} molecule {b}: margin {margin:.3e}")
        if margin <= MARGIN:
            continue
        compared += 1
        for k in range(K):
            if not np.isfinite(rsc[k]):
                assert not finite[b, k], (b, k)
                continue
            assert int(ends[b, k]) == rend[k], (b, k)
            assert np.array_equal(ids[b, k].cpu().numpy(), rid[k]), (b, k)
            assert torch.equal(toks[b][k], torch.from_numpy(rid[k][:rend[k]])), (b, k)
            assert abs(float(scores[b, k]) - rsc[k]) < 1e-4, (b, k, float(scores[b, k]), rsc[k])
    assert compared >= 5, compared


# ---------------------------------------------------------------------------------------------- 4. invariants
@pytest.mark.parametrize("K", [8, 16])
@pytest.mark.parametrize("max_len", [3, 20])
def test_constrained_decode_invariants(K, max_len):
    """bf16, B = 37: every finite hypothesis is well-formed, ends in <eos> and is padded after it; beam 0 is finite; scores are sorted
    with -inf last; at K = 16, max_len = 3 exactly the alphabet's 10 atoms give a hypothesis; reruns are bit-equal; the same latents
    without the constraint give an ill-formed best hypothesis (the test can fail)."""
    model, _ = _model(torch.bfloat16)
    B = 37
    z = _latents(B, seed=5)
    a = model._beam_search(z, K, max_len, syntax=True)
    b = model._beam_search(z, K, max_len, syntax=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    finite = _finite_rows_check(model, *a, max_len)
    if K == 16 and max_len == 3:
        assert (finite.sum(1) == N_ATOMS).all(), finite.sum(1)
    if max_len == 20:
        assert finite.all()
    free = model._beam_search(z, K, max_len)
    assert not bool(model.syntax_valid(free[0][:, 0]).all())
    assert not all(SY.row_valid(r, model.vocabulary) for r in free[0][:, 0].cpu().numpy())


# ---------------------------------------------------------------------------------------------- 5. scores
def test_f32_scores_agree_with_score():
    """The constrained score is not renormalised: it is log p(tokens | z) as VAE.score reports it (1e-4)."""
    model, _ = _model(torch.float32)
    B, K = 6, 3
    z = _latents(B, seed=4, scale=0.7)
    toks, scores = model.decode(z, beam_width=K, max_len=14, return_tokens=True, syntax=True)
    keep = [(b, k) for b in range(B) for k in range(K) if np.isfinite(float(scores[b, k]))]
    assert len(keep) == B * K
    got = model.score([toks[b][k] for b, k in keep], z[[b for b, _ in keep]])
    want = torch.stack([scores[b, k] for b, k in keep])
    assert float((got - want).abs().max()) < 1e-4


def test_bf16_scores_equal_float64_scores_of_the_chosen_sequences():
    """bf16: each finite score is the float64 teacher-forced log p of the sequence the GPU chose, within 2e-2 per counted token (the
    bound of test_gpu_moses_decode.py: bf16 keeps 8 significant bits on the weights and on the hidden state the head reads; with
    |logits| of a few units that moves each log-softmax by ~1e-2 at most, and the errors of successive tokens add up)."""
    model, p64 = _model(torch.bfloat16)
    z = _latents(7, seed=3, scale=0.7)
    toks, scores = model.decode(z, beam_width=4, max_len=12, return_tokens=True, syntax=True)
    worst = 0.0
    for b in range(7):
        for k in range(4):
            s = float(scores[b, k])
            assert np.isfinite(s)
            ids = toks[b][k].numpy()
            lp, _, _ = BR.teacher_forced(p64, z[b].double().cpu().numpy(), ids)
            worst = max(worst, abs(s - lp.sum()) / (len(ids) - 1))
    print(f"worst per-token score error {worst:.3e}")
    assert worst < 2e-2, worst


# ---------------------------------------------------------------------------------------------- 6. launch count
def test_constrained_decode_launches_four_kernels_per_token():
    """Per generated token ONE GRU wavefront pass (3 launches) + exactly ONE beam launch; one finalize launch."""
    model, _ = _model(torch.bfloat16)
    z = _latents(64, seed=6)
    model.decode(z, beam_width=4, max_len=6, syntax=True)                             # warm
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        model.decode(z, beam_width=4, max_len=26, syntax=True)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert sum(1 for n_ in names if "moses_beam_step" in n_) == 25, sorted(set(names))
    steps = sum(1 for n_ in names if "gru_step" in n_ or "lstm_step" in n_ or "step_fwd" in n_)
    assert steps == 3 * 25, (steps, sorted(set(names)))
    assert sum(1 for n_ in names if "moses_beam_finalize" in n_) == 1


# ---------------------------------------------------------------------------------------------- 7. reconstruction
def test_moses_reconstruction_with_syntax_equals_decode_and_score_by_hand():
    model, _ = _model(torch.float32)
    collate = VC.get_collate_fn(model.vocabulary)
    batches = [collate(GOOD[:5]), collate(GOOD[5:])]
    dec, _ = model.decode(_latents(4, seed=9), max_len=20, syntax=True)          # what the model itself decodes can come back exactly
    batches.append(collate(dec))
    frac, mean_lp = mv.moses_reconstruction(model, batches, beam_width=2, max_len=30, syntax=True)
    hits, lps, n = 0, [], 0
    for batch in batches:
        with torch.no_grad():
            mu, _, _ = model.forward_encoder(batch, eps=torch.zeros(len(batch), model.d_z, device=dev))
        strings, _ = model.decode(mu, beam_width=2, max_len=30, syntax=True)
        assert all(SY.valid_smiles(s) for s in strings)
        hits += sum(s == model.tensor2string(x) for s, x in zip(strings, batch))
        lps.append(model.score(batch, mu).double())
        n += len(batch)
    assert frac == hits / n
    assert abs(mean_lp - float(torch.cat(lps).sum()) / n) < 1e-9 * abs(mean_lp)
    assert mean_lp < 0
    plain = mv.moses_reconstruction(model, batches, beam_width=2, max_len=30)
    assert plain == mv.moses_reconstruction(model, batches, beam_width=2, max_len=30, syntax=False) and plain[1] == mean_lp


# ---------------------------------------------------------------------------------------------- 8. at scale
def test_constrained_decode_at_scale():
    """B = 1024, K = 8, max_len = 100 (bf16) completes; every finite hypothesis passes syntax_valid and beam 0 is finite."""
    model, _ = _model(torch.bfloat16)
    z = _latents(1024, seed=7)
    ids, ends, scores = model._beam_search(z, 8, 100, syntax=True)
    torch.cuda.synchronize()
    assert ids.shape == (1024, 8, 100)
    finite = torch.isfinite(scores)
    assert bool(finite[:, 0].all()) and not bool(torch.isnan(scores).any())
    ok = model.syntax_valid(ids.view(1024 * 8, 100)).view(1024, 8)
    assert bool(ok[finite].all())
    e = ends[finite]
    assert bool(((e >= 3) & (e <= 100)).all()) and bool((ids[finite].gather(1, (e - 1)[:, None])[:, 0] == model.eos).all())


# ---------------------------------------------------------------------------------------------- 9. the f32 head above 64 KB of LDS
def test_f32_vocabulary_of_40_tokens_opts_into_large_lds():
    """f32, V = 40 (the alphabet plus 11 characters outside the grammar): the head takes 80 KB of LDS, so the syntax instantiations need
    their own opt-in.  The decode completes with every invariant holding, and the characters outside the grammar are never emitted."""
    extra = "XYZWQJKMTUV"
    v = VC.OneHotVocab(set(ALPHABET) | set(extra))
    assert len(v) == 40
    torch.manual_seed(40)
    model = MV.VAE(v, dtype=torch.float32).to(dev).eval()
    z = _latents(5, seed=40, scale=2.0)
    ids, ends, scores = model._beam_search(z, 4, 10, syntax=True)
    finite = _finite_rows_check(model, ids, ends, scores, 10)
    assert finite.all()
    assert not np.isin(ids.cpu().numpy(), [v.c2i[c] for c in extra] + [v.unk]).any()

