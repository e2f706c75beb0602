"""GPU tests of the latent diagnostics: mvae_gauss_iw_draw, mvae_group_logmeanexp and mvae_gauss_pairwise_lse against float64
(tests/latent_ref.py), VAE.iw_log_likelihood on the g3 model against the float64 decoder of tests/beam_ref.py, and
train.moses_latent_diagnostics against latent_ref computed from the same draws."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import molecular_vae_amd as mv                  # noqa: E402
from molecular_vae_amd import ops               # noqa: E402
from molecular_vae_amd.vocab import pad_batch   # noqa: E402
import latent_ref as LR                         # noqa: E402
import test_gpu_moses_decode as DEC             # noqa: E402  (module import: its tests are not collected here)

dev = torch.device("cuda")


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _seqs(model, n, seed, distinct=False):
    """n molecules of 1 .. 11 letters, sorted by length descending (distinct=True: no two of the same length)."""
    rs = np.random.RandomState(seed)
    lens = rs.permutation(np.arange(1, 12))[:n] if distinct else rs.randint(1, 12, n)
    out = [model.string2tensor("".join(chr(ord("a") + c) for c in rs.randint(0, 26, L)), device="cpu") for L in lens]
    return sorted(out, key=lambda t: -t.numel())


def _normals(seed, offset, shape):
    return np.asarray(ops.normal_draw(seed, offset, int(np.prod(shape)))[0]).reshape(shape)


# ---------------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("dz", [160, 161])
@pytest.mark.parametrize("injected", [False, True])
def test_iw_draw_matches_float64(dz, injected):
    B, K, ld, seed, off = 7, 5, dz + 5, 1234, 77
    rs = np.random.RandomState(dz)
    mu_l, lv_l = rs.standard_normal((B, ld)) * 2, rs.uniform(-6, 3, (B, ld))
    eps64 = rs.standard_normal((B, K, dz)) if injected else _normals(seed, off, (B, K, dz))
    z, logw = torch.empty(B * K, dz, device=dev), torch.empty(B * K, device=dev)
    eps_t = _f32(eps64.reshape(B * K, dz)) if injected else None
    ops.gauss_iw_draw(_f32(mu_l), _f32(lv_l), z, logw, B, K, dz, eps=eps_t, seed=seed, offset=off, ld=ld)
    mu, lv = mu_l.astype(np.float32)[:, :dz].astype(np.float64), lv_l.astype(np.float32)[:, :dz].astype(np.float64)
    if injected:
        e = eps64.astype(np.float32).astype(np.float64)
    else:                                   # the library's fp32 normals on the same counters (mvae_normal_fill: the same device function)
        e = ops.normal_fill(torch.empty(B * K * dz, device=dev), 1.0, seed, off).double().cpu().numpy().reshape(B, K, dz)
        assert np.all(np.abs(e - eps64) <= 1e-4 * (1 + np.abs(eps64)))
    z64, lw64 = LR.iw_draw(mu, lv, e)
    zg, lwg = z.cpu().double().numpy().reshape(B, K, dz), logw.cpu().double().numpy().reshape(B, K)
    assert np.all(np.abs(zg - z64) <= 1e-5 * (np.abs(mu)[:, None] + np.exp(0.5 * lv)[:, None] * np.abs(e)) + 1e-30)
    scale = np.sum(e ** 2 + np.abs(lv)[:, None] + z64 ** 2, -1)
    assert np.all(np.abs(lwg - lw64) <= 1e-5 * scale)


@pytest.mark.parametrize("K", [1, 3, 500, 4097])
def test_group_logmeanexp_matches_float64(K):
    G = 6
    rs = np.random.RandomState(K)
    a, b = rs.uniform(-1e4, 1e4, (G, K)), rs.uniform(-10, 10, (G, K))
    a[1] = -np.inf                                                       # an all -inf group
    if K > 1:
        a[3, K // 2] = np.nan                                            # a NaN stays in its group
    at, bt = _f32(a), _f32(b)
    lme, mean = torch.empty(G, device=dev), torch.empty(G, device=dev)
    ops.group_logmeanexp(at, lme, mean, G, K, b=bt)
    lme2, mean2 = torch.empty(G, device=dev), torch.empty(G, device=dev)
    ops.group_logmeanexp(at, lme2, mean2, G, K, b=bt)
    bits = lambda t: t.view(torch.int32)                                   # bitwise reproducible (NaN included)
    assert torch.equal(bits(lme), bits(lme2)) and torch.equal(bits(mean), bits(mean2))
    v = a.astype(np.float32).astype(np.float64) + b.astype(np.float32).astype(np.float64)
    ref_lme, ref_mean = LR.logsumexp(v, 1) - np.log(K), v.mean(1)
    g_lme, g_mean = lme.cpu().double().numpy(), mean.cpu().double().numpy()
    assert g_lme[1] == -np.inf and g_mean[1] == -np.inf
    ok = [g for g in range(G) if g != 1 and not (K > 1 and g == 3)]
    if K > 1:
        assert np.isnan(g_lme[3]) and np.isnan(g_mean[3])
    assert np.all(np.isfinite(g_lme[ok]))
    assert np.all(np.abs(g_lme[ok] - ref_lme[ok]) <= 1e-6 * np.maximum(1.0, np.abs(ref_lme[ok])) + 1e-5)
    assert np.all(np.abs(g_mean[ok] - ref_mean[ok]) <= 1e-5 * np.abs(v[ok]).mean(1) + 1e-6)
    ops.group_logmeanexp(bt, lme2, mean2, G, K)                          # b = NULL
    assert np.allclose(lme2.cpu().double().numpy(), LR.logsumexp(b.astype(np.float32), 1) - np.log(K), rtol=1e-6, atol=1e-5)


@pytest.mark.parametrize("Nz,Nx,dz", [(1, 1, 1), (63, 257, 160), (4099, 300, 161), (300, 4099, 160)])
def test_gauss_pairwise_lse_matches_float64(Nz, Nx, dz):
    rs = np.random.RandomState(Nz + Nx + dz)
    ldz, ldp = dz + 3, dz + 7
    mu_l = rs.standard_normal((Nx, ldp)) * 1.5
    lv_l = rs.uniform(-20, 5, (Nx, ldp))
    mu, lv = mu_l.astype(np.float32)[:, :dz].astype(np.float64), lv_l.astype(np.float32)[:, :dz].astype(np.float64)
    j = np.arange(Nz) % Nx                                               # points drawn near some of the posteriors, far from the others
    z_l = np.zeros((Nz, ldz))
    z_l[:, :dz] = mu[j] + np.exp(0.5 * lv[j]) * rs.standard_normal((Nz, dz))
    z = z_l.astype(np.float32)[:, :dz].astype(np.float64)
    zt, mut, lvt = _f32(z_l), _f32(mu_l), _f32(lv_l)
    out, out2 = torch.empty(Nz, device=dev), torch.empty(Nz, device=dev)
    ops.gauss_pairwise_lse(zt, mut, lvt, out, Nz, Nx, dz, ldz=ldz, ldp=ldp)
    ops.gauss_pairwise_lse(zt, mut, lvt, out2, Nz, Nx, dz, ldz=ldz, ldp=ldp)
    assert torch.equal(out, out2)                                        # bitwise reproducible
    ref, top = LR.pairwise_lse(z, mu, lv)
    got = out.cpu().double().numpy()
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - ref) <= 1e-5 * np.maximum(1.0, np.abs(top)))


def _pairwise(z, mu, lv, Nz, Nx, dz):
    out = torch.empty(Nz, device=dev)
    ops.gauss_pairwise_lse(_f32(z), _f32(mu), _f32(lv), out, Nz, Nx, dz)
    return out.cpu().double().numpy()


@pytest.mark.parametrize("Nz,Nx", [(300, 4099), (4099, 4099)])
def test_gauss_pairwise_lse_sums_overlapping_posteriors_over_every_slot(Nz, Nx):
    """Posteriors that overlap (mu ~ 0.05 N(0, 1), logvar in [-0.3, 0.3]), as in a model near posterior collapse: the log-sum-exp is
    more than a nat (median ~4 nats) above its largest term, and more than half a nat of it (median ~2) comes from columns over 200 away
    from the largest, i.e. from other slots of the column split (43 and 26 slots here): a kernel returning the max, or a merge that kept
    only the winning slot, is off by far more than the tolerance (~3e-3 here)."""
    dz = 160
    lib = mv._lib.load()
    assert lib.mvae_gauss_pairwise_lse_workspace(Nz, Nx, dz) >= 20 * Nz * 8          # the merge of many slots runs
    rs = np.random.RandomState(Nz + Nx + dz + 1)
    mu = (rs.standard_normal((Nx, dz)) * 0.05).astype(np.float32).astype(np.float64)
    lv = rs.uniform(-0.3, 0.3, (Nx, dz)).astype(np.float32).astype(np.float64)
    j = rs.randint(0, Nx, Nz)
    z = (mu[j] + np.exp(0.5 * lv[j]) * rs.standard_normal((Nz, dz))).astype(np.float32).astype(np.float64)
    lp = LR.gauss_logpdf_pairs(z, mu, lv)
    ref, top, arg = LR.logsumexp(lp, 1), lp.max(1), lp.argmax(1)
    near = np.array([LR.logsumexp(lp[i, max(0, arg[i] - 200):arg[i] + 201]) for i in range(Nz)])
    assert (ref - top).min() > 1.0 and np.median(ref - top) > 3.0 and (ref - near).min() > 0.5      # the test's own premise
    got = _pairwise(z, mu, lv, Nz, Nx, dz)
    assert np.all(np.abs(got - ref) <= 1e-5 * np.maximum(1.0, np.abs(top)))


def test_gauss_pairwise_lse_of_identical_posteriors_is_log_n_above_one():
    """Nx copies of one posterior (a collapsed encoder): out = log N(z; mu, sigma^2) + log Nx, every column of every slot counted once."""
    Nz, Nx, dz = 300, 4099, 160
    rs = np.random.RandomState(8)
    mu1, lv1 = rs.standard_normal(dz) * 0.3, rs.uniform(-1, 0.5, dz)
    mu, lv = np.tile(mu1, (Nx, 1)).astype(np.float32).astype(np.float64), np.tile(lv1, (Nx, 1)).astype(np.float32).astype(np.float64)
    z = (mu[:Nz] + np.exp(0.5 * lv[:Nz]) * rs.standard_normal((Nz, dz))).astype(np.float32).astype(np.float64)
    one = LR.gauss_logpdf_pairs(z, mu[:1], lv[:1])[:, 0]
    got = _pairwise(z, mu, lv, Nz, Nx, dz)
    assert np.all(np.abs(got - (one + np.log(Nx))) <= 1e-5 * np.maximum(1.0, np.abs(one)))


# ---------------------------------------------------------------------------------------------------------------------- iw_log_likelihood
def _enc(model, seqs):
    """mu, logvar [B, d_z] of length-sorted seqs (forward_encoder with eps = 0)."""
    B = len(seqs)
    mu, _, lv = model.forward_encoder([s.to(dev) for s in seqs], eps=torch.zeros(B, model.d_z, device=dev))
    return mu.detach().double().cpu().numpy(), lv.detach().double().cpu().numpy()


def test_iw_single_draw_is_score_plus_log_weight(golden_dir):
    model, _ = DEC._g3_model(golden_dir, torch.float32)
    seqs = _seqs(model, 9, seed=1)
    B, dz = len(seqs), model.d_z
    eps = torch.randn(B, 1, dz, generator=torch.Generator().manual_seed(2))
    log_px, elbo = model.iw_log_likelihood(seqs, n_samples=1, eps=eps)
    assert log_px.shape == (B,) and log_px.dtype == torch.float32 and log_px.device.type == "cuda"
    assert torch.equal(log_px, elbo)
    mu, lv = _enc(model, seqs)
    z = (torch.from_numpy(mu).float() + torch.exp(0.5 * torch.from_numpy(lv).float()) * eps[:, 0]).to(dev)
    e, zd = eps[:, 0].double().numpy(), z.double().cpu().numpy()
    want = model.score(seqs, z).double().cpu().numpy() + 0.5 * np.sum(e ** 2 + lv - zd ** 2, 1)
    assert np.all(np.abs(log_px.double().cpu().numpy() - want) <= 1e-5 * (1 + np.abs(want)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_iw_log_likelihood_matches_float64(golden_dir, dtype):
    """f32: within 1e-4 (1 + |log p|) of the float64 decoder on the same draws; bf16: within 2e-2 per counted token (the bound of
    test_bf16_scores_equal_float64_scores_of_the_chosen_sequences).  log p_K >= elbo_K for every molecule."""
    model, p64 = DEC._g3_model(golden_dir, dtype)
    seqs = _seqs(model, 6, seed=3)
    B, K, dz = len(seqs), 4, model.d_z
    eps = torch.randn(B, K, dz, generator=torch.Generator().manual_seed(4))
    log_px, elbo = model.iw_log_likelihood(seqs, n_samples=K, eps=eps)
    mu, lv = _enc(model, seqs)
    logw, _ = LR.log_weights(p64, [s.numpy() for s in seqs], mu, lv, eps.double().numpy())
    ref_px, ref_elbo = LR.iw_estimates(logw)
    g_px, g_elbo = log_px.double().cpu().numpy(), elbo.double().cpu().numpy()
    if dtype == torch.float32:
        tol = 1e-4 * (1 + np.abs(ref_px))
    else:
        tol = 2e-2 * np.array([s.numel() - 1 for s in seqs])
    assert np.all(np.abs(g_px - ref_px) <= tol) and np.all(np.abs(g_elbo - ref_elbo) <= tol)
    assert np.all(g_px >= g_elbo)


def test_iw_log_likelihood_bound_permutation_and_seeds(golden_dir):
    model, _ = DEC._g3_model(golden_dir, torch.float32)
    seqs = _seqs(model, 8, seed=5, distinct=True)
    a_px, a_elbo = model.iw_log_likelihood(seqs, n_samples=50, seed=9)
    assert torch.all(a_px >= a_elbo) and torch.all(torch.isfinite(a_px))
    b_px, b_elbo = model.iw_log_likelihood(seqs, n_samples=50, seed=9)
    assert torch.equal(a_px, b_px) and torch.equal(a_elbo, b_elbo)         # the same seed: bitwise the same
    c_px, _ = model.iw_log_likelihood(seqs, n_samples=50, seed=10)
    assert not torch.equal(a_px, c_px)
    perm = [3, 0, 7, 5, 1, 6, 2, 4]
    p_px, p_elbo = model.iw_log_likelihood([seqs[i] for i in perm], n_samples=50, seed=9)
    assert torch.equal(p_px, a_px[perm]) and torch.equal(p_elbo, a_elbo[perm])
    strings = [model.tensor2string(s) for s in seqs]
    s_px, _ = model.iw_log_likelihood(strings, n_samples=50, seed=9)
    assert torch.equal(s_px, a_px)
    counter = model.noise_stream.state()["counter"]
    d_px, _ = model.iw_log_likelihood(seqs, n_samples=50)
    e_px, _ = model.iw_log_likelihood(seqs, n_samples=50)
    assert not torch.equal(d_px, e_px) and model.noise_stream.state()["counter"] == counter + 2 * 8 * 50 * model.d_z


def test_iw_log_likelihood_over_the_row_budget_matches_single_molecule_calls(golden_dir):
    """B * K = 12 000 rows: several decoder passes of whole molecules; K = 5 000: one molecule's draws over several passes."""
    model, _ = DEC._g3_model(golden_dir, torch.float32)
    seqs = _seqs(model, 40, seed=6)
    B, K, dz = 40, 300, model.d_z
    eps = torch.randn(B, K, dz, generator=torch.Generator().manual_seed(7))
    log_px, elbo = model.iw_log_likelihood(seqs, n_samples=K, eps=eps)
    one = [model.iw_log_likelihood([seqs[b]], n_samples=K, eps=eps[b:b + 1]) for b in range(B)]
    px1, el1 = torch.cat([o[0] for o in one]), torch.cat([o[1] for o in one])
    assert torch.allclose(log_px, px1, rtol=1e-5, atol=0) and torch.allclose(elbo, el1, rtol=1e-5, atol=0)
    K2 = 5000
    eps2 = torch.randn(2, K2, dz, generator=torch.Generator().manual_seed(8))
    px, el = model.iw_log_likelihood(seqs[:2], n_samples=K2, eps=eps2)
    h = [model.iw_log_likelihood(seqs[:2], n_samples=K2 // 2, eps=eps2[:, i * (K2 // 2):(i + 1) * (K2 // 2)]) for i in range(2)]
    want_px = torch.logaddexp(h[0][0].double(), h[1][0].double()) - math.log(2)
    assert torch.allclose(px.double(), want_px, rtol=1e-5, atol=0)
    assert torch.allclose(el.double(), (h[0][1].double() + h[1][1].double()) / 2, rtol=1e-5, atol=0)


# ---------------------------------------------------------------------------------------------------------------------- diagnostics
def test_moses_latent_diagnostics_match_latent_ref(golden_dir):
    model, p64 = DEC._g3_model(golden_dir, torch.float32)
    model.train()
    batches = [_seqs(model, 12, seed=11), _seqs(model, 9, seed=12)]
    K, seed, dz = 6, 21, model.d_z
    res = mv.moses_latent_diagnostics(model, batches, n_samples=K, seed=seed)
    assert model.training
    assert set(res) == {"n_molecules", "n_tokens", "nll", "nll_per_token", "ppl", "elbo", "kl", "mi", "au"}
    assert all(isinstance(v, float) for v in res.values())
    mus, lvs, nll, elbo, off = [], [], [], [], 0
    for seqs in batches:                                   # length-sorted batches: draw row b*K + k is molecule b's k-th draw
        mu, lv = _enc(model, seqs)
        eps = _normals(seed, off, (len(seqs), K, dz))
        off += len(seqs) * K * dz
        logw, _ = LR.log_weights(p64, [s.numpy() for s in seqs], mu, lv, eps)
        px, el = LR.iw_estimates(logw)
        nll.append(-px); elbo.append(el); mus.append(mu); lvs.append(lv)
    mu, lv = np.concatenate(mus), np.concatenate(lvs)
    N = mu.shape[0]
    zt, lw = torch.empty(N, dz, device=dev), torch.empty(N, device=dev)          # the draw kernel (held to float64 above) on the same counters
    ops.gauss_iw_draw(_f32(mu), _f32(lv), zt, lw, N, 1, dz, seed=seed, offset=off)
    z = zt.double().cpu().numpy()
    ntok = sum(s.numel() - 1 for b in batches for s in b)
    nll = np.concatenate(nll)
    assert res["n_molecules"] == N and res["n_tokens"] == ntok
    assert abs(res["nll_per_token"] - nll.sum() / ntok) <= 1e-4 * abs(nll.sum() / ntok)
    assert abs(res["nll"] - nll.mean()) <= 1e-4 * abs(nll.mean()) and abs(res["ppl"] - math.exp(res["nll_per_token"])) < 1e-9 * res["ppl"]
    assert abs(res["elbo"] - np.concatenate(elbo).mean()) <= 1e-4 * abs(np.concatenate(elbo).mean())
    assert abs(res["kl"] - LR.kl(mu, lv)) <= 1e-9 * abs(LR.kl(mu, lv))
    assert res["au"] == LR.active_units(mu)
    _, top = LR.pairwise_lse(z, mu, lv)
    assert abs(res["mi"] - LR.mutual_info(mu, lv, z)) <= 1e-5 * max(1.0, float(np.abs(top).mean()))
    model.eval()
    mv.moses_latent_diagnostics(model, batches[:1], n_samples=2, seed=seed)
    assert not model.training


def test_moses_latent_diagnostics_counts_active_units_and_takes_padded_batches(golden_dir):
    """The g3 encoder's mu varies by ~4e-4 per dimension (no active unit): 40 rows of its last q_mu layer scaled by 30 make about 40
    dimensions active, which `au` must count as latent_ref does.  Device PaddedBatches give the same results as id lists."""
    model, _ = DEC._g3_model(golden_dir, torch.float32)
    with torch.no_grad():
        model.q_mu[2].weight[:40].mul_(30.0)
    mv._lib.PARAM_EPOCH[0] += 1
    batches = [_seqs(model, 16, seed=13), _seqs(model, 16, seed=14)]
    res = mv.moses_latent_diagnostics(model, batches, n_samples=3, seed=4)
    mu = np.concatenate([_enc(model, b)[0] for b in batches])
    au = LR.active_units(mu)
    assert 0 < au < model.d_z and res["au"] == au
    padded = [pad_batch([s.to(dev) for s in b], model.pad) for b in batches]
    assert padded[0].lengths.is_cuda
    assert mv.moses_latent_diagnostics(model, padded, n_samples=3, seed=4) == res
