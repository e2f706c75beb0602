"""CPU tests of the replicated-batch step reference in gpu_helpers (what tests/test_gpu_step_sizes.py measures the large-batch steps with):
the layout of the copies at the five batch sizes, the invariance the reference rests on (a batch of D molecules x B / D copies has the loss
and the parameter gradients of the D-row batch, and its rows are the D rows repeated), and two deliberately wrong steps that the checker
must refuse."""
import numpy as np
import pytest

import gpu_helpers as gh
from gpu_helpers import O, rel

D = gh.STEP_D
SMALL_B, SMALL_L = 48, 120


@pytest.mark.parametrize("B,L", gh.STEP_SHAPES, ids=[f"B{b}" for b, _ in gh.STEP_SHAPES])
def test_copies_of_a_molecule_sit_at_no_fixed_distance(B, L):
    """A kernel that reads the wrong row must meet a different molecule.  Offset condition: for every row offset k the share of rows r with
    mol[r] == mol[(r + k) % B] is at most 1/8.  Block condition: no aligned block of 16 rows holds more than 8 copies of one molecule."""
    idx, eps, mol = gh.replicated_batch(D, B, L, gh.FULL["c"], 1000 + B)
    assert idx.shape == (B, L) and idx.dtype == np.int64 and eps.shape == (B, gh.FULL["o"]) and eps.dtype == np.float32 and mol.shape == (B,)
    assert (np.bincount(mol, minlength=D) == B // D).all()
    first = np.array([int(np.flatnonzero(mol == m)[0]) for m in range(D)])
    assert np.array_equal(idx, idx[first][mol]) and np.array_equal(eps, eps[first][mol])          # rows of one molecule are equal ...
    assert len({idx[r].tobytes() for r in first}) == D and len({eps[r].tobytes() for r in first}) == D      # ... and the D molecules differ
    assert 0.5e-2 < eps.std() < 2e-2
    share = max(float((mol == np.roll(mol, -k)).mean()) for k in range(1, B))
    assert share <= 1 / 8, share
    worst = max(int(np.bincount(mol[s:s + 16], minlength=D).max()) for s in range(0, B, 16))
    assert worst <= 8, worst
    again = gh.replicated_batch(D, B, L, gh.FULL["c"], 1000 + B)
    assert all(np.array_equal(a, b) for a, b in zip((idx, eps, mol), again))


def test_copies_make_float32_summation_errors_add_up():
    """Why the f32 weight-gradient errors of test_gpu_step_sizes.py grow in proportion to B and are still no defect: the copies of a row
    contribute bit-identical terms to a contraction over the T*B rows, and an f32 accumulator that stays in one binade rounds identical
    addends identically, so the copies' rounding errors add up where those of distinct rows cancel.  A sequential float32 sum over
    K = 120 * 128 same-sign terms: the replicated layout errs several times more than distinct rows, both far inside the bound of 5e-4."""
    T, B, N = 120, 128, 200
    rs = np.random.RandomState(0)

    def err(x):
        s64 = x.astype(np.float64).sum(0)
        return float(np.abs(np.cumsum(x, axis=0, dtype=np.float32)[-1] - s64).max() / np.abs(s64).max())
    _, _, mol = gh.replicated_batch(D, B, 4, gh.FULL["c"], 1000 + B)
    base = ((1 + 0.3 * rs.standard_normal((T, D, N))) / B).astype(np.float32)
    distinct = ((1 + 0.3 * rs.standard_normal((T * B, N))) / B).astype(np.float32)
    e_rep, e_dis = err(base[:, mol, :].reshape(T * B, N)), err(distinct)
    print(f"sequential f32 sum over K = {T * B}: replicated rows {e_rep:.1e}, distinct rows {e_dis:.1e}")
    assert 2 * e_dis < e_rep < 5e-4 and e_dis < 4 * np.sqrt(T * B) * 2.0 ** -24


@pytest.fixture(scope="module")
def small():
    """One 16-row oracle call (the shared reference) and one 48-row call on the replicated batch, at the full dims."""
    sr = gh.step_reference(SMALL_B, SMALL_L)
    full = O.molvae_loss_and_grads({k: v.astype(np.float64) for k, v in sr["params"].items()}, sr["idx"], sr["eps"].astype(np.float64),
                                   max_len=SMALL_L, num_lstm=gh.FULL["n_enc"], num_gru=gh.FULL["n_dec"])
    return sr, full


def test_replicated_batch_has_the_loss_and_gradients_of_its_distinct_rows(small):
    sr, full = small
    ref, mol = sr["ref"], sr["mol"]
    assert ref["mu"].shape[0] == D and full["mu"].shape[0] == SMALL_B
    for k in ("loss", "xent", "kl"):
        assert abs(full[k] - ref[k]) <= 1e-13 * abs(ref[k]), k
    for k in ("mu", "logvar", "recon"):
        assert rel(full[k], ref[k][mol]) <= 1e-13, k
    worst = max(gh.grad_report(full["grads"], ref["grads"]).values())
    print(f"replication invariance, {D} rows against {SMALL_B}: largest relative gradient difference {worst:.1e}")
    assert worst <= 1e-12, worst
    gn = float(np.sqrt(sum(float((g ** 2).sum()) for g in full["grads"].values())))
    assert abs(gn - sr["gnorm"]) <= 1e-13 * sr["gnorm"]
    assert gh.step_reference(SMALL_B, SMALL_L) is sr                          # cached: the variants of one shape share one oracle run


def _faithful_step(sr, full):
    """What a correct step at B = 48 hands to the checker: float32 roundings of the float64 48-row run."""
    f = lambda a: np.asarray(a, np.float32)
    return dict(loss=float(np.float32(full["loss"])), mu=f(full["mu"]), logvar=f(full["logvar"]), recon=f(full["recon"]),
                parts=f([full["loss"], full["xent"], full["kl"]]), grads={k: f(g) for k, g in full["grads"].items()},
                gnorm=float(np.float32(sr["gnorm"])))


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_a_deliberately_wrong_step_fails_the_checker(small, mode):
    sr, full = small
    good = _faithful_step(sr, full)
    assert not gh.step_failures(gh.step_errors(good, sr), sr, mode)
    # 1. the gradient of one weight matrix scaled by 1 + 2^-3
    k = "decoder.gru.weight_hh_l2"
    wrong = dict(good, grads=dict(good["grads"], **{k: good["grads"][k] * np.float32(1.125)}))
    bad = gh.step_failures(gh.step_errors(wrong, sr), sr, mode)
    assert set(bad) == {"grad." + k} and 0.12 < bad["grad." + k][0] < 0.13, bad
    # 2. one 16-row block of recon taken from the neighbouring block
    recon = good["recon"].copy()
    recon[16:32] = good["recon"][0:16]
    errs = gh.step_errors(dict(good, recon=recon), sr)
    bad = gh.step_failures(errs, sr, mode)
    print(f"{mode}: recon block taken from its neighbour: error {errs['recon']:.2e}, bound {gh.STEP_BOUNDS[mode]['recon']:.0e}")
    # With these weights two molecules' recon rows differ by 1e-3 .. 2.6e-3 of the largest probability: 100 times the f32 bound, but inside
    # the bf16 bound of 5e-3.  So misplaced recon rows are refused through the f32 variants (the same launches, indexing and dispatch on B);
    # in bf16 mode a misplaced row shows in mu / logvar (bound 1e-5, rows differ by 2e-2) and in the gradients, not in recon.
    assert errs["recon"] > 1e-3
    if mode == "f32":
        assert set(bad) == {"recon"}, bad
    mu = good["mu"].copy()
    mu[16:32] = good["mu"][0:16]
    bad = gh.step_failures(gh.step_errors(dict(good, mu=mu), sr), sr, mode)
    assert set(bad) == {"mu"} and bad["mu"][0] > 1e-2, bad
    # 3. and what the error measure used to let through: one NaN in one gradient, a NaN loss
    g = good["grads"]["encoder.conv_2.0.weight"].copy()
    g.flat[12345] = np.nan
    bad = gh.step_failures(gh.step_errors(dict(good, loss=float("nan"), grads=dict(good["grads"], **{"encoder.conv_2.0.weight": g})), sr), sr, mode)
    assert set(bad) == {"loss", "grad.encoder.conv_2.0.weight"}, bad
