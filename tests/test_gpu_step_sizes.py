"""GPU tests (pytest -m gpu) of one MolecularVAE training step against float64 at the batch sizes the dispatchers treat differently.

The reference is gpu_helpers.step_reference: 16 distinct molecules, each present B / 16 times in a seeded order, have exactly the loss and the
parameter gradients of the 16-row batch (tests/test_step_reference_host.py), so one 16-row numpy oracle run per shape serves all B rows.
Known limit: an error that only exchanges copies of the same molecule stays invisible; the layout conditions asserted in that host test bound
how often a misplaced row can meet its own copy.

What each shape reaches (rnn_fwd_impl / rnn_bwd_impl in csrc/rnn.hip, WGRAD_LATE_TB and MVAE_ENC_DW_BATCH in models.py); each is the smallest
shape that takes its branches.  The decoder tiles named are the bf16 ones; the float32 variants run the same step, launch order and Python
side on the f32 row tiles (forward 64 or 128 rows, backward 64 x 64 fused), which the dispatchers also pick from B:

    B     L    T*B     decoder LSTM forward                    decoder LSTM backward               Python side
    128   120  15360   weights-resident pass on a 256-CU       weights-resident pass, else the     dW launches released late
                       device, else the 128 x 64 gate-major    (128 x 64, 4-way split) pairs
    256   120  30720   weights-resident, as two passes         weights-resident, as two passes,    still under WGRAD_LATE_TB
                                                               else (128 x 128, 4-way split)
    512   120  61440   64-unit wave-specialised tile           (128 x 64, unsplit)                 over WGRAD_LATE_TB; encoder dW batched
    1024  120  122880  256 x 256 gate-major tile               (128 x 128, unsplit)                B*L over 65536 (the benchmark's step)
    2048  33   67584   256 x 256 gate-major tile               (256 x 128, unsplit)                the shortest L that stays over 65536

Per shape four variants: {float32, bfloat16} x {model(idx) + loss function, model.elbo(idx)}, each with a FusedAdam built first so that the
gradients land in its flat buffer as in train_step.  Compared over all B rows: loss, the xent / kl parts (elbo path), mu, logvar, recon
(model path), every parameter gradient (rel), and the pre-clip gradient norm of the optimiser step.  Bounds: gpu_helpers.STEP_BOUNDS, the
ones test_g2_full_dims_f32_and_bf16, test_g2_fixture_through_decoder_elbo and test_training_trajectory_vs_stock_torch_cpu_port use at
B <= 16.

Largest errors measured on an MI355X (256 CUs; worst of the two paths; `grad` is the worst parameter; kl is absolute, its bound 5.6e-6;
B = 16 is the same 16 rows unreplicated, measured alongside and not part of the suite).  The slowest variant takes 1.1 s, after one oracle
run of 1.1 s per shape:

    B     L    mode       loss     xent       kl       mu   logvar    recon     grad    gnorm
    16    120  f32     1.9e-08  2.6e-08  8.8e-10  7.1e-07  7.1e-07  3.2e-07  1.7e-06  6.8e-08
    16    120  bf16    2.0e-06  2.0e-06  8.8e-10  7.1e-07  7.1e-07  5.7e-04  7.6e-03  2.2e-04
    16    33   f32     2.8e-09  4.9e-08  1.3e-09  7.3e-07  8.1e-07  3.2e-07  2.0e-06  2.3e-08
    16    33   bf16    2.0e-06  2.0e-06  1.3e-09  7.3e-07  8.1e-07  5.8e-04  1.2e-02  6.3e-05
    128   120  f32     1.7e-07  1.3e-07  3.2e-09  8.9e-07  6.2e-07  4.3e-07  1.6e-05  8.0e-08
    128   120  bf16    1.7e-06  1.6e-06  3.2e-09  8.9e-07  6.2e-07  5.9e-04  8.6e-03  3.9e-04
    256   120  f32     9.2e-08  6.7e-08  1.3e-09  1.1e-06  8.5e-07  4.2e-07  3.2e-05  2.6e-08
    256   120  bf16    9.2e-08  6.7e-08  1.3e-09  1.1e-06  8.5e-07  6.4e-04  7.5e-03  2.9e-04
    512   120  f32     3.6e-08  2.3e-08  7.3e-10  1.0e-06  9.0e-07  5.0e-07  5.0e-05  8.5e-08
    512   120  bf16    2.8e-06  2.8e-06  7.3e-10  1.0e-06  9.0e-07  5.8e-04  7.4e-03  1.7e-04
    1024  120  f32     3.9e-08  1.5e-08  7.9e-09  1.6e-06  1.0e-06  4.6e-07  1.2e-04  6.6e-08
    1024  120  bf16    1.2e-06  1.1e-06  7.9e-09  1.6e-06  1.0e-06  5.7e-04  9.3e-03  1.6e-04
    2048  33   f32     7.8e-08  8.2e-08  3.2e-09  1.9e-06  1.4e-06  4.3e-07  1.1e-04  1.7e-08
    2048  33   bf16    7.8e-08  8.2e-08  3.2e-09  1.9e-06  1.4e-06  6.6e-04  6.3e-03  5.0e-05

Everything is flat in B except the f32 gradients, which grow in proportion to B (1.7e-6 at 16, 1.2e-4 at 1024; bound 5e-4), in the decoder's
weight gradients only (weight_hh_l*, weight_ih_l1..3: the contractions over K = T*B rows); their biases, column sums of the same dG, stay at
3e-7.  That growth belongs to the replicated batch, not to the size: the B / 16 copies of a row contribute bit-identical products, and an
f32 accumulator takes bit-identical addends with the same rounding error while it stays in one binade, so the copies' errors add up instead
of cancelling (error ~ B / 16 * sqrt(16 * T) * 2^-24 instead of sqrt(T * B) * 2^-24).  A sequential float32 sum of such rows on the CPU gives
1.7e-6 / 1.7e-5 / 1.3e-4 at B = 16 / 128 / 1024 and 1.3e-5 for 1024 distinct rows (test_step_reference_host.py restates it at B = 128).  So
this reference overstates the f32 weight-gradient error of a batch of distinct rows by up to sqrt(B / 16); it never understates it.
"""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_helpers as gh                        # noqa: E402
from gpu_helpers import mv                      # noqa: E402
from molecular_vae_amd import ops               # noqa: E402

dev = torch.device("cuda")
MODES = {"f32": torch.float32, "bf16": torch.bfloat16}


def run_step(B, L, mode, path):
    """One step of `path` ("model": model(idx) + make_loss_function; "elbo": model.elbo) at (B, L) -> (errors, reference, PERSIST_STATS
    before and after).  The model and everything it cached are freed before returning."""
    sr = gh.step_reference(B, L)
    model = mv.MolecularVAE(i=L, dtype=MODES[mode])
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sr["params"].items()})
    model = model.to(dev)
    optimizer = mv.FusedAdam(model.parameters(), lr=8e-4, max_grad_norm=3.0)
    idx = torch.from_numpy(sr["idx"]).to(dev)
    eps = torch.from_numpy(sr["eps"]).to(dev)
    ops.persist_check(sync=True)
    before = dict(ops.PERSIST_STATS)
    optimizer.zero_grad(set_to_none=True)
    out = {}
    if path == "model":
        recon, mu, logvar = model(idx, eps=eps)
        ohe = torch.nn.functional.one_hot(idx, gh.FULL["c"]).float()
        loss = mv.make_loss_function(L)(recon, ohe, mu, logvar)
        out["recon"] = recon.detach().cpu().numpy()
        del ohe
    else:
        loss, mu, logvar = model.elbo(idx, eps=eps)
    loss.backward()
    torch.cuda.synchronize()
    if path == "elbo":
        out["parts"] = model.elbo_parts.cpu().numpy()
        assert float(out["parts"][0]) == float(loss.detach())
    out.update(loss=float(loss.detach()), mu=mu.detach().cpu().numpy(), logvar=logvar.detach().cpu().numpy(),
               grads={k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()})      # read before the optimiser step
    optimizer.step()
    out["gnorm"] = float(optimizer.last_grad_norm)
    skipped = float(optimizer.skipped_steps)
    ops.persist_check(sync=True)
    after = dict(ops.PERSIST_STATS)
    errs = gh.step_errors(out, sr)
    del model, optimizer, loss, mu, logvar, out, idx, eps
    if path == "model":
        del recon
    gc.collect()
    ops.release_caches(); torch.cuda.empty_cache()
    assert skipped == 0, "the optimiser skipped the step"
    return errs, sr, before, after


def summary(errs):
    """The largest error per quantity, the gradients as one figure with the parameter it belongs to."""
    s = {k: v for k, v in errs.items() if not k.startswith("grad.")}
    worst = max((k for k in errs if k.startswith("grad.")), key=lambda k: (not np.isfinite(errs[k]), errs[k]))
    s["grad"] = errs[worst]
    return s, worst[5:]


@pytest.mark.parametrize("path", ["model", "elbo"])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("B,L", gh.STEP_SHAPES, ids=[f"B{b}xL{l}" for b, l in gh.STEP_SHAPES])
def test_step_matches_float64(B, L, mode, path):
    errs, sr, before, after = run_step(B, L, mode, path)
    s, worst = summary(errs)
    print(f"\nstep B={B} L={L} {mode} {path}: " + " ".join(f"{k}={v:.2e}" for k, v in s.items()) + f" (worst gradient: {worst})")
    bad = gh.step_failures(errs, sr, mode)
    assert not bad, bad
    if mode == "bf16" and B in (128, 256) and torch.cuda.get_device_properties(dev).multi_processor_count == 256:
        # the weights-resident decoder passes are what these two sizes are here for
        assert after["launches"] > before["launches"] and after["bwd_launches"] > before["bwd_launches"], (before, after)
    assert after["failures"] == before["failures"] and after["reruns"] == before["reruns"], (before, after)
