"""Shared helpers for the GPU parity tests: run the HIP path and the numpy oracle on the same seeded inputs."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import np_oracle as O          # noqa: E402  (checker only)
from oracle import initparams as ip        # noqa: E402
import molecular_vae_amd as mv             # noqa: E402

G1 = dict(i=24, o=16, c=12, emb=30, h_enc=56, n_enc=2, h_dec=32, n_dec=2, B=3, seed=101, gain=2.0)


def rel(a, b):
    """Largest |a - b| over the largest |b|: a is the side under test, b the reference.  inf as soon as a holds one non-finite element:
    callers filter with `v > tol`, which a NaN never satisfies, so NaN output used to pass every such filter."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    if not np.isfinite(a).all():
        return float("inf")
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def build_modules(dims, params, dtype, dev="cuda"):
    enc = mv.MolEncoder(i=dims["i"], o=dims["o"], c=dims["c"], word_embedding_size=dims["emb"], h_size=dims["h_enc"],
                        num_lstm=dims["n_enc"])
    dec = mv.MolDecoder(i=dims["o"], o=dims["i"], c=dims["c"], num_gru=dims["n_dec"], h_size=dims["h_dec"], dtype=dtype)
    enc.load_state_dict({k[len("encoder."):]: torch.from_numpy(np.asarray(v, np.float32)) for k, v in params.items()
                         if k.startswith("encoder.")})
    dec.load_state_dict({k[len("decoder."):]: torch.from_numpy(np.asarray(v, np.float32)) for k, v in params.items()
                         if k.startswith("decoder.")})
    import weakref
    dec.__dict__["_peer"] = weakref.ref(enc)      # pair them as MolecularVAE does: exercises the side-stream weight-gradient fork
    return enc.to(dev), dec.to(dev)


def run_hip(enc, dec, idx, eps, max_len):
    dev = next(enc.parameters()).device
    tidx = torch.from_numpy(idx).to(dev)
    teps = torch.from_numpy(np.asarray(eps, np.float32)).to(dev)
    C = enc.embedding.num_embeddings
    for m in (enc, dec):
        m.zero_grad(set_to_none=True)
    z, mu, logvar = enc(tidx, teps)
    dec.__dict__["_z_from_peer"] = True           # as MolecularVAE.forward does: z is the paired encoder's output, so the fork is allowed
    recon = dec(z)
    dec.__dict__["_z_from_peer"] = False
    ohe = torch.nn.functional.one_hot(tidx, C).float()
    loss = mv.bce_kl_loss(recon, ohe, mu, logvar, max_len)
    loss.backward()
    torch.cuda.synchronize()
    grads = {"encoder." + k: p.grad.detach().cpu().numpy() for k, p in enc.named_parameters()}
    grads.update({"decoder." + k: p.grad.detach().cpu().numpy() for k, p in dec.named_parameters()})
    return dict(loss=float(loss.detach()), z=z.detach().cpu().numpy(), mu=mu.detach().cpu().numpy(),
                logvar=logvar.detach().cpu().numpy(), recon=recon.detach().cpu().numpy(), grads=grads)


def g1_dims_params(dt=np.float64):
    shapes = ip.molvae_shapes(G1["i"], G1["o"], G1["c"], G1["emb"], G1["h_enc"], G1["n_enc"], G1["h_dec"], G1["n_dec"])
    return ip.init_params(shapes, G1["seed"], G1["gain"], dt)


FULL = dict(i=120, o=292, c=35, emb=30, h_enc=72, n_enc=3, h_dec=1024, n_dec=4)


def grad_report(hip_grads, ref_grads):
    """per-parameter relative error (max-norm) -> dict"""
    return {k: rel(hip_grads[k], ref_grads[k]) for k in ref_grads}


# ------------------------------------------------------------------------------------------------ the replicated-batch step reference
# Both terms of the ELBO are means over the batch, so a batch of D distinct molecules, each present B / D times, has exactly the loss and
# the parameter gradients of the D-row batch, and its mu / logvar / recon rows are the D reference rows repeated: one D-row oracle run is an
# exact float64 reference for a step at any multiple of D.  Known limit: an error that only exchanges copies of the same molecule stays
# invisible; the layout conditions tests/test_step_reference_host.py asserts on `mol` bound how often a misplaced row can meet its own copy.
STEP_D = 16
STEP_SHAPES = ((128, 120), (256, 120), (512, 120), (1024, 120), (2048, 33))      # (B, L): tests/test_gpu_step_sizes.py names the branches
# the bounds of test_g2_full_dims_f32_and_bf16, test_g2_fixture_through_decoder_elbo (loss, xent, kl, latents, recon, gradients) and
# test_training_trajectory_vs_stock_torch_cpu_port (gradient norm); kl is absolute: 1e-4 * |kl| + 1e-7
STEP_BOUNDS = {"f32": dict(loss=1e-5, xent=1e-5, mu=1e-5, logvar=1e-5, recon=1e-5, grad=5e-4, gnorm=1e-4),
               "bf16": dict(loss=1e-4, xent=1e-4, mu=1e-5, logvar=1e-5, recon=5e-3, grad=5e-2, gnorm=5e-2)}


def replicated_batch(D, B, L, C, seed):
    """(idx [B, L] int64, eps [B, o] float32, mol [B]): D distinct seeded molecules with their noise rows (scale 1e-2), row r of the batch
    being molecule mol[r]; mol is D molecules x B / D copies in a seeded random order."""
    assert B % D == 0
    mol = np.tile(np.arange(D), B // D)[np.random.RandomState(seed).permutation(B)]
    idx_d = ip.seeded_indices(seed, D, L, C)
    eps_d = ip.seeded_eps(seed, D, FULL["o"])
    return idx_d[mol], eps_d[mol], mol


_STEP_REF = {}


def step_params(L):
    return ip.init_params(ip.molvae_shapes(L, FULL["o"], FULL["c"], FULL["emb"], FULL["h_enc"], FULL["n_enc"], FULL["h_dec"], FULL["n_dec"]),
                          202, 1.5, np.float32)


def step_reference(B, L, D=STEP_D):
    """The float64 oracle on the D distinct rows of replicated_batch(D, B, L, 35, 1000 + B), run once per (B, L) and shared: dict(idx, eps,
    mol, params, ref, gnorm).  Nothing in it may be written to."""
    key = (B, L, D)
    if key not in _STEP_REF:
        idx, eps, mol = replicated_batch(D, B, L, FULL["c"], 1000 + B)
        first = np.array([int(np.flatnonzero(mol == m)[0]) for m in range(D)])
        params = step_params(L)
        ref = O.molvae_loss_and_grads({k: v.astype(np.float64) for k, v in params.items()}, idx[first], eps[first].astype(np.float64),
                                      max_len=L, num_lstm=FULL["n_enc"], num_gru=FULL["n_dec"])
        ref.pop("stages", None)
        gnorm = float(np.sqrt(sum(float((g ** 2).sum()) for g in ref["grads"].values())))
        _STEP_REF.clear()          # one shape at a time (its users run shape by shape): the float64 gradients are 270 MB each
        _STEP_REF[key] =dict(idx=idx, eps=eps, mol=mol, params=params, ref=ref, gnorm=gnorm)
    return _STEP_REF[key]


def step_errors(out, sr):
    """Every figure tests/test_gpu_step_sizes.py bounds, for one step's outputs `out` against step_reference's `sr`: out holds loss, mu,
    logvar, grads (by parameter name), gnorm, and where the path has them recon and parts = (total, xent, kl).  All B rows are compared,
    against the reference rows gathered with mol.  kl is an absolute error, everything else relative."""
    ref, mol = sr["ref"], sr["mol"]
    e = {"loss": abs(out["loss"] - ref["loss"]) / abs(ref["loss"]),
         "mu": rel(out["mu"], ref["mu"][mol]), "logvar": rel(out["logvar"], ref["logvar"][mol]),
         "gnorm": abs(out["gnorm"] - sr["gnorm"]) / sr["gnorm"]}
    if out.get("recon") is not None:
        e["recon"] = rel(out["recon"], ref["recon"][mol])
    if out.get("parts") is not None:
        e["xent"] = abs(float(out["parts"][1]) - ref["xent"]) / abs(ref["xent"])
        e["kl"] = abs(float(out["parts"][2]) - ref["kl"])
    assert set(out["grads"]) == set(ref["grads"])
    for k, g in ref["grads"].items():
        e["grad." + k] = rel(out["grads"][k], g)
    return e


def step_failures(errs, sr, mode):
    """The figures of step_errors that are not inside STEP_BOUNDS[mode] (written so that a NaN figure is a failure)."""
    tol = STEP_BOUNDS[mode]
    bad = {}
    for k, v in errs.items():
        bound = 1e-4 * abs(sr["ref"]["kl"]) + 1e-7 if k == "kl" else tol["grad" if k.startswith("grad.") else k]
        if not (v <= bound):
            bad[k] = (v, bound)
    return bad
