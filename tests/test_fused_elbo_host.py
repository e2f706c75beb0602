"""CPU tests of the index-target ELBO surface (MolecularVAE.elbo, functional.decoder_elbo, elbo_train_step, evaluate_elbo): the C entry
points are declared, bound and exported at ABI 12, the names are exported by the package, and the argument checks refuse CPU tensors and
malformed targets before anything is launched."""
import ctypes
import os
import re

import pytest
import torch

import molecular_vae_amd as mv
from molecular_vae_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mvae_bce_kl_logits_workspace", "mvae_bce_kl_logits_fwd", "mvae_bce_kl_logits_bwd")


def test_logits_elbo_entry_points_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvae.h")).read(), flags=re.S)
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", header).group(1)) == 12 == L.ABI_VERSION
    lib = L.load()
    assert lib.mvae_abi_version() == 12
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert lib.mvae_bce_kl_logits_workspace(1024, 120) >= 16


def test_logits_elbo_entry_points_refuse_bad_arguments_before_launching():
    """Everything below returns before any HIP call (no device needed): missing buffers, bad sizes / leading dimensions, C > 128,
    a short workspace, an unknown dtype."""
    lib = L.load()
    fake = ctypes.c_void_p(256)                                  # never dereferenced: every call below is refused first
    ws_need = lib.mvae_bce_kl_logits_workspace(4, 8)
    fwd = lambda B=4, Lq=8, C=35, ldl=35, logits=fake, idx=fake, m=16, loss=fake, ws=fake, ws_bytes=ws_need: lib.mvae_bce_kl_logits_fwd(
        B, Lq, C, logits, ldl, idx, m, fake, fake, 8.0, loss, None, ws, ws_bytes, None)
    assert fwd(logits=None) == -1 and fwd(idx=None) == -1 and fwd(loss=None) == -1
    assert fwd(B=0) == -1 and fwd(C=0) == -1 and fwd(ldl=34) == -1 and fwd(m=0) == -1
    assert fwd(C=129, ldl=129) == -3
    assert fwd(ws=None) == -2 and fwd(ws_bytes=ws_need - 1) == -2
    bwd = lambda dtype=L.MVAE_F32, C=35, ldd=40, dl=fake, dlT=None, ldT=0, dmu=fake: lib.mvae_bce_kl_logits_bwd(
        dtype, 4, 8, C, fake, 35, fake, 16, fake, fake, 8.0, None, dl, ldd, dlT, ldT, dmu, fake, None)
    assert bwd(dl=None) == -1 and bwd(dmu=None) == -1 and bwd(ldd=34) == -1
    assert bwd(dlT=fake, ldT=31) == -1 and bwd(dtype=7) == -1 and bwd(C=200, ldd=200) == -1      # ldl = 35 < C as well
    assert lib.mvae_bce_kl_logits_bwd(L.MVAE_F32, 4, 8, 200, fake, 200, fake, 16, fake, fake, 8.0, None, fake, 200, None, 0, fake, fake,
                                      None) == -3


def test_new_names_are_exported():
    for name in ("decoder_elbo", "elbo_train_step", "evaluate_elbo"):
        assert name in mv.__all__ and callable(getattr(mv, name)), name
    assert callable(mv.MolecularVAE.elbo) and callable(mv.MolDecoder.elbo)
    from molecular_vae_amd import functional, train
    assert mv.decoder_elbo is functional.decoder_elbo and mv.elbo_train_step is train.elbo_train_step
    assert mv.evaluate_elbo is train.evaluate_elbo


def _small():
    torch.manual_seed(0)
    return mv.MolecularVAE(i=24, o=16, c=12, dtype=torch.float32)


def test_elbo_refuses_cpu_tensors():
    model = _small()
    x = torch.randint(0, 12, (3, 24))
    with pytest.raises(L.MvaeError, match="MI355X"):
        model.elbo(x)
    z, mu, lv = torch.zeros(3, 16), torch.zeros(3, 16), torch.zeros(3, 16)
    with pytest.raises(L.MvaeError, match="MI355X"):
        mv.decoder_elbo(model.decoder, z, x, mu, lv, 24)
    assert model.elbo_parts is None


@pytest.mark.parametrize("bad", [torch.zeros(3, 24, dtype=torch.int32), torch.zeros(3, 24), torch.zeros(3, 23, dtype=torch.int64),
                                 torch.zeros(3, 24, 12, dtype=torch.int64), torch.zeros(72, dtype=torch.int64)])
def test_elbo_refuses_targets_of_the_wrong_shape_or_dtype(bad):
    model = _small()
    with pytest.raises(L.MvaeError, match="int64"):
        model.elbo(bad)
    z, mu, lv = torch.zeros(3, 16), torch.zeros(3, 16), torch.zeros(3, 16)
    with pytest.raises(L.MvaeError, match="int64"):
        mv.decoder_elbo(model.decoder, z, bad, mu, lv, 24)


def test_decoder_elbo_refuses_a_batch_mismatch_and_bad_latents():
    dec = _small().decoder
    x = torch.zeros(3, 24, dtype=torch.int64)
    with pytest.raises(L.MvaeError, match="int64"):
        mv.decoder_elbo(dec, torch.zeros(4, 16), x, torch.zeros(4, 16), torch.zeros(4, 16), 24)
    with pytest.raises(L.MvaeError, match="mu / logvar"):
        mv.decoder_elbo(dec, torch.zeros(3, 16), x, torch.zeros(3, 16), torch.zeros(3, 15), 24)
