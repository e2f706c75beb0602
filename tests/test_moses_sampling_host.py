"""CPU tests of the filtered sampling surface (mvae_moses_sample_filtered_step, VAE.sample(top_k=, top_p=, return_logp=), moses_generate):
the entry point is declared, bound and exported at ABI 12, argument checks refuse before anything is launched, and the float64 reference
filter / draw / hash of tests/sample_ref.py follow the documented rule on hand-made rows."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import molecular_vae_amd as mv
from molecular_vae_amd import _lib as L, mosesvae as MV, vocab as VC, ops
import sample_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mvae_moses_sample_filtered_step"


def test_filtered_step_is_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvae.h")).read(), flags=re.S)
    assert int(re.search(r"#define MVAE_ABI_VERSION (\d+)", header).group(1)) == 12 == L.ABI_VERSION
    lib = L.load()
    assert lib.mvae_abi_version() == 12
    assert re.search(r"\b" + NAME + r"\s*\(", header)
    assert NAME in L.SIGNATURES and hasattr(lib, NAME)
    assert len(L.SIGNATURES[NAME][1]) == len(L.SIGNATURES["mvae_moses_sample_step"][1]) + 4      # top_k, top_p, logq, hash
    assert callable(ops.moses_sample_filtered_step)
    assert "moses_generate" in mv.__all__ and mv.moses_generate is mv.train.moses_generate
    assert callable(MV.VAE._sample_tokens)


def test_filtered_step_refuses_bad_arguments_before_launching():
    """Everything below returns before any HIP call (no device needed)."""
    lib = L.load()
    fake = ctypes.c_void_p(256)                                  # never dereferenced: every call below is refused first

    def step(top_k=0, top_p=1.0, V=30, H=512, dtype=L.MVAE_F32, temp=1.0, x=fake, W=2048):
        return getattr(lib, NAME)(dtype, 8, V, H, fake, H + 8, fake, H + 8, None, temp, top_k, top_p, 1, 1, 1, fake, W, fake, fake, x, 16, fake,
                                  fake, fake, None, None, None)
    assert step(top_k=-1) == -1 and step(top_k=31) == -1
    assert step(top_p=0.0) == -1 and step(top_p=-0.5) == -1 and step(top_p=float("nan")) == -1
    assert step(V=65) == -1 and step(x=None) == -1 and step(dtype=7) == -1
    assert step(temp=0.0) == -1 and step(W=6) == -1
    assert step(V=64, H=1024) == -3                             # the head does not fit the LDS
    old = lib.mvae_moses_sample_step(L.MVAE_F32, 8, 64, 1024, fake, 1032, fake, 1032, None, 1.0, 1, 1, 1, fake, 2048, fake, fake, fake, 16, fake,
                                     fake, fake, None)
    assert old == -3                                             # the same code as the unfiltered entry


def _cpu_model():
    torch.manual_seed(0)
    return MV.VAE(VC.OneHotVocab(list("abc")), dtype=torch.float32)              # V = 7 (3 symbols + 4 specials)


def test_sample_refuses_bad_filters_and_has_no_cpu_fallback():
    model = _cpu_model()
    for k in (0, -3, 1.5):
        with pytest.raises(ValueError, match="top_k"):
            model.sample(2, max_len=4, top_k=k)
    for p in (0.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="top_p"):
            model.sample(2, max_len=4, top_p=p)
        with pytest.raises(ValueError, match="top_p"):
            mv.moses_generate(model, 4, top_p=p)
    with pytest.raises(ValueError, match="top_k"):
        mv.moses_generate(model, 4, top_k=0)
    with pytest.raises(ValueError, match="n_samples"):
        mv.moses_generate(model, 0)
    with pytest.raises(ValueError, match="z must be"):
        mv.moses_generate(model, 4, z=torch.zeros(3, model.d_z))
    for kw in (dict(top_k=2), dict(top_p=0.5), dict(top_k=100, top_p=2.0), dict(return_logp=True), dict()):
        with pytest.raises(L.MvaeError, match="MI355X only"):                   # a CPU model: no fallback
            model.sample(2, max_len=4, **kw)
    with pytest.raises(L.MvaeError, match="MI355X only"):
        mv.moses_generate(model, 4, top_k=2)
    assert model._check_filters(None, None) == (0, 1.0) and model._check_filters(7, 1.0) == (0, 1.0)
    assert model._check_filters(3, 0.25) == (3, 0.25) and model._check_filters(6, 5.0) == (6, 1.0)


def test_reference_filter_breaks_ties_by_class_id():
    p = np.array([0.1, 0.3, 0.3, 0.1, 0.2])
    assert SR.filter_keep(p, top_k=1).tolist() == [False, True, False, False, False]
    assert SR.filter_keep(p, top_k=2).tolist() == [False, True, True, False, False]
    assert SR.filter_keep(p, top_k=4).tolist() == [True, True, True, False, True]
    # classes by rank: 1, 2, 4, 0, 3 with before = 0, .3, .6, .8, .9
    assert SR.filter_keep(p, top_p=0.85).tolist() == [True, True, True, False, True]
    assert SR.filter_keep(p, top_p=0.75).tolist() == [False, True, True, False, True]


def test_reference_top_p_keeps_the_shortest_prefix_reaching_the_mass_and_at_least_one_class():
    p = np.array([0.05, 0.5, 0.15, 0.3])
    assert SR.filter_keep(p, top_p=0.4).tolist() == [False, True, False, False]          # 0.5 alone reaches 0.4
    assert SR.filter_keep(p, top_p=0.6).tolist() == [False, True, False, True]           # 0.5 < 0.6 <= 0.8
    assert SR.filter_keep(p, top_p=0.8 + 1e-9).tolist() == [False, True, True, True]
    assert SR.filter_keep(p, top_p=1e-9).tolist() == [False, True, False, False]         # never empty
    assert SR.filter_keep(p * 7.0, top_p=0.6).tolist() == [False, True, False, True]     # relative to sum(p)
    # the two filters intersect, each on the unfiltered p
    assert SR.filter_keep(p, top_k=3, top_p=0.6).tolist() == [False, True, False, True]
    assert SR.filter_keep(p, top_k=1, top_p=0.99).tolist() == [False, True, False, False]
    a, b = SR.filter_margins(p, top_k=2, top_p=0.6)
    assert abs(a[0] - np.log(0.3 / 0.15)) < 1e-12 and abs(b[0] - 0.1) < 1e-12
    a, b = SR.filter_margins(p)
    assert np.isinf(a).all() and np.isinf(b).all()


def test_reference_no_op_filters_keep_everything_and_the_draw_is_the_inverse_cdf():
    rs = np.random.RandomState(3)
    p = rs.random_sample((50, 9))
    assert SR.filter_keep(p, top_k=9, top_p=1.0).all() and SR.filter_keep(p).all() and SR.filter_keep(p, top_k=0).all()
    u = rs.random_sample(50)
    pn = p / p.sum(1, keepdims=True)
    want = np.minimum((np.cumsum(pn, 1) <= u[:, None]).sum(1), 8)
    assert (SR.draw(p, np.ones_like(p, bool), u) == want).all()
    keep = SR.filter_keep(p, top_k=3)
    w = SR.draw(p, keep, u)
    assert keep[np.arange(50), w].all() and (keep.sum(1) == 3).all()
    # a uniform at the very top falls on the last KEPT class
    k1 = np.array([True, False, True, False])
    assert SR.draw(np.full(4, 0.25), k1, 1.0)[0] == 2 and SR.draw(np.full(4, 0.25), k1, 0.0)[0] == 0
    assert SR.draw(np.full(4, 0.25), k1, 0.5)[0] == 2 and SR.draw(np.full(4, 0.25), k1, 0.49)[0] == 0
    assert abs(SR.draw_margin(np.full(4, 0.25), k1, 0.4)[0] - 0.05) < 1e-12


def test_reference_hash_is_fnv1a_64():
    """Published FNV-1a 64-bit test vectors (Fowler / Noll / Vo): "" , "a", "foobar"."""
    assert SR.fnv1a64(b"") == 0xcbf29ce484222325
    assert SR.fnv1a64(b"a") == 0xaf63dc4c8601ec8c
    assert SR.fnv1a64(b"foobar") == 0x85944171f73967e8
    assert SR.as_int64(SR.fnv1a64(b"")) == -3750763034362895579 == MV.VAE._FNV_BASIS
