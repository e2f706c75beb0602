"""The dynamic-LDS opt-in is an attribute of (kernel function, DEVICE): a launcher that remembers "done" once per process refuses its first
launch on every further device (the runtime rejects a launch that asks for more dynamic LDS than the kernel may take there).  Two entries
that take more than the default 64 KB run on device 0 and then on the LAST visible device, and are held to float64 on both -- with the helpers
and the bounds of the suites that own these entries:

  * ops.gemm_nt, bf16: test_gpu_gemm_kernels._nt_both (the exact integer recipe + gemm_ref.nt_bound on random bf16 values).
    M = N = 128, K = 256 would NOT do: launch_gemm_nt's plan takes 128 x 128 tiles only from 192 of them on, and the 64 x 64 tile with its
    ring of 4 is 4 * (64 + 64) * 128 B = exactly 64 KB.  The smallest shape on the large tile: M = 192 * 128 + 1, N = 5, K = 256 = 4 K-steps
    (the LDS-direct loop) -- 193 x 1 tiles of 128 x 128 (eff(193) = 0.754 >= 0.8 eff(385 tiles of 64 x 64) = 0.602), ring depth 4:
    4 * (128 + 128) * 128 B = 128 KB; 193 >= 128 tiles: no split-K.
  * the LSTM wavefront forward, ops.rnn_fwd(persist=False), bf16, layers = 2, T = 2, B = 64, H = 64: rnn_fwd_impl takes
    lstm_step_fwd_kernel<bf16_t, 64, 32, 3> (64 rows x (32 units x 4 gates), ring depth 3 on a 256-CU device -- 4 tiles, nothing to gain from
    a third resident workgroup): 3 * (64 + 128) * 128 B = 72 KB.  test_gpu_lstm_kernels._run / _check: lstm_ref.check_slabs' bf16 bound
    (4 x the CPU floor + one bf16 ulp per (layer, step) slab) on hs, cs and the four saved gate slots.
"""
import functools

import pytest
import torch

import lstm_ref as R                                 # noqa: E402
import test_gpu_gemm_kernels as TG                   # noqa: E402
import test_gpu_lstm_kernels as TL                   # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second visible device")]

GEMM_SHAPE = (192 * 128 + 1, 5, 256)
LSTM_SHAPE = dict(dtname="bf16", T=2, B=64, H=64, NL=2)


@functools.lru_cache(maxsize=1)
def _lstm_case():
    return R.build_case(seed=12, **LSTM_SHAPE)


@pytest.mark.parametrize("entry", ["gemm_nt", "lstm_wavefront_fwd"])
def test_lds_opt_in_reaches_a_second_device(entry):
    last = torch.cuda.device_count() - 1
    for d in (0, last):                              # device 0 first: whatever the process remembers about the opt-in, it has it by then
        with torch.cuda.device(d):
            if entry == "gemm_nt":
                TG._nt_both(GEMM_SHAPE, TG.BF16, 31, f"device {d}: 193 tiles of 128 x 128, ring 4")
            else:
                c = _lstm_case()
                o = TL._run(c, persist=False, backward=False)
                assert all(t.device.index == d for t in o["hs"])
                TL._check(c, o, only=("hs", "cs", "gate_i", "gate_f", "gate_g", "gate_o"))
