"""CPU tests of gpu_helpers.rel, the error measure the model-level GPU checks filter with (`if v > tol`): non-finite output on the side under
test must come out as inf, because a NaN is never `> tol`; finite input keeps the value it always had."""
import numpy as np
import pytest

from gpu_helpers import rel


def _old_rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_rel_is_inf_when_the_kernel_side_is_not_finite(bad):
    b = np.linspace(-1.0, 1.0, 12).reshape(3, 4)
    assert rel(np.full_like(b, bad), b) == float("inf")
    a = b.copy()
    a[1, 2] = bad
    assert rel(a, b) == float("inf")
    assert rel(np.float32(bad), 1.0) == float("inf")                       # scalars and float32 too
    assert rel(a.astype(np.float32), b) == float("inf")


def test_one_bad_element_in_a_large_array_is_found_and_fails_the_callers_filter():
    rs = np.random.RandomState(0)
    b = rs.standard_normal((4096, 1024))
    a = b.astype(np.float32)
    assert rel(a, b) < 1e-6
    a[4095, 1023] = np.nan
    v = rel(a, b)
    assert v == float("inf") and v > 5e-2 and not (v <= 5e-2)                  # what `if v > tol` and `not (v <= tol)` see
    assert not (_old_rel(a, b) > 5e-2)                                         # the hole: the old measure slipped through `v > tol`


def test_finite_input_is_unchanged():
    rs = np.random.RandomState(1)
    for shape in ((), (7,), (3, 5), (2, 3, 4)):
        b = rs.standard_normal(shape)
        a = b + 1e-3 * rs.standard_normal(shape)
        assert rel(a, b) == _old_rel(a, b)
        assert rel(a.astype(np.float32), b.astype(np.float32)) == _old_rel(a.astype(np.float32), b.astype(np.float32))
    assert rel(np.zeros(4), np.zeros(4)) == 0.0
    assert rel([1.0, 2.0], [1.0, 4.0]) == 0.5
    assert rel(np.array([3], np.int64), np.array([2.0])) == 0.5
