"""No GPU: the conditions the GPU cases of tests/test_gpu_ftrl.py rest on, checked on tests/ftrl_ref.py alone.  The
tolerance must not hide the update's two FTRL-specific terms -- with the first touch starting from z = 0, or the
sigma v term dropped, some checked value moves by at least 8 budgets -- and with the cases' lambda1 at least a
tenth of the touched coordinates lie safely inside the threshold, so the exact-zero assertion has ground."""

import numpy as np
import pytest

import ftrl_ref as Fr


@pytest.mark.parametrize("k,loss", Fr.CASES)
@pytest.mark.parametrize("variant", ["z0", "nosigma"])
def test_tolerance_does_not_hide_the_update(k, loss, variant):
    ref, _ = Fr.run_case(k, loss)
    other, _ = Fr.run_case(k, loss, variant)
    bw, bV = ref.budget()
    worst = max(np.max(np.abs(other.model.w - ref.model.w) / bw), np.max(np.abs(other.model.V - ref.model.V) / bV))
    print(f"k={k} {loss} {variant}: worst move {worst:.1f} budgets")
    assert worst >= 8.0


@pytest.mark.parametrize("k,loss", Fr.CASES)
def test_a_tenth_of_the_touched_coordinates_is_zeroed(k, loss):
    ref, _ = Fr.run_case(k, loss)
    touched, zeroed = ref.zeroed(Fr.REG)
    print(f"k={k} {loss}: {zeroed.sum()} of {touched.sum()} touched coordinates inside the threshold")
    assert zeroed.sum() >= 0.1 * touched.sum()
    tab = np.column_stack([ref.model.w, ref.model.V])
    assert np.all(tab[zeroed] == 0.0) and np.any(tab[touched & ~zeroed] != 0.0)
