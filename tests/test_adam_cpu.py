"""No GPU: the conditions the GPU cases of tests/test_gpu_adam.py rest on, checked on tests/adam_ref.py alone.  With
the cases' EPS the budget stays sharp -- nine in ten touched coordinates move by 8 budgets or more over the three
steps -- and it does not hide what makes the update lazy AdamW: the decay of stale moments, the bias correction
and the decoupling of the weight decay each move some checked value out of its budget."""

import math

import numpy as np
import pytest

import adagrad_ref as Ar
import adam_ref as Am
from oracle import fm_ref as R


def tables(ref):
    bw, bV = ref.budget()
    return np.column_stack([ref.model.w, ref.model.V]), np.column_stack([bw, bV])


@pytest.mark.parametrize("k,loss", Am.CASES)
def test_touched_coordinates_move_by_many_budgets(k, loss):
    _, ids, w, V = Am.three_step_case(k, loss)
    ref, _ = Am.run_case(k, loss)
    start = np.zeros((Am.F_CASE, 1 + k))
    start[ids] = np.column_stack([w, V])
    tab, budget = tables(ref)
    moved = (np.abs(tab - start) / budget)[ref.touched]
    print(f"k={k} {loss}: {np.mean(moved >= 8.0):.3f} of the touched coordinates move by 8 budgets or more")
    assert np.mean(moved >= 8.0) >= 0.9


@pytest.mark.parametrize("k,loss", Am.CASES)
@pytest.mark.parametrize("variant", ["lazy", "nobias", "coupled"])
def test_tolerance_does_not_hide_the_update(k, loss, variant):
    ref, _ = Am.run_case(k, loss)
    other, _ = Am.run_case(k, loss, variant)
    (tab, budget), (tab2, _) = tables(ref), tables(other)
    over = np.abs(tab2 - tab) / budget
    worst = over[Am.ID_13].max() if variant == "lazy" else over[ref.touched].max()  # d = 2 at ID_13 alone
    print(f"k={k} {loss} {variant}: worst move {worst:.1f} budgets")
    assert worst > 1.0


def test_first_step_by_hand():
    """b1, b2 -> 0 and wd = 0: u = gh / (|gh| + eps), with gh read off an SGD step of the AdaGrad reference."""
    k, tiny = 4, 1e-12
    batches, ids, w, V = Am.three_step_case(k, "squared")
    models = [R.Model.empty(Am.F_CASE, k) for _ in range(2)]
    for model in models:
        model.load(ids, w, V)
    Ar.AdaRef(models[0], Ar.G0, "sgd").step(batches[0], 4, 1.0, 0.0)
    ref = Am.AdamRef(models[1], b1=tiny, b2=tiny, wd=0.0)
    ref.step(batches[0], 4, Am.STEP, 0.0)
    start = np.zeros((Am.F_CASE, 1 + k))
    start[ids] = np.column_stack([w, V])
    gh = (start - np.column_stack([models[0].w, models[0].V])) / (1.0 / math.sqrt(4))
    want = start - Am.STEP / math.sqrt(4) * gh / (np.abs(gh) + Am.EPS)
    np.testing.assert_allclose(np.column_stack([models[1].w, models[1].V]), want, rtol=1e-9, atol=1e-12)
    assert np.any(gh[ref.touched] != 0.0)
