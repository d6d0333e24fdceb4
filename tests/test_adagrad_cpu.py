"""No GPU: tests/adagrad_ref.py against a plain per-coordinate loop on a hand case, and the suite's usual
condition on the GPU cases' tolerance -- it must not hide the feature: with G' replaced by G, or the
accumulator dropped (SGD at the same eta), some checked value moves by at least 8 budgets."""

import math

import numpy as np
import pytest

import adagrad_ref as A
from oracle import fm_ref as R


def test_reference_against_a_per_coordinate_loop():
    k, F, g0, step, reg, m = 2, 4, 0.25, 0.5, 0.05, 4
    csr = R.CSR(np.array([0, 2, 3, 3, 5]), np.array([0, 2, 2, 0, 3], np.int32), np.array([1.0, -0.5, 2.0, 0.0, 1.5]),
                np.array([1.0, 0.0, 1.0, -1.0]))
    w, V = np.array([0.1, -0.2, 0.3, 0.0]), np.array([[0.1, -0.3], [0.2, 0.1], [-0.4, 0.25], [0.0, 0.0]])
    model = R.Model.empty(F, k)
    model.load(np.arange(3, dtype=np.int32), w[:3], V[:3])  # id 3 is absent before the step
    fw = R.forward(model, csr)  # the oracle's scores and vfxiSum, before the step
    ref = A.AdaRef(model, g0)
    out = ref.step(csr, 4, step, reg)
    g = np.zeros((F, 1 + k))  # per coordinate [w | V]: the entries' gradients, one by one
    for s in range(m):
        for j in range(csr.row_ptr[s], csr.row_ptr[s + 1]):
            i, x = csr.col[j], csr.val[j]
            g[i, 0] += x * fw.pred[s] - csr.label[s]
            g[i, 1:] += (fw.vfxi_sum[s] * x - V[i] * x * x) * (fw.pred[s] - csr.label[s])
    eta, tab, G = step / 2.0, np.column_stack([w, V]), np.full((F, 1 + k), g0)
    for i in range(F):
        for c in range(1 + k):
            if i != 1:  # id 1 is untouched: thresholded only, its G kept
                G[i, c] += (g[i, c] / m) ** 2
                tab[i, c] -= eta * (g[i, c] / m) / math.sqrt(G[i, c])
            tab[i, c] = math.copysign(max(abs(tab[i, c]) - eta * reg, 0.0), tab[i, c])
    np.testing.assert_allclose(np.column_stack([model.w, model.V]), tab, rtol=1e-14, atol=0)
    assert np.array_equal(np.column_stack([ref.Gw, ref.GV]), np.float32(G).astype(np.float64))
    assert (out.n_unique, out.n_loss_rows, bool(model.present[3])) == (3, 3, True)


@pytest.mark.parametrize("k,loss", A.CASES)
@pytest.mark.parametrize("variant", ["stale", "sgd"])
def test_tolerance_does_not_hide_the_accumulator(k, loss, variant):
    ref, _ = A.run_case(k, loss)
    other, _ = A.run_case(k, loss, variant)
    bw, bV = ref.budget()
    worst = max(np.max(np.abs(other.model.w - ref.model.w) / bw), np.max(np.abs(other.model.V - ref.model.V) / bV))
    print(f"k={k} {loss} {variant}: worst move {worst:.1f} budgets")
    assert worst >= 8.0
