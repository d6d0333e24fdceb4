"""The evaluation's reference (fm_evaluate*, include/fm_hip.h): exact sums of the error terms formed as
the kernel forms them, and the error budget of a device sum.

From the labels y and a prediction vector p -- the call's own `pred`, so the check separates the sums
from the predictions, which are held to the oracle on their own -- every term is formed in IEEE fp64
exactly as the kernel forms it, e = y - p, |e| and e * e (each one rounding), and summed exactly with
math.fsum.  The device adds the same terms in another order, so its sum of n terms t_i differs from
the exact one by at most

    (n + 1) * 2^-53 * fsum(|t_i|):

the standard bound for a reordered fp64 sum (n - 1 additions, each within 2^-53 of its exact result,
first order in 2^-53; n units cover the second-order terms at any n a test uses), with one more unit
for e * e where the compiler contracts it into the addition (an fma keeps the product unrounded, which
moves that term by up to 2^-53 |t_i| against the rounded product summed here).  It is derived, not
tuned to what the code gives.
"""

from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

U = 2.0 ** -53


@dataclass(frozen=True)
class Sum:
    value: float   # fsum of the terms
    budget: float  # |device sum - value| allowed

    def holds(self, got: float) -> bool:
        return abs(float(got) - self.value) <= self.budget

    def miss(self, got: float) -> str:
        return f"got {float(got)!r}, exact {self.value!r}, off {abs(float(got) - self.value):.3e}, budget {self.budget:.3e}"


def budget(terms) -> float:
    t = np.asarray(terms, dtype=np.float64)
    return (len(t) + 1) * U * math.fsum(np.abs(t).tolist())


def exact(terms) -> Sum:
    t = np.asarray(terms, dtype=np.float64)
    return Sum(math.fsum(t.tolist()), budget(t))


@dataclass(frozen=True)
class Ref:
    n_rows: int
    err: Sum
    abs_err: Sum
    sq_err: Sum


def sums(labels, pred) -> Ref:
    y = np.asarray(labels, dtype=np.float64)
    p = np.asarray(pred, dtype=np.float64)
    assert y.shape == p.shape and y.ndim == 1
    e = y - p  # one rounding per element, as the kernel's e = y - p
    return Ref(len(y), exact(e), exact(np.abs(e)), exact(e * e))


def check(rec, labels, pred, n_unlearned=None) -> Ref:
    """rec (an EvalSums) against the sums over `pred`; returns the reference."""
    ref = sums(labels, pred)
    assert rec.n_rows == ref.n_rows, (rec.n_rows, ref.n_rows)
    if n_unlearned is not None:
        assert rec.n_unlearned == n_unlearned, (rec.n_unlearned, n_unlearned)
    assert ref.err.holds(rec.sum_err), "sum_err: " + ref.err.miss(rec.sum_err)
    assert ref.abs_err.holds(rec.sum_abs_err), "sum_abs_err: " + ref.abs_err.miss(rec.sum_abs_err)
    assert ref.sq_err.holds(rec.sum_sq_err), "sum_sq_err: " + ref.sq_err.miss(rec.sum_sq_err)
    return ref


def learned_rows(model, csr, num_features) -> np.ndarray:
    """bool [rows]: the row holds at least one entry whose id the model has (id < num_features and
    present) -- the complement is what n_unlearned counts."""
    ok = (csr.col >= 0) & (csr.col < num_features)
    ok[ok] = model.present[csr.col[ok]]
    rows = np.repeat(np.arange(csr.n_rows), np.diff(csr.row_ptr))
    return np.bincount(rows[ok], minlength=csr.n_rows) > 0
