"""The fp64 NumPy reference of a single-table step under FM_OPT_ADAGRAD, and the three-step cases that
tests/test_adagrad_cpu.py and tests/test_gpu_adagrad.py share.

Forward and per-sample (r, yh): tests/objective_ref.py's (the non-squared losses read the fp32 score).  For a
touched coordinate with gradient sum g, gh = g / m:  G' = G + gh^2,  v' = S_lam(v - eta gh / sqrt(G')),
G <- fp32(G'), as the device stores it.  The model's rows are current (the device thresholds lazily).

Budget of a checked value: RTOL |ref| + ATOL (the suite's) + over the steps that touched it
eta 2^-22 T / sqrt(G'), T = sum_e |term_e|' / m: the fp32 rounding of S, r and yh carried through the step, where
|term_e|' takes a term's parts apart, (|S x| + |v| x^2) |r| and |x - 1| |yh| + |r|: the device forms A = sum S (x r) and
b = sum x^2 r on their own and subtracts once, so the inputs' rounding does not cancel where S x and v x^2 do
(tests/test_gpu_optimizer_edges.py met this: an entry alone in its row has a term of exactly 0).

variant "stale" divides by sqrt(G), "sgd" drops the accumulator: what the sensitivity test swaps in.
"""

import math

import numpy as np

import objective_ref as O
from oracle import fm_ref as R
from problems import f32, make_rows

RTOL, ATOL = 1e-5, 1e-8


class AdaRef:
    def __init__(self, model: R.Model, g0: float, variant: str = "adagrad"):
        F, k = model.V.shape
        self.model, self.variant = model, variant
        self.Gw = np.full(F, f32(g0), dtype=np.float64)
        self.GV = np.full((F, k), f32(g0), dtype=np.float64)
        self.xw, self.xV = np.zeros(F), np.zeros((F, k))  # the steps' rounding allowances

    def step(self, csr: R.CSR, t: int, step_size: float, reg_param: float, loss: str = "squared", group: int = 0):
        model = self.model
        m = csr.n_rows
        yhat, S, has = O.scores(model, csr, fast=True)
        r, yh, loss_sum, n_loss = O.objective(loss, yhat if loss == "squared" else f32(yhat), csr.label, has, group)
        eta = step_size / math.sqrt(t)
        lam = eta * reg_param
        rows = np.repeat(np.arange(m), np.diff(csr.row_ptr))
        ids = csr.col.astype(np.int64)
        x = csr.val
        term_w = (x - 1.0) * yh[rows] + r[rows]
        term_V = (S[rows] * x[:, None] - model.V[ids] * (x * x)[:, None]) * r[rows][:, None]
        gw, gV, Tw, TV = np.zeros_like(self.Gw), np.zeros_like(self.GV), np.zeros_like(self.Gw), np.zeros_like(self.GV)
        np.add.at(gw, ids, term_w)
        np.add.at(gV, ids, term_V)
        # the parts of a term taken apart: the device sums S (x r) and x^2 r on their own and forms A - v b once, so
        # the fp32 rounding of S, r and yh scales with |S x r| + |v x^2 r|, not with their difference (an entry alone
        # in its row has S x = v x^2: a term of exactly 0 whose parts are not small)
        np.add.at(Tw, ids, np.abs(x - 1.0) * np.abs(yh[rows]) + np.abs(r[rows]))
        np.add.at(TV, ids, (np.abs(S[rows] * x[:, None]) + np.abs(model.V[ids]) * (x * x)[:, None]) * np.abs(r[rows])[:, None])
        u = np.unique(ids)
        for G, g, T, val, extra in ((self.Gw, gw, Tw, model.w, self.xw), (self.GV, gV, TV, model.V, self.xV)):
            gh = g[u] / m
            Gn = G[u] + gh * gh
            den = {"adagrad": np.sqrt(Gn), "stale": np.sqrt(G[u]), "sgd": 1.0}[self.variant]
            val[u] = val[u] - eta * gh / den
            extra[u] += eta * 2.0 ** -22 * (T[u] / m) / np.sqrt(Gn)
            G[u] = f32(Gn)
        model.present[u] = True
        p = model.present
        model.w[p] = R.soft_threshold(model.w[p], lam)
        model.V[p] = R.soft_threshold(model.V[p], lam)
        return R.StepResult(executed=True, loss_sum=loss_sum, n_rows=m, n_loss_rows=n_loss, n_unique=len(u))

    def budget(self):
        """(budget of w [F], of V [F, k]) for the table as it stands."""
        return RTOL * np.abs(self.model.w) + ATOL + self.xw, RTOL * np.abs(self.model.V) + ATOL + self.xV


# ------------------------------------------------------------------------------------------- cases
F_CASE, POOL = 300, 280
ID_13, ID_NEW = 290, 291  # touched in steps 1 and 3 only (G kept, L1 pending); absent before step 2
G0, STEP, REG = 0.1, 0.4, 1e-2
CASES = [(k, loss) for k in (4, 16, 20) for loss in ("squared", "logistic", "bpr")]
GROUP = {"squared": 0, "logistic": 0, "bpr": 5}


def three_step_case(k: int, loss: str):
    """(batches [3], ids, w, V): 255 rows of 0 .. 8 pool ids each (problems.make_rows: explicit zeros, unit
    values), row 7 empty, row 1 holding ID_13 in batches 1 and 3 and ID_NEW in 2 and 3; the table lacks ID_NEW."""
    batches = []
    for step in range(3):
        lens = np.random.default_rng(10 * k + step).integers(0, 9, 255)
        lens[1], lens[7] = 4, 0
        csr, ids, w, V = make_rows(100 * k + len(loss) + step, lens, F_CASE, k, pool=POOL)
        at = csr.row_ptr[1]
        if step != 1:
            csr.col[at], csr.val[at] = ID_13, 0.75
        if step != 0:
            csr.col[at + 1], csr.val[at + 1] = ID_NEW, -1.5
        batches.append(csr)
    keep = ids != ID_NEW
    return batches, ids[keep], w[keep], V[keep]


def run_case(k: int, loss: str, variant: str = "adagrad"):
    """The case's three steps on the reference: (AdaRef, [StepResult])."""
    batches, ids, w, V = three_step_case(k, loss)
    model = R.Model.empty(F_CASE, k)
    model.load(ids, w, V)
    ref = AdaRef(model, G0, variant)
    return ref, [ref.step(b, t + 1, STEP, REG, loss, GROUP[loss]) for t, b in enumerate(batches)]
