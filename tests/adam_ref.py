"""The fp64 NumPy reference of a single-table step under FM_OPT_ADAM (lazy AdamW), sharing tests/adagrad_ref.py's
three-step cases with tests/test_adam_cpu.py and tests/test_gpu_adam.py.

Forward and per-sample (r, yh): tests/objective_ref.py's.  For a touched row, d = tau - last (1 at its first touch),
and per coordinate with gradient sum g, gh = g / rows, eta = step / sqrt(t), c = 1 / (1 - b^tau) (include/fm_hip.h):
    m' = b1^d m + (1 - b1) gh,   v' = b2^d v + (1 - b2) gh^2
    x' = S_lam(x - eta (u + wd x)),   u = c1 m' / (sqrt(c2 v') + eps)
m and v are stored through f32, as the device stores them.  The model's rows are current (the device thresholds lazily).

Budget of a checked value: RTOL |ref| + ATOL (the suite's) + over the steps that touched it
    eta dg (c1 (1 - b1) + |u| sqrt(c2 (1 - b2))) / (sqrt(c2 v') + eps),   dg = 2^-22 T / rows,
T the taken-apart term sum of tests/adagrad_ref.py.  The bracket bounds |d u / d gh|: its second part uses
(1 - b2) gh^2 <= v'.  Adam normalises the gradient, so a gh that is fp32 rounding noise next to eps would move a
coordinate by O(eta) (an entry alone in its row has a term of exactly 0 whose parts are not small): the cases run
with an EPS well above that noise, and tests/test_adam_cpu.py asserts that the budget stays sharp with it.

variant "lazy" takes d = 1 always, "nobias" c1 = c2 = 1, "coupled" adds wd x to gh before the moments: what the
sensitivity test swaps in.
"""

import math

import numpy as np

import objective_ref as O
from adagrad_ref import ATOL, CASES, F_CASE, GROUP, ID_13, ID_NEW, REG, RTOL, STEP, three_step_case  # noqa: F401
from oracle import fm_ref as R
from problems import f32

B1, B2, EPS, WD = 0.9, 0.99, 1e-3, 0.01


class AdamRef:
    def __init__(self, model: R.Model, b1=B1, b2=B2, eps=EPS, wd=WD, variant: str = "adam"):
        F, k = model.V.shape
        self.model, self.b1, self.b2, self.eps, self.wd, self.variant = model, b1, b2, eps, wd, variant
        self.mw, self.vw, self.mV, self.vV = np.zeros(F), np.zeros(F), np.zeros((F, k)), np.zeros((F, k))
        self.last, self.tau = np.zeros(F, dtype=np.int64), 0
        self.xw, self.xV = np.zeros(F), np.zeros((F, k))  # the steps' rounding allowances
        self.touched = np.zeros(F, dtype=bool)

    def step(self, csr: R.CSR, t: int, step_size: float, reg_param: float, loss: str = "squared", group: int = 0):
        model, b1, b2 = self.model, self.b1, self.b2
        rows_n = csr.n_rows
        self.tau += 1
        yhat, S, has = O.scores(model, csr, fast=True)
        r, yh, loss_sum, n_loss = O.objective(loss, yhat if loss == "squared" else f32(yhat), csr.label, has, group)
        eta = step_size / math.sqrt(t)
        lam = eta * reg_param
        rows = np.repeat(np.arange(rows_n), np.diff(csr.row_ptr))
        ids = csr.col.astype(np.int64)
        x = csr.val
        term_w = (x - 1.0) * yh[rows] + r[rows]
        term_V = (S[rows] * x[:, None] - model.V[ids] * (x * x)[:, None]) * r[rows][:, None]
        gw, gV, Tw, TV = np.zeros_like(self.mw), np.zeros_like(self.mV), np.zeros_like(self.mw), np.zeros_like(self.mV)
        np.add.at(gw, ids, term_w)
        np.add.at(gV, ids, term_V)
        # a term's parts taken apart (tests/adagrad_ref.py explains)
        np.add.at(Tw, ids, np.abs(x - 1.0) * np.abs(yh[rows]) + np.abs(r[rows]))
        np.add.at(TV, ids, (np.abs(S[rows] * x[:, None]) + np.abs(model.V[ids]) * (x * x)[:, None]) * np.abs(r[rows])[:, None])
        u = np.unique(ids)
        d = np.where(self.last[u] > 0, self.tau - self.last[u], 1).astype(np.float64)
        if self.variant == "lazy":
            d = np.ones_like(d)
        c1, c2 = (1.0, 1.0) if self.variant == "nobias" else (1.0 / (1.0 - b1 ** self.tau), 1.0 / (1.0 - b2 ** self.tau))
        for m, v, g, T, val, extra, dd in ((self.mw, self.vw, gw, Tw, model.w, self.xw, d),
                                           (self.mV, self.vV, gV, TV, model.V, self.xV, d[:, None])):
            cur, gh, wd = val[u], g[u] / rows_n, self.wd
            if self.variant == "coupled":
                gh, wd = gh + wd * cur, 0.0
            mn = b1 ** dd * m[u] + (1.0 - b1) * gh
            vn = b2 ** dd * v[u] + (1.0 - b2) * gh * gh
            den = np.sqrt(c2 * vn) + self.eps
            un = c1 * mn / den
            val[u] = cur - eta * (un + wd * cur)
            dg = 2.0 ** -22 * T[u] / rows_n
            extra[u] += eta * dg * (c1 * (1.0 - b1) + np.abs(un) * math.sqrt(c2 * (1.0 - b2))) / den
            m[u], v[u] = f32(mn), f32(vn)
        self.last[u] = self.tau
        self.touched[u] = True
        model.present[u] = True
        p = model.present
        model.w[p] = R.soft_threshold(model.w[p], lam)
        model.V[p] = R.soft_threshold(model.V[p], lam)
        return R.StepResult(executed=True, loss_sum=loss_sum, n_rows=rows_n, n_loss_rows=n_loss, n_unique=len(u))

    def budget(self):
        """(budget of w [F], of V [F, k]) for the table as it stands."""
        return RTOL * np.abs(self.model.w) + ATOL + self.xw, RTOL * np.abs(self.model.V) + ATOL + self.xV


def run_case(k: int, loss: str, variant: str = "adam", **hyper):
    """The case's three steps on the reference: (AdamRef, [StepResult])."""
    batches, ids, w, V = three_step_case(k, loss)
    model = R.Model.empty(F_CASE, k)
    model.load(ids, w, V)
    ref = AdamRef(model, variant=variant, **hyper)
    return ref, [ref.step(b, t + 1, STEP, REG, loss, GROUP[loss]) for t, b in enumerate(batches)]
