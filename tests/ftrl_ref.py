"""The fp64 NumPy reference of a single-table step under FM_OPT_FTRL, sharing tests/adagrad_ref.py's three-step
cases with tests/test_ftrl_cpu.py and tests/test_gpu_ftrl.py.

Forward and per-sample (r, yh): tests/objective_ref.py's.  For a touched coordinate with gradient sum g,
gh = g / m, alpha = step size as given, lambda1 = reg_param (include/fm_hip.h, FM_OPT_FTRL):
    if n == 0: z = -v (beta / alpha + lambda2) - sgn(v) lambda1
    n' = n + gh^2,  z' = z + gh - ((sqrt(n') - sqrt(n)) / alpha) v
    v' = 0 if |z'| <= lambda1 else -(z' - sgn(z') lambda1) / den,  den = (beta + sqrt(n')) / alpha + lambda2
z and n are stored through f32, as the device stores them.  Untouched rows do not move.

Budget of a checked value: RTOL |ref| + ATOL (the suite's) + over the steps that touched it
(2^-22 (T / m) (1 + |v| / alpha) + 2^-24 (|z'| + |v| sqrt(n') / alpha)) / den,  T = sum_e |term_e|' (a term's parts taken apart, as
tests/adagrad_ref.py explains: (|S x| + |v| x^2) |r| and |x - 1| |yh| + |r|):
the fp32 rounding of S, r, yh and of the stored state, pushed through the update's derivative.

variant "z0" leaves z = 0 at the first touch, "nosigma" drops the sigma v term: what the sensitivity test swaps in.
"""

import numpy as np

import objective_ref as O
from adagrad_ref import ATOL, CASES, F_CASE, GROUP, RTOL, three_step_case  # noqa: F401  (shared with the tests)
from oracle import fm_ref as R
from problems import f32

BETA, L2, STEP, REG = 0.004, 0.005, 0.4, 1e-2


class FtrlRef:
    def __init__(self, model: R.Model, beta: float = BETA, l2: float = L2, variant: str = "ftrl"):
        F, k = model.V.shape
        self.model, self.beta, self.l2, self.variant = model, beta, l2, variant
        self.zw, self.nw, self.zV, self.nV = np.zeros(F), np.zeros(F), np.zeros((F, k)), np.zeros((F, k))
        self.xw, self.xV = np.zeros(F), np.zeros((F, k))  # the steps' rounding allowances
        self.lw, self.lV = np.full(F, np.inf), np.full((F, k), np.inf)  # |z'| of the last touch (inf: never touched)

    def step(self, csr: R.CSR, t: int, step_size: float, reg_param: float, loss: str = "squared", group: int = 0):
        model, alpha, l1 = self.model, step_size, reg_param
        m = csr.n_rows
        yhat, S, has = O.scores(model, csr, fast=True)
        r, yh, loss_sum, n_loss = O.objective(loss, yhat if loss == "squared" else f32(yhat), csr.label, has, group)
        rows = np.repeat(np.arange(m), np.diff(csr.row_ptr))
        ids = csr.col.astype(np.int64)
        x = csr.val
        term_w = (x - 1.0) * yh[rows] + r[rows]
        term_V = (S[rows] * x[:, None] - model.V[ids] * (x * x)[:, None]) * r[rows][:, None]
        gw, gV, Tw, TV = np.zeros_like(self.zw), np.zeros_like(self.zV), np.zeros_like(self.zw), np.zeros_like(self.zV)
        np.add.at(gw, ids, term_w)
        np.add.at(gV, ids, term_V)
        # the parts of a term taken apart: the device sums S (x r) and x^2 r on their own and forms A - v b once, so
        # the fp32 rounding of S, r and yh scales with |S x r| + |v x^2 r|, not with their difference (an entry alone
        # in its row has S x = v x^2: a term of exactly 0 whose parts are not small)
        np.add.at(Tw, ids, np.abs(x - 1.0) * np.abs(yh[rows]) + np.abs(r[rows]))
        np.add.at(TV, ids, (np.abs(S[rows] * x[:, None]) + np.abs(model.V[ids]) * (x * x)[:, None]) * np.abs(r[rows])[:, None])
        u = np.unique(ids)
        for z, n, g, T, val, extra, last in ((self.zw, self.nw, gw, Tw, model.w, self.xw, self.lw),
                                             (self.zV, self.nV, gV, TV, model.V, self.xV, self.lV)):
            v, gh, z0, n0 = val[u], g[u] / m, z[u], n[u]
            if self.variant != "z0":
                z0 = np.where(n0 == 0.0, -v * (self.beta / alpha + self.l2) - np.sign(v) * l1, z0)
            nn = n0 + gh * gh
            sigma = 0.0 if self.variant == "nosigma" else (np.sqrt(nn) - np.sqrt(n0)) / alpha
            zn = z0 + gh - sigma * v
            den = (self.beta + np.sqrt(nn)) / alpha + self.l2
            val[u] = np.where(np.abs(zn) <= l1, 0.0, -(zn - np.sign(zn) * l1) / den)
            extra[u] += (2.0 ** -22 * (T[u] / m) * (1.0 + np.abs(v) / alpha)
                         + 2.0 ** -24 * (np.abs(zn) + np.abs(v) * np.sqrt(nn) / alpha)) / den
            z[u], n[u], last[u] = f32(zn), f32(nn), np.abs(zn)
        model.present[u] = True
        return R.StepResult(executed=True, loss_sum=loss_sum, n_rows=m, n_loss_rows=n_loss, n_unique=len(u))

    def budget(self):
        """(budget of w [F], of V [F, k]) for the table as it stands."""
        return RTOL * np.abs(self.model.w) + ATOL + self.xw, RTOL * np.abs(self.model.V) + ATOL + self.xV

    def zeroed(self, reg_param: float):
        """(touched coordinates, those safely inside the threshold: |z'| <= lambda1 (1 - 1e-3)) as [F, 1 + k] masks."""
        last = np.column_stack([self.lw, self.lV])
        return np.isfinite(last), last <= reg_param * (1.0 - 1e-3)


def run_case(k: int, loss: str, variant: str = "ftrl"):
    """The case's three steps on the reference: (FtrlRef, [StepResult])."""
    batches, ids, w, V = three_step_case(k, loss)
    model = R.Model.empty(F_CASE, k)
    model.load(ids, w, V)
    ref = FtrlRef(model, variant=variant)
    return ref, [ref.step(b, t + 1, STEP, REG, loss, GROUP[loss]) for t, b in enumerate(batches)]
