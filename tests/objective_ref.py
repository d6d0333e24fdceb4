"""The fp64 NumPy reference of a single-table step under a training objective (fm_config.loss).

A step is: the forward (oracle.fm_ref.forward), the objective -- which turns the scores into one
derivative r_s per sample and a loss -- and the update with its soft threshold, restated from
oracle.fm_ref.sgd_step_fast for a general per-sample pair (r, yh):

    g_w(entry) = (x - 1) * yh_s + r_s          g_V(entry) = (vfxiSum_s * x - v * x * x) * r_s

With (r, yh) = (yhat - y, yhat) that is the reference's squared step, its own g_w = x * yhat - y included
(SURVEY P1); with yh := r it is g_w = x * r, the gradient of a loss whose derivative by the score is r.

round_scores=True rounds yhat to fp32 before the objective reads it: the device's contract (the
objective stage reads the score as the forward stored it).
"""

from __future__ import annotations

import math

import numpy as np

from oracle import fm_ref as R

LOSSES = ("squared", "logistic", "bpr")


def sigmoid(z):
    """sigma(z) from exp(-|z|): finite for every finite z."""
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def softplus(z):
    """max(z, 0) + log1p(exp(-|z|))"""
    z = np.asarray(z, dtype=np.float64)
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def scores(model: R.Model, csr: R.CSR, fast: bool = False):
    """(yhat [B], vfxi_sum [B, k], has_entries [B]); a row without entries scores w0.  fast: the
    vectorised forward of sgd_step_fast instead of fm_ref.forward's loop (the same sums in the same
    entry order; for the batches of tens of thousands of rows)."""
    if not fast:
        fw = R.forward(model, csr)
        return np.where(fw.has_entries, fw.pred, model.w0), fw.vfxi_sum, fw.has_entries
    m, k = csr.n_rows, model.k
    rows = np.repeat(np.arange(m), np.diff(csr.row_ptr))
    ids = csr.col.astype(np.int64)
    x = csr.val
    V = model.V[ids]
    vfxi_sum = np.zeros((m, k))
    np.add.at(vfxi_sum, rows, V * x[:, None])
    wsum = np.zeros(m)
    np.add.at(wsum, rows, model.w[ids] * x)
    vv = np.zeros(m)
    np.add.at(vv, rows, np.sum(V * V, axis=1) * x * x)
    yhat = 0.5 * (np.sum(vfxi_sum * vfxi_sum, axis=1) - vv) + wsum + model.w0
    return yhat, vfxi_sum, np.diff(csr.row_ptr) > 0


def objective(loss: str, yhat, label, has_entries, group: int = 0):
    """(r [B], yh [B], loss_sum, n_loss_rows) of the scores yhat under `loss`."""
    yhat = np.asarray(yhat, dtype=np.float64)
    if loss == "squared":
        d = (yhat - label)[has_entries]
        return yhat - label, yhat, float(np.sum(d * d)), int(has_entries.sum())
    if loss == "logistic":
        r = sigmoid(yhat) - label
        terms = (softplus(yhat) - label * yhat)[has_entries]
        return r, r, float(np.sum(terms)), int(has_entries.sum())
    assert loss == "bpr" and group >= 2 and len(yhat) % group == 0, (loss, group, len(yhat))
    y2 = yhat.reshape(-1, group)
    nd = y2[:, 1:] - y2[:, :1]  # -d_j
    sg = sigmoid(nd)
    r = np.concatenate([-sg.sum(axis=1, keepdims=True), sg], axis=1).reshape(-1)
    return r, r, float(np.sum(softplus(nd))), int(nd.size)


def update(model: R.Model, csr: R.CSR, vfxi_sum, r, yh, t: int, step_size: float, reg_param: float) -> int:
    """sgd_step_fast's update and soft threshold with the per-sample (r, yh), in place; returns the
    number of distinct ids touched."""
    m, k = csr.n_rows, model.k
    eta = step_size / math.sqrt(t)
    lam = eta * reg_param
    rows = np.repeat(np.arange(m), np.diff(csr.row_ptr))
    ids = csr.col.astype(np.int64)
    x = csr.val
    vfxi = model.V[ids] * x[:, None]
    g_w = (x - 1.0) * yh[rows] + r[rows]
    g_v = (vfxi_sum[rows] * x[:, None] - vfxi * x[:, None]) * r[rows][:, None]
    F = len(model.w)
    GW = np.zeros(F)
    np.add.at(GW, ids, g_w)
    GV = np.zeros((F, k))
    np.add.at(GV, ids, g_v)
    touched = np.unique(ids)
    w_new = model.w.copy()
    V_new = model.V.copy()
    w_new[touched] = model.w[touched] - (GW[touched] / m) * eta
    V_new[touched] = model.V[touched] - GV[touched] * (eta / m)
    pres = model.present.copy()
    pres[touched] = True
    model.w[pres] = R.soft_threshold(w_new[pres], lam)
    model.V[pres] = R.soft_threshold(V_new[pres], lam)
    model.present = pres
    return len(touched)


def step(model: R.Model, csr: R.CSR, t: int, step_size: float, reg_param: float, loss: str = "squared", group: int = 0,
         round_scores: bool = False, fast: bool = False) -> R.StepResult:
    """One step under `loss`, in place on model (1/m stays 1 / n_rows, also under "bpr")."""
    if csr.n_rows == 0:
        return R.StepResult(executed=False)
    yhat, vfxi_sum, has = scores(model, csr, fast)
    if round_scores:
        yhat = yhat.astype(np.float32).astype(np.float64)
    r, yh, loss_sum, n_loss = objective(loss, yhat, csr.label, has, group)
    n_unique = update(model, csr, vfxi_sum, r, yh, t, step_size, reg_param)
    return R.StepResult(executed=True, loss_sum=loss_sum, n_rows=csr.n_rows, n_loss_rows=n_loss, n_unique=n_unique)
