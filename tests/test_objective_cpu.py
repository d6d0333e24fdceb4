"""CPU: the training objectives (fm_config.loss) before any kernel runs.

  * tests/objective_ref.py, the fp64 reference the GPU tests compare against, is itself pinned: with the
    squared pair (r, yh) = (yhat - y, yhat) it is oracle.fm_ref.sgd_step_fast, and under "logistic" /
    "bpr" its update of w and of V is one gradient step of torch's fp64 automatic differentiation of
    the loss each objective names (as tests/test_oracle_autograd.py pins the squared step's V);
  * the stable forms at saturated scores, and what rounding the score to fp32 can move;
  * the ctypes mirror of fm_config, and the estimator's refusals (no GPU: they raise before any context
    is made).
"""

import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import objective_ref as O
from oracle import fm_ref as R
from problems import make_problem

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _model(F, k, ids, w, V, absent_every=0):
    present = np.ones(F, bool)
    if absent_every:
        present[::absent_every] = False
    m = R.Model.empty(F, k)
    m.load(ids[present], w[present], V[present])
    return m


# ------------------------------------------------------------------ the reference against the oracle
@pytest.mark.parametrize("seed,k,reg", [(3, 4, 1e-4), (4, 8, 0.0), (5, 3, 2e-2)])
@pytest.mark.parametrize("fast", [False, True])
def test_squared_pair_reproduces_the_oracle_step(seed, k, reg, fast):
    F = 60
    csr, ids, w, V = make_problem(seed, 50, F, k, 7, hot=5)
    a, b = _model(F, k, ids, w, V, 7), _model(F, k, ids, w, V, 7)
    for t in (1, 2, 3):
        ro = R.sgd_step_fast(a, csr, t, 0.4, reg)
        go = O.step(b, csr, t, 0.4, reg, "squared", fast=fast)
        assert go.loss_sum == pytest.approx(ro.loss_sum, rel=1e-15, abs=0.0)
        assert (go.n_rows, go.n_loss_rows, go.n_unique) == (ro.n_rows, ro.n_loss_rows, ro.n_unique)
    np.testing.assert_allclose(b.w, a.w, rtol=1e-15, atol=1e-15)
    np.testing.assert_allclose(b.V, a.V, rtol=1e-15, atol=1e-15)
    assert np.array_equal(a.present, b.present)


def test_fast_scores_are_the_loop_forwards():
    csr, ids, w, V = make_problem(11, 80, 50, 6, 5)
    m = _model(50, 6, ids, w, V)
    m.w0 = 0.25
    ya, Sa, ha = O.scores(m, csr, fast=False)
    yb, Sb, hb = O.scores(m, csr, fast=True)
    assert not ha.all() and np.array_equal(ha, hb)  # the problem has rows without entries
    assert np.all(ya[~ha] == 0.25) and np.all(yb[~hb] == 0.25)
    np.testing.assert_allclose(yb, ya, rtol=1e-15, atol=1e-15)
    np.testing.assert_allclose(Sb, Sa, rtol=1e-15, atol=1e-15)


# ----------------------------------------------------------------- the reference against autograd
def _torch_forward(w, V, csr, w0):
    rows = torch.from_numpy(np.repeat(np.arange(csr.n_rows), np.diff(csr.row_ptr)))
    ids = torch.from_numpy(csr.col.astype(np.int64))
    x = torch.from_numpy(csr.val)
    Vx = V[ids] * x[:, None]
    S = torch.zeros(csr.n_rows, V.shape[1], dtype=torch.float64).index_add(0, rows, Vx)
    vv = torch.zeros(csr.n_rows, dtype=torch.float64).index_add(0, rows, (Vx * Vx).sum(1))
    wx = torch.zeros(csr.n_rows, dtype=torch.float64).index_add(0, rows, w[ids] * x)
    return 0.5 * ((S * S).sum(1) - vv) + wx + w0


def _torch_loss(loss, yhat, csr, group):
    sp = torch.nn.functional.softplus
    if loss == "logistic":
        has = torch.from_numpy(np.diff(csr.row_ptr) > 0)
        y = torch.from_numpy(csr.label)
        return (sp(yhat) - y * yhat)[has].sum()
    y2 = yhat.reshape(-1, group)
    return sp(-(y2[:, :1] - y2[:, 1:])).sum()


@pytest.mark.parametrize("loss,group,n_rows", [("logistic", 0, 50), ("bpr", 2, 50), ("bpr", 5, 50), ("bpr", 17, 51)])
@pytest.mark.parametrize("seed,k,reg", [(3, 4, 1e-4), (4, 8, 0.0), (5, 3, 2e-2)])
def test_step_is_the_autograd_gradient_step(loss, group, n_rows, seed, k, reg):
    F, t, step_size, w0 = 60, 3, 0.4, 0.125
    csr, ids, w, V = make_problem(seed, n_rows, F, k, 7, hot=5)  # a tenth of the rows are empty
    model = _model(F, k, ids, w, V, 7)  # some rows absent: the batch may still touch them
    model.w0 = w0
    w_0, V_0, present = model.w.copy(), model.V.copy(), model.present.copy()
    out = O.step(model, csr, t, step_size, reg, loss, group)
    eta = step_size / math.sqrt(t)
    lam, m = eta * reg, csr.n_rows
    wt = torch.tensor(w_0, requires_grad=True)
    Vt = torch.tensor(V_0, requires_grad=True)
    L = _torch_loss(loss, _torch_forward(wt, Vt, csr, w0), csr, group)
    gw, gV = torch.autograd.grad(L, (wt, Vt))
    assert out.loss_sum == pytest.approx(float(L.detach()), rel=1e-12)
    touched = np.unique(csr.col)
    rows = present.copy()
    rows[touched] = True
    for got, start, g in ((model.w, w_0, gw.numpy()), (model.V, V_0, gV.numpy())):
        exp = start.copy()
        exp[touched] = start[touched] - (eta / m) * g[touched]
        exp[rows] = R.soft_threshold(exp[rows], lam)
        np.testing.assert_allclose(got, exp, rtol=1e-12, atol=1e-15)
    assert np.array_equal(model.present, rows)
    empty = int((np.diff(csr.row_ptr) == 0).sum())
    assert empty > 0
    assert out.n_loss_rows == (m - empty if loss == "logistic" else (m // group) * (group - 1))


def test_bpr_reads_no_label_and_counts_pairs():
    csr, ids, w, V = make_problem(8, 40, 30, 4, 5)
    a, b = _model(30, 4, ids, w, V), _model(30, 4, ids, w, V)
    other = R.CSR(csr.row_ptr, csr.col, csr.val, csr.label + 3.0)
    oa = O.step(a, csr, 1, 0.3, 0.0, "bpr", 4)
    ob = O.step(b, other, 1, 0.3, 0.0, "bpr", 4)
    assert oa.loss_sum == ob.loss_sum and oa.n_loss_rows == ob.n_loss_rows == 30
    assert np.array_equal(a.w, b.w) and np.array_equal(a.V, b.V)


# ------------------------------------------------------------------------------- the stable forms
@pytest.mark.parametrize("z", [50.0, -50.0, 1000.0, -1000.0, 0.0, 745.2, -745.2])
def test_stable_forms_at_saturated_scores(z):
    s, p = float(O.sigmoid(z)), float(O.softplus(z))
    assert math.isfinite(s) and math.isfinite(p) and 0.0 <= s <= 1.0 and p >= 0.0
    # against the closed forms where they are exact to fp64: sigma(-z) = 1 - sigma(z), softplus(z) - softplus(-z) = z,
    # softplus(z) -> z and sigma(z) -> exp(z) / 1 in the tails
    assert s + float(O.sigmoid(-z)) == pytest.approx(1.0, abs=2e-16)
    assert p - float(O.softplus(-z)) == pytest.approx(z, rel=1e-15, abs=1e-15)
    if z >= 50.0:
        assert p == pytest.approx(z, rel=1e-15) and s == pytest.approx(1.0, abs=1e-15)
    if z <= -50.0:
        assert s == pytest.approx(math.exp(z), rel=1e-14, abs=0.0) and p == pytest.approx(math.exp(z), rel=1e-14, abs=0.0)
    if z == 0.0:
        assert s == 0.5 and p == pytest.approx(math.log(2.0), rel=1e-15)


@pytest.mark.parametrize("scale", [1.0, 50.0, 1000.0])
def test_objectives_stay_finite_at_saturated_scores(scale):
    rng = np.random.default_rng(0)
    yhat = scale * np.concatenate([rng.normal(size=60), [1.0, -1.0, 1.0, 1.0, -1.0, -1.0]])
    y = (rng.random(66) < 0.5).astype(np.float64)
    has = np.ones(66, bool)
    for loss, g in (("logistic", 0), ("bpr", 2), ("bpr", 6), ("bpr", 66)):
        r, yh, ls, n = O.objective(loss, yhat, y, has, g)
        assert np.all(np.isfinite(r)) and math.isfinite(ls) and ls >= 0.0 and r is yh
        if loss == "bpr":
            np.testing.assert_allclose(r.reshape(-1, g).sum(axis=1), 0.0, atol=1e-12 * g)  # a group's r sums to zero


# ------------------------------------------------------------------- what the fp32 score can move
@pytest.mark.parametrize("scale", [0.5, 8.0, 50.0])
def test_rounding_the_scores_moves_r_by_a_quarter_ulp_each(scale):
    """|sigma'| <= 1/4, and rounding to fp32 moves a score by at most 2^-24 |yhat|: a logistic r reads one
    score, a BPR negative's r two, a positive's 2 per negative."""
    rng = np.random.default_rng(1)
    g, G = 5, 400
    yhat = scale * rng.normal(size=g * G)
    y = (rng.random(g * G) < 0.3).astype(np.float64)
    has = np.ones(g * G, bool)
    y32 = yhat.astype(np.float32).astype(np.float64)
    q = 2.0 ** -24 * np.abs(yhat) / 4.0
    slack = 1e-16  # the fp64 rounding of the two evaluations themselves
    r0 = O.objective("logistic", yhat, y, has)[0]
    r1 = O.objective("logistic", y32, y, has)[0]
    assert np.all(np.abs(r1 - r0) <= q + slack)
    r0 = O.objective("bpr", yhat, y, has, g)[0].reshape(G, g)
    r1 = O.objective("bpr", y32, y, has, g)[0].reshape(G, g)
    q2 = q.reshape(G, g)
    pair = q2[:, 1:] + q2[:, :1]  # a negative's bound: its own score and its positive's
    assert np.all(np.abs(r1 - r0)[:, 1:] <= pair + slack)
    assert np.all(np.abs(r1 - r0)[:, 0] <= pair.sum(axis=1) + g * slack)


def test_round_scores_option_is_the_fp32_score():
    csr, ids, w, V = make_problem(9, 60, 40, 4, 6)
    a, b = _model(40, 4, ids, w, V), _model(40, 4, ids, w, V)
    O.step(a, csr, 1, 0.5, 0.0, "logistic")
    O.step(b, csr, 1, 0.5, 0.0, "logistic", round_scores=True)
    assert not np.array_equal(a.w, b.w)
    np.testing.assert_allclose(b.w, a.w, rtol=1e-6, atol=1e-9)


# ------------------------------------------------------------------------------ the C layout
def test_ctypes_config_mirror_has_loss_at_the_c_offset(tmp_path):
    from fm_spark_amd import _native as N

    src = tmp_path / "off.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fm_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", offsetof(fm_config, loss), offsetof(fm_config, wire), '
                   'sizeof(fm_config)); return 0; }\n')
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    loss_off, wire_off, size = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert N.fm_config.loss.offset == loss_off
    assert N.fm_config.wire.offset == wire_off
    assert C.sizeof(N.fm_config) == size
    assert N.fm_config._fields_[-1][0] == "loss"  # a new last field: 0 keeps the squared step
    assert (N.FM_LOSS_SQUARED, N.FM_LOSS_LOGISTIC, N.FM_LOSS_BPR) == (0, 1, 2)
    header = open(os.path.join(ROOT, "include", "fm_hip.h")).read()
    for name, val in (("FM_LOSS_SQUARED", 0), ("FM_LOSS_LOGISTIC", 1), ("FM_LOSS_BPR", 2)):
        assert re.search(rf"#define {name} {val}\b", header)
    for fn in ("fm_batch_set_group", "fm_batch_group"):
        assert fn in N.SIGNATURES and re.search(rf"\b{fn}\(", header)


# --------------------------------------------------------------------------- the estimator's rules
def _frame(labels):
    from fm_spark_amd.ml import DataFrame
    from fm_spark_amd.linalg import Vectors

    n = len(labels)
    return DataFrame({"label": [float(v) for v in labels], "features": [Vectors.sparse(4, [(i % 4, 1.0)]) for i in range(n)]})


def test_set_loss_and_its_refusals():
    from fm_spark_amd.ml import FactorizationMachinesSGD

    est = FactorizationMachinesSGD()
    assert est.getLoss() == "squared"
    assert est.setLoss("logistic") is est and est.getLoss() == "logistic"
    assert est.setLoss("bpr").getLoss() == "bpr"
    with pytest.raises(ValueError, match="loss must be"):
        est.setLoss("hinge")
    for loss in ("logistic", "bpr"):
        with pytest.raises(ValueError, match="validationData"):
            FactorizationMachinesSGD().setLoss(loss).setValidationData(_frame([0, 1]))
        with pytest.raises(ValueError, match="validationData"):
            FactorizationMachinesSGD().setValidationData(_frame([0, 1])).setLoss(loss)
        with pytest.raises(ValueError, match="one GPU"):
            FactorizationMachinesSGD().setLoss(loss).setParallel("sharded", 2)
        with pytest.raises(ValueError, match="one GPU"):
            FactorizationMachinesSGD().setParallel("replicated", 2).setLoss(loss)
    # squared keeps both, and un-setting either lets the loss through
    FactorizationMachinesSGD().setValidationData(_frame([0, 1])).setParallel("sharded", 2).setLoss("squared")
    FactorizationMachinesSGD().setValidationData(_frame([0, 1])).setValidationData(None).setLoss("logistic")
    FactorizationMachinesSGD().setLoss("logistic").setParallel(None)


def test_fit_refuses_before_touching_a_device():
    from fm_spark_amd.ml import FactorizationMachinesSGD

    with pytest.raises(ValueError, match=r"labels in \[0, 1\]"):
        FactorizationMachinesSGD().setLoss("logistic").fit(_frame([0.0, 1.0, 2.0]))
    with pytest.raises(ValueError, match=r"labels in \[0, 1\]"):
        FactorizationMachinesSGD().setLoss("logistic").fit(_frame([0.0, -0.5]))
    with pytest.raises(ValueError, match=r"labels in \[0, 1\]"):
        FactorizationMachinesSGD().setLoss("logistic").fit(_frame([0.0, float("nan")]))
    with pytest.raises(ValueError, match="bpr.*fitInteractions"):
        FactorizationMachinesSGD().setLoss("bpr").fit(_frame([0.0, 1.0]))
    # params that arrived through copy(extra) meet the same rules at fit
    est = FactorizationMachinesSGD().setLoss("logistic").copy({"parallel": "sharded"})
    with pytest.raises(ValueError, match="one GPU"):
        est.fit(_frame([0.0, 1.0]))
    est = FactorizationMachinesSGD().copy({"loss": "bpr", "negativesPerPositive": 0})
    ctxs, cands = _frame([0, 0]), _frame([0, 0, 0])
    from fm_spark_amd.ml import DataFrame

    inter = DataFrame({"context": [0, 1], "candidate": [1, 2]})
    with pytest.raises(ValueError, match="negativesPerPositive >= 1"):
        est.fitInteractions(ctxs, cands, inter)


def test_engine_refuses_an_unknown_loss_name():
    from fm_spark_amd.engine import FMContext

    with pytest.raises(ValueError, match="loss must be"):
        FMContext(4, 2, loss="hinge")
