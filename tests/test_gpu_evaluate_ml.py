"""The evaluation through the spark.ml mirror: FactorizationMachinesModel.evaluate,
RegressionEvaluator.evaluateModel, CrossValidator.setEvaluateOnDevice and fit's setValidationData.

The device's sums and NumPy's are both reorderings of the same fp64 terms, each within eval_ref's budget
of the exact sum, so two of them differ by at most twice that budget; the metric bounds below carry it
through each formula (plus the roundings of the formula's own operations, 2^-53 relative each).
"""

import numpy as np
import pytest

import eval_ref
from fm_spark_amd.linalg import Vectors

pytestmark = pytest.mark.gpu

U = eval_ref.U


def _frame(seed, n, nf=60, parts=3, labels="binary"):
    from fm_spark_amd.ml import DataFrame

    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        z = int(rng.integers(0, 7))  # some rows without entries
        ids = rng.choice(nf, z, replace=False)
        x = np.float32(rng.normal(0.0, 1.0, z)).astype(np.float64)
        y = float(rng.integers(0, 2)) if labels == "binary" else float(np.float32(rng.normal(0.3, 0.5)))
        rows.append((y, Vectors.sparse(nf, [(int(i), float(v)) for i, v in zip(ids, x)])))
    return DataFrame.from_rows(rows, ["label", "features"], num_partitions=parts)


def _est():
    from fm_spark_amd.ml import FactorizationMachinesSGD

    return (FactorizationMachinesSGD().setDimFactorization(6).setMaxIter(5).setStepSize(0.5).setRegParam(1e-4)
            .setMiniBatchFraction(0.15).setNumFeatures(60).setSeed(4))


def test_model_evaluate_matches_the_evaluator_over_transform(gpu):
    from fm_spark_amd.tuning import RegressionEvaluator

    train, held = _frame(1, 400), _frame(2, 257, nf=64, labels="real")  # ids 60..63: beyond the table
    model = _est().fit(train).setMinLabel(-0.2).setMaxLabel(1.1)
    out = model.transform(held)
    y = np.asarray(held["label"])
    p = np.asarray(out["prediction"])
    s = model.evaluate(held)
    ref = eval_ref.check(s, y, p)  # the device's sums over transform's own predictions
    n = len(y)
    ss_tot = float(np.sum((y - y.mean()) ** 2))
    dmse = 2 * ref.sq_err.budget / n + 4 * U * s.mse
    got = {"mae": s.mae, "mse": s.mse, "rmse": s.rmse, "r2": s.r2(ss_tot)}
    bound = {
        "mae": 2 * ref.abs_err.budget / n + 4 * U * s.mae,
        "mse": dmse,
        # a - b = (a^2 - b^2) / (a + b), and one rounding per square root
        "rmse": dmse / (2 * s.rmse) * (1 + 1e-6) + 4 * U * s.rmse,
        "r2": 2 * ref.sq_err.budget / ss_tot + 6 * U * (1 + s.sum_sq_err / ss_tot),
    }
    for m in ("mae", "mse", "rmse", "r2"):
        ev = RegressionEvaluator().setMetricName(m)
        host = ev.evaluate(out)
        print(m, repr(got[m]), repr(host), "bound", bound[m])
        assert abs(got[m] - host) <= bound[m], (m, got[m], host, bound[m])
        assert ev.evaluateModel(model, held) == got[m]
    assert s.n_rows == n and s.n_unlearned >= 1


def test_cross_validator_on_device(gpu):
    from fm_spark_amd.tuning import CrossValidator, ParamGridBuilder, RegressionEvaluator

    df = _frame(3, 300)
    est = _est().setMaxIter(3)
    grid = ParamGridBuilder().addGrid(est.regParam, [1e-4, 0.2]).addGrid(est.stepSize, [0.5, 0.05]).build()
    res = {}
    for on in (False, True):
        cv = (CrossValidator().setEstimator(est).setEstimatorParamMaps(grid).setNumFolds(2)
              .setEvaluator(RegressionEvaluator().setMetricName("mae")).setEvaluateOnDevice(on))
        assert cv.getEvaluateOnDevice() is on
        res[on] = cv.fit(df)
    a, b = np.asarray(res[False].avgMetrics), np.asarray(res[True].avgMetrics)
    # labels in {0, 1}, predictions clamped to [0, 1]: every |e| <= 1, so a fold of n <= 300 rows has a
    # budget of at most (n + 1) n 2^-53 per sum and its two mae differ by at most 2 (n + 1) 2^-53 (+ the
    # divisions' roundings); the average over the folds no more
    bound = 2 * (300 + 3) * U
    print("avgMetrics", a.tolist(), b.tolist(), "bound", bound)
    assert np.all(np.abs(a - b) <= bound)
    gaps = np.abs(a[:, None] - a[None, :])[~np.eye(len(a), dtype=bool)]
    assert gaps.min() > 2 * bound  # not tied: both runs pick the same grid point
    for x, y in zip(res[False].bestModel._ctx.export_tables(), res[True].bestModel._ctx.export_tables()):
        np.testing.assert_array_equal(x, y)


def test_fit_with_validation_data(gpu):
    train, held = _frame(5, 400), _frame(6, 120, nf=64)
    plain = _est().fit(train)
    fits = {p: _est().setValidationData(held, every=2).fit(train, pipelined=p) for p in (True, False)}
    hist = {p: m.validationHistory for p, m in fits.items()}
    assert [it for it, _ in hist[True]] == [it for it, _ in hist[False]] == [2, 4, 5]
    assert [s for _, s in hist[True]] == [s for _, s in hist[False]]  # bitwise, on a single table
    assert [s.epoch for _, s in hist[True]] == [2, 4, 5]
    assert all(s.n_rows == 120 for _, s in hist[True])
    assert plain.validationHistory == []
    for m in fits.values():
        for x, y in zip(m._ctx.export_tables(), plain._ctx.export_tables()):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(m._ctx.loss_history(), plain._ctx.loss_history())
    # the last record is the fitted model's evaluation of the frame (model.evaluate uploads the frame's
    # rows as they are and the kernel drops the ids beyond the table; fit dropped them before its upload,
    # so the entries sit in other lanes: the same terms in another order)
    last, own = hist[True][-1][1], fits[True].evaluate(held)
    assert (own.n_rows, own.n_unlearned, own.epoch) == (last.n_rows, last.n_unlearned, last.epoch)
    np.testing.assert_allclose([own.sum_err, own.sum_abs_err, own.sum_sq_err],
                               [last.sum_err, last.sum_abs_err, last.sum_sq_err], rtol=1e-9, atol=1e-9)
    # off again
    assert _est().setValidationData(held).setValidationData(None).fit(train).validationHistory == []


def test_fit_with_validation_data_on_several_gpus(gpu):
    train, held = _frame(5, 400), _frame(6, 120, nf=64)
    single = _est().setValidationData(held, every=2).fit(train)
    multi = (_est().setParallel("sharded", n_gpus=2, devices=[0, 0], transport="copy", wire="fp64")
             .setValidationData(held, every=2).fit(train))
    assert [it for it, _ in multi.validationHistory] == [it for it, _ in single.validationHistory]
    for (_, a), (_, b) in zip(multi.validationHistory, single.validationHistory):
        assert (a.n_rows, a.n_unlearned, a.epoch) == (b.n_rows, b.n_unlearned, b.epoch)
        # the two models' predictions agree as test_fit_and_transform_on_several_gpus holds them (rtol
        # 1e-5, atol 1e-7 of values in [0, 1]): each of the 120 errors moves by at most 1.01e-5, and each
        # square, of an error of at most 1, by twice that
        np.testing.assert_allclose([a.sum_err, a.sum_abs_err, a.sum_sq_err], [b.sum_err, b.sum_abs_err, b.sum_sq_err],
                                   rtol=0, atol=120 * 2.1e-5)
