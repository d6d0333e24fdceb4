"""The binary evaluation through the spark.ml mirror: FactorizationMachinesModel.evaluateBinary,
BinaryClassificationEvaluator.evaluateModel, CrossValidator.setEvaluateOnDevice with it, and fit's
setBinaryValidationData.

Integers (class and confusion counts, two_u) are exact wherever two paths see the same scores.  The device's
log loss sum and NumPy's are both within tests/binary_ref.py's budget of the exact sum over the same scores,
so they differ by at most twice that budget."""

import math

import numpy as np
import pytest

import binary_ref as B
from fm_spark_amd.linalg import Vectors

pytestmark = pytest.mark.gpu


def _frame(seed, n, nf=60, parts=3):
    from fm_spark_amd.ml import DataFrame

    rng = np.random.default_rng(seed)
    truth = np.random.default_rng(99).normal(0.0, 1.5, 64)  # the labels follow the features: there is something to learn
    rows = []
    for _ in range(n):
        z = int(rng.integers(0, 7))  # some rows without entries
        ids = rng.choice(nf, z, replace=False)
        x = np.float32(rng.normal(0.0, 1.0, z)).astype(np.float64)
        y = float(rng.random() < 1.0 / (1.0 + math.exp(-float(np.dot(truth[ids], x)))))
        rows.append((y, Vectors.sparse(nf, [(int(i), float(v)) for i, v in zip(ids, x)])))
    return DataFrame.from_rows(rows, ["label", "features"], num_partitions=parts)


def _est(loss="logistic"):
    from fm_spark_amd.ml import FactorizationMachinesSGD

    return (FactorizationMachinesSGD().setDimFactorization(6).setMaxIter(5).setStepSize(0.5).setRegParam(1e-4)
            .setMiniBatchFraction(0.15).setNumFeatures(60).setSeed(4).setLoss(loss))


def test_evaluate_binary_matches_numpy_over_transform(gpu):
    from fm_spark_amd.tuning import BinaryClassificationEvaluator, binary_sums

    train, held = _frame(1, 400), _frame(2, 257, nf=64)  # ids 60..63: beyond the table, dropped by both paths
    model = _est().fit(train)
    out = model.transform(held)
    y = np.asarray(held["label"])
    raw = np.asarray(out["rawPrediction"])
    s = model.evaluateBinary(held)
    ref = B.check(s, raw, y, loss_budgets=1.0)  # the device's record over transform's own scores
    host = binary_sums(raw, y)
    assert B.integers_of(host) == B.integers_of(s)
    assert abs(host.sum_log_loss - s.sum_log_loss) <= 2 * ref.loss.budget
    assert 0 < s.n_pos < 257 and s.epoch == 5
    for m, got in (("areaUnderROC", s.auc), ("accuracy", s.accuracy), ("logLoss", s.logLoss)):
        ev = BinaryClassificationEvaluator().setMetricName(m)
        assert ev.evaluateModel(model, held) == got
        if m == "logLoss":
            assert abs(ev.evaluate(out) - got) <= 2 * ref.loss.budget / 257 + 4 * B.U * got
        else:
            assert ev.evaluate(out) == got  # the same integers through the same division
    assert s.auc > 0.5  # it did learn something
    # a squared model is scored by its unclamped score too, which transform does not show
    sq = _est("squared").fit(train)
    r = sq.evaluateBinary(held)
    assert r.n_rows == 257 and r.n_pos == s.n_pos and math.isfinite(r.logLoss)
    assert "rawPrediction" not in sq.transform(held).columns


def test_fit_with_binary_validation_data(gpu):
    train, held = _frame(5, 400), _frame(6, 120)
    plain = _est().fit(train)
    fits = {p: _est().setBinaryValidationData(held, every=2).fit(train, pipelined=p) for p in (True, False)}
    hist = {p: m.binaryValidationHistory for p, m in fits.items()}
    assert [it for it, _ in hist[True]] == [it for it, _ in hist[False]] == [2, 4, 5]
    assert [s for _, s in hist[True]] == [s for _, s in hist[False]]  # bitwise
    assert [s.epoch for _, s in hist[True]] == [2, 4, 5]
    assert all(s.n_rows == 120 and s.executed for _, s in hist[True])
    assert plain.binaryValidationHistory == [] and all(m.validationHistory == [] for m in fits.values())
    for m in fits.values():  # evaluating changed nothing of the fit
        for x, y in zip(m._ctx.export_tables(), plain._ctx.export_tables()):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(m._ctx.loss_history(), plain._ctx.loss_history())
    # the last record is the fitted model's own evaluation of the frame (every id of it fits the table, so
    # both upload the same rows: the same scores)
    last, own = hist[True][-1][1], fits[True].evaluateBinary(held)
    assert B.integers_of(own) == B.integers_of(last) and own.epoch == last.epoch
    assert own.sum_log_loss == last.sum_log_loss
    # a squared fit takes it as well, beside validationData; each history has its own records
    both = _est("squared").setValidationData(held, every=3).setBinaryValidationData(held, every=2).fit(train)
    assert [it for it, _ in both.validationHistory] == [3, 5] and [it for it, _ in both.binaryValidationHistory] == [2, 4, 5]
    assert type(both.validationHistory[0][1]).__name__ == "EvalSums"
    assert type(both.binaryValidationHistory[0][1]).__name__ == "BinarySums"
    # off again
    assert _est().setBinaryValidationData(held).setBinaryValidationData(None).fit(train).binaryValidationHistory == []


def test_cross_validator_with_the_binary_evaluator(gpu):
    from fm_spark_amd.tuning import BinaryClassificationEvaluator, CrossValidator, ParamGridBuilder

    df = _frame(3, 300)
    est = _est().setMaxIter(3)
    grid = ParamGridBuilder().addGrid(est.regParam, [1e-4, 0.2]).addGrid(est.stepSize, [0.5, 0.05]).build()
    res = {}
    for metric in ("logLoss", "areaUnderROC"):
        for on in (False, True):
            cv = (CrossValidator().setEstimator(est).setEstimatorParamMaps(grid).setNumFolds(2)
                  .setEvaluator(BinaryClassificationEvaluator().setMetricName(metric)).setEvaluateOnDevice(on))
            res[metric, on] = cv.fit(df)
    # areaUnderROC: exact integers through the same division on both paths
    assert res["areaUnderROC", False].avgMetrics == res["areaUnderROC", True].avgMetrics
    # logLoss.  Three steps of at most 0.5 from a draw of sd 0.01 leave every |score| far below 100 (asserted
    # on the best model below), so a row's term is at most 2 * 100 + ln 2 < 201 and a fold of n <= 300 rows has a
    # budget of at most (n + 1) 201 n U for the reordered sum plus n (12 + 3 * 100 + 2 * 201) U of per-term
    # allowance (binary_ref: e, L <= 1; m + L, |y s| <= 101; |t| < 201); the means differ by at most twice that
    # over n, plus the divisions' roundings
    n = 300
    bound = 2 * ((n + 1) * 201 + (12 + 300 + 402)) * B.U + 4 * B.U * 201
    a, b = np.asarray(res["logLoss", False].avgMetrics), np.asarray(res["logLoss", True].avgMetrics)
    print("avgMetrics", a.tolist(), b.tolist(), "bound", bound)
    assert np.all(np.abs(a - b) <= bound)
    gaps = np.abs(a[:, None] - a[None, :])[~np.eye(len(a), dtype=bool)]
    assert gaps.min() > 2 * bound  # not tied: both runs pick the same grid point
    best = res["logLoss", True].bestModel
    assert np.max(np.abs(np.asarray(best.transform(df)["rawPrediction"]))) < 100.0
    for x, y in zip(res["logLoss", False].bestModel._ctx.export_tables(), best._ctx.export_tables()):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(res["areaUnderROC", False].bestModel._ctx.export_tables(), res["areaUnderROC", True].bestModel._ctx.export_tables()):
        np.testing.assert_array_equal(x, y)
