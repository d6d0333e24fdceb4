"""CPU: the binary evaluation's host side -- tests/binary_ref.py's sorted two_u against the definition,
BinarySums' metrics and BinaryClassificationEvaluator on hand cases, the estimator's setter rules, and the
binding of the new C-ABI calls."""

import ctypes as C
import math

import numpy as np
import pytest

import binary_ref as B


# ------------------------------------------------------------------------------- the reference itself
def _tied_case(rng, n):
    """scores with heavy ties, both infinities, both zeros and denormals; 0/1 labels"""
    pool = np.array([-math.inf, math.inf, 0.0, -0.0, 5e-324, -5e-324, 2.2e-308, 1.0, -1.0, 1.0 + 2.0 ** -52, 0.5, 3.0])
    s = rng.choice(pool, n)
    mix = rng.random(n) < 0.3
    s = np.where(mix, np.round(rng.normal(0.0, 1.0, n), 1), s)
    return s, (rng.random(n) < rng.choice([0.1, 0.5, 0.9])).astype(np.float64)


@pytest.mark.parametrize("seed", range(40))
def test_sorted_two_u_is_the_quadratic_count(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 60))
    s, y = _tied_case(rng, n)
    want = B.two_u_quadratic(s, y)
    assert B.two_u_sorted(s, y) == want
    assert B.two_u_fast(s, y) == want
    from fm_spark_amd.tuning import binary_sums

    rec = binary_sums(s, y)
    assert B.integers_of(rec) == B.record(s, y, with_loss=False).integers


def test_signed_zeros_tie():
    s = np.array([0.0, -0.0, -0.0, 0.0])
    y = np.array([1.0, 0.0, 1.0, 0.0])
    assert B.two_u_quadratic(s, y) == 4  # every pair ties
    assert B.two_u_sorted(s, y) == 4 and B.two_u_fast(s, y) == 4
    # without the canonical zero a sort by the bit image would put -0.0 strictly below +0.0
    assert np.array([-0.0]).view(np.uint64)[0] != np.array([0.0]).view(np.uint64)[0]


def test_one_class_only_counts_nothing():
    s = np.array([0.3, -1.0, 0.3])
    assert B.two_u_sorted(s, np.ones(3)) == 0 and B.two_u_sorted(s, np.zeros(3)) == 0


def test_loss_terms_and_budget():
    s = np.array([0.0, 2.0, -2.0, 700.0, -700.0, 40.0])
    y = np.array([1.0, 0.0, 1.0, 1.0, 0.0, 0.25])
    t = B.loss_terms(s, y)
    assert np.all(np.isfinite(t))
    assert t[0] == pytest.approx(math.log(2.0))
    assert t[1] == pytest.approx(math.log1p(math.exp(2.0))) and t[2] == pytest.approx(t[1])
    assert t[3] == 0.0  # saturated and right: exp(-700) vanishes beside 700
    assert t[4] == pytest.approx(math.exp(-700.0))  # softplus(-700) = log1p(exp(-700))
    assert t[5] == pytest.approx(30.0)
    ref = B.log_loss(s, y)
    assert ref.value == pytest.approx(float(np.sum(t)))
    # the allowance at y = 1, s = 700 is absolute in |s|: about 3 U s, though the term itself is 0
    a = B.term_allowance(s, y)
    assert 2.9 * B.U * 700.0 <= a[3] <= 3.1 * B.U * 700.0
    assert ref.budget >= float(np.sum(a)) and ref.budget < 1e-11


# ------------------------------------------------------------------------------------ BinarySums
def test_binary_sums_properties_on_a_hand_case():
    from fm_spark_amd.engine import BinarySums

    # 10 rows, 4 positive; tp 3, fp 2 -> fn 1, tn 4; two_u 36 of 2 * 4 * 6 = 48
    r = BinarySums(10, 4, 7, 3, 2, 36, 5.0)
    assert r.n_neg == 6
    assert r.logLoss == 0.5
    assert r.auc == 0.75
    assert r.accuracy == 0.7
    assert r.precision == 0.6
    assert r.recall == 0.75
    assert r.f1 == pytest.approx(2 * 0.6 * 0.75 / (0.6 + 0.75))
    with pytest.raises(Exception):
        r.tp = 1  # frozen


def test_binary_sums_nan_where_a_denominator_is_zero():
    from fm_spark_amd.engine import BinarySums

    empty = BinarySums(0, 0, 0, 0, 0, 0, 0.0, executed=False)
    for name in ("logLoss", "auc", "accuracy", "precision", "recall", "f1"):
        assert math.isnan(getattr(empty, name)), name
    all_pos = BinarySums(5, 5, 0, 0, 0, 0, 1.0)  # nothing predicted positive
    assert math.isnan(all_pos.auc) and math.isnan(all_pos.precision)
    assert all_pos.recall == 0.0 and all_pos.accuracy == 0.0 and all_pos.f1 == 0.0 and all_pos.logLoss == 0.2
    all_neg = BinarySums(5, 0, 0, 0, 0, 0, 1.0)
    assert math.isnan(all_neg.auc) and math.isnan(all_neg.recall) and math.isnan(all_neg.precision) and math.isnan(all_neg.f1)
    assert all_neg.accuracy == 1.0


# ------------------------------------------------------------------------------------- evaluator
def _scored_frame(scores, labels, raw="rawPrediction", label="label"):
    from fm_spark_amd.ml import DataFrame

    return DataFrame({label: [float(v) for v in labels], raw: [float(v) for v in scores]})


def test_evaluator_metrics_on_a_hand_case():
    from fm_spark_amd.tuning import BinaryClassificationEvaluator

    #            pos    neg   pos   neg   neg
    scores = [2.0, 2.0, -1.0, 0.5, -3.0]
    labels = [1.0, 0.0, 1.0, 0.0, 0.0]
    # pairs (pos, neg): 2.0 v {2.0 tie, 0.5 win, -3 win} = 1 + 2 + 2; -1.0 v {2.0, 0.5 lose, -3 win} = 2 -> two_u 7 of 12
    ev = BinaryClassificationEvaluator()
    assert ev.getMetricName() == "areaUnderROC" and ev.isLargerBetter()
    assert ev.getRawPredictionCol() == "rawPrediction" and ev.getLabelCol() == "label"
    f = _scored_frame(scores, labels)
    assert ev.evaluate(f) == pytest.approx(7 / 12)
    acc = ev.setMetricName("accuracy")
    assert acc is ev and ev.isLargerBetter()
    assert ev.evaluate(f) == pytest.approx(2 / 5)  # right: row 0 (tp) and row 4 (tn)
    ev.setMetricName("logLoss")
    assert not ev.isLargerBetter()
    want = sum(math.log1p(math.exp(s)) - y * s for s, y in zip(scores, labels)) / 5
    assert ev.evaluate(f) == pytest.approx(want, rel=1e-14)
    with pytest.raises(ValueError, match="unsupported metric"):
        ev.setMetricName("areaUnderPR")
    # settable columns
    g = _scored_frame(scores, labels, raw="z", label="click")
    ev2 = BinaryClassificationEvaluator().setRawPredictionCol("z").setLabelCol("click")
    assert ev2.evaluate(g) == pytest.approx(7 / 12)
    with pytest.raises(Exception):
        BinaryClassificationEvaluator().evaluate(g)  # no rawPrediction column (a squared model's frame)


def test_evaluator_one_class_is_nan():
    from fm_spark_amd.tuning import BinaryClassificationEvaluator

    assert math.isnan(BinaryClassificationEvaluator().evaluate(_scored_frame([1.0, 2.0], [1.0, 1.0])))


def test_evaluate_model_reads_the_models_record():
    from fm_spark_amd.engine import BinarySums
    from fm_spark_amd.tuning import BinaryClassificationEvaluator

    class Fake:
        def evaluateBinary(self, frame):
            assert frame == "the frame"
            return BinarySums(10, 4, 7, 3, 2, 36, 5.0)

    ev = BinaryClassificationEvaluator()
    assert ev.evaluateModel(Fake(), "the frame") == 0.75
    assert ev.setMetricName("logLoss").evaluateModel(Fake(), "the frame") == 0.5
    assert ev.setMetricName("accuracy").evaluateModel(Fake(), "the frame") == 0.7


# ---------------------------------------------------------------------------------- setter rules
def _frame(labels):
    from fm_spark_amd.linalg import Vectors
    from fm_spark_amd.ml import DataFrame

    n = len(labels)
    return DataFrame({"label": [float(v) for v in labels], "features": [Vectors.sparse(4, [(i % 4, 1.0)]) for i in range(n)]})


def test_binary_validation_setter_rules():
    from fm_spark_amd.ml import DataFrame, FactorizationMachinesSGD

    f = _frame([0, 1])
    for loss in ("squared", "logistic"):
        est = FactorizationMachinesSGD().setLoss(loss).setBinaryValidationData(f, every=3)
        assert est._params["binaryValidationData"] == (f, 3)
        assert FactorizationMachinesSGD().setBinaryValidationData(f).setLoss(loss)._params["binaryValidationData"] == (f, 1)
    assert FactorizationMachinesSGD().setBinaryValidationData(f).setBinaryValidationData(None)._params["binaryValidationData"] is None
    # independent of validationData: both may be set (squared), and neither disturbs the other
    est = FactorizationMachinesSGD().setValidationData(f, 2).setBinaryValidationData(f, 5)
    assert est._params["validationData"] == (f, 2) and est._params["binaryValidationData"] == (f, 5)
    assert est.copy()._params["binaryValidationData"] == (f, 5)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="every"):
            FactorizationMachinesSGD().setBinaryValidationData(f, bad)
    # bpr, either order
    with pytest.raises(ValueError, match="binaryValidationData"):
        FactorizationMachinesSGD().setLoss("bpr").setBinaryValidationData(f)
    with pytest.raises(ValueError, match="binaryValidationData"):
        FactorizationMachinesSGD().setBinaryValidationData(f).setLoss("bpr")
    # multi-GPU, either order, and through copy(extra) at fit
    with pytest.raises(ValueError, match="binaryValidationData"):
        FactorizationMachinesSGD().setParallel("sharded", 2).setBinaryValidationData(f)
    with pytest.raises(ValueError, match="binaryValidationData"):
        FactorizationMachinesSGD().setBinaryValidationData(f).setParallel("replicated", 2)
    with pytest.raises(ValueError, match="binaryValidationData"):
        FactorizationMachinesSGD().setBinaryValidationData(f).copy({"parallel": "sharded"}).fit(_frame([0.0, 1.0]))
    FactorizationMachinesSGD().setBinaryValidationData(f).setParallel(None)
    # fitInteractions
    inter = DataFrame({"context": [0, 1], "candidate": [1, 2]})
    with pytest.raises(ValueError, match="binaryValidationData"):
        FactorizationMachinesSGD().setLoss("logistic").setBinaryValidationData(f).fitInteractions(_frame([0, 0]), _frame([0, 0, 0]), inter)


def test_validation_data_refusal_stands_and_points_to_the_new_setter():
    from fm_spark_amd.ml import FactorizationMachinesSGD

    f = _frame([0, 1])
    with pytest.raises(ValueError, match="validationData.*setBinaryValidationData"):
        FactorizationMachinesSGD().setLoss("logistic").setValidationData(f)
    with pytest.raises(ValueError, match="validationData.*setBinaryValidationData"):
        FactorizationMachinesSGD().setValidationData(f).setLoss("logistic")


def test_model_keeps_a_binary_validation_history():
    import inspect

    from fm_spark_amd import ml

    src = inspect.getsource(ml.FactorizationMachinesModel.__init__)
    assert "binaryValidationHistory" in src
    assert hasattr(ml.FactorizationMachinesModel, "evaluateBinary")


# ------------------------------------------------------------------------------------- binding
def test_binding_and_record_layout():
    from fm_spark_amd import _native as N

    lib = N.load()
    assert C.sizeof(N.fm_binary_out) == 56
    assert [f[0] for f in N.fm_binary_out._fields_] == ["n_rows", "n_pos", "epoch", "tp", "fp", "two_u", "sum_log_loss"]
    for name in ("fm_binary_metrics", "fm_evaluate_binary", "fm_evaluate_binary_batch", "fm_eval_binary_history"):
        assert name in N.SIGNATURES and hasattr(lib, name)
    out = N.fm_binary_out()
    n = C.c_int64()
    assert lib.fm_binary_metrics(None, None, None, 0, C.byref(out)) == -1
    assert b"null" in lib.fm_last_error()
    assert lib.fm_evaluate_binary(None, None, None, C.byref(out)) == -1
    assert lib.fm_evaluate_binary_batch(None, None, None, None) == -1
    assert lib.fm_eval_binary_history(None, None, 0, C.byref(n)) == -1
