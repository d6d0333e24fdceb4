"""The evaluation's host side, without a GPU: EvalSums' metric formulas, the evaluateModel /
setEvaluateOnDevice plumbing over a stub model, the C-ABI's declaration and binding, and eval_ref's
budget against a legitimate reordering (NumPy's pairwise sum)."""

import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

import eval_ref
from fm_spark_amd import _native as N
from fm_spark_amd.engine import EvalSums
from fm_spark_amd.ml import DataFrame
from fm_spark_amd.tuning import CrossValidator, RegressionEvaluator

ROOT = Path(__file__).resolve().parent.parent


def _sums(y, p, epoch=0):
    e = y - p
    return EvalSums(len(y), 0, epoch, math.fsum(e.tolist()), math.fsum(np.abs(e).tolist()), math.fsum((e * e).tolist()))


@pytest.mark.parametrize("seed,n", [(0, 1), (1, 17), (2, 1000)])
def test_metric_formulas_match_the_numpy_evaluator(seed, n):
    rng = np.random.default_rng(seed)
    y, p = rng.normal(0.3, 1.0, n), rng.normal(0.3, 1.0, n)
    s = _sums(y, p)
    df = DataFrame({"label": y.tolist(), "prediction": p.tolist()})
    for m, got in (("mae", s.mae), ("mse", s.mse), ("rmse", s.rmse)):
        assert got == pytest.approx(RegressionEvaluator().setMetricName(m).evaluate(df), rel=1e-12, abs=0)
    assert s.bias == pytest.approx(float(np.mean(y - p)), rel=1e-9, abs=1e-15)
    if n > 1:
        ss_tot = float(np.sum((y - y.mean()) ** 2))
        assert s.r2(ss_tot) == pytest.approx(RegressionEvaluator().setMetricName("r2").evaluate(df), rel=1e-12, abs=1e-12)


class _StubModel:
    """a model whose predictions are a column of the frame"""

    def __init__(self, calls):
        self._params = {"labelCol": "label", "minLabel": 0.0, "maxLabel": 1.0}
        self.calls = calls

    def copy(self, extra=None):
        return self

    def evaluate(self, df):
        self.calls.append("evaluate")
        return _sums(np.asarray(df["label"]), np.asarray(df["p"]))

    def transform(self, df):
        self.calls.append("transform")
        return df.with_column("prediction", df["p"])


class _StubEstimator:
    def __init__(self, calls):
        self.calls = calls

    def copy(self, extra=None):
        return self

    def fit(self, df):
        return _StubModel(self.calls)


@pytest.mark.parametrize("metric", ["mae", "mse", "rmse", "r2"])
def test_evaluate_model_takes_the_models_sums(metric):
    rng = np.random.default_rng(3)
    y, p = rng.normal(size=50), rng.normal(size=50)
    df = DataFrame({"label": y.tolist(), "p": p.tolist()})
    calls = []
    ev = RegressionEvaluator().setMetricName(metric)
    got = ev.evaluateModel(_StubModel(calls), df)
    assert calls == ["evaluate"]
    assert got == pytest.approx(ev.evaluate(df.with_column("prediction", p.tolist())), rel=1e-12, abs=1e-12)


def test_cross_validator_switches_the_path():
    rng = np.random.default_rng(4)
    df = DataFrame({"label": rng.normal(size=40).tolist(), "p": rng.normal(size=40).tolist()}, [20, 20])
    metrics = {}
    for on in (False, True):
        calls = []
        cv = (CrossValidator().setEstimator(_StubEstimator(calls)).setEstimatorParamMaps([{}])
              .setEvaluator(RegressionEvaluator().setMetricName("mae")).setNumFolds(2))
        assert cv.getEvaluateOnDevice() is False  # the default path stays
        cv.setEvaluateOnDevice(on)
        metrics[on] = cv.fit(df).avgMetrics
        assert calls == (["evaluate"] if on else ["transform"]) * 2
    assert metrics[True] == pytest.approx(metrics[False], rel=1e-12)


def test_header_and_binding_agree():
    header = (ROOT / "include" / "fm_hip.h").read_text()
    for name in ("fm_evaluate", "fm_evaluate_batch", "fm_eval_history"):
        assert re.search(r"^int %s\(fm_ctx\*" % name, header, flags=re.M), name
        assert name in N.SIGNATURES and N.SIGNATURES[name][0] is C.c_int
    body = re.search(r"typedef struct fm_eval_out \{(.*?)\} fm_eval_out;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int64_t|double)\s+(\w+);", body)
    ctype = {"int64_t": C.c_int64, "double": C.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(N.fm_eval_out._fields_)
    assert C.sizeof(N.fm_eval_out) == 48
    assert N.SIGNATURES["fm_evaluate_batch"][1][-2:] == [C.POINTER(C.c_double), C.POINTER(N.fm_eval_out)]
    assert "fm_evaluate" in (ROOT / "INTEGRATION.md").read_text()


def test_validation_data_param():
    from fm_spark_amd.ml import FactorizationMachinesSGD

    est = FactorizationMachinesSGD()
    assert est._params["validationData"] is None  # off by default
    df = DataFrame({"label": [0.0], "features": [None]})
    assert est.setValidationData(df, every=3)._params["validationData"] == (df, 3)
    assert est.copy()._params["validationData"] == (df, 3)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            est.setValidationData(df, every=bad)
    assert est.setValidationData(None)._params["validationData"] is None


@pytest.mark.parametrize("seed,n", [(0, 9), (1, 257), (2, 4099)])
def test_budget_holds_for_a_legitimate_reordering(seed, n):
    """NumPy sums pairwise, another order than fsum's exact one: it must sit inside the budget, and
    the budget must be tight enough to tell a wrong sum -- one term dropped -- from a right one."""
    rng = np.random.default_rng(seed)
    p = rng.random(n)
    y = p + np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (0.37 + 1e-3 * rng.random(n))  # cancelling errors
    ref = eval_ref.sums(y, p)
    e = y - p
    for s, terms in ((ref.err, e), (ref.abs_err, np.abs(e)), (ref.sq_err, e * e)):
        assert s.holds(float(np.sum(terms)))
        assert s.holds(float(np.sum(terms[::-1])))
        assert s.holds(float(np.sum(rng.permutation(terms))))
        acc = 0.0
        for t in terms:  # left to right
            acc += float(t)
        assert s.holds(acc)
        assert 0.0 < s.budget < 1e-6  # far below one term (>= 0.37^2)
        assert not s.holds(float(np.sum(terms[:-1])))
