"""The spark.ml tuning pieces the reference's demo drives the estimator with
(FactorizationMachinesSample.scala:41-70): ``ParamGridBuilder``, ``CrossValidator`` /
``CrossValidatorModel`` and ``RegressionEvaluator``, restated from Spark 2.1.0 (spark-mllib_2.11,
pinned in build.sbt:7-12) so that ``CrossValidator`` runs over ``FactorizationMachinesSGD`` exactly
as it does in Spark: it only calls ``copy`` / ``fit`` / ``transform``, so each fold and grid point
trains on the device through the same C-ABI, with several models alive at once (independent
fm_ctx handles).

Fold assignment replays ``MLUtils.kFold(dataset.toDF.rdd, numFolds, seed)``:
``PartitionwiseSampledRDD`` seeds partition p with the p-th ``java.util.Random(seed).nextLong()``,
and ``BernoulliCellSampler(lb, ub)`` keeps a row when its ``XORShiftRandom.nextDouble()`` lies in
``[lb, ub)`` with ``lb = (fold - 1) / numFolds`` and ``ub = fold / numFolds`` computed in Float; the
training set is the complement.  The default seed is ``"org.apache.spark.ml.tuning.CrossValidator"
.hashCode`` (HasSeed).
"""

from __future__ import annotations

import itertools

import numpy as np

from .engine import BinarySums
from .ml import DataFrame, Param
from .sampler import next_doubles

__all__ = ["Param", "ParamGridBuilder", "CrossValidator", "CrossValidatorModel", "RegressionEvaluator", "RankingEvaluator",
           "BinaryClassificationEvaluator", "binary_sums", "ranking_metric", "k_fold"]


def java_string_hash(s: str) -> int:
    """java.lang.String.hashCode (signed 32-bit, over UTF-16 code units)."""
    h = 0
    units = s.encode("utf-16-be")
    for i in range(0, len(units), 2):
        h = (31 * h + ((units[i] << 8) | units[i + 1])) & 0xFFFFFFFF
    return h - (1 << 32) if h >= (1 << 31) else h


class JavaRandom:
    """java.util.Random (48-bit LCG): the per-partition seeds of PartitionwiseSampledRDD."""

    _MULT, _ADD, _MASK = 0x5DEECE66D, 0xB, (1 << 48) - 1

    def __init__(self, seed: int):
        self.seed = (seed ^ self._MULT) & self._MASK

    def _next(self, bits: int) -> int:
        self.seed = (self.seed * self._MULT + self._ADD) & self._MASK
        r = self.seed >> (48 - bits)
        return r - (1 << bits) if r >= (1 << (bits - 1)) else r  # (int) cast of the top bits

    def next_long(self) -> int:
        v = (self._next(32) << 32) + self._next(32)
        v &= (1 << 64) - 1
        return v - (1 << 64) if v >= (1 << 63) else v


class ParamGridBuilder:
    """org.apache.spark.ml.tuning.ParamGridBuilder: the cartesian product of the added grids."""

    def __init__(self):
        self._grid = {}

    def addGrid(self, param, values):
        self._grid[param.name if isinstance(param, Param) else str(param)] = list(values)
        return self

    def baseOn(self, *pairs):
        for param, value in pairs:
            self.addGrid(param, [value])
        return self

    def build(self):
        names = list(self._grid)
        return [dict(zip(names, combo)) for combo in itertools.product(*(self._grid[n] for n in names))]


class RegressionEvaluator:
    """org.apache.spark.ml.evaluation.RegressionEvaluator (RegressionMetrics over
    (prediction, label)): rmse (default), mse, r2, mae."""

    def __init__(self):
        self._params = {"metricName": "rmse", "predictionCol": "prediction", "labelCol": "label"}

    def setMetricName(self, v):
        if v not in ("rmse", "mse", "r2", "mae"):
            raise ValueError(f"unsupported metric {v!r}")
        self._params["metricName"] = v
        return self

    def setPredictionCol(self, v):
        self._params["predictionCol"] = v
        return self

    def setLabelCol(self, v):
        self._params["labelCol"] = v
        return self

    def getMetricName(self):
        return self._params["metricName"]

    def isLargerBetter(self) -> bool:
        return self._params["metricName"] == "r2"

    def evaluate(self, dataset: DataFrame) -> float:
        p = np.asarray(dataset[self._params["predictionCol"]], dtype=np.float64)
        y = np.asarray(dataset[self._params["labelCol"]], dtype=np.float64)
        err = y - p
        m = self._params["metricName"]
        if m == "mae":
            return float(np.mean(np.abs(err)))
        mse = float(np.mean(err * err))
        if m == "mse":
            return mse
        if m == "rmse":
            return float(np.sqrt(mse))
        ss_tot = float(np.sum((y - y.mean()) ** 2))
        return 1.0 - float(np.sum(err * err)) / ss_tot  # r2

    def evaluateModel(self, model, dataset: DataFrame) -> float:
        """The metric of model.transform(dataset) from the error sums the device reduces
        (model.evaluate -> fm_evaluate): no prediction column is built.  The model's labelCol is the
        label; r2 takes SS_tot from the frame's labels here, with evaluate's two-pass formula.  The
        value differs from evaluate(model.transform(dataset)) by the summation order only."""
        s = model.evaluate(dataset)
        m = self._params["metricName"]
        if m == "mae":
            return float(s.mae)
        if m == "mse":
            return float(s.mse)
        if m == "rmse":
            return float(s.rmse)
        y = np.asarray(dataset[model._params["labelCol"]], dtype=np.float64)
        return float(s.r2(float(np.sum((y - y.mean()) ** 2))))


def binary_sums(score, label) -> BinarySums:
    """The binary record (engine.BinarySums, epoch 0) of scores read as logits against labels, in NumPy,
    with the device's definitions (include/fm_hip.h, fm_binary_out): positive where label > 0.5, predicted
    positive where score > 0, the log loss term max(s, 0) + log1p(exp(-|s|)) - label * s, and two_u over the
    ascending scores: a run [s, e) of equal scores with cp positives / A negatives before a position adds
    (cp[e] - cp[s]) (A[s] + A[e]).  -0.0 and +0.0 are one score."""
    s = np.asarray(score, dtype=np.float64) + 0.0
    y = np.asarray(label, dtype=np.float64)
    if s.shape != y.shape or s.ndim != 1:
        raise ValueError("score and label must be 1-d arrays of one length")
    n = len(s)
    pos = y > 0.5
    hit = s > 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        loss = float(np.sum(np.maximum(s, 0.0) + np.log1p(np.exp(-np.abs(s))) - y * s)) if n else 0.0
    order = np.argsort(s, kind="stable")
    ss, sp = s[order], pos[order]
    cp = np.concatenate([[0], np.cumsum(sp, dtype=np.int64)])
    heads = np.flatnonzero(np.concatenate([[True], ss[1:] != ss[:-1]])) if n else np.zeros(0, np.int64)
    ends = np.concatenate([heads[1:], [n]]).astype(np.int64) if n else heads
    two_u = sum(int(cp[e] - cp[b]) * int((b - cp[b]) + (e - cp[e])) for b, e in zip(heads.tolist(), ends.tolist()))
    return BinarySums(n, int(pos.sum()), 0, int(np.sum(pos & hit)), int(np.sum(~pos & hit)), int(two_u), loss)


class BinaryClassificationEvaluator:
    """org.apache.spark.ml.evaluation.BinaryClassificationEvaluator's shape over a raw score read as a
    logit: metricName areaUnderROC (default; exact, ties counted as half), logLoss (mean softplus(score) -
    label * score) or accuracy (score > 0 against label > 0.5).

    ``evaluate(frame)`` runs in NumPy over rawPredictionCol (default "rawPrediction") and labelCol.  Only a
    model fitted with loss "logistic" writes ``rawPrediction`` in transform; a squared model's frame has none
    and evaluate raises the frame's own missing-column error -- its ``prediction`` is clamped to [minLabel,
    maxLabel], which is no logit, though setRawPredictionCol("prediction") will rank by it for areaUnderROC
    (ties wherever the clamp binds).  ``evaluateModel(model, frame)`` asks the device
    (model.evaluateBinary -> fm_evaluate_binary), which scores every model by its unclamped score; for a
    logistic model the two agree in the integers and differ in logLoss by the summation order only."""

    def __init__(self):
        self._params = {"metricName": "areaUnderROC", "rawPredictionCol": "rawPrediction", "labelCol": "label"}

    def setMetricName(self, v):
        if v not in ("areaUnderROC", "logLoss", "accuracy"):
            raise ValueError(f"unsupported metric {v!r}")
        self._params["metricName"] = v
        return self

    def setRawPredictionCol(self, v):
        self._params["rawPredictionCol"] = v
        return self

    def setLabelCol(self, v):
        self._params["labelCol"] = v
        return self

    def getMetricName(self):
        return self._params["metricName"]

    def getRawPredictionCol(self):
        return self._params["rawPredictionCol"]

    def getLabelCol(self):
        return self._params["labelCol"]

    def isLargerBetter(self) -> bool:
        return self._params["metricName"] != "logLoss"

    def metric(self, sums: BinarySums) -> float:
        """this evaluator's metric of a record"""
        m = self._params["metricName"]
        return float(sums.auc if m == "areaUnderROC" else sums.logLoss if m == "logLoss" else sums.accuracy)

    def evaluate(self, dataset: DataFrame) -> float:
        return self.metric(binary_sums(dataset[self._params["rawPredictionCol"]], dataset[self._params["labelCol"]]))

    def evaluateModel(self, model, dataset: DataFrame) -> float:
        """The metric from the record the device forms (model.evaluateBinary): no score column is built.
        The model's labelCol is the label."""
        return self.metric(model.evaluateBinary(dataset))


RANKING_METRICS = ("ndcgAtK", "precisionAtK", "recallAtK", "hitRateAtK", "meanAveragePrecision", "meanReciprocalRank",
                   "auc")


def ranking_metric(name: str, k: int, ptr, position, n_eligible):
    """(mean over the contexts used, number of contexts used) of one ranking metric, from exact
    positions: context u's targets sit at ptr[u] .. ptr[u + 1] of ``position`` (0-based ranks among the
    context's n_eligible[u] eligible rows; -1: a target that is not eligible, left out).  Relevance is
    binary: a row is relevant where it is a target (the definitions of Spark's RankingMetrics).
    With p_0 < p_1 < ... the T positions of a context's eligible targets:
      precisionAtK          #{p_j < k} / k
      recallAtK             #{p_j < k} / T
      hitRateAtK            1 where some p_j < k
      ndcgAtK               sum_{p_j < k} 1 / log2(p_j + 2)  over  sum_{i < min(k, T)} 1 / log2(i + 2)
      meanAveragePrecision  (1 / T) sum_j (j + 1) / (p_j + 1), over the full ranking
      meanReciprocalRank    1 / (p_0 + 1)
      auc                   the share of (target, eligible non-target) pairs with the target ranked
                            first: sum_j ((N - 1 - p_j) - (T - 1 - j)) / (T (N - T)), N = n_eligible[u]
    A context without an eligible target -- for auc also one without an eligible non-target -- is
    left out of the mean; with no context left the value is NaN."""
    if name not in RANKING_METRICS:
        raise ValueError(f"unsupported metric {name!r}")
    k = int(k)
    if k < 1:
        raise ValueError("k must be >= 1")
    ptr = np.asarray(ptr, dtype=np.int64)
    position = np.asarray(position, dtype=np.int64)
    n_eligible = np.asarray(n_eligible, dtype=np.int64)
    if ptr.ndim != 1 or len(ptr) < 1 or len(n_eligible) != len(ptr) - 1 or ptr[0] != 0 or ptr[-1] != len(position):
        raise ValueError("ptr must hold one offset per context and one more, from 0 to len(position)")
    total, used = 0.0, 0
    for u in range(len(ptr) - 1):
        p = position[ptr[u]:ptr[u + 1]]
        p = np.sort(p[p >= 0])
        T, n = len(p), int(n_eligible[u])
        if T == 0 or (name == "auc" and n <= T):
            continue
        hits = int(np.sum(p < k))
        if name == "precisionAtK":
            v = hits / k
        elif name == "recallAtK":
            v = hits / T
        elif name == "hitRateAtK":
            v = float(hits > 0)
        elif name == "ndcgAtK":
            v = float(np.sum(1.0 / np.log2(p[:hits] + 2.0)) / np.sum(1.0 / np.log2(np.arange(min(k, T)) + 2.0)))
        elif name == "meanAveragePrecision":
            v = float(np.mean((np.arange(T) + 1.0) / (p + 1.0)))
        elif name == "meanReciprocalRank":
            v = 1.0 / (float(p[0]) + 1.0)
        else:  # auc: non-targets behind target j = rows behind it minus targets behind it
            v = float(np.sum((n - 1 - p) - (T - 1 - np.arange(T)))) / (T * (n - T))
        total += v
        used += 1
    return (total / used if used else float("nan")), used


class RankingEvaluator:
    """Ranking quality of held-out rows from their exact positions (fm_rank_positions): for every
    context, where its targets land among everything it has not seen.  metricName: ndcgAtK (default),
    precisionAtK, recallAtK, hitRateAtK, meanAveragePrecision, meanReciprocalRank, auc
    (``ranking_metric`` has the definitions); k (default 10) for the AtK ones.  After an evaluation
    ``numContextsUsed`` holds the number of contexts the mean was taken over."""

    def __init__(self):
        self._params = {"metricName": "ndcgAtK", "k": 10}
        self.numContextsUsed = None

    def setMetricName(self, v):
        if v not in RANKING_METRICS:
            raise ValueError(f"unsupported metric {v!r}")
        self._params["metricName"] = v
        return self

    def getMetricName(self):
        return self._params["metricName"]

    def setK(self, v):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError("k must be an integer >= 1")
        self._params["k"] = int(v)
        return self

    def getK(self) -> int:
        return self._params["k"]

    def isLargerBetter(self) -> bool:
        return True

    def evaluatePositions(self, ptr, position, n_eligible) -> float:
        """The metric from positions alone (pure NumPy, see ranking_metric)."""
        value, self.numContextsUsed = ranking_metric(self._params["metricName"], self._params["k"], ptr, position, n_eligible)
        return value

    def evaluateModel(self, model, contexts: DataFrame, candidates: DataFrame, targets, exclude=None) -> float:
        """The metric of `model` for the contexts' target rows among `candidates` minus each context's
        ``exclude`` list (the arguments of model.rankPositions): one device call for the positions."""
        ptr, _, position, _, n_eligible = model._rank_positions(contexts, candidates, targets, exclude)
        return self.evaluatePositions(ptr, position, n_eligible)


def k_fold(dataset: DataFrame, num_folds: int, seed: int):
    """MLUtils.kFold replay: [(training, validation)] per fold, partitions preserved."""
    if num_folds < 2:
        raise ValueError("numFolds must be >= 2")
    rnd = JavaRandom(seed)
    xs = [next_doubles(rnd.next_long(), n) for n in dataset.partition_sizes]  # sampler.setSeed(split.seed)
    folds = []
    nf = np.float32(num_folds)
    for fold in range(1, num_folds + 1):
        lb = float(np.float32(fold - 1) / nf)
        ub = float(np.float32(fold) / nf)
        val_idx, tr_idx, val_sizes, tr_sizes = [], [], [], []
        off = 0
        for x in xs:
            keep = (x >= lb) & (x < ub)
            rows = np.arange(off, off + len(x))
            val_idx.append(rows[keep])
            tr_idx.append(rows[~keep])
            val_sizes.append(int(keep.sum()))
            tr_sizes.append(int((~keep).sum()))
            off += len(x)
        folds.append((_take(dataset, np.concatenate(tr_idx), tr_sizes),
                      _take(dataset, np.concatenate(val_idx), val_sizes)))
    return folds


def _take(df: DataFrame, rows, sizes) -> DataFrame:
    return DataFrame({k: [v[int(r)] for r in rows] for k, v in df.columns.items()}, sizes)


class CrossValidatorModel:
    def __init__(self, uid, best_model, avg_metrics):
        self.uid = uid
        self.bestModel = best_model
        self.avgMetrics = list(avg_metrics)

    def transform(self, dataset: DataFrame) -> DataFrame:
        return self.bestModel.transform(dataset)


class CrossValidator:
    """org.apache.spark.ml.tuning.CrossValidator (Spark 2.1.0 fit): per fold, fit every param map
    on the training part, sum the evaluator's metric on the validation part, average over folds,
    refit the best param map (first best: maxBy / minBy) on the whole dataset."""

    def __init__(self, uid: str | None = None):
        self.uid = uid or "cv"
        self._params = {"numFolds": 3, "seed": java_string_hash("org.apache.spark.ml.tuning.CrossValidator")}
        self._est = self._epm = self._eval = None
        self._on_device = False

    def setEvaluateOnDevice(self, value: bool):
        """True: each fold's metric comes from evaluator.evaluateModel(model, validation) -- the error
        sums reduced on the device -- instead of evaluator.evaluate(model.transform(validation)).
        Default False: the two differ in summation order, so the default path stays as it is."""
        self._on_device = bool(value)
        return self

    def getEvaluateOnDevice(self) -> bool:
        return self._on_device

    def setEstimator(self, est):
        self._est = est
        return self

    def setEstimatorParamMaps(self, epm):
        self._epm = list(epm)
        return self

    def setEvaluator(self, ev):
        self._eval = ev
        return self

    def setNumFolds(self, n: int):
        self._params["numFolds"] = int(n)
        return self

    def setSeed(self, s: int):
        self._params["seed"] = int(s)
        return self

    def getSeed(self) -> int:
        return self._params["seed"]

    def fit(self, dataset: DataFrame) -> CrossValidatorModel:
        est, epm, ev = self._est, self._epm, self._eval
        if est is None or epm is None or ev is None:
            raise ValueError("estimator, estimatorParamMaps and evaluator must be set")
        metrics = np.zeros(len(epm))
        for training, validation in k_fold(dataset, self._params["numFolds"], self._params["seed"]):
            for i, pm in enumerate(epm):
                model = est.copy(pm).fit(training)
                mparams = {k: v for k, v in pm.items() if k in model._params}  # copyValues: the model's own params
                if self._on_device:
                    metrics[i] += ev.evaluateModel(model.copy(mparams), validation)
                else:
                    metrics[i] += ev.evaluate(model.copy(mparams).transform(validation))
        metrics /= self._params["numFolds"]
        best = int(np.argmax(metrics)) if ev.isLargerBetter() else int(np.argmin(metrics))
        best_model = est.copy(epm[best]).fit(dataset)
        return CrossValidatorModel(self.uid, best_model, metrics)
