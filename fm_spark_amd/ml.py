"""Host-side mirror of the reference's spark.ml API over the C-ABI.

    FactorizationMachinesSGD   <- FactorizationMachinesSGD.scala:28-86, 254-256 (Estimator)
    FactorizationMachinesModel <- FactorizationMachinesModel.scala:43-133, 135-241 (Model)
    Strength, FactorizedInteraction <- FactorizationMachinesModel.scala:281, :289
    VectorSum                  <- FactorizationMachines.scala:45-81 (UDAF)

Same names, Params, defaults and error behaviour as the Scala classes.  The per-iteration
work of ``fit`` (the foldLeft body, SGD.scala:116-211) runs as one fm_step per mini-batch on
the GPU; the mini-batches come from the randomSplit replay (fm_random_split).  ``DataFrame``
is a minimal local stand-in for a Spark DataFrame: named columns plus a partitioning (the
partitioning matters: randomSplit sorts and samples per partition).

Scala-side integration (JNI) is described in INTEGRATION.md; this module is what the parity
tests drive.
"""

from __future__ import annotations

import logging
import math
import uuid
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from . import _native as N
from .engine import BinarySums, EvalSums, FMContext, normalize_row_lists
from .linalg import DenseVector, Vector, Vectors, active_map

log = logging.getLogger("org.apache.spark.ml.fm")


@dataclass(frozen=True)
class Param:
    """A named parameter of an estimator (org.apache.spark.ml.param.Param): ``fm.regParam``;
    param maps (ParamGridBuilder, ``copy(extra)``) are keyed by its name."""

    parent: str
    name: str


# ------------------------------------------------------------------------ DataFrame
class DataFrame:
    """Columns by name + partition sizes (rows laid out partition after partition)."""

    def __init__(self, columns: dict, partition_sizes=None):
        self.columns = {k: list(v) for k, v in columns.items()}
        n = len(next(iter(self.columns.values()))) if self.columns else 0
        for k, v in self.columns.items():
            if len(v) != n:
                raise ValueError(f"column {k} has {len(v)} rows, expected {n}")
        self.partition_sizes = list(partition_sizes) if partition_sizes is not None else [n]
        if sum(self.partition_sizes) != n:
            raise ValueError("partition sizes do not add up to the row count")

    @staticmethod
    def from_rows(rows, names, num_partitions: int = 1) -> "DataFrame":
        """Seq(rows).toDF(names) on local[num_partitions]: ParallelCollectionRDD slicing,
        slice i = [i*n/p, (i+1)*n/p)."""
        rows = list(rows)
        cols = {nm: [r[i] for r in rows] for i, nm in enumerate(names)}
        n = len(rows)
        sizes = [((i + 1) * n) // num_partitions - (i * n) // num_partitions for i in range(num_partitions)]
        return DataFrame(cols, sizes)

    @property
    def schema(self):
        return list(self.columns)

    def count(self) -> int:
        return sum(self.partition_sizes)

    def __len__(self):
        return self.count()

    def collect(self):
        names = self.schema
        return [dict(zip(names, vals)) for vals in zip(*[self.columns[n] for n in names])]

    def with_column(self, name, values) -> "DataFrame":
        cols = dict(self.columns)
        cols[name] = list(values)
        return DataFrame(cols, self.partition_sizes)

    def __getitem__(self, name):
        return self.columns[name]


# ------------------------------------------------------------------------ table rows
class Strength(NamedTuple):
    """Strength(id: Int, strength: Double), FactorizationMachinesModel.scala:281."""

    id: int
    strength: float


class FactorizedInteraction(NamedTuple):
    """FactorizedInteraction(id: Int, vec: DenseVector), FactorizationMachinesModel.scala:289."""

    id: int
    vec: DenseVector


def _explode(vectors):
    """explode(udfVecToMap(features)) (Model.scala:148-153, :244-250) -> CSR arrays."""
    row_ptr = np.zeros(len(vectors) + 1, dtype=np.int64)
    cols, vals = [], []
    for i, v in enumerate(vectors):
        m = active_map(v)
        for j in sorted(m):
            cols.append(j)
            vals.append(m[j])
        row_ptr[i + 1] = len(cols)
    return row_ptr, np.asarray(cols, dtype=np.int32), np.asarray(vals, dtype=np.float64)


def _sigmoid(z):
    """sigma(z) from exp(-|z|): finite for every finite z."""
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _check_schema(df: DataFrame, features_col: str, label_col: str | None):
    """validateAndTransformSchema (FactorizationMachines.scala:33-37): features must be
    vectors (VectorUDT), the label a double."""
    if features_col not in df.columns:
        raise ValueError(f"Column {features_col} does not exist.")
    for v in df.columns[features_col]:
        if not isinstance(v, Vector):
            raise ValueError(f"Column {features_col} must be of type VectorUDT")
    if label_col is not None:
        if label_col not in df.columns:
            raise ValueError(f"Column {label_col} does not exist.")
        for y in df.columns[label_col]:
            if not isinstance(y, (float, np.floating)):
                raise ValueError(f"Column {label_col} must be of type DoubleType")


# ------------------------------------------------------------------------- VectorSum
class VectorSum:
    """UDAF summing k-vectors per group (FactorizationMachines.scala:45-81), on the device:
    the stable radix sort groups the keys, each group is summed in fp64 in input order."""

    def __init__(self, vec_size: int, ctx: FMContext | None = None):
        self.vec_size = int(vec_size)
        self._ctx = ctx

    def __call__(self, keys, vectors):
        ctx = self._ctx or FMContext(1, 1)
        vecs = np.zeros((len(vectors), self.vec_size))
        for i, v in enumerate(vectors):
            if v is None:
                continue  # update: if (input.isNullAt(0)) return  (FactorizationMachines.scala:57)
            a = v.to_array()
            vecs[i, :] = a[: self.vec_size]
        k, s = ctx.vector_sum_by_key(np.asarray(keys, dtype=np.int32), vecs)
        return {int(kk): DenseVector(ss) for kk, ss in zip(k, s)}


# ----------------------------------------------------------------------------- Model
class FactorizationMachinesModel:
    """FactorizationMachinesModel.scala:43-241.  The Strength / FactorizedInteraction tables
    live on the device (fm_ctx); ``dimensionStrength`` / ``factorizedInteraction`` export them."""

    def __init__(self, uid: str, dimFactorization: int, globalBias: float, dimensionStrength=None,
                 factorizedInteraction=None, *, num_features: int | None = None, ctx: FMContext | None = None,
                 device: int = 0):
        self.uid = uid
        self.dimFactorization = int(dimFactorization)
        self.globalBias = float(globalBias)
        self._params = {"sampleIdCol": "sampleId", "featuresCol": "features", "predictionCol": "prediction",
                        "labelCol": "label", "minLabel": 0.0, "maxLabel": 1.0,  # Model.scala:54-61
                        # not in the reference: the objective the model was fitted with (setLoss)
                        "loss": "squared", "rawPredictionCol": "rawPrediction"}
        self.parent = None
        # fit with setValidationData: [(iteration, EvalSums)] of the held-out frame during the fit
        self.validationHistory = []
        # fit with setBinaryValidationData: [(iteration, BinarySums)] likewise
        self.binaryValidationHistory = []
        if ctx is not None:
            self._ctx = ctx
        else:
            ds = list(dimensionStrength or [])
            fi = list(factorizedInteraction or [])
            ids = sorted({s.id for s in ds} | {f.id for f in fi})
            F = num_features if num_features is not None else (max(ids) + 1 if ids else 1)
            self._ctx = FMContext(F, self.dimFactorization, device=device, w0=self.globalBias)
            if ids:
                w = {s.id: s.strength for s in ds}
                vec = {f.id: f.vec.to_array() for f in fi}
                ids_a = np.asarray(ids, dtype=np.int32)
                w_a = np.asarray([w.get(i, 0.0) for i in ids])
                V_a = np.asarray([vec.get(i, np.zeros(self.dimFactorization)) for i in ids])
                self._ctx.load_tables(ids_a, w_a, V_a)

    # params ----------------------------------------------------------------------------
    def setMinLabel(self, value: float):
        self._params["minLabel"] = float(value)
        return self

    def setMaxLabel(self, value: float):
        self._params["maxLabel"] = float(value)
        return self

    def getMinLabel(self) -> float:
        return self._params["minLabel"]

    def getMaxLabel(self) -> float:
        return self._params["maxLabel"]

    def copy(self, extra: dict | None = None) -> "FactorizationMachinesModel":
        """Model.scala:63-66: same tables, params copied then overridden by extra."""
        m = FactorizationMachinesModel(self.uid, self.dimFactorization, self.globalBias, ctx=self._ctx)
        m._params = dict(self._params)
        m._params.update(extra or {})
        m.parent = self.parent
        m.validationHistory = list(self.validationHistory)
        m.binaryValidationHistory = list(self.binaryValidationHistory)
        return m

    # tables ------------------------------------------------------------------------------
    @property
    def dimensionStrength(self):
        ids, w, _ = self._ctx.export_tables()
        return [Strength(int(i), float(x)) for i, x in zip(ids, w)]

    @property
    def factorizedInteraction(self):
        ids, _, V = self._ctx.export_tables()
        return [FactorizedInteraction(int(i), DenseVector(v)) for i, v in zip(ids, V)]

    # transform / predict ---------------------------------------------------------------
    def transformSchema(self, schema):
        if self._params["loss"] == "logistic":
            return list(schema) + [self._params["rawPredictionCol"], self._params["predictionCol"]]
        return list(schema) + [self._params["predictionCol"]]

    def transform(self, dataset: DataFrame) -> DataFrame:
        """Model.scala:69-87 + predict :90-133: inner-join semantics for unknown ids, clamp to
        [minLabel, maxLabel], rows without a learned feature get globalBias (na.fill).

        A model fitted with loss "logistic" adds two columns instead: ``rawPrediction``, the unclamped
        score (fm_predict with -inf / +inf; globalBias for a row without a learned feature), and
        ``prediction`` = sigma(rawPrediction), the probability of label 1.  minLabel / maxLabel are not
        applied there: they bound a regression's label, not a score.  Models of the other losses
        transform as the reference's ("bpr" scores order candidates; they are no label estimate)."""
        fcol = self._params["featuresCol"]
        _check_schema(dataset, fcol, None)
        rp, col, val = _explode(dataset[fcol])
        csr = N.CSRHost(rp, col, val, np.zeros(dataset.count()))
        if self._params["loss"] == "logistic":
            raw = self._ctx.predict(csr, -np.inf, np.inf)
            out = dataset.with_column(self._params["rawPredictionCol"], [float(z) for z in raw])
            return out.with_column(self._params["predictionCol"], [float(q) for q in _sigmoid(raw)])
        pred = self._ctx.predict(csr, self.getMinLabel(), self.getMaxLabel())
        return dataset.with_column(self._params["predictionCol"], [float(p) for p in pred])

    def evaluate(self, dataset: DataFrame) -> EvalSums:
        """The error sums of transform(dataset) against labelCol, reduced on the device in one pass
        (fm_evaluate): no prediction column is built or downloaded.  The predictions are transform's
        (clamped to [minLabel, maxLabel], globalBias for a row without a learned feature); mae, mse,
        rmse and bias are properties of the result, r2 takes SS_tot from the caller's labels."""
        fcol, lcol = self._params["featuresCol"], self._params["labelCol"]
        _check_schema(dataset, fcol, lcol)
        rp, col, val = _explode(dataset[fcol])
        csr = N.CSRHost(rp, col, val, np.asarray(dataset[lcol], dtype=np.float64))
        return self._ctx.evaluate(csr, self.getMinLabel(), self.getMaxLabel())

    def evaluateBinary(self, dataset: DataFrame) -> BinarySums:
        """The binary record of dataset's rows against labelCol, formed on the device in one call
        (fm_evaluate_binary): no score column is built or downloaded.  The score is transform's
        ``rawPrediction`` -- the unclamped score, globalBias for a row without a learned feature -- read as
        a logit whatever loss the model was fitted with; a label > 0.5 is a positive.  logLoss, auc (exact,
        ties counted as half), accuracy, precision, recall and f1 are properties of the result."""
        fcol, lcol = self._params["featuresCol"], self._params["labelCol"]
        _check_schema(dataset, fcol, lcol)
        rp, col, val = _explode(dataset[fcol])
        csr = N.CSRHost(rp, col, val, np.asarray(dataset[lcol], dtype=np.float64))
        return self._ctx.evaluate_binary(csr)

    def recommend(self, contexts: DataFrame, candidates: DataFrame, numItems: int, exclude=None, only=None) -> DataFrame:
        """The numItems best rows of `candidates` for every row of `contexts` (the shape of
        ALSModel.recommendForUserSubset): both frames carry featuresCol; the result is `contexts` plus
        a ``recommendations`` column, per row a list of (candidate_row, prediction) in rank order.  A
        pair's prediction is transform's for the row made of the two rows' entries, clamped to
        [minLabel, maxLabel]; the order is that of the unclamped score, ties by candidate row
        (fm_rank_candidates, include/fm_hip.h).  numItems outside [1, min(len(candidates), 1024)]
        raises ValueError; a model whose table is row-sharded refuses with FMError, as calcLossGrad.

        exclude / only (one of them; giving both raises ValueError): per row of `contexts` a list of
        row indices of `candidates` -- ``exclude``: rows never recommended to that context (what the
        user has already rated); ``only``: the rows ranked for it (a retrieval stage's candidates).
        The restriction is applied before the selection (fm_rank_candidates_select), so a context gets
        numItems recommendations whenever it has that many eligible rows; with fewer, its list is
        shorter.  Without the arguments the call and its result are the unrestricted ones."""
        fcol = self._params["featuresCol"]
        if exclude is not None and only is not None:
            raise ValueError("give exclude= or only=, not both")
        n_cand = candidates.count()
        if isinstance(numItems, bool) or not isinstance(numItems, (int, np.integer)):
            raise ValueError("numItems must be an integer")
        if not 1 <= int(numItems) <= min(n_cand, N.FM_RANK_MAX_TOP):
            raise ValueError(f"numItems must be in [1, min(len(candidates), {N.FM_RANK_MAX_TOP})], got {numItems}")
        _check_schema(contexts, fcol, None)
        _check_schema(candidates, fcol, None)
        rows = []
        for df in (contexts, candidates):
            rp, col, val = _explode(df[fcol])
            rows.append(N.CSRHost(rp, col, val, np.zeros(df.count())))
        if exclude is None and only is None:
            idx, score = self._ctx.rank(rows[0], rows[1], int(numItems), self.getMinLabel(), self.getMaxLabel())
        else:
            idx, score = self._ctx.rank(rows[0], rows[1], int(numItems), self.getMinLabel(), self.getMaxLabel(),
                                        exclude=exclude, only=only)
        recs = [[(int(i), float(s)) for i, s in zip(ri, rs) if i >= 0] for ri, rs in zip(idx, score)]
        return contexts.with_column("recommendations", recs)

    def rankPositions(self, contexts: DataFrame, candidates: DataFrame, targets, exclude=None) -> DataFrame:
        """Where each context's target rows (its held-out positives, say) rank among the rows of
        `candidates` it has not seen: one row per target with the columns ``context`` (row of
        `contexts`), ``candidate`` (row of `candidates`), ``position`` (0-based rank in recommend's order
        over all candidate rows except the context's ``exclude`` list; exact however many candidates
        there are) and ``score`` (recommend's prediction for the pair).  targets / exclude: per row of
        `contexts` a list of row indices of `candidates`, as recommend's lists.  A target that is also
        excluded has position -1 and score NaN.  One device call (fm_rank_positions); a row-sharded
        model refuses with FMError, as recommend."""
        ptr, rows, position, score, _ = self._rank_positions(contexts, candidates, targets, exclude)
        ctx_of = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
        return DataFrame({"context": ctx_of.tolist(), "candidate": rows.tolist(), "position": position.tolist(),
                          "score": score.tolist()})

    def _rank_positions(self, contexts, candidates, targets, exclude):
        """rankPositions' arrays (ptr, rows, position, score) and each context's number of eligible rows."""
        fcol = self._params["featuresCol"]
        _check_schema(contexts, fcol, None)
        _check_schema(candidates, fcol, None)
        rows = []
        for df in (contexts, candidates):
            rp, col, val = _explode(df[fcol])
            rows.append(N.CSRHost(rp, col, val, np.zeros(df.count())))
        n_ctx, n_cand = contexts.count(), candidates.count()
        out = self._ctx.rank_positions(rows[0], rows[1], targets, self.getMinLabel(), self.getMaxLabel(), exclude=exclude)
        n_eligible = np.full(n_ctx, n_cand, dtype=np.int64)
        if exclude is not None:
            n_eligible -= np.diff(normalize_row_lists(exclude, n_ctx)[0])
        return (*out, n_eligible)

    def calcLossGrad(self, dfSampleIndexed: DataFrame, initialSd: float, seed: int = 0) -> DataFrame:
        """Model.scala:135-234: one row per active entry with columns label, sampleId,
        featureId, prediction, loss, deltaWi, deltaVi (deltaVi before the (pred - label) factor).
        Ids the model lacks get per-entry N(0, initialSd^2) draws (:144-146, 170-171); the
        reference's draws are unseeded, here they are keyed by `seed` and the entry.  A model whose
        table is row-sharded over several GPUs (setParallel("sharded")) refuses it with FMError:
        the per-entry rows would need every owner's rows on one device (fm_loss_grad, include/fm_hip.h);
        a replicated or single-GPU model answers it."""
        if not initialSd > 0.0:
            raise ValueError("requirement failed: initSd (initial Standard Deviation) must be > 0.0")
        fcol, lcol = self._params["featuresCol"], self._params["labelCol"]
        _check_schema(dfSampleIndexed, fcol, lcol)
        rp, col, val = _explode(dfSampleIndexed[fcol])
        labels = np.asarray(dfSampleIndexed[lcol], dtype=np.float64)
        csr = N.CSRHost(rp, col, val, labels)
        pred, loss, dw, dv = self._ctx.loss_grad(csr, initial_sd=initialSd, seed=seed)
        rows = np.repeat(np.arange(len(labels)), np.diff(rp))
        sids = dfSampleIndexed["sampleId"] if "sampleId" in dfSampleIndexed.columns else list(range(len(labels)))
        return DataFrame({
            lcol: [float(labels[r]) for r in rows],
            "sampleId": [sids[r] for r in rows],
            "featureId": [int(c) for c in col],
            self._params["predictionCol"]: pred.tolist(),
            "loss": loss.tolist(),
            "deltaWi": dw.tolist(),
            "deltaVi": [DenseVector(v) for v in dv],
        })

    @staticmethod
    def addSampleId(dataset: DataFrame, columnName: str = "sampleId") -> DataFrame:
        """monotonically_increasing_id (Model.scala:268-272): (partition << 33) + row index."""
        ids = []
        for p, n in enumerate(dataset.partition_sizes):
            ids.extend((p << 33) + r for r in range(n))
        return dataset.with_column(columnName, ids)


# ------------------------------------------------------------------------- Estimator
class FactorizationMachinesSGD:
    """FactorizationMachinesSGD.scala:28-256 (Estimator[FactorizationMachinesModel])."""

    _DEFAULTS = {  # SGD.scala:61-74
        "dimFactorization": 10, "featuresCol": "features", "labelCol": "label", "predictionCol": "prediction",
        "sampleIdCol": "sampleId", "maxIter": 10, "miniBatchFraction": 0.1, "regParam": 0.1, "stepSize": 1.0,
        "minLabel": 0.0, "maxLabel": 1.0, "initialSd": 0.01,
        # HasFitIntercept, mixed into the estimator's params (FactorizationMachines.scala:18), Spark's
        # default true; the reference never reads it (w0 stays 0.0, SGD.scala:246), nor does fit here
        "fitIntercept": True,
        # not in the reference: the init draw is unseeded there; device / seed here
        "seed": 0, "device": 0, "numFeatures": None,
        # not in the reference: the table over several GPUs of this process (include/fm_hip.h
        # fm_config.parallel), in place of Spark's hash-partitioned model Datasets
        "parallel": None, "nGpus": 1, "devices": None, "transport": "auto", "wire": "fp32",
        # not in the reference: a held-out frame evaluated on the device during fit, (frame, every)
        "validationData": None,
        # not in the reference: a held-out frame whose log loss and AUC the device forms during fit, (frame, every)
        "binaryValidationData": None,
        # not in the reference: negatives drawn per positive by fitInteractions
        "negativesPerPositive": 4,
        # not in the reference (its loss is the squared error, SGD.scala:134-146): the step's objective
        "loss": "squared",
    }

    def __init__(self, uid: str | None = None):
        self.uid = uid or "fm_" + uuid.uuid4().hex[:12]  # Identifiable.randomUID("fm")
        self._params = dict(self._DEFAULTS)

    # setters / getters (SGD.scala:35-59) ------------------------------------------------
    def _set(self, name, value):
        self._params[name] = value
        return self

    def setDimFactorization(self, v: int):
        if int(v) < 1:  # IntParam, ParamValidators.gtEq(1) (FactorizationMachines.scala:26)
            raise ValueError("dimFactorization must be >= 1")
        return self._set("dimFactorization", int(v))

    def setFeaturesCol(self, v): return self._set("featuresCol", v)
    def setLabelCol(self, v): return self._set("labelCol", v)
    def setPredictionCol(self, v): return self._set("predictionCol", v)
    def setMaxIter(self, v): return self._set("maxIter", int(v))
    def setMiniBatchFraction(self, v): return self._set("miniBatchFraction", float(v))
    def setRegParam(self, v): return self._set("regParam", float(v))
    def setStepSize(self, v): return self._set("stepSize", float(v))
    def setMinLabel(self, v): return self._set("minLabel", float(v))
    def setMaxLabel(self, v): return self._set("maxLabel", float(v))
    def setInitialSd(self, v): return self._set("initialSd", float(v))
    def setSeed(self, v): return self._set("seed", int(v))
    def setNumFeatures(self, v): return self._set("numFeatures", int(v))

    def setParallel(self, mode, n_gpus: int = 1, devices=None, transport: str = "auto", wire: str = "fp32"):
        """Train (and transform) on n_gpus GPUs of this process: mode "sharded" splits the table's
        rows by id % R (owner-computes), "replicated" keeps a copy per GPU (gradient all-reduce);
        the mini-batches split by rows across the GPUs.  transport "copy" shares one device.
        wire "fp64" (sharded only): the owners' partial sums cross unrounded, so every sample is
        summed in fp64 as on one GPU (fm_config.wire); the fitted model transforms with the same wire."""
        if wire not in ("fp32", "fp64"):
            raise ValueError('wire must be "fp32" or "fp64"')
        if mode not in (None, "none") and self._params["loss"] != "squared":
            raise ValueError(f'loss "{self._params["loss"]}" trains on one GPU: multi-GPU objectives are not built yet')
        if mode not in (None, "none") and self._params["binaryValidationData"] is not None:
            raise ValueError("binaryValidationData needs a single-GPU estimator: the binary evaluation is not multi-GPU")
        self._set("parallel", mode)
        self._set("wire", wire)
        self._set("nGpus", int(n_gpus))
        self._set("devices", None if devices is None else [int(d) for d in devices])
        return self._set("transport", transport)

    def setValidationData(self, dataset: DataFrame | None, every: int = 1):
        """A held-out frame (featuresCol, labelCol) evaluated during fit, on the device: after every
        `every`-th executed iteration and after the last, its error sums against the model as it
        stands (FactorizationMachinesModel.evaluate's, clamped to this estimator's [minLabel,
        maxLabel]) are appended to the fitted model's ``validationHistory`` as (iteration, EvalSums),
        and one log line per entry follows the loss lines.  The frame is uploaded once; ids the
        training data lacks drop out, as in transform.  The pipelined fit only enqueues the
        evaluations (fm_evaluate_batch without out) and reads them when the loop has run; the
        synchronous fit and multi-GPU estimators evaluate synchronously.  None (default): off."""
        if dataset is None:
            return self._set("validationData", None)
        if self._params["loss"] != "squared":
            raise ValueError(f'validationData needs loss "squared", not "{self._params["loss"]}": the device evaluation\'s '
                             "sums are regression sums (device log-loss and AUC are not built yet); log loss and AUC "
                             "during fit: setBinaryValidationData")
        if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or int(every) < 1:
            raise ValueError("every must be an integer >= 1")
        return self._set("validationData", (dataset, int(every)))

    def setBinaryValidationData(self, dataset: DataFrame | None, every: int = 1):
        """A held-out frame (featuresCol, labelCol) whose binary record -- log loss, exact AUC and the
        confusion counts at score > 0 (FactorizationMachinesModel.evaluateBinary's) -- is formed on the device
        during fit, after every `every`-th executed iteration and after the last, and appended to the fitted
        model's ``binaryValidationHistory`` as (iteration, BinarySums), with one log line per entry.  Upload,
        schedule and read-back are validationData's: the pipelined fit only enqueues
        (fm_evaluate_binary_batch without out).  Accepted with loss "squared" and "logistic" (the score is
        read as a logit); "bpr", a multi-GPU estimator and fitInteractions refuse it.  Independent of
        validationData: either, both or neither may be set.  None (default): off."""
        if dataset is None:
            return self._set("binaryValidationData", None)
        if self._params["loss"] == "bpr":
            raise ValueError('binaryValidationData needs loss "squared" or "logistic": "bpr" scores order candidates, '
                             "they are no logit of a label")
        if self._params["parallel"] not in (None, "none"):
            raise ValueError("binaryValidationData needs a single-GPU estimator: the binary evaluation is not multi-GPU")
        if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or int(every) < 1:
            raise ValueError("every must be an integer >= 1")
        return self._set("binaryValidationData", (dataset, int(every)))

    def setNegativesPerPositive(self, n: int):
        """fitInteractions draws n negatives for every positive of a mini-batch (0 .. 1024; default 4)."""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= int(n) <= 1024:
            raise ValueError("negativesPerPositive must be an integer in [0, 1024]")
        return self._set("negativesPerPositive", int(n))

    def setLoss(self, loss: str):
        """The objective each step descends (fm_config.loss): "squared" (default, the reference's),
        "logistic" -- log loss of sigma(score) against labels in [0, 1], for click / binary labels and for
        fitInteractions' 1.0 / 0.0 rows -- or "bpr" -- the pairwise ranking loss of every positive against
        the negatives drawn for it, fitInteractions only (a frame has no groups).  Both run on one GPU
        and without validationData (ValueError with either set); "logistic" takes binaryValidationData
        (log loss and AUC during fit), "bpr" does not."""
        if loss not in ("squared", "logistic", "bpr"):
            raise ValueError('loss must be "squared", "logistic" or "bpr"')
        if loss != "squared":
            if self._params["parallel"] not in (None, "none"):
                raise ValueError(f'loss "{loss}" trains on one GPU: multi-GPU objectives are not built yet')
            if self._params["validationData"] is not None:
                raise ValueError(f'loss "{loss}" cannot evaluate validationData: the device evaluation\'s sums are '
                                 "regression sums (device log-loss and AUC are not built yet); log loss and AUC "
                                 "during fit: setBinaryValidationData")
        if loss == "bpr" and self._params["binaryValidationData"] is not None:
            raise ValueError('loss "bpr" cannot evaluate binaryValidationData: its scores are no logit of a label')
        return self._set("loss", loss)

    def getLoss(self): return self._params["loss"]
    def getNegativesPerPositive(self): return self._params["negativesPerPositive"]
    def getDimFactorization(self): return self._params["dimFactorization"]
    def getMaxIter(self): return self._params["maxIter"]
    def getMiniBatchFraction(self): return self._params["miniBatchFraction"]
    def getRegParam(self): return self._params["regParam"]
    def getStepSize(self): return self._params["stepSize"]
    def getMinLabel(self): return self._params["minLabel"]
    def getMaxLabel(self): return self._params["maxLabel"]
    def getInitialSd(self): return self._params["initialSd"]
    def getFitIntercept(self): return self._params["fitIntercept"]

    def copy(self, extra: dict | None = None) -> "FactorizationMachinesSGD":
        """defaultCopy (SGD.scala:254): same uid, params overridden by extra (keyed by name or Param)."""
        c = FactorizationMachinesSGD(self.uid)
        c._params = dict(self._params)
        for key, value in (extra or {}).items():
            name = key.name if isinstance(key, Param) else key
            if name == "fitIntercept" and not isinstance(value, (bool, np.bool_)):
                raise TypeError("fitIntercept is a BooleanParam")  # Spark's BooleanParam rejects non-booleans
            c._params[name] = value
        return c

    def transformSchema(self, schema):
        return schema

    def _check_loss(self):
        """setLoss's rules again, for params that arrived through copy(extra)."""
        p = self._params
        if p["loss"] not in ("squared", "logistic", "bpr"):
            raise ValueError('loss must be "squared", "logistic" or "bpr"')
        if p["loss"] != "squared" and p["parallel"] not in (None, "none"):
            raise ValueError(f'loss "{p["loss"]}" trains on one GPU: multi-GPU objectives are not built yet')
        if p["loss"] != "squared" and p["validationData"] is not None:
            raise ValueError(f'loss "{p["loss"]}" cannot evaluate validationData: the device evaluation\'s sums are '
                             "regression sums")
        if p["binaryValidationData"] is not None:
            if p["loss"] == "bpr":
                raise ValueError('loss "bpr" cannot evaluate binaryValidationData: its scores are no logit of a label')
            if p["parallel"] not in (None, "none"):
                raise ValueError("binaryValidationData needs a single-GPU estimator: the binary evaluation is not multi-GPU")

    # fit (SGD.scala:76-216) --------------------------------------------------------------
    def fit(self, dataset: DataFrame, initial_tables=None, pipelined: bool | None = None) -> FactorizationMachinesModel:
        """createInitialModel (:218-252) + addSampleId + runMiniBatchSGD (:88-216).
        ``initial_tables`` = (ids, w, V) injects M0 (the reference's draw is unseeded, P9).
        ``pipelined`` (default: on): the dataset is kept on the device (every GPU of a multi-GPU estimator
        gathers its share of a split from its own copy)
        -- dfData.cache(), :93 --, each randomSplit split is gathered there from its row list
        (fm_batch_from_rows) and sorted on the side stream while the previous iteration steps, and
        the steps only enqueue; the loss log lines (:139) are written, in iteration order, when the
        loop has run.  False: every split crosses PCIe as a host CSR and its step returns its loss
        (the same model: the splits hold the same rows in the same order)."""
        p = self._params
        self._check_loss()
        if p["loss"] == "bpr":
            raise ValueError('loss "bpr" needs groups of a positive and its negatives: a frame has none (fitInteractions)')
        _check_schema(dataset, p["featuresCol"], p["labelCol"])
        k = p["dimFactorization"]
        vectors = dataset[p["featuresCol"]]
        labels = np.asarray(dataset[p["labelCol"]], dtype=np.float64)
        if p["loss"] == "logistic" and len(labels) and not (np.all(labels >= 0.0) and np.all(labels <= 1.0)):
            raise ValueError('loss "logistic" needs labels in [0, 1]')
        rp, col, val = _explode(vectors)
        F = p["numFeatures"] or (int(col.max()) + 1 if len(col) else 1)
        ctx = FMContext(F, k, device=p["device"], seed=p["seed"], init_sd=p["initialSd"], w0=0.0,
                        parallel=p["parallel"], n_gpus=p["nGpus"], devices=p["devices"], transport=p["transport"],
                        wire=p["wire"], loss=p["loss"])
        if pipelined is None:
            pipelined = True
        # randomSplit(Array.fill(maxIter)(miniBatchFraction), 1234L) (:111-112)
        order_cols = []
        extra = None
        for name in dataset.schema:
            if name == p["labelCol"]:
                order_cols.append("L")
            elif name == p["featuresCol"]:
                order_cols.append("F")
            else:
                vals = dataset[name]
                if extra is not None or not all(isinstance(v, (int, np.integer)) for v in vals):
                    raise ValueError(f"randomSplit replay supports one extra integer column, not {name!r}")
                extra = np.asarray(vals, dtype=np.int64)
                order_cols.append("I")
        from .sampler import random_split

        split_of, _, order = random_split(dataset.partition_sizes, labels, vectors,
                                          [p["miniBatchFraction"]] * p["maxIter"], 1234, "".join(order_cols),
                                          extra=extra)
        # split i's rows in per-partition sorted order (the order Spark's sampled partitions keep)
        splits = [order[split_of[order] == i] for i in range(p["maxIter"])]
        data = None
        if pipelined and len(labels):
            # dfData.cache() (:93): the exploded dataset uploaded once, laid out split after split (the
            # rows no split samples last, for createInitialModel), so every iteration's mini-batch is a
            # contiguous range of it, stepped in place (fm_batch_split_view); it crosses PCIe in its own
            # row order and the device lays it out (fm_batch_layout_splits): no permuted host copy
            rest = order[split_of[order] < 0]
            lay = np.concatenate(splits + [rest]).astype(np.int64)
            split_rows = np.concatenate([[0], np.cumsum([len(r) for r in splits] + [len(rest)])])
            data = ctx.batch_layout_splits(N.CSRHost(rp, col, val, labels), split_rows, lay)
        elif initial_tables is None and len(labels):
            data = ctx.batch(N.CSRHost(rp, col, val, labels))
        if initial_tables is not None:
            ctx.load_tables(*initial_tables)
        elif len(col):
            # createInitialModel (:224-241): the draw for every distinct active feature id, on the
            # device over the whole dataset's entries
            ctx.init_from_batch(data)
        val_run = bin_run = None
        if p["validationData"] is not None:
            val_run = _Validation.upload(ctx, p["validationData"], p["featuresCol"], p["labelCol"], F, p["minLabel"],
                                         p["maxLabel"])
        if p["binaryValidationData"] is not None:
            bin_run = _Validation.upload(ctx, p["binaryValidationData"], p["featuresCol"], p["labelCol"], F, p["minLabel"],
                                         p["maxLabel"], binary=True)
        val_runs = [v for v in (val_run, bin_run) if v is not None]
        if pipelined:
            if data is not None:
                run_minibatch_sgd_splits(ctx, data, p["stepSize"], p["regParam"], n_iter=p["maxIter"],
                                         validation=val_runs)
            else:
                for i in range(p["maxIter"]):
                    log.warning("Iteration (%d/%d). The size of sampled batch is zero", i + 1, p["maxIter"])
        else:
            n_exec = sum(1 for rows in splits if len(rows))
            j = 0
            for i, rows in enumerate(splits):
                it = i + 1  # iter = index + 1 (:119)
                if len(rows) == 0:
                    log.warning("Iteration (%d/%d). The size of sampled batch is zero", it, p["maxIter"])
                    continue
                csr = _select_csr(rp, col, val, labels, rows)
                out = ctx.step(csr, it, p["stepSize"], p["regParam"])
                log.info("Loss of Iteration (%d/%d): %s", it, p["maxIter"], out.loss_sum)
                j += 1
                for v in val_runs:
                    if v.due(j, n_exec):
                        v.evaluate(ctx, it, sync=True)
            for v in val_runs:
                v.finish(ctx, p["maxIter"])
        model = FactorizationMachinesModel(self.uid, k, 0.0, ctx=ctx)
        model.setMinLabel(p["minLabel"]).setMaxLabel(p["maxLabel"])
        model._params["loss"] = p["loss"]
        model.parent = self
        if val_run is not None:
            model.validationHistory = val_run.history
            val_run.close()
        if bin_run is not None:
            model.binaryValidationHistory = bin_run.history
            bin_run.close()
        return model


    def fitInteractions(self, contexts: DataFrame, candidates: DataFrame, interactions: DataFrame, exclude=None,
                        initial_tables=None) -> FactorizationMachinesModel:
        """Fit on implicit feedback: `interactions` holds the integer columns ``context`` (row of
        `contexts`) and ``candidate`` (row of `candidates`) -- rankPositions' names -- one row per
        positive; both frames carry featuresCol, as recommend's.  A training row is a context row's
        entries followed by a candidate row's, the row recommend and rankPositions score; positives are
        labelled 1.0 (what loss "logistic" reads; "bpr" reads the groups -- each positive and the negatives
        behind it -- and needs negativesPerPositive >= 1) and each gets negativesPerPositive negatives labelled 0.0, drawn on the device
        uniformly over the candidate rows not on its context's ``exclude`` list (default: the context's
        interacted rows, built on the device from the interactions: fm_lists_from_pairs).  Both frames and
        the lists go to the device once and every mini-batch is assembled there
        (fm_batch_sample_pairs_lists): with n interactions, m = max(1, round(miniBatchFraction * n)) and perm =
        default_rng(seed).permutation(n), iteration t = 1 .. maxIter takes the positives
        perm[((t - 1) * m + arange(m)) % n] in that order with the draw seed splitmix64(seed) ^ t, into
        one of two batches in turn, sorted on the side stream while the previous iteration steps; the
        steps only enqueue and the loss lines are written after the loop, as the pipelined fit's.
        ``initial_tables`` = (ids, w, V) replaces the seeded draw over every id of either frame.  A
        multi-GPU estimator (setParallel) and a set validationData raise ValueError: not built yet."""
        p = self._params
        self._check_loss()
        if p["loss"] == "bpr" and p["negativesPerPositive"] < 1:
            raise ValueError('loss "bpr" needs negativesPerPositive >= 1: a positive is ranked against its negatives')
        if p["parallel"] is not None:
            raise ValueError("fitInteractions runs on one GPU: a multi-GPU estimator (setParallel) is not supported yet")
        if p["validationData"] is not None:
            raise ValueError("fitInteractions does not evaluate validationData yet")
        if p["binaryValidationData"] is not None:
            raise ValueError("fitInteractions does not evaluate binaryValidationData: its metric is a ranking metric over "
                             "held-out positives (RankingEvaluator)")
        fcol = p["featuresCol"]
        _check_schema(contexts, fcol, None)
        _check_schema(candidates, fcol, None)
        pairs = []
        for name in ("context", "candidate"):
            if name not in interactions.columns:
                raise ValueError(f"Column {name} does not exist.")
            vals = interactions[name]
            if not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in vals):
                raise ValueError(f"Column {name} must hold integers")
            pairs.append(np.asarray(vals, dtype=np.int64))
        pos_ctx, pos_cand = pairs
        n_ctx, n_cand, n = contexts.count(), candidates.count(), len(pos_ctx)
        if n and not (0 <= pos_ctx.min() and pos_ctx.max() < n_ctx and 0 <= pos_cand.min() and pos_cand.max() < n_cand):
            raise ValueError("interactions name a row outside contexts / candidates")
        if exclude is not None:
            exclude = normalize_row_lists(exclude, n_ctx)
        rows = [_explode(df[fcol]) for df in (contexts, candidates)]
        k = p["dimFactorization"]
        top = max([int(col.max()) + 1 for _, col, _ in rows if len(col)], default=1)
        ctx = FMContext(p["numFeatures"] or top, k, device=p["device"], seed=p["seed"], init_sd=p["initialSd"], w0=0.0,
                        loss=p["loss"])
        bu, bc = (ctx.batch(N.CSRHost(rp, col, val, np.zeros(len(rp) - 1))) for rp, col, val in rows)
        # the exclude lists, resident for the whole loop: the given ones (normalised above, once), else what
        # the interactions say each context has seen, built on the device from the pairs themselves
        if exclude is not None:
            ex = ctx._row_lists(exclude, n_cand)
        else:
            ex = ctx.row_lists_from_pairs(pos_ctx, pos_cand, n_ctx, n_cand)
        if initial_tables is not None:
            ctx.load_tables(*initial_tables)
        else:
            ctx.init_from_batch(bu)  # createInitialModel's draw (:224-241) for every id of either frame
            ctx.init_from_batch(bc)
        from .data import splitmix64

        n_iter, n_neg = p["maxIter"], p["negativesPerPositive"]
        m = max(1, int(round(p["miniBatchFraction"] * n)))
        perm = np.random.default_rng(p["seed"]).permutation(n)
        seed0 = int(splitmix64(np.uint64(p["seed"] & (2**64 - 1))))
        bufs = [None, None]

        def sample(t):
            take = perm[((t - 1) * m + np.arange(m)) % n]
            bufs[t % 2] = ctx._sample_pairs(bu, bc, pos_ctx[take], pos_cand[take], n_neg, ex, 1.0, 0.0, seed0 ^ t,
                                            bufs[t % 2], False)
            bufs[t % 2].prepare()

        e0 = ctx.epoch
        work = list(range(n_iter)) if n else []
        if work:
            sample(1)
        for t in range(1, len(work) + 1):
            ctx.step_batch(bufs[t % 2], t, p["stepSize"], p["regParam"], sync=False)
            if t < len(work):
                sample(t + 1)  # drawn, gathered and sorted while step t runs (the batch step t - 1 read)
        ctx.sync()
        _log_losses(ctx, e0, work, n_iter, n_iter)
        for b in (*bufs, bu, bc, ex):
            if b is not None:
                b.close()
        model = FactorizationMachinesModel(self.uid, k, 0.0, ctx=ctx)
        model.setMinLabel(p["minLabel"]).setMaxLabel(p["maxLabel"])
        model._params["loss"] = p["loss"]
        model.parent = self
        return model


class _Validation:
    """fit's held-out frame (setValidationData; binary: setBinaryValidationData): one device batch of the
    fit's context, the iterations at which it was evaluated and, once the loop has run, their records."""

    def __init__(self, batch, lo: float, hi: float, every: int, binary: bool = False):
        self.batch, self.lo, self.hi, self.every, self.binary = batch, lo, hi, every, binary
        self.history = []   # [(iteration, EvalSums)]; binary: [(iteration, BinarySums)]
        self._queued = []   # iterations whose evaluation was only enqueued
        self._h0 = 0        # the context's evaluation records before this fit's first

    @staticmethod
    def upload(ctx: FMContext, spec, features_col: str, label_col: str, num_features: int, lo: float, hi: float,
               binary: bool = False):
        df, every = spec
        _check_schema(df, features_col, label_col)
        rp, col, val = _explode(df[features_col])
        # ids the table cannot hold are dropped by the evaluation as by transform; the upload of a
        # resident batch refuses them, so they drop out here
        keep = col < num_features
        if not keep.all():
            rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))[keep]
            rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=len(rp) - 1))]).astype(np.int64)
            col, val = col[keep], val[keep]
        y = np.asarray(df[label_col], dtype=np.float64)
        batch = ctx.batch(N.CSRHost(rp, col, val, y)) if len(y) else None
        v = _Validation(batch, float(lo), float(hi), every, binary)
        v._h0 = len(v._records(ctx))
        return v

    def _records(self, ctx: FMContext) -> list:
        return ctx.eval_binary_history() if self.binary else ctx.eval_history()

    def _evaluate(self, ctx: FMContext, sync: bool):
        if self.binary:
            return ctx.evaluate_binary_batch(self.batch, sync=sync)
        return ctx.evaluate_batch(self.batch, self.lo, self.hi, sync=sync)

    def due(self, n_done: int, n_total: int) -> bool:
        """after the n_done-th executed iteration of n_total"""
        return self.batch is not None and (n_done % self.every == 0 or n_done == n_total)

    def evaluate(self, ctx: FMContext, iteration: int, sync: bool):
        if sync:
            self.history.append((iteration, self._evaluate(ctx, True)))
        else:
            self._evaluate(ctx, False)
            self._queued.append(iteration)

    def finish(self, ctx: FMContext, n_iter: int):
        """The enqueued evaluations' records read (one host synchronisation), and the log lines."""
        if self._queued:
            recs = self._records(ctx)[self._h0:]
            self.history.extend(zip(self._queued, recs))
            self._queued = []
        for it, s in self.history:
            if self.binary:
                log.info("Binary validation of Iteration (%d/%d): logLoss %s auc %s accuracy %s (%d rows, %d positive)",
                         it, n_iter, s.logLoss, s.auc, s.accuracy, s.n_rows, s.n_pos)
                continue
            log.info("Validation of Iteration (%d/%d): mae %s rmse %s bias %s (%d rows, %d without a learned feature)",
                     it, n_iter, s.mae, s.rmse, s.bias, s.n_rows, s.n_unlearned)

    def close(self):
        if self.batch is not None:
            self.batch.close()
            self.batch = None


def _select_csr(rp, col, val, labels, rows) -> N.CSRHost:
    """The host CSR of the given rows (the synchronous fit's per-split batch)."""
    rows = np.asarray(rows, dtype=np.int64)
    lens = rp[rows + 1] - rp[rows]
    sub_rp = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=sub_rp[1:])
    idx = np.repeat(rp[rows] - sub_rp[:-1], lens) + np.arange(sub_rp[-1], dtype=np.int64)
    return N.CSRHost(sub_rp, col[idx], val[idx], labels[rows])


def run_minibatch_sgd_resident(ctx: FMContext, data, splits, step_size: float, reg_param: float,
                               max_iter: int | None = None, bufs: list | None = None):
    """The foldLeft of runMiniBatchSGD (FactorizationMachinesSGD.scala:114-211) over a dataset kept
    on the device (`data`, dfData.cache() at :93): split i's rows (`splits[i]`, the randomSplit row
    lists) are gathered there (fm_batch_from_rows, on the copy stream) two iterations ahead into one
    of three batches used in turn, and sorted on the side stream (fm_batch_prepare) while iteration
    i - 1 steps, so a sort never waits for its split's copy and gather; every step only enqueues
    (fm_step_batch with out = NULL).  An empty split is skipped with the reference's warning
    (:126-128).  The loss log lines (:134-139) are written in iteration order after the loop, from
    the device's loss history.  Returns the loss sums of the executed iterations.  `bufs`: a list of
    three batches (or Nones) to refill and leave open for the caller (another loop reuses their
    device buffers); by default they are made here and closed at the end."""
    n_iter = len(splits) if max_iter is None else max_iter
    work = [(i, rows) for i, rows in enumerate(splits) if len(rows)]
    own = bufs is None
    if own:
        bufs = [None, None, None]
    nb = len(bufs)

    def gather(j):
        bufs[j % nb] = ctx.batch_from_rows(data, work[j][1], into=bufs[j % nb])

    e0 = ctx.epoch
    if work:
        gather(0)
        bufs[0].prepare()
    if len(work) > 1:
        gather(1)
    for j, (i, _) in enumerate(work):
        ctx.step_batch(bufs[j % nb], i + 1, step_size, reg_param, sync=False)  # iter = index + 1 (:119)
        if j + 1 < len(work):
            bufs[(j + 1) % nb].prepare()  # sorted on the side stream while this step runs
        if j + 2 < len(work):
            gather(j + 2)  # copied and gathered on the copy stream behind step j - 1
    ctx.sync()
    out = _log_losses(ctx, e0, [i for i, _ in work], len(splits), n_iter)
    if own:
        for b in bufs:
            if b is not None:
                b.close()
    return out


def _log_losses(ctx, e0, iters, n_splits, n_iter):
    """The loss log lines of SGD.scala:134-139 (and the zero-size warning of :126-128) for splits
    0 .. n_splits - 1, in iteration order, from the device's loss history of the executed iterations
    `iters` (their steps start at epoch e0); returns their losses."""
    hist = ctx.loss_history()[e0:]
    done = {i: float(hist[j]) for j, i in enumerate(iters)}
    for i in range(n_splits):
        if i in done:
            log.info("Loss of Iteration (%d/%d): %s", i + 1, n_iter, done[i])
        else:
            log.warning("Iteration (%d/%d). The size of sampled batch is zero", i + 1, n_iter)
    return [done[i] for i in iters]


def run_minibatch_sgd_splits(ctx: FMContext, data, step_size: float, reg_param: float, n_iter: int | None = None,
                             bufs: list | None = None, validation=None):
    """The foldLeft of runMiniBatchSGD (FactorizationMachinesSGD.scala:114-211) over a dataset kept on
    the device laid out split after split (`data`, FMContext.batch_splits: dfData.cache() at :93 with
    the randomSplit splits of :111-112 in iteration order): iteration i steps split i in place
    (fm_batch_split_view re-points one of two batches used in turn -- no copy, no gather), sorted on
    the side stream (fm_batch_prepare) while iteration i - 1 steps; every step only enqueues.  An
    empty split is skipped with the reference's warning (:126-128); the loss log lines (:134-139) are
    written in iteration order after the loop.  n_iter: the iterations are splits 0 .. n_iter - 1
    (default: every split; fit's dataset ends with a split of the rows no iteration samples and
    passes maxIter).  `bufs`: a list of two views (or Nones) to re-point and leave open for the
    caller.  `validation` (fit's setValidationData / setBinaryValidationData: a _Validation or a list of them):
    each one's frame is evaluated between the steps it names,
    on the main stream behind the step -- enqueued only on a single-table context (the records are
    read once, after the loop), synchronously on a multi-GPU one; its log lines follow the loss
    lines.  Returns the loss sums of the executed iterations."""
    sizes = np.diff(np.asarray(data.split_rows))
    n_iter = len(sizes) if n_iter is None else int(n_iter)
    if n_iter > len(sizes):
        raise ValueError("n_iter exceeds the dataset's splits")
    work = [i for i in range(n_iter) if sizes[i] > 0]
    validations = [] if validation is None else [validation] if isinstance(validation, _Validation) else list(validation)
    own = bufs is None
    if own:
        bufs = [None, None]
    nb = len(bufs)

    def view(j):
        bufs[j % nb] = ctx.split_view(data, work[j], into=bufs[j % nb])

    e0 = ctx.epoch
    if work:
        view(0)
        bufs[0].prepare()
    for j, i in enumerate(work):
        ctx.step_batch(bufs[j % nb], i + 1, step_size, reg_param, sync=False)  # iter = index + 1 (:119)
        if j + 1 < len(work):
            view(j + 1)  # re-points the batch step j - 1 read (its sort waits for that step)
            bufs[(j + 1) % nb].prepare()  # sorted on the side stream while this step runs
        for v in validations:
            if v.due(j + 1, len(work)):
                v.evaluate(ctx, i + 1, sync=ctx.parallel is not None)
    ctx.sync()
    out = _log_losses(ctx, e0, work, n_iter, n_iter)
    for v in validations:
        v.finish(ctx, n_iter)
    if own:
        for b in bufs:
            if b is not None:
                b.close()
    return out


# fm.regParam, fm.dimFactorization, ...: the Param handles spark.ml tuning keys grids by
for _name in ("dimFactorization", "featuresCol", "labelCol", "predictionCol", "maxIter", "miniBatchFraction",
              "regParam", "stepSize", "minLabel", "maxLabel", "initialSd", "seed", "fitIntercept"):
    setattr(FactorizationMachinesSGD, _name, property(lambda self, _n=_name: Param(self.uid, _n)))
del _name
