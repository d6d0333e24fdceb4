"""GPU: the training objectives through the estimator -- FactorizationMachinesSGD.setLoss with
fitInteractions ("bpr", "logistic") and fit ("logistic"), and the logistic model's transform -- against a
host replay on tests/objective_ref.py: the same permutation and mini-batches, the negatives the device
call reports (`sampled`), and the reference's steps with the device's contract (round_scores=True).

Parity tolerance of the multi-step replays: tests/test_gpu_pairs_ml.py's,
    |dev - ref| <= RTOL |ref| + ATOL + n_upd 2^-22 peak
(n_upd: the steps whose batch held the row's id; peak: the largest |w| or |V| the reference's row has held)."""

import math

import numpy as np
import pytest

import objective_ref as O
import pair_ref as P
from oracle import fm_ref as R
from test_gpu_parity import ATOL, RTOL
from test_gpu_pairs_ml import estimator, frames

pytestmark = pytest.mark.gpu


def device_negatives(p, n_iter):
    """The negatives fitInteractions' iterations draw, as the device call itself reports them (`sampled`):
    [n_iter] arrays [m, NEG], from the estimator's permutation rule and draw seeds."""
    from fm_spark_amd._native import CSRHost
    from fm_spark_amd.data import splitmix64
    from fm_spark_amd.engine import FMContext

    ctx = FMContext(p.F, P.K)
    zero = lambda rows: CSRHost(rows[0], rows[1], rows[2], np.zeros(len(rows[0]) - 1))  # noqa: E731
    bu, bc = ctx.batch(zero(p.contexts)), ctx.batch(zero(p.candidates))
    ex = ctx.row_lists_from_pairs(p.pos_ctx, p.pos_cand, p.U, p.C)
    seed0 = int(splitmix64(np.uint64(P.SEED)))
    out = []
    for t in range(1, n_iter + 1):
        take = P.batch_positives(len(p.pos_ctx), P.SEED, P.FRAC, t)
        b, sampled = ctx._sample_pairs(bu, bc, p.pos_ctx[take], p.pos_cand[take], P.NEG, ex, 1.0, 0.0, seed0 ^ t, None, True)
        assert b.group == 1 + P.NEG
        out.append((take, sampled.copy()))
        b.close()
    for x in (bu, bc, ex):
        x.close()
    ctx.close()
    return out


def assert_replay(model, ref, n_upd, peak, what):
    ids, w, V = model._ctx.export_tables()
    np.testing.assert_array_equal(ids, np.nonzero(ref.present)[0])
    slack = (n_upd * 2.0 ** -22 * peak)[ids]
    rw = np.abs(w - ref.w[ids]) / (RTOL * np.abs(ref.w[ids]) + ATOL + slack)
    rV = np.abs(V - ref.V[ids]) / (RTOL * np.abs(ref.V[ids]) + ATOL + slack[:, None])
    print(f"{what}: deviation / budget w {rw.max():.3f} V {rV.max():.3f}")
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(V))
    assert rw.max() <= 1.0 and rV.max() <= 1.0


def replay(ref, batches, loss, group, step, reg):
    """objective_ref steps over (t, csr) with the bookkeeping of the tolerance; returns (n_upd, peak, losses)."""
    F = len(ref.w)
    n_upd, losses = np.zeros(F), []
    track = lambda pk: np.maximum(pk, np.maximum(np.abs(ref.w), np.max(np.abs(ref.V), axis=1)))  # noqa: E731
    peak = track(np.zeros(F))
    for t, csr in batches:
        losses.append(O.step(ref, csr, t, step, reg, loss, group, round_scores=True, fast=True).loss_sum)
        n_upd[np.unique(csr.col)] += 1
        peak = track(peak)
    return n_upd, peak, losses


@pytest.mark.parametrize("loss", ["bpr", "logistic"])
def test_fit_interactions_six_iterations_match_the_replay(gpu, loss):
    p, contexts, candidates, interactions = frames()
    est = estimator(6).setLoss(loss)
    assert est.getLoss() == loss
    model = est.fitInteractions(contexts, candidates, interactions)
    assert model._ctx.epoch == 6 and model._ctx.loss == loss and model._params["loss"] == loss
    batches = []
    for t, (take, sampled) in enumerate(device_negatives(p, 6), start=1):
        assert np.array_equal(sampled, P.sample_negatives(int(P.splitmix64(P.U64(P.SEED))) ^ t, p.pos_ctx[take], P.NEG,
                                                          p.excl_ptr, p.excl_rows, p.C))
        batches.append((t, P.concat_pairs(p.contexts, p.candidates, *P.sampled_pairs(p.pos_ctx[take], p.pos_cand[take], sampled))))
    ref = P.initial_model(p)
    n_upd, peak, losses = replay(ref, batches, loss, 1 + P.NEG, P.STEP, P.REG)
    got = model._ctx.loss_history()
    print(f"fitInteractions {loss}: losses device {got.tolist()} replay {losses}")
    assert len(got) == 6 and np.all(np.isfinite(got))
    assert got[0] == pytest.approx(losses[0], rel=RTOL)  # the first step starts from equal tables
    assert_replay(model, ref, n_upd, peak, f"fitInteractions {loss}, 6 iterations")
    # the scores order candidates whatever the loss: recommend and rankPositions are the raw score's
    recs = model.recommend(contexts, candidates, 4, exclude=p.train)["recommendations"][0]
    assert len(recs) == 4


def binary_frame(seed=3, n=400, nf=40, parts=3):
    from fm_spark_amd.linalg import Vectors
    from fm_spark_amd.ml import DataFrame

    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        idx = np.sort(rng.choice(nf, int(rng.integers(0, 6)), replace=False))
        x = np.float32(rng.normal(size=len(idx))).astype(np.float64)
        score = x[idx < 8].sum()
        rows.append((float(rng.random() < 1.0 / (1.0 + math.exp(-2.0 * score))),
                     Vectors.sparse(nf, [(int(i), float(v)) for i, v in zip(idx, x)])))
    return DataFrame.from_rows(rows, ["label", "features"], num_partitions=parts), nf


@pytest.mark.parametrize("pipelined", [True, False])
def test_fit_logistic_matches_the_reference_fit(gpu, pipelined):
    from fm_spark_amd.ml import FactorizationMachinesSGD, _explode
    from fm_spark_amd.sampler import random_split

    df, nf = binary_frame()
    k, n_iter, frac, step, reg = 6, 5, 0.3, 0.8, 1e-3
    rng = np.random.default_rng(4)
    ids = np.arange(nf, dtype=np.int32)
    w0 = np.float32(rng.normal(0, 0.1, nf)).astype(np.float64)
    V0 = np.float32(rng.normal(0, 0.1, (nf, k))).astype(np.float64)
    est = (FactorizationMachinesSGD().setDimFactorization(k).setMaxIter(n_iter).setMiniBatchFraction(frac).setStepSize(step)
           .setRegParam(reg).setNumFeatures(nf).setLoss("logistic"))
    model = est.fit(df, initial_tables=(ids, w0, V0), pipelined=pipelined)
    # the reference fit: randomSplit's replay (SGD.scala:111-112), then one reference step per non-empty split
    labels = np.asarray(df["label"], dtype=np.float64)
    rp, col, val = _explode(df["features"])
    split_of, _, order = random_split(df.partition_sizes, labels, df["features"], [frac] * n_iter, 1234, "LF")
    ref = R.Model.empty(nf, k)
    ref.load(ids, w0, V0)
    batches = []
    for i in range(n_iter):
        rows = order[split_of[order] == i]
        if len(rows):
            lens = (rp[rows + 1] - rp[rows]).astype(np.int64)
            ent = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in rows]).astype(np.int64) if lens.sum() else np.zeros(0, np.int64)
            batches.append((i + 1, R.CSR(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), col[ent].astype(np.int32),
                                         val[ent], labels[rows])))
    assert len(batches) >= 4
    n_upd, peak, losses = replay(ref, batches, "logistic", 0, step, reg)
    got = model._ctx.loss_history()
    print(f"fit logistic: losses device {got.tolist()} replay {losses}")
    assert len(got) == len(losses) and got[0] == pytest.approx(losses[0], rel=RTOL)  # the first step starts from equal tables
    assert_replay(model, ref, n_upd, peak, f"fit logistic (pipelined={pipelined})")


def test_logistic_transform_is_sigma_of_the_unclamped_score(gpu):
    from fm_spark_amd._native import CSRHost
    from fm_spark_amd.ml import FactorizationMachinesSGD, _explode

    df, nf = binary_frame(seed=5, n=120)
    est = (FactorizationMachinesSGD().setDimFactorization(4).setMaxIter(3).setStepSize(4.0).setRegParam(0.0).setNumFeatures(nf)
           .setInitialSd(0.5).setLoss("logistic"))
    model = est.fit(df)
    assert model.transformSchema(df.schema)[-2:] == ["rawPrediction", "prediction"]
    out = model.setMinLabel(0.4).setMaxLabel(0.6).transform(df)  # not applied to a logistic model
    raw, pred = np.asarray(out["rawPrediction"]), np.asarray(out["prediction"])
    rp, col, val = _explode(df["features"])
    unclamped = model._ctx.predict(CSRHost(rp, col, val, np.zeros(df.count())), -math.inf, math.inf)
    assert raw.tobytes() == unclamped.tobytes()
    assert np.array_equal(pred, O.sigmoid(raw))
    assert (np.abs(raw) > 1.0).any() and (pred < 0.4).any() and (pred > 0.6).any() and np.all((pred > 0) & (pred < 1))
    assert model.copy().transform(df)["prediction"] == out["prediction"]
    # a squared model transforms as ever: one column, clamped
    sq = (FactorizationMachinesSGD().setDimFactorization(4).setMaxIter(2).setNumFeatures(nf).fit(df)
          .setMinLabel(0.4).setMaxLabel(0.6))
    o2 = sq.transform(df)
    assert "rawPrediction" not in o2.schema
    learned = np.diff(rp) > 0
    assert np.all((np.asarray(o2["prediction"])[learned] >= 0.4) & (np.asarray(o2["prediction"])[learned] <= 0.6))
