"""GPU: FactorizationMachinesSGD.fitInteractions on the planted recommender problem (tests/pair_ref.py)
against the fp64 oracle stepped over pair_ref's batches -- the same permutation rule, seeds and row order
-- and the fitted model through recommend and RankingEvaluator.

Parity tolerance: the multi-step one of tests/test_gpu_long_run.py,
    |dev - ref| <= RTOL |ref| + ATOL + n_upd 2^-22 peak
(n_upd: the steps whose batch held the row's id; peak: the largest |w| or |V| the oracle's row has held)."""

import numpy as np
import pytest

import pair_ref as P
from oracle import fm_ref as R
from test_gpu_parity import ATOL, RTOL

pytestmark = pytest.mark.gpu


def frames():
    from fm_spark_amd.linalg import SparseVector
    from fm_spark_amd.ml import DataFrame

    p = P.planted()
    contexts = DataFrame({"features": [SparseVector(p.F, [u], [1.0]) for u in range(p.U)]})
    candidates = DataFrame({"features": [SparseVector(p.F, [p.U + c], [1.0]) for c in range(p.C)]})
    interactions = DataFrame({"context": [int(v) for v in p.pos_ctx], "candidate": [int(v) for v in p.pos_cand]})
    return p, contexts, candidates, interactions


def estimator(n_iter):
    from fm_spark_amd.ml import FactorizationMachinesSGD

    return (FactorizationMachinesSGD().setDimFactorization(P.K).setInitialSd(P.SD).setStepSize(P.STEP).setRegParam(P.REG)
            .setMiniBatchFraction(P.FRAC).setMaxIter(n_iter).setNegativesPerPositive(P.NEG).setSeed(P.SEED))


@pytest.fixture(scope="module")
def fitted(gpu):
    p, contexts, candidates, interactions = frames()
    return estimator(P.ITERS).fitInteractions(contexts, candidates, interactions)


def test_six_iterations_match_the_oracle(gpu):
    p, contexts, candidates, interactions = frames()
    model = estimator(6).fitInteractions(contexts, candidates, interactions)
    ids, w, V = model._ctx.export_tables()
    assert model._ctx.epoch == 6
    ref = P.initial_model(p)
    n_upd, peak = np.zeros(p.F), np.zeros(p.F)
    track = lambda: np.maximum(peak, np.maximum(np.abs(ref.w), np.max(np.abs(ref.V), axis=1)))
    peak = track()
    for t in range(1, 7):
        b = P.iteration_batch(p, t)
        R.sgd_step_fast(ref, b, t, P.STEP, P.REG)
        n_upd[np.unique(b.col)] += 1
        peak = track()
    np.testing.assert_array_equal(ids, np.arange(p.F))
    slack = n_upd * 2.0 ** -22 * peak
    rw = np.abs(w - ref.w) / (RTOL * np.abs(ref.w) + ATOL + slack)
    rV = np.abs(V - ref.V) / (RTOL * np.abs(ref.V) + ATOL + slack[:, None])
    print(f"fitInteractions parity, 6 iterations: deviation / budget w {rw.max():.3f} V {rV.max():.3f}")
    assert rw.max() <= 1.0 and rV.max() <= 1.0


def test_the_fit_learns_the_held_out_rows(gpu, fitted):
    """precisionAtK(8) of the held-out rows, exclude = the training rows, no less than the oracle run's minus
    0.1 (fp32 tables flipping near-ties among the 232 eligible rows); untrained it is about 0.04."""
    from fm_spark_amd.tuning import RankingEvaluator

    p, contexts, candidates, _ = frames()
    oracle = P.held_out_metric("precisionAtK", 8, P.oracle_fit(P.ITERS)[0], p)
    got = RankingEvaluator().setMetricName("precisionAtK").setK(8).evaluateModel(fitted, contexts, candidates, p.held,
                                                                                   exclude=p.train)
    print(f"planted fit: precisionAtK(8) device {got:.4f}, oracle {oracle:.4f}")
    assert oracle >= 0.95
    assert got >= oracle - 0.1


def test_recommend_returns_held_out_rows(gpu, fitted):
    p, contexts, candidates, _ = frames()
    recs = fitted.recommend(contexts, candidates, 8, exclude=p.train)["recommendations"][0]
    assert len(recs) == 8 and set(c for c, _ in recs) <= set(p.held[0].tolist())


def test_unsupported_estimators_raise(gpu):
    p, contexts, candidates, interactions = frames()
    with pytest.raises(ValueError, match="multi-GPU"):
        estimator(2).setParallel("sharded", 2, devices=[0, 0], transport="copy").fitInteractions(contexts, candidates,
                                                                                                 interactions)
    held = contexts.with_column("label", [0.0] * p.U)
    with pytest.raises(ValueError, match="validationData"):
        estimator(2).setValidationData(held).fitInteractions(contexts, candidates, interactions)
