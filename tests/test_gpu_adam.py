"""GPU: the lazy AdamW rule of the window update stage (fm_config.optimizer = FM_OPT_ADAM; fm_adam.hip on
fm_window.h) through the C-ABI and the estimator, against tests/adam_ref.py and its budget.  The stage's geometry is
FTRL's, so the run lengths come from the same seams (tests/test_gpu_ftrl.py)."""

import numpy as np
import pytest

import adam_ref as Am
import runs
from fm_spark_amd import _native as N
from oracle import fm_ref as R
from problems import f32
from test_gpu_ftrl import assert_within_budget, geometry_lengths, run_steps

pytestmark = pytest.mark.gpu

HYPER = dict(opt_init=Am.EPS, opt_l2=Am.WD, opt_beta1=Am.B1, opt_beta2=Am.B2)


def new_ctx(F, k, ids, w, V, **kw):
    from fm_spark_amd.engine import FMContext

    ctx = FMContext(F, k, **{"optimizer": "adam", **HYPER, **kw})
    ctx.load_tables(ids, w, V)
    return ctx


@pytest.mark.parametrize("k,loss", Am.CASES + [(40, "squared"), (132, "squared")])
@pytest.mark.parametrize("prepare", [False, True])
def test_three_steps_against_the_reference(gpu, k, loss, prepare):
    batches, ids, w, V = Am.three_step_case(k, loss)
    ref, ros = Am.run_case(k, loss)
    ctx = new_ctx(Am.F_CASE, k, ids, w, V, loss=loss)
    assert ctx.fuse_active is False
    for go, ro in zip(run_steps(ctx, batches, loss, prepare), ros):
        assert go.loss_sum == pytest.approx(ro.loss_sum, rel=Am.RTOL, abs=Am.ATOL)
        assert (go.n_rows, go.n_loss_rows, go.n_unique) == (ro.n_rows, ro.n_loss_rows, ro.n_unique)
    assert_within_budget(ref, ctx.export_tables(), f"k={k} {loss} prepared={prepare}")
    ctx.close()


@pytest.mark.parametrize("k", [16, 20])
@pytest.mark.parametrize("lead", [0, 7])
def test_run_geometry_two_steps(gpu, k, lead):
    """Runs at every edge of a stretch and a window, stepped twice: the second step reads the moments and `last`
    that the first wrote at every close site (in a stretch, at the window's close, in the fold)."""
    lib = N.load()
    W, g = int(lib.fm_seam_ftrl_window()) & 0xFFFF, int(lib.fm_seam_ftrl_stretch(k))
    lengths = geometry_lengths(W, g, lead)
    F = len(lengths) + 2
    csr, ids, w, V = runs.make_runs(11 + k, lengths, F, k)
    model = R.Model.empty(F, k)
    model.load(ids, w, V)
    ref = Am.AdamRef(model)
    ros = [ref.step(csr, t, Am.STEP, Am.REG) for t in (1, 2)]
    ctx = new_ctx(F, k, ids, w, V)
    for go, ro in zip(run_steps(ctx, [csr, csr]), ros):
        assert go.n_unique == ro.n_unique == len(lengths)
        assert go.loss_sum == pytest.approx(ro.loss_sum, rel=Am.RTOL, abs=Am.ATOL)
    assert_within_budget(ref, ctx.export_tables(), f"geometry k={k} W={W} g={g} lead={lead}")
    ctx.close()


def test_untouched_rows_keep_their_record(gpu):
    k = 16
    batches, ids, w, V = Am.three_step_case(k, "squared")
    ctx = new_ctx(Am.F_CASE, k, ids, w, V)
    away = np.setdiff1d(ids, batches[0].col).astype(np.int32)
    assert len(away) > 0
    before = ctx.export_rows(away)
    b = batches[0]
    ctx.step(N.CSRHost(b.row_ptr, b.col, b.val, b.label), 1, Am.STEP, 0.0)  # no L1: nothing pending on them either
    assert all(np.array_equal(x, y) for x, y in zip(before, ctx.export_rows(away)))
    ctx.close()


def test_loss_bits_determinism_reset_and_reserve(gpu):
    """Two contexts give equal bits over three steps (so a row keeps its state while others are touched, the same
    way in both); after load_tables + optimizer_reset the first step replays: state zero and tau back at 0."""
    k, loss = 16, "logistic"
    batches, ids, w, V = Am.three_step_case(k, loss)
    sgd = new_ctx(Am.F_CASE, k, ids, w, V, loss=loss, optimizer="sgd", fuse=False)
    first_loss = run_steps(sgd, batches[:1], loss)[0].loss_sum
    sgd.close()
    tabs, lib = [], N.load()
    for reset_before_third in (False, False, True):
        ctx = new_ctx(Am.F_CASE, k, ids, w, V, loss=loss)
        b = ctx.batch(N.CSRHost(*(getattr(batches[0], f) for f in ("row_ptr", "col", "val", "label"))))
        ctx.reserve(b.n_rows, b.nnz)
        allocs = int(lib.fm_device_allocs_live())
        assert ctx.step_batch(b, 1, Am.STEP, Am.REG).loss_sum == first_loss  # an SGD context's, bit for bit
        assert int(lib.fm_device_allocs_live()) == allocs  # a reserved step allocates nothing
        after_one = ctx.export_tables()
        run_steps(ctx, batches[1:2], loss, ts=[2])
        if reset_before_third:
            ctx.load_tables(ids, w, V)
            ctx.optimizer_reset()
            ctx.step_batch(b, 1, Am.STEP, Am.REG)
            assert all(np.array_equal(x, y) for x, y in zip(ctx.export_rows(after_one[0]), after_one[1:]))
        else:
            run_steps(ctx, batches[2:], loss, ts=[3])
        tabs.append(ctx.export_tables())
        b.close()
        ctx.close()
    assert all(np.array_equal(x, y) for x, y in zip(tabs[0], tabs[1]))


def test_refusals(gpu):
    from fm_spark_amd.engine import FMContext

    nan = float("nan")
    for field, bad in (("opt_beta1", (-0.1, 1.0, nan)), ("opt_beta2", (1.5, float("inf"), nan)),
                       ("opt_init", (0.0, -1.0, nan)), ("opt_l2", (-1.0, nan))):
        for value in bad:
            with pytest.raises(N.FMError, match=field):
                FMContext(8, 4, optimizer="adam", **{field: value})
    for kw in ({"fuse": True}, {"parallel": "replicated"}, {"parallel": "sharded"}, {"shard_count": 2}):
        with pytest.raises(N.FMError, match="FM_OPT_ADAM"):
            FMContext(8, 4, optimizer="adam", **kw)
    with pytest.raises(ValueError, match="adam"):
        FMContext(8, 4, optimizer="adamw")
    ctx = FMContext(8, 4, optimizer="adam")  # eps 1e-8, the default rates
    b = ctx.batch(N.CSRHost(np.array([0, 1]), np.array([0], np.int32), np.array([1.0]), np.array([1.0])))
    lib, h, bh = N.load(), ctx.handle, b.handle
    calls = [lambda: lib.fm_repl_grad(h, bh, None), lambda: lib.fm_repl_apply(h, None, 1, 0.1, 0.0, 1),
             lambda: lib.fm_shard_route(h, bh, None, None, None), lambda: lib.fm_shard_combine(h, bh, None, None)]
    for call in calls:
        with pytest.raises(N.FMError, match="FM_OPT_ADAM"):
            N.check(call())
    b.close()
    ctx.close()
    group = FMContext(8, 4, parallel="replicated", transport="copy")
    with pytest.raises(N.FMError, match="multi-GPU"):
        group.optimizer_reset()
    group.close()


def test_fit_equals_the_engine_loop(gpu):
    """setOptimizer("adam") with the logistic loss through fit: bit for bit the engine-level loop over the same
    splits (tests/test_gpu_ftrl.py's replay)."""
    from fm_spark_amd.engine import FMContext
    from fm_spark_amd.ml import FactorizationMachinesSGD, _explode
    from fm_spark_amd.sampler import random_split
    from test_gpu_objective_ml import binary_frame

    df, nf = binary_frame()
    k, n_iter, frac, hyper = 6, 5, 0.3, dict(opt_init=1e-6, opt_l2=0.02, opt_beta1=0.8, opt_beta2=0.95)
    rng = np.random.default_rng(4)
    tables = np.arange(nf, dtype=np.int32), f32(rng.normal(0, 0.1, nf)), f32(rng.normal(0, 0.1, (nf, k)))
    est = (FactorizationMachinesSGD().setDimFactorization(k).setMaxIter(n_iter).setMiniBatchFraction(frac).setStepSize(0.05)
           .setRegParam(1e-3).setNumFeatures(nf).setLoss("logistic").setOptimizer("adam").setEpsilon(hyper["opt_init"])
           .setL2(hyper["opt_l2"]).setBeta1(hyper["opt_beta1"]).setBeta2(hyper["opt_beta2"]))
    assert (est.getOptimizer(), est.getBeta1(), est.copy().getBeta2(), est.getEpsilon()) == ("adam", 0.8, 0.95, 1e-6)
    assert (FactorizationMachinesSGD().getBeta1(), FactorizationMachinesSGD().getBeta2()) == (0.9, 0.999)
    with pytest.raises(ValueError, match="beta1"):
        est.copy().setBeta1(1.0)
    with pytest.raises(ValueError, match="one GPU"):
        est.copy().setParallel("replicated")
    labels, (rp, col, val) = np.asarray(df["label"], dtype=np.float64), _explode(df["features"])
    split_of, _, order = random_split(df.partition_sizes, labels, df["features"], [frac] * n_iter, 1234, "LF")
    ctx = FMContext(nf, k, loss="logistic", optimizer="adam", **hyper)
    ctx.load_tables(*tables)
    for i in range(n_iter):
        rows = order[split_of[order] == i]
        ent = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in rows]).astype(np.int64)
        brp = np.concatenate([[0], np.cumsum(rp[rows + 1] - rp[rows])]).astype(np.int64)
        ctx.step(N.CSRHost(brp, col[ent].astype(np.int32), val[ent], labels[rows]), i + 1, 0.05, 1e-3)
    model = est.fit(df, initial_tables=tables)
    assert all(np.array_equal(x, y) for x, y in zip(model._ctx.export_tables(), ctx.export_tables()))
    ctx.close()
