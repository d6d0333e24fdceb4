"""GPU: the FTRL-Proximal stage of the single-table step (fm_config.optimizer = FM_OPT_FTRL; fm_ftrl.hip) through
the C-ABI and the estimator, against tests/ftrl_ref.py and its budget.  The window W and the lane groups' stretch
are read from the built library (the seams fm_seam_ftrl_window / fm_seam_ftrl_stretch, fm_internal.h), so the run
lengths follow a retuned kernel."""

import numpy as np
import pytest

import ftrl_ref as Fr
import runs
from fm_spark_amd import _native as N
from oracle import fm_ref as R
from problems import f32

pytestmark = pytest.mark.gpu


def new_ctx(F, k, ids, w, V, **kw):
    from fm_spark_amd.engine import FMContext

    kw.setdefault("optimizer", "ftrl")
    ctx = FMContext(F, k, opt_init=Fr.BETA, opt_l2=Fr.L2, **kw)
    ctx.load_tables(ids, w, V)
    return ctx


def assert_within_budget(ref, tab, what):
    gids, gw, gV = tab
    pids = np.nonzero(ref.model.present)[0]
    np.testing.assert_array_equal(gids, pids)
    bw, bV = ref.budget()
    ew, eV = np.abs(gw - ref.model.w[pids]) / bw[pids], np.abs(gV - ref.model.V[pids]) / bV[pids]
    print(f"{what}: largest error over budget w {ew.max():.3f} V {eV.max():.3f}")
    assert np.all(np.isfinite(gw)) and np.all(np.isfinite(gV))
    assert ew.max() <= 1.0 and eV.max() <= 1.0


def run_steps(ctx, batches, loss="squared", prepare=False, ts=None):
    outs = []
    for t, csr in zip(ts or range(1, len(batches) + 1), batches):
        b = ctx.batch(N.CSRHost(csr.row_ptr, csr.col, csr.val, csr.label))
        if Fr.GROUP[loss]:
            b.set_group(Fr.GROUP[loss])
        if prepare:
            b.prepare()
        outs.append(ctx.step_batch(b, t, Fr.STEP, Fr.REG))
        b.close()
    return outs


@pytest.mark.parametrize("k,loss", Fr.CASES + [(40, "squared"), (100, "squared"), (132, "squared")])
@pytest.mark.parametrize("prepare", [False, True])
def test_three_steps_against_the_reference(gpu, k, loss, prepare):
    """... and, on the same table, the exact zeros: what the reference zeroes safely inside the threshold is 0.0."""
    batches, ids, w, V = Fr.three_step_case(k, loss)
    ref, ros = Fr.run_case(k, loss)
    ctx = new_ctx(Fr.F_CASE, k, ids, w, V, loss=loss)
    assert ctx.fuse_active is False
    for go, ro in zip(run_steps(ctx, batches, loss, prepare), ros):
        assert go.loss_sum == pytest.approx(ro.loss_sum, rel=Fr.RTOL, abs=Fr.ATOL)
        assert (go.n_rows, go.n_loss_rows, go.n_unique) == (ro.n_rows, ro.n_loss_rows, ro.n_unique)
    tab = ctx.export_tables()
    assert_within_budget(ref, tab, f"k={k} {loss} prepared={prepare}")
    touched, zeroed = ref.zeroed(Fr.REG)
    assert zeroed.sum() >= 0.1 * touched.sum()
    assert np.all(np.column_stack([tab[1], tab[2]])[zeroed[tab[0]]] == 0.0)
    ctx.close()


def geometry_lengths(W, g, lead):
    """test_run_geometry's runs (shared with tests/test_gpu_optimizer_edges.py, which runs them at other k)."""
    return [lead] * (lead > 0) + [1, 2, g - 1, g, g + 1, W - 1, W, W + 1, 2 * W, 3 * W + 1, 1, 16 * W + 5, 3, 1]


@pytest.mark.parametrize("k", [16, 20])
@pytest.mark.parametrize("lead", [0, 7])
def test_run_geometry(gpu, k, lead):
    """Runs at every edge of a stretch (g) and a window (W); behind a leading run of 7 they straddle the edges at
    other offsets."""
    lib = N.load()
    W, g = int(lib.fm_seam_ftrl_window()) & 0xFFFF, int(lib.fm_seam_ftrl_stretch(k))
    assert int(lib.fm_seam_ftrl_window()) >> 16 == int(lib.fm_seam_ftrl_stretch(16))
    lengths = geometry_lengths(W, g, lead)
    F = len(lengths) + 2
    csr, ids, w, V = runs.make_runs(11 + k, lengths, F, k)
    model = R.Model.empty(F, k)
    model.load(ids, w, V)
    ref = Fr.FtrlRef(model)
    ro = ref.step(csr, 1, Fr.STEP, Fr.REG)
    ctx = new_ctx(F, k, ids, w, V)
    (go,) = run_steps(ctx, [csr])
    assert go.n_unique == ro.n_unique == len(lengths)
    assert go.loss_sum == pytest.approx(ro.loss_sum, rel=Fr.RTOL, abs=Fr.ATOL)
    assert_within_budget(ref, ctx.export_tables(), f"geometry k={k} W={W} g={g} lead={lead}")
    ctx.close()


def test_untouched_rows_keep_their_bits(gpu):
    k = 16
    batches, ids, w, V = Fr.three_step_case(k, "squared")
    ctx = new_ctx(Fr.F_CASE, k, ids, w, V)
    away = np.setdiff1d(ids, batches[0].col).astype(np.int32)
    assert len(away) > 0 and Fr.REG > 0
    before = ctx.export_rows(away)
    run_steps(ctx, batches[:1])
    assert all(np.array_equal(a, b) for a, b in zip(before, ctx.export_rows(away)))
    ctx.close()


def test_loss_bits_determinism_reset_and_reserve(gpu):
    k, loss = 16, "logistic"
    batches, ids, w, V = Fr.three_step_case(k, loss)
    sgd = new_ctx(Fr.F_CASE, k, ids, w, V, loss=loss, optimizer="sgd", fuse=False)
    first_loss = run_steps(sgd, batches[:1], loss)[0].loss_sum
    sgd.close()
    tabs, lib = [], N.load()
    for reset_before_third in (False, False, True):
        ctx = new_ctx(Fr.F_CASE, k, ids, w, V, loss=loss)
        b = ctx.batch(N.CSRHost(*(getattr(batches[0], f) for f in ("row_ptr", "col", "val", "label"))))
        ctx.reserve(b.n_rows, b.nnz)
        allocs = int(lib.fm_device_allocs_live())
        assert ctx.step_batch(b, 1, Fr.STEP, Fr.REG).loss_sum == first_loss  # an SGD context's, bit for bit
        assert int(lib.fm_device_allocs_live()) == allocs  # a reserved step allocates nothing
        after_one = ctx.export_tables()
        run_steps(ctx, batches[1:2], loss, ts=[2])
        if reset_before_third:  # with the first table back, the first step again
            ctx.load_tables(ids, w, V)
            ctx.optimizer_reset()
            ctx.step_batch(b, 1, Fr.STEP, Fr.REG)
            assert all(np.array_equal(x, y) for x, y in zip(ctx.export_rows(after_one[0]), after_one[1:]))
        else:
            run_steps(ctx, batches[2:], loss, ts=[3])
        tabs.append(ctx.export_tables())
        b.close()
        ctx.close()
    assert all(np.array_equal(x, y) for x, y in zip(tabs[0], tabs[1]))  # two contexts, equal bits


def test_refusals(gpu):
    from fm_spark_amd.engine import FMContext

    for field, bad in (("opt_init", (0.0, -1.0, float("nan"))), ("opt_l2", (-1.0, float("nan")))):
        for value in bad:
            with pytest.raises(N.FMError, match=field):
                FMContext(8, 4, optimizer="ftrl", **{field: value})
    for kw in ({"fuse": True}, {"parallel": "replicated"}, {"parallel": "sharded"}, {"shard_count": 2}):
        with pytest.raises(N.FMError, match="FM_OPT_FTRL"):
            FMContext(8, 4, optimizer="ftrl", **kw)
    ctx = FMContext(8, 4, optimizer="ftrl")
    b = ctx.batch(N.CSRHost(np.array([0, 1]), np.array([0], np.int32), np.array([1.0]), np.array([1.0])))
    lib, h, bh = N.load(), ctx.handle, b.handle
    calls = [lambda: lib.fm_repl_grad(h, bh, None), lambda: lib.fm_repl_apply(h, None, 1, 0.1, 0.0, 1),
             lambda: lib.fm_shard_route(h, bh, None, None, None), lambda: lib.fm_shard_combine(h, bh, None, None)]
    for call in calls:
        with pytest.raises(N.FMError, match="FM_OPT_FTRL"):
            N.check(call())
    b.close()
    ctx.close()


def test_fit_equals_the_engine_loop(gpu):
    """setOptimizer("ftrl") with the logistic loss through fit: bit for bit the engine-level loop over the same
    splits (the suite's own replay: tests/test_gpu_objective_ml.py)."""
    from fm_spark_amd.engine import FMContext
    from fm_spark_amd.ml import FactorizationMachinesSGD, _explode
    from fm_spark_amd.sampler import random_split
    from test_gpu_objective_ml import binary_frame

    df, nf = binary_frame()
    k, n_iter, frac, beta, l2 = 6, 5, 0.3, 0.02, 0.01
    rng = np.random.default_rng(4)
    tables = np.arange(nf, dtype=np.int32), f32(rng.normal(0, 0.1, nf)), f32(rng.normal(0, 0.1, (nf, k)))
    est = (FactorizationMachinesSGD().setDimFactorization(k).setMaxIter(n_iter).setMiniBatchFraction(frac).setStepSize(0.8)
           .setRegParam(1e-3).setNumFeatures(nf).setLoss("logistic").setOptimizer("ftrl").setInitialAccumulator(beta).setL2(l2))
    assert (est.getOptimizer(), est.getL2(), est.copy().getL2()) == ("ftrl", l2, l2)
    with pytest.raises(ValueError, match="one GPU"):
        est.copy().setParallel("replicated")
    labels, (rp, col, val) = np.asarray(df["label"], dtype=np.float64), _explode(df["features"])
    split_of, _, order = random_split(df.partition_sizes, labels, df["features"], [frac] * n_iter, 1234, "LF")
    ctx = FMContext(nf, k, loss="logistic", optimizer="ftrl", opt_init=beta, opt_l2=l2)
    ctx.load_tables(*tables)
    for i in range(n_iter):
        rows = order[split_of[order] == i]
        ent = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in rows]).astype(np.int64)
        brp = np.concatenate([[0], np.cumsum(rp[rows + 1] - rp[rows])]).astype(np.int64)
        ctx.step(N.CSRHost(brp, col[ent].astype(np.int32), val[ent], labels[rows]), i + 1, 0.8, 1e-3)
    model = est.fit(df, initial_tables=tables)
    assert all(np.array_equal(x, y) for x, y in zip(model._ctx.export_tables(), ctx.export_tables()))
    ctx.close()
