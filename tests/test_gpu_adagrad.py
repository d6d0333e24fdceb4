"""GPU: the AdaGrad stage of the single-table step (fm_config.optimizer; fm_adagrad.hip) through the C-ABI and
the estimator, against tests/adagrad_ref.py and its budget.  The piece length L is read from the built
library (the seam fm_seam_adagrad_piece, fm_internal.h), so the run lengths follow a retuned kernel."""

import numpy as np
import pytest

import adagrad_ref as A
import runs
from fm_spark_amd import _native as N
from oracle import fm_ref as R
from problems import f32

pytestmark = pytest.mark.gpu

def piece():
    return int(N.load().fm_seam_adagrad_piece())  # (an int-returning C function: ctypes' default signature)


def new_ctx(F, k, ids, w, V, **kw):
    from fm_spark_amd.engine import FMContext

    kw.setdefault("optimizer", "adagrad")
    kw.setdefault("opt_init", A.G0)
    ctx = FMContext(F, k, **kw)
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
        if A.GROUP[loss]:
            b.set_group(A.GROUP[loss])
        if prepare:
            b.prepare()
        outs.append(ctx.step_batch(b, t, A.STEP, A.REG))
        b.close()
    return outs


@pytest.mark.parametrize("k,loss", A.CASES)
@pytest.mark.parametrize("prepare", [False, True])
def test_three_steps_against_the_reference(gpu, k, loss, prepare):
    batches, ids, w, V = A.three_step_case(k, loss)
    ref, ros = A.run_case(k, loss)
    ctx = new_ctx(A.F_CASE, k, ids, w, V, loss=loss)
    assert ctx.fuse_active is False
    for go, ro in zip(run_steps(ctx, batches, loss, prepare), ros):
        assert go.loss_sum == pytest.approx(ro.loss_sum, rel=A.RTOL, abs=A.ATOL)
        assert (go.n_rows, go.n_loss_rows, go.n_unique) == (ro.n_rows, ro.n_loss_rows, ro.n_unique)
    assert_within_budget(ref, ctx.export_tables(), f"k={k} {loss} prepared={prepare}")
    ctx.close()


def geometry_lengths(L):
    """test_run_geometry's runs (shared with tests/test_gpu_optimizer_edges.py, which runs them at other k)."""
    return [1, 2, L - 1, L, L + 1, 2 * L, 3 * L + 1, 1, 16 * L + 5, 3, 1]


@pytest.mark.parametrize("k", [16, 20])
def test_run_geometry(gpu, k):
    L = piece()
    lengths = geometry_lengths(L)
    F = len(lengths) + 2
    csr, ids, w, V = runs.make_runs(11 + k, lengths, F, k)
    model = R.Model.empty(F, k)
    model.load(ids, w, V)
    ref = A.AdaRef(model, A.G0)
    ro = ref.step(csr, 1, A.STEP, A.REG)
    ctx = new_ctx(F, k, ids, w, V)
    (go,) = run_steps(ctx, [csr])
    assert go.n_unique == ro.n_unique == len(lengths)
    assert go.loss_sum == pytest.approx(ro.loss_sum, rel=A.RTOL, abs=A.ATOL)
    assert_within_budget(ref, ctx.export_tables(), f"geometry k={k} L={L}")
    ctx.close()


@pytest.mark.parametrize("k", [16, 20])
def test_a_run_gives_the_same_bits_at_another_offset(gpu, k):
    """Rows 0 .. n - 1 hold one entry each of id X (a run of 3 L + 1); the other 77 rows hold one entry each of
    ids above X, or below it: the run begins the sorted view, or lies 77 entries in."""
    n, fill, X, F = 3 * piece() + 1, 77, 100, 200
    rng = np.random.default_rng(k)
    x, y = f32(rng.normal(0, 1, n + fill)), f32(rng.normal(0, 1, n + fill))
    w, V = f32(rng.normal(0, 0.1, F)), f32(rng.normal(0, 0.1, (F, k)))
    rows = []
    for base in (X + 1, 0):  # the filler ids' rows hold the same values wherever they lie
        col = np.concatenate([np.full(n, X), base + np.arange(fill) % 50]).astype(np.int32)
        Vb, wb = V.copy(), w.copy()
        Vb[base:base + 50], wb[base:base + 50] = V[101:151], w[101:151]
        ctx = new_ctx(F, k, np.arange(F, dtype=np.int32), wb, Vb)
        run_steps(ctx, [R.CSR(np.arange(n + fill + 1, dtype=np.int64), col, x, y)])
        rows.append(ctx.export_rows(np.array([X], np.int32)))
        ctx.close()
    assert all(np.array_equal(a, b) for a, b in zip(*rows))


def test_loss_bits_determinism_reset_and_reserve(gpu):
    k, loss = 16, "logistic"
    batches, ids, w, V = A.three_step_case(k, loss)
    sgd = new_ctx(A.F_CASE, k, ids, w, V, loss=loss, optimizer="sgd", fuse=False)
    first_loss = run_steps(sgd, batches[:1], loss)[0].loss_sum
    sgd.close()
    tabs, lib = [], N.load()
    for reset_before_third in (False, False, True):
        ctx = new_ctx(A.F_CASE, k, ids, w, V, loss=loss)
        b = ctx.batch(N.CSRHost(*(getattr(batches[0], f) for f in ("row_ptr", "col", "val", "label"))))
        ctx.reserve(b.n_rows, b.nnz)
        allocs = int(lib.fm_device_allocs_live())
        assert ctx.step_batch(b, 1, A.STEP, A.REG).loss_sum == first_loss  # an SGD context's, bit for bit
        assert int(lib.fm_device_allocs_live()) == allocs  # a reserved step allocates nothing
        after_one = ctx.export_tables()
        run_steps(ctx, batches[1:2], loss, ts=[2])
        if reset_before_third:  # with the first table back, the first step again
            ctx.load_tables(ids, w, V)
            ctx.optimizer_reset()
            ctx.step_batch(b, 1, A.STEP, A.REG)
            assert all(np.array_equal(x, y) for x, y in zip(ctx.export_rows(after_one[0]), after_one[1:]))
        else:
            run_steps(ctx, batches[2:], loss, ts=[3])
        tabs.append(ctx.export_tables())
        b.close()
        ctx.close()
    assert all(np.array_equal(x, y) for x, y in zip(tabs[0], tabs[1]))  # two contexts, equal bits
    ref, _ = A.run_case(k, loss, "sgd")  # the third step read the accumulators: far from an SGD third step
    assert np.abs(tabs[0][2] - ref.model.V[tabs[0][0]]).max() > 1e-3


def test_refusals(gpu):
    from fm_spark_amd.engine import FMContext

    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(N.FMError, match="opt_init"):
            FMContext(8, 4, optimizer="adagrad", opt_init=bad)
    for kw in ({"fuse": True}, {"parallel": "replicated"}, {"parallel": "sharded"}, {"shard_count": 2}):
        with pytest.raises(N.FMError, match="FM_OPT_ADAGRAD"):
            FMContext(8, 4, optimizer="adagrad", **kw)
    # a table beyond 256 MB, where the default fuses an SGD context
    for opt, fuses in (("sgd", True), ("adagrad", False)):
        big = FMContext(2_200_000, 16, optimizer=opt)
        assert big.fuse_active is fuses
        big.close()
    group = FMContext(8, 4, parallel="replicated", transport="copy")
    with pytest.raises(N.FMError, match="multi-GPU"):
        group.optimizer_reset()
    group.close()
    ctx = FMContext(8, 4, optimizer="adagrad")
    b = ctx.batch(N.CSRHost(np.array([0, 1]), np.array([0], np.int32), np.array([1.0]), np.array([1.0])))
    lib, h, bh = N.load(), ctx.handle, b.handle
    calls = [lambda: lib.fm_repl_grad(h, bh, None), lambda: lib.fm_repl_apply(h, None, 1, 0.1, 0.0, 1),
             lambda: lib.fm_shard_route(h, bh, None, None, None),
             lambda: lib.fm_shard_owner_prepare(h, bh, None, None, 0, None, None),
             lambda: lib.fm_shard_owner_forward(h, bh, None), lambda: lib.fm_shard_combine(h, bh, None, None),
             lambda: lib.fm_shard_owner_update(h, bh, None, 1, 0.1, 0.0, 1)]
    for call in calls:
        with pytest.raises(N.FMError, match="FM_OPT_ADAGRAD"):
            N.check(call())
    b.close()
    ctx.close()


def test_fit_and_fit_interactions_equal_the_engine_loop(gpu):
    """setOptimizer("adagrad") through the estimator: bit for bit the engine-level loop over the same batches
    (the suite's own replays of both: tests/test_gpu_objective_ml.py, tests/test_gpu_pairs_ml.py)."""
    import pair_ref as P
    from fm_spark_amd.data import splitmix64
    from fm_spark_amd.engine import FMContext
    from fm_spark_amd.ml import FactorizationMachinesSGD, _explode
    from fm_spark_amd.sampler import random_split
    from test_gpu_objective_ml import binary_frame
    from test_gpu_pairs_ml import estimator, frames

    def same(model, ctx):
        assert all(np.array_equal(x, y) for x, y in zip(model._ctx.export_tables(), ctx.export_tables()))
        ctx.close()

    # fit: randomSplit's batches, one host step each
    df, nf = binary_frame()
    k, n_iter, frac, g0 = 6, 5, 0.3, 0.5
    rng = np.random.default_rng(4)
    tables = np.arange(nf, dtype=np.int32), f32(rng.normal(0, 0.1, nf)), f32(rng.normal(0, 0.1, (nf, k)))
    est = (FactorizationMachinesSGD().setDimFactorization(k).setMaxIter(n_iter).setMiniBatchFraction(frac).setStepSize(0.8)
           .setRegParam(1e-3).setNumFeatures(nf).setLoss("logistic").setOptimizer("adagrad").setInitialAccumulator(g0))
    assert (est.getOptimizer(), est.getInitialAccumulator(), est.copy().getOptimizer()) == ("adagrad", g0, "adagrad")
    labels, (rp, col, val) = np.asarray(df["label"], dtype=np.float64), _explode(df["features"])
    split_of, _, order = random_split(df.partition_sizes, labels, df["features"], [frac] * n_iter, 1234, "LF")
    ctx = FMContext(nf, k, loss="logistic", optimizer="adagrad", opt_init=g0)
    ctx.load_tables(*tables)
    for i in range(n_iter):
        rows = order[split_of[order] == i]
        ent = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in rows]).astype(np.int64)
        brp = np.concatenate([[0], np.cumsum(rp[rows + 1] - rp[rows])]).astype(np.int64)
        ctx.step(N.CSRHost(brp, col[ent].astype(np.int32), val[ent], labels[rows]), i + 1, 0.8, 1e-3)
    same(est.fit(df, initial_tables=tables), ctx)
    # fitInteractions: the pairs drawn on the device, stepped unprepared
    p, contexts, candidates, interactions = frames()
    tables = np.arange(p.F, dtype=np.int32), f32(rng.normal(0, 0.1, p.F)), f32(rng.normal(0, 0.1, (p.F, P.K)))
    est = estimator(4).setLoss("bpr").setOptimizer("adagrad")
    ctx = FMContext(p.F, P.K, loss="bpr", optimizer="adagrad", opt_init=est.getInitialAccumulator())
    ctx.load_tables(*tables)
    bu, bc = (ctx.batch(N.CSRHost(r[0], r[1], r[2], np.zeros(len(r[0]) - 1))) for r in (p.contexts, p.candidates))
    ex = ctx.row_lists_from_pairs(p.pos_ctx, p.pos_cand, p.U, p.C)
    for t in range(1, 5):
        take = P.batch_positives(len(p.pos_ctx), P.SEED, P.FRAC, t)
        b = ctx._sample_pairs(bu, bc, p.pos_ctx[take], p.pos_cand[take], P.NEG, ex, 1.0, 0.0,
                              int(splitmix64(np.uint64(P.SEED))) ^ t, None, False)
        ctx.step_batch(b, t, P.STEP, P.REG)
    same(est.fitInteractions(contexts, candidates, interactions, initial_tables=tables), ctx)
