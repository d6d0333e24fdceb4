"""GPU: fm_batch_layout_splits -- the cached dataset uploaded in its own row order and laid out split
after split on the device (dfData.cache() + randomSplit, FactorizationMachinesSGD.scala:93, 111-112)
-- against fm_batch_create_splits over the host CSR of the same rows gathered on the host.

Both paths convert (float)val once and do integer work otherwise, so every comparison is exact:
the views' sizes, their predictions, every step's result and the exported tables, on two contexts
loaded identically."""

import logging
import os

import numpy as np
import pytest

from fm_spark_amd.linalg import SparseVector, Vectors
from problems import f32, make_problem
from test_gpu_parity import to_host
from test_gpu_resident_fit import _dataset, _select

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _split_rows(sels):
    return np.concatenate([[0], np.cumsum([len(x) for x in sels])]).astype(np.int64)


def _lay(sels):
    return np.concatenate([np.asarray(x, dtype=np.int64) for x in sels]) if sels else np.zeros(0, np.int64)


def _both(ctx_a, ctx_b, data, sels):
    """(the dataset laid out on the device, the dataset laid out on the host) of the same row lists."""
    lay, sr = _lay(sels), _split_rows(sels)
    return ctx_a.batch_layout_splits(to_host(data), sr, lay), ctx_b.batch_splits(to_host(_select(data, lay)), sr)


_CASE1 = {}


def _case1_problem():
    """~6,000 rows of up to 39 entries (three 16-lane trips), ~40 % of the values exactly 1.0 (the
    compact stream's unit branch) mixed with valued entries inside rows and across trips; rows with
    exactly 0, 1, 15, 16, 17 and 33 entries, one all-unit row and one row without a unit value."""
    if _CASE1:
        return _CASE1["p"]
    from oracle import fm_ref as R

    F, k = 50_000, 16
    data, ids, w, V = make_problem(1301, 6000, F, k, 20, empty_frac=0.1, hot=7)
    rng = np.random.default_rng(21)
    rows = [[data.col[data.row_ptr[i]:data.row_ptr[i + 1]].copy(), data.val[data.row_ptr[i]:data.row_ptr[i + 1]].copy()]
            for i in range(data.n_rows)]
    for c, v in rows:
        v[rng.random(len(v)) < 0.4] = 1.0
    lens = np.diff(data.row_ptr)
    assert lens.max() > 32
    special = {}
    for j, n in enumerate((0, 1, 15, 16, 17, 33)):
        r = 100 + 7 * j
        c = np.sort(rng.choice(F, size=n, replace=False)).astype(np.int32)
        v = f32(rng.normal(0.0, 1.0, size=n))
        v[rng.random(n) < 0.4] = 1.0
        rows[r] = [c, v]
        special[n] = r
    long_rows = np.flatnonzero(lens > 32)
    long_rows = long_rows[~np.isin(long_rows, list(special.values()))]
    unit_row, valued_row = int(long_rows[0]), int(long_rows[1])
    rows[unit_row][1][:] = 1.0
    rows[valued_row][1][rows[valued_row][1] == 1.0] = 0.5
    rp = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int64)
    csr = R.CSR(row_ptr=rp, col=np.concatenate([c for c, _ in rows]).astype(np.int32),
                val=np.concatenate([v for _, v in rows]).astype(np.float64), label=data.label)
    got = np.diff(csr.row_ptr)
    for n, r in special.items():
        assert got[r] == n
    assert np.all(csr.val[rp[unit_row]:rp[unit_row + 1]] == 1.0) and got[unit_row] > 32
    assert not np.any(csr.val[rp[valued_row]:rp[valued_row + 1]] == 1.0) and got[valued_row] > 32
    frac = np.mean(csr.val == 1.0)
    assert 0.3 < frac < 0.5
    picked = np.asarray(list(special.values()) + [unit_row, valued_row], dtype=np.int64)
    _CASE1["p"] = (F, k, csr, ids, w, V, picked)
    return _CASE1["p"]


@pytest.mark.parametrize("fuse,prepare", [(False, False), (False, True), (True, True)])
def test_layout_splits_bitwise_equal_host_layout(gpu, fuse, prepare):
    """Every stepped split of the device-laid-out dataset against the same split of the host-laid-out
    one: sizes, predictions, step results, then the tables.  Row lists: an empty split first, a
    permutation prefix, a sorted list with repeats, an empty split, a short split (the rows of forced
    lengths, the all-unit and the all-valued row), the last ten rows, a final split never stepped."""
    from fm_spark_amd.engine import FMContext

    F, k, data, ids, w, V, picked = _case1_problem()
    rng = np.random.default_rng(4)
    sels = [np.arange(0), rng.permutation(6000)[:1500], np.sort(rng.choice(6000, 2000, replace=True)), np.arange(0),
            rng.permutation(picked), np.arange(5990, 6000), np.arange(3000)]
    a, b = FMContext(F, k, fuse=fuse), FMContext(F, k, fuse=fuse)
    a.load_tables(ids, w, V)
    b.load_tables(ids, w, V)
    da, db = _both(a, b, data, sels)
    assert (da.n_rows, da.nnz) == (db.n_rows, db.nnz)
    va = vb = None
    for t, sel in enumerate(sels[:-1], start=1):
        va, vb = a.split_view(da, t - 1, into=va), b.split_view(db, t - 1, into=vb)
        assert (va.n_rows, va.nnz) == (vb.n_rows, vb.nnz)
        assert va.n_rows == len(sel)
        if len(sel):
            assert np.array_equal(a.predict_batch(va, 0.0, 1.0), b.predict_batch(vb, 0.0, 1.0))
        if prepare:
            va.prepare()
            vb.prepare()
        oa, ob = a.step_batch(va, t, 0.3, 1e-3), b.step_batch(vb, t, 0.3, 1e-3)
        assert (oa.loss_sum, oa.n_rows, oa.n_loss_rows, oa.n_unique, oa.executed) == \
            (ob.loss_sum, ob.n_rows, ob.n_loss_rows, ob.n_unique, ob.executed)
        assert oa.executed is bool(len(sel))
    for x, y in zip(a.export_tables(), b.export_tables()):
        assert np.array_equal(x, y)
    a.close()
    b.close()


def test_layout_splits_grid_stride_wrap(gpu):
    """40,000 laid-out rows against the launch's 32,768 teams: the row loop wraps.  The reversed
    permutation in 3 splits; every split's predictions and one step on split 0."""
    from fm_spark_amd.engine import FMContext
    from oracle import fm_ref as R

    F, k, D = 5000, 4, 40_000
    rng = np.random.default_rng(31)
    lens = rng.integers(0, 6, size=D)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(rp[-1])
    # distinct ids within a row: a random base per row plus a stride per entry
    within = np.arange(nnz) - np.repeat(rp[:-1], lens)
    col = ((np.repeat(rng.integers(0, F, size=D), lens) + 617 * within) % F).astype(np.int32)
    val = f32(rng.normal(0.0, 1.0, size=nnz))
    val[rng.random(nnz) < 0.4] = 1.0
    data = R.CSR(row_ptr=rp, col=col, val=val, label=(rng.random(D) < 0.25).astype(np.float64))
    ids = np.arange(F, dtype=np.int32)
    w, V = f32(rng.normal(0.0, 0.1, F)), f32(rng.normal(0.0, 0.1, (F, k)))
    order = np.arange(D, dtype=np.int64)[::-1]
    sels = [order[:13_000], order[13_000:33_333], order[33_333:]]
    a, b = FMContext(F, k), FMContext(F, k)
    a.load_tables(ids, w, V)
    b.load_tables(ids, w, V)
    da, db = _both(a, b, data, sels)
    views = []
    for s in range(3):
        va, vb = a.split_view(da, s), b.split_view(db, s)
        assert (va.n_rows, va.nnz) == (vb.n_rows, vb.nnz) and va.n_rows == len(sels[s])
        assert np.array_equal(a.predict_batch(va, 0.0, 1.0), b.predict_batch(vb, 0.0, 1.0))
        views.append((va, vb))
    oa, ob = a.step_batch(views[0][0], 1, 0.3, 1e-3), b.step_batch(views[0][1], 1, 0.3, 1e-3)
    assert (oa.loss_sum, oa.n_rows, oa.n_loss_rows, oa.n_unique) == (ob.loss_sum, ob.n_rows, ob.n_loss_rows, ob.n_unique)
    for x, y in zip(a.export_tables(), b.export_tables()):
        assert np.array_equal(x, y)
    a.close()
    b.close()


def test_layout_splits_rules(gpu):
    """order and split_rows are checked; a dataset of empty splits has nothing to do; the dataset
    itself is not stepped or prepared; createInitialModel and fm_batch_from_rows accept it as they
    accept the host-laid-out dataset."""
    from fm_spark_amd._native import FMError
    from fm_spark_amd.engine import FMContext

    F, k = 3000, 8
    data, ids, w, V = make_problem(1312, 900, F, k, 6)
    D = data.n_rows
    host = to_host(data)
    ctx = FMContext(F, k, seed=9)
    for bad in (-1, D):
        with pytest.raises(FMError, match="row index out of"):
            ctx.batch_layout_splits(host, [0, 3], [0, bad, 1])
    with pytest.raises((FMError, ValueError)):
        ctx.batch_layout_splits(host, [1, 3], [0, 1, 2])
    with pytest.raises((FMError, ValueError)):
        ctx.batch_layout_splits(host, [0, 3, 2], [0, 1])
    with pytest.raises((FMError, ValueError)):
        ctx.batch_layout_splits(host, [0, 3, 2, 3], [0, 1, 2])
    # every split empty
    e = ctx.batch_layout_splits(host, [0, 0, 0], np.zeros(0, np.int64))
    assert (e.n_rows, e.nnz) == (0, 0)
    for s in range(2):
        assert ctx.step_batch(ctx.split_view(e, s), 1, 0.3, 1e-3).executed is False
    # a full permutation: createInitialModel draws the plain dataset's rows
    rng = np.random.default_rng(5)
    perm = rng.permutation(D)
    sels = [perm[:300], perm[300:]]
    d = ctx.batch_layout_splits(host, _split_rows(sels), _lay(sels))
    with pytest.raises(FMError, match="split views"):
        ctx.step_batch(d, 1, 0.3, 1e-3)
    with pytest.raises(FMError, match="split views"):
        d.prepare()
    n1 = ctx.init_from_batch(d)
    ref = FMContext(F, k, seed=9)
    n2 = ref.init_from_batch(ref.batch(to_host(data)))
    assert n1 == n2
    for x, y in zip(ctx.export_tables(), ref.export_tables()):
        assert np.array_equal(x, y)
    # fm_batch_from_rows over either dataset: row i is laid-out row i
    dr = ref.batch_splits(to_host(_select(data, _lay(sels))), _split_rows(sels))
    rows = np.concatenate([rng.permutation(D)[:400], [0, 0, D - 1]])
    o1 = ctx.step_batch(ctx.batch_from_rows(d, rows), 1, 0.3, 1e-3)
    o2 = ref.step_batch(ref.batch_from_rows(dr, rows), 1, 0.3, 1e-3)
    assert (o1.loss_sum, o1.n_rows, o1.n_loss_rows, o1.n_unique) == (o2.loss_sum, o2.n_rows, o2.n_loss_rows, o2.n_unique)
    for x, y in zip(ctx.export_tables(), ref.export_tables()):
        assert np.array_equal(x, y)
    ctx.close()
    ref.close()


@pytest.mark.parametrize("mode", ["sharded", "replicated"])
def test_layout_splits_on_a_multi_gpu_context(gpu, mode):
    """Three ranks on one device (COPY transport): every rank lays out its share of every split from
    the whole source.  Ragged splits, one with fewer rows than ranks, one empty; two iterations of the
    split-view loop against the host-laid-out dataset: losses and tables, bitwise."""
    from fm_spark_amd.engine import FMContext
    from fm_spark_amd.ml import run_minibatch_sgd_splits

    F, k, R = 3000, 8, 3
    data, ids, w, V = make_problem(1315, 2500, F, k, 9, hot=4)
    rng = np.random.default_rng(13)
    sels = [rng.permutation(2500)[:901], np.arange(0), np.sort(rng.choice(2500, 1300)), rng.permutation(2500)[:2],
            rng.permutation(2500)[:100]]

    def run(on_device):
        ctx = FMContext(F, k, parallel=mode, n_gpus=R, devices=[0] * R, transport="copy")
        ctx.load_tables(ids, w, V)
        lay, sr = _lay(sels), _split_rows(sels)
        d = (ctx.batch_layout_splits(to_host(data), sr, lay) if on_device
             else ctx.batch_splits(to_host(_select(data, lay)), sr))
        losses = []
        for _ in range(2):
            losses += run_minibatch_sgd_splits(ctx, d, 0.3, 1e-3, n_iter=4)
        tab = ctx.export_tables()
        ctx.close()
        return (d.n_rows, d.nnz), losses, tab

    a, b = run(True), run(False)
    assert a[0] == b[0]
    assert len(a[1]) == 6 and a[1] == b[1]
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(x, y)


def _fit_problems():
    from fm_spark_amd.data import read_libsvm
    from fm_spark_amd.ml import DataFrame, FactorizationMachinesSGD

    labels, pairs, nf = read_libsvm(os.path.join(GOLD, "sample.txt"))
    g = np.load(os.path.join(GOLD, "c1_sample.npz"))
    df = DataFrame({"label": [float(y) for y in labels], "features": [Vectors.sparse(nf, p) for p in pairs]},
                   g["part_sizes"].tolist())
    est = (FactorizationMachinesSGD().setDimFactorization(int(g["k"])).setMaxIter(int(g["max_iter"]))
           .setStepSize(float(g["step"])).setRegParam(float(g["reg"])).setNumFeatures(int(g["F"])).setSeed(5))
    yield "sample.txt", df, est, int(g["max_iter"])
    est = (FactorizationMachinesSGD().setDimFactorization(8).setMaxIter(5).setMiniBatchFraction(0.15)
           .setStepSize(0.5).setRegParam(1e-4).setNumFeatures(20_000).setSeed(5))
    yield "random", _dataset(2000, 20_000, 77, 4), est, 5


def test_pipelined_fit_lays_out_on_the_device(gpu, caplog, monkeypatch):
    """fit(pipelined=True) builds no permuted host copy: with ml._select_csr replaced by a function
    that raises it completes, and gives the synchronous fit's model and loss log lines (compared as
    test_pipelined_fit_matches_synchronous_fit compares them)."""
    import fm_spark_amd.ml as ml

    def boom(*a, **kw):
        raise AssertionError("the pipelined fit called _select_csr")

    for name, df, est, it in _fit_problems():
        logs, tabs = [], []
        for pipe in (True, False):
            caplog.clear()
            with monkeypatch.context() as mp:
                if pipe:
                    mp.setattr(ml, "_select_csr", boom)
                with caplog.at_level(logging.INFO, logger="org.apache.spark.ml.fm"):
                    m = est.copy().fit(df, pipelined=pipe)
            logs.append([(r.levelname, r.getMessage()) for r in caplog.records])
            tabs.append(m._ctx.export_tables())
        assert len(logs[0]) == it and len(logs[1]) == it, name
        for (l1, m1), (l2, m2) in zip(*logs):
            assert l1 == l2
            h1, v1 = m1.rsplit(" ", 1)
            h2, v2 = m2.rsplit(" ", 1)
            assert h1 == h2
            if l1 == "INFO":
                assert float(v1) == pytest.approx(float(v2), rel=1e-9)
        np.testing.assert_array_equal(tabs[0][0], tabs[1][0])
        np.testing.assert_allclose(tabs[0][1], tabs[1][1], rtol=1e-5, atol=1e-8)
        np.testing.assert_allclose(tabs[0][2], tabs[1][2], rtol=1e-5, atol=1e-8)
