"""fm_evaluate / fm_evaluate_batch / fm_eval_history (include/fm_hip.h): the error sums of predict
against the labels, reduced on the device.

The sums are held to eval_ref's exact sums over the call's own predictions within the derived budget of
a reordered fp64 sum; the predictions to the oracle and to fm_predict with the predict tests' tolerance
(rtol 1e-5, atol 1e-7, tests/test_gpu_group.py).  Shapes are a few hundred rows over a table of a few
hundred ids; the team shapes come from the forward's launch log, not from a copy of the dispatch.
"""

import ctypes as C
import math

import numpy as np
import pytest

import eval_ref
from oracle import fm_ref as R_
from problems import f32, make_problem

pytestmark = pytest.mark.gpu

EVALUATE = 7  # FwdMode kEvaluate (fm_spark_amd/csrc/fm_internal.h)
F, N_PRESENT, W0 = 400, 300, 0.25
CLAMPS = ((0.0, 1.0), (-math.inf, math.inf))


def _host(c):
    from fm_spark_amd._native import CSRHost

    return CSRHost(c.row_ptr, c.col, c.val, c.label)


def _tables(k, seed=3):
    rng = np.random.default_rng(seed)
    present = np.sort(rng.choice(F, size=N_PRESENT, replace=False)).astype(np.int32)
    w = f32(rng.normal(0.0, 0.1, F))
    V = f32(rng.normal(0.0, 0.1, (F, k)))
    return present, w, V


def _model(k, present, w, V):
    m = R_.Model.empty(F, k, w0=W0)
    m.load(present, w[present], V[present])
    return m


def _single(k, present, w, V, **kw):
    from fm_spark_amd.engine import FMContext

    ctx = FMContext(F, k, w0=W0, **kw)
    ctx.load_tables(present, w[present], V[present])
    return ctx


_TEAM = {}


def _team(k):
    """lanes per sample of the evaluation at this k, read from the forward's launch log"""
    import forward_probe as fp

    if k not in _TEAM:
        present, w, V = _tables(k)
        ctx = _single(k, present, w, V)
        csr = R_.CSR(np.array([0, 1], np.int64), present[:1].copy(), np.ones(1), np.zeros(1))
        with fp.grid_cap(1):
            ctx.evaluate(_host(csr), 0.0, 1.0)
            log = fp.read_log()
        ctx.close()
        assert [r.mode for r in log] == [EVALUATE], log
        _TEAM[k] = log[0].team
    return _TEAM[k]


def _rows(n, k, present, seed, out_of_range=True):
    """n rows: the edge rows first -- 3 TEAM + 1 entries, no entry, one entry, only absent ids, only
    ids >= F, those two mixed with learned ids -- then random rows; values shrunk on long rows."""
    rng = np.random.default_rng(seed)
    team = _team(k)
    absent = np.setdiff1d(np.arange(F), present)
    beyond = np.arange(F, F + 30)
    kinds = [
        rng.choice(present, size=3 * team + 1, replace=False),
        np.zeros(0, np.int64),
        rng.choice(present, size=1),
        rng.choice(absent, size=3, replace=False),
        beyond[:4] if out_of_range else rng.choice(absent, size=2, replace=False),
        np.concatenate([rng.choice(present, size=5, replace=False), rng.choice(absent, size=2, replace=False),
                        beyond[4:7] if out_of_range else np.zeros(0, np.int64)]),
    ]
    rp, cols, vals = [0], [], []
    for i in range(n):
        ids = kinds[i] if i < len(kinds) else rng.choice(F, size=int(rng.integers(0, 14)), replace=False)
        ids = np.sort(np.asarray(ids, dtype=np.int64))
        x = f32(rng.normal(0.0, 1.0, len(ids)) * min(1.0, 4.0 / math.sqrt(max(len(ids), 1))))
        cols += ids.tolist()
        vals += x.tolist()
        rp.append(len(cols))
    return R_.CSR(np.asarray(rp, np.int64), np.asarray(cols, np.int32), np.asarray(vals, np.float64), np.zeros(n))


def _cancelling_labels(ref_pred):
    """labels around the predictions so that the signed errors largely cancel: sum_err is then a small
    number left over from large terms, where the order of summation shows"""
    n = len(ref_pred)
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    return ref_pred + sign * (0.37 + 1e-3 * np.arange(n) / max(n, 1))


def _in_range(csr):
    keep = csr.col < F
    rows = np.repeat(np.arange(csr.n_rows), np.diff(csr.row_ptr))[keep]
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=csr.n_rows))]).astype(np.int64)
    return R_.CSR(rp, csr.col[keep], csr.val[keep], csr.label)


# ----------------------------------------------------------------- 1. sums against the call's own pred
@pytest.mark.parametrize("n", [1, 7, 8, 9, 257])
@pytest.mark.parametrize("k", [3, 16, 80, 132])
def test_sums_match_the_calls_own_predictions(gpu, k, n):
    present, w, V = _tables(k)
    model = _model(k, present, w, V)
    ctx = _single(k, present, w, V)
    csr = _rows(n, k, present, seed=100 + n)
    for lo, hi in CLAMPS:
        ref_pred = R_.predict(model, csr, lo, hi, num_features=F)
        csr.label = _cancelling_labels(ref_pred)
        n_unl = int((~eval_ref.learned_rows(model, csr, F)).sum())
        # the host rows (ids >= F included)
        rec, pred = ctx.evaluate(_host(csr), lo, hi, want_pred=True)
        ref = eval_ref.check(rec, csr.label, pred, n_unlearned=n_unl)
        print(f"k={k} n={n} clamp=({lo},{hi}) sum_err={rec.sum_err!r} exact={ref.err.value!r} budget={ref.err.budget:.3e}")
        np.testing.assert_allclose(pred, ref_pred, rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(pred, ctx.predict(_host(csr), lo, hi), rtol=1e-5, atol=1e-7)
        assert rec.executed and rec.epoch == 0
        if n >= 7:  # the labels do cancel: at most one term of ~0.37 is left of n
            assert abs(rec.sum_err) < 0.4 and rec.sum_abs_err > 0.36 * n
        # the same rows resident (ids >= F cannot be uploaded: dropped beforehand, as the kernel drops them)
        b = ctx.batch(_host(_in_range(csr)))
        rec_b, pred_b = ctx.evaluate_batch(b, lo, hi, want_pred=True)
        eval_ref.check(rec_b, csr.label, pred_b, n_unlearned=n_unl)
        np.testing.assert_allclose(pred_b, ctx.predict_batch(b, lo, hi), rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(pred_b, ref_pred, rtol=1e-5, atol=1e-7)
        assert ctx.evaluate_batch(b, lo, hi) == rec_b  # without pred: the same record
        b.close()
    ctx.close()


# ------------------------------------------------- 2. teams walking several samples, many blocks folded
@pytest.mark.parametrize("k", [3, 16])
def test_grid_caps_and_many_blocks(gpu, k):
    import forward_probe as fp

    present, w, V = _tables(k)
    model = _model(k, present, w, V)
    ctx = _single(k, present, w, V)
    csr = _rows(300, k, present, seed=7, out_of_range=False)
    csr.label = _cancelling_labels(R_.predict(model, csr, 0.0, 1.0, num_features=F))
    b = ctx.batch(_host(csr))
    base_rec, base_pred = ctx.evaluate_batch(b, 0.0, 1.0, want_pred=True)
    eval_ref.check(base_rec, csr.label, base_pred)
    for cap in (1, 2, 3):
        with fp.grid_cap(cap):
            rec, pred = ctx.evaluate_batch(b, 0.0, 1.0, want_pred=True)
            log = fp.read_log()
        assert [(r.mode, r.blocks, r.rows) for r in log] == [(EVALUATE, cap, 300)], log
        assert log[0].team == _team(k)
        np.testing.assert_array_equal(pred, base_pred)
        assert (rec.n_rows, rec.n_unlearned) == (base_rec.n_rows, base_rec.n_unlearned)
        eval_ref.check(rec, csr.label, pred)
    b.close()
    # the default grid over 2049 rows: hundreds of per-block records folded
    big = make_problem(11, 2049, F, k, 6, labels="real")[0]
    pb = R_.predict(model, big, 0.0, 1.0, num_features=F)
    big.label = _cancelling_labels(pb)
    bb = ctx.batch(_host(big))
    rec, pred = ctx.evaluate_batch(bb, 0.0, 1.0, want_pred=True)
    assert 2049 // (fp.consts().block // _team(k)) >= 100  # blocks of the launch
    eval_ref.check(rec, big.label, pred, n_unlearned=int((~eval_ref.learned_rows(model, big, F)).sum()))
    np.testing.assert_allclose(pred, pb, rtol=1e-5, atol=1e-7)
    bb.close()
    ctx.close()


# ------------------------------------------------------------------- 3. determinism and side effects
def _last_stats(ctx):
    from fm_spark_amd import _native as N

    ls, nl, nu = C.c_double(), C.c_int64(), C.c_int64()
    N.check(N.load().fm_last_stats(ctx.handle, C.byref(ls), C.byref(nl), C.byref(nu)), "fm_last_stats")
    return ls.value, nl.value, nu.value


def test_deterministic_and_without_side_effects(gpu):
    k = 16
    present, w, V = _tables(k)
    model = _model(k, present, w, V)
    train = make_problem(21, 200, F, k, 6)[0]
    held = make_problem(22, 150, F, k, 6, labels="real")[0]
    ctxs = [_single(k, present, w, V) for _ in range(2)]  # the second never evaluates
    bt = [c.batch(_host(train)) for c in ctxs]
    for t in (1, 2):
        R_.sgd_step_fast(model, train, t, 0.3, 0.05)
        for c, b in zip(ctxs, bt):
            c.step_batch(b, t, 0.3, 0.05)
    ctx = ctxs[0]
    before = (ctx.epoch, ctx.loss_history().tobytes(), _last_stats(ctx))
    bh = ctx.batch(_host(held))
    # no export so far: the rows' lazy L1 is pending when the evaluation reads them
    rec1, pred1 = ctx.evaluate_batch(bh, 0.0, 1.0, want_pred=True)
    rec2, pred2 = ctx.evaluate_batch(bh, 0.0, 1.0, want_pred=True)
    assert rec1 == rec2 and rec1.epoch == 2
    np.testing.assert_array_equal(pred1, pred2)
    eval_ref.check(rec1, held.label, pred1)
    np.testing.assert_allclose(pred1, R_.predict(model, held, 0.0, 1.0, num_features=F), rtol=1e-5, atol=1e-7)
    assert (ctx.epoch, ctx.loss_history().tobytes(), _last_stats(ctx)) == before
    for a, b in zip(ctx.export_tables(), ctxs[1].export_tables()):
        np.testing.assert_array_equal(a, b)
    for c in ctxs:
        c.close()


# ----------------------------------------------------------------------------------------- 4. history
def test_history_of_enqueued_evaluations(gpu):
    k = 16
    present, w, V = _tables(k)
    data = make_problem(31, 240, F, k, 6, labels="real")[0]
    split_rows = np.array([0, 80, 160, 240])
    sel = np.random.default_rng(5).permutation(240)[:70]
    recs = {}
    for sync in (False, True):
        ctx = _single(k, present, w, V)
        ds = ctx.batch_splits(_host(data), split_rows)
        view = ctx.split_view(ds, 0)
        flat = ctx.batch(_host(data))
        got = [ctx.evaluate_batch(view, 0.0, 1.0, sync=sync)]            # epoch 0, a split view
        view.prepare()
        ctx.step_batch(view, 1, 0.3, 0.05, sync=False)
        picked = ctx.batch_from_rows(flat, sel)
        got.append(ctx.evaluate_batch(picked, 0.0, 1.0, sync=sync))      # epoch 1, a gathered batch
        view = ctx.split_view(ds, 1, into=view)
        ctx.step_batch(view, 2, 0.3, 0.05, sync=False)
        picked = ctx.batch_from_rows(flat, sel[::-1].copy(), into=picked)  # refilled: the evaluation waits for the gather
        got.append(ctx.evaluate_batch(picked, -math.inf, math.inf, sync=sync))  # epoch 2
        hist = ctx.eval_history()
        assert len(hist) == 3 and [h.epoch for h in hist] == [0, 1, 2]
        if sync:
            assert hist == got
        else:
            assert got == [None, None, None]
        recs[sync] = hist
        for x in (picked, view, flat, ds):
            x.close()
        ctx.close()
    assert recs[False] == recs[True]
    assert recs[True][1].n_rows == 70 and recs[True][0].n_rows == 80


def test_history_grows_past_its_first_capacity(gpu):
    k = 3
    present, w, V = _tables(k)
    ctx = _single(k, present, w, V)
    small = make_problem(41, 8, F, k, 5, labels="real")[0]
    other = make_problem(42, 8, F, k, 5, labels="real")[0]
    bs, bo = ctx.batch(_host(small)), ctx.batch(_host(other))
    first = [ctx.evaluate_batch(bo, 0.0, 1.0), ctx.evaluate_batch(bs, 0.0, 1.0), ctx.evaluate_batch(bo, -1.0, 2.0)]
    for _ in range(4100 - 3):
        ctx.evaluate_batch(bs, 0.0, 1.0, sync=False)
    hist = ctx.eval_history()
    assert len(hist) == 4100
    assert hist[:3] == first                       # kept across the growth at 4096
    assert all(h == first[1] for h in hist[3:])    # equal inputs, equal bits, before and after it
    bs.close()
    bo.close()
    ctx.close()


# ------------------------------------------------------------------------- 5. arguments and lifetime
def test_arguments_and_lifetime(gpu):
    from fm_spark_amd import _native as N
    from fm_spark_amd.engine import FMContext

    lib = N.load()
    k = 16
    present, w, V = _tables(k)
    bytes0, allocs0 = lib.fm_device_bytes_live(), lib.fm_device_allocs_live()
    ctx = _single(k, present, w, V)
    other = FMContext(F, k)
    csr = make_problem(51, 100, F, k, 6, labels="real")[0]
    b = ctx.batch(_host(csr))
    empty = ctx.batch(_host(R_.CSR(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0), np.zeros(0))))
    ds = ctx.batch_splits(_host(csr), np.array([0, 50, 100]))
    foreign = other.batch(_host(csr))
    ctx.evaluate_batch(b, 0.0, 1.0, want_pred=True)  # the buffers grow here
    live = (lib.fm_device_bytes_live(), lib.fm_device_allocs_live())
    rec = ctx.evaluate_batch(b, 0.0, 1.0, want_pred=True)[0]
    assert (lib.fm_device_bytes_live(), lib.fm_device_allocs_live()) == live
    n_hist = len(ctx.eval_history())
    # zero rows: nothing to do, a zeroed record, nothing appended
    z = ctx.evaluate_batch(empty, 0.0, 1.0)
    assert not z.executed and (z.n_rows, z.n_unlearned, z.sum_err, z.sum_abs_err, z.sum_sq_err) == (0, 0, 0.0, 0.0, 0.0)
    z = ctx.evaluate(_host(R_.CSR(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0), np.zeros(0))), 0.0, 1.0)
    assert not z.executed and z.n_rows == 0
    # errors, not crashes
    with pytest.raises(N.FMError, match="by split"):
        ctx.evaluate_batch(ds, 0.0, 1.0)
    with pytest.raises(N.FMError, match="another context"):
        ctx.evaluate_batch(foreign, 0.0, 1.0)
    pred = np.zeros(100)
    assert lib.fm_evaluate_batch(ctx.handle, b.handle, 0.0, 1.0, N.ptr(pred, C.c_double), None) == -1
    assert b"pred needs out" in lib.fm_last_error()
    out = N.fm_eval_out()
    assert lib.fm_evaluate_batch(None, b.handle, 0.0, 1.0, None, C.byref(out)) == -1
    assert lib.fm_evaluate_batch(ctx.handle, None, 0.0, 1.0, None, C.byref(out)) == -1
    assert lib.fm_evaluate(ctx.handle, None, 0.0, 1.0, None, C.byref(out)) == -1
    n = C.c_int64()
    assert lib.fm_eval_history(None, None, 0, C.byref(n)) == -1
    assert len(ctx.eval_history()) == n_hist
    assert (lib.fm_device_bytes_live(), lib.fm_device_allocs_live()) == live
    assert ctx.evaluate_batch(ds_view := ctx.split_view(ds, 1), 0.0, 1.0).n_rows == 50  # a split's view is accepted
    assert ctx.evaluate_batch(b, 0.0, 1.0) == rec
    for x in (ds_view, ds, b, empty, foreign):
        x.close()
    ctx.close()
    other.close()
    assert (lib.fm_device_bytes_live(), lib.fm_device_allocs_live()) == (bytes0, allocs0)


# --------------------------------------------------------------------- 6. multi-GPU on one device
def _group(k, R, mode, wire):
    from fm_spark_amd.engine import FMContext

    return FMContext(F, k, w0=W0, parallel=mode, n_gpus=R, devices=[0] * R, transport="copy", wire=wire)


@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("mode,wire", [("replicated", "fp32"), ("sharded", "fp32"), ("sharded", "fp64")])
def test_multi_gpu_evaluation(gpu, mode, wire, R):
    from fm_spark_amd import _native as N

    k = 16
    present, w, V = _tables(k)
    model = _model(k, present, w, V)
    ctx = _group(k, R, mode, wire)
    ctx.load_tables(present, w[present], V[present])
    n_hist = 0
    for n in (257, R - 1):  # the second: fewer rows than ranks, so a rank's part is empty (R = 1: no rows)
        csr = _rows(n, k, present, seed=60 + n)
        for lo, hi in CLAMPS:
            ref_pred = R_.predict(model, csr, lo, hi, num_features=F)
            csr.label = _cancelling_labels(ref_pred)
            n_unl = int((~eval_ref.learned_rows(model, csr, F)).sum())
            rec, pred = ctx.evaluate(_host(csr), lo, hi, want_pred=True)
            if n == 0:
                assert not rec.executed and rec.n_rows == 0
                continue
            n_hist += 1
            eval_ref.check(rec, csr.label, pred, n_unlearned=n_unl)
            np.testing.assert_allclose(pred, ctx.predict(_host(csr), lo, hi), rtol=1e-5, atol=1e-7)
            assert ctx.evaluate(_host(csr), lo, hi) == rec  # without pred, again: equal bits
            n_hist += 1
            b = ctx.batch(_host(_in_range(csr)))
            rec_b, pred_b = ctx.evaluate_batch(b, lo, hi, want_pred=True)
            n_hist += 1
            eval_ref.check(rec_b, csr.label, pred_b, n_unlearned=n_unl)
            np.testing.assert_allclose(pred_b, ctx.predict_batch(b, lo, hi), rtol=1e-5, atol=1e-7)
            assert N.load().fm_evaluate_batch(ctx.handle, b.handle, lo, hi, None, None) == -1
            assert b"a multi-GPU context evaluates synchronously" in N.load().fm_last_error()
            b.close()
    hist = ctx.eval_history()
    assert len(hist) == n_hist and all(h.epoch == 0 for h in hist)
    ctx.close()
