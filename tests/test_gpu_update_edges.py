"""GPU: the segmented update (fm_update.hip: k_segment_update, k_segment_combine, k_split_*) at its group,
wave, block, combine and split edges, against the fp64 oracle.

Random batches leave to chance where a run of equal keys falls against the kernels' boundaries; these
batches prescribe it.  tests/runs.py builds a batch whose sorted view is a given list of runs,
tests/update_cases.py writes the layouts in the units the library reports through its geometry seam
(tests/update_probe.py: entries per lane group, wave and block, the combine's ranges, the split's chunk
-- no constant of the kernels is written here), and runs.classify says which branches a layout
reaches; every test asserts that first (uc.assert_case and the builder's own check), as
tests/test_runs_cpu.py does for the same cases without a GPU.

Every case is two steps with reg_param > 0 on a table where every other designated row is absent: the
first batch touches none of the second batch's rows, so they arrive with an L1 catch-up pending and the
absent ones turn present.  The whole table is compared with oracle.fm_ref.sgd_step_fast at the project's
tolerance (RTOL 1e-5, ATOL 1e-8), the counts exactly, the loss to RTOL, and a second run must repeat the
first bit for bit.  The designated boundary entries (the first and last of a piece, a wave, a chunk, of
N) take |x| = 6 in rows labelled +-10, and the case asserts on the oracle alone that any one of them
moves its row by at least eight times what the comparison tolerates: a dropped or doubled boundary
entry fails.

Modes: unprepared and prepared unfused (bit for bit), fused (k <= 16: the layout is the compacted view,
singleton features sprinkled into the full one), the replicated mode's emit at world 1 (the gradient
buffer itself against the NumPy replicated phase, then the applied table) and a sharded context at
world 1 with the fp64 wire (both SegSource shapes).  The split's own layouts, and one test at the
smallest batch whose chunk counts take k_split_scan into a second round.
"""

import time

import numpy as np
import pytest

import runs
import update_cases as uc
from oracle import fm_ref as R
from test_gpu_fuse import _assert_same
from test_gpu_parity import ATOL, RTOL, assert_tables, to_host

pytestmark = pytest.mark.gpu

CASES = [(n, k) for n in uc.LAYOUTS for k in uc.ks_of(n)]


def _case(name, k, fused=False):
    import update_probe

    c = uc.case(name, k, update_probe.geometry(k), fused)
    uc.assert_case(c)
    return c


def _single(c, *, fuse, prepare):
    """The case's two steps on a single-table context: ([(loss, n_unique, n_loss_rows)], tables), n_rows."""
    from fm_spark_amd.engine import FMContext

    ctx = FMContext(c.F, c.k, fuse=fuse)
    assert ctx.fuse_active == (fuse and c.k <= uc.K_FUSED_MAX)
    ctx.load_tables(c.keep, c.w[c.keep], c.V[c.keep])
    dbs = [ctx.batch(to_host(b)) for b in c.batches]
    losses, n_rows = [], []
    for t, (b, step) in enumerate(zip(dbs, c.steps), start=1):
        if prepare:
            b.prepare()
        o = ctx.step_batch(b, t, step, c.reg)
        losses.append((o.loss_sum, o.n_unique, o.n_loss_rows))
        n_rows.append(o.n_rows)
    out = ctx.export_tables()
    for b in dbs:
        b.close()
    ctx.close()
    return (losses, out), n_rows


def _sharded(c):
    from fm_spark_amd.engine import FMContext

    ctx = FMContext(c.F, c.k, parallel="sharded", n_gpus=1, devices=[0], transport="copy", wire="fp64")
    ctx.load_tables(c.keep, c.w[c.keep], c.V[c.keep])
    losses, n_rows = [], []
    for t, (b, step) in enumerate(zip(c.batches, c.steps), start=1):
        o = ctx.step(to_host(b), t, step, c.reg)
        losses.append((o.loss_sum, o.n_unique, o.n_loss_rows))
        n_rows.append(o.n_rows)
    out = ctx.export_tables()
    ctx.close()
    return (losses, out), n_rows


def _assert_oracle(c, res, n_rows):
    losses, tables = res
    for (loss, nu, nl), m, ro in zip(losses, n_rows, c.outs):
        assert (nu, nl, m) == (ro.n_unique, ro.n_loss_rows, ro.n_rows)
        assert loss == pytest.approx(ro.loss_sum, rel=RTOL)
    assert_tables(c.model, tables)


def _assert_bitwise(a, b):
    (la, ta), (lb, tb) = a, b
    assert la == lb
    for x, y in zip(ta, tb):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("name,k", CASES)
def test_unfused_inline_and_prepared(gpu, name, k):
    c = _case(name, k)
    inline, n_rows = _single(c, fuse=False, prepare=False)
    _assert_oracle(c, inline, n_rows)
    prepared, _ = _single(c, fuse=False, prepare=True)
    _assert_bitwise(inline, prepared)  # the side-stream sort changes scheduling only
    _assert_bitwise(inline, _single(c, fuse=False, prepare=False)[0])  # and a second run repeats the first


@pytest.mark.parametrize("name,k", [(n, k) for n, k in CASES if uc.fusable(n, k)])
def test_fused(gpu, name, k):
    """The layout is what the segmented update consumes after the split dropped the sprinkled singletons."""
    c = _case(name, k, fused=True)
    fused, n_rows = _single(c, fuse=True, prepare=True)
    _assert_oracle(c, fused, n_rows)
    _assert_same(fused, _single(c, fuse=False, prepare=True)[0])
    _assert_bitwise(fused, _single(c, fuse=True, prepare=True)[0])


def _fp32_input_slack(model, csr, F, kp):
    """What a gradient sum [F][kp + 4] may differ by because the device forms every term from fp32 inputs
    (the sample's S row -- itself a sum of v x over the row's entries, kept in fp32 --, its r and yhat, the
    row's current V: relative error 2^-24 each) before it sums in fp64.  Where a sum cancels -- the row's
    v x in S, S x against v x^2, r where yhat meets the label -- the result is off by that share of its
    TERMS, which RTOL |sum| does not cover.  With |S| = sum_j |v_j x_j| over the sample's entries:
      g_V,e = (S x - v x^2) r :  (|S| |x| + |v| x^2) |r| for S and v,  |S x - v x^2| Y for r;
      g_w,e = x yhat - y      :  (|x - 1| + 1) Y  (formed as (x - 1) yhat + r from the sample's fp32 yhat and r),
    Y = |y| + sum |w x| + (sum_f |S|_f^2 + sum v^2 x^2) / 2, the magnitudes yhat and r are formed from; four
    roundings per term."""
    k, m = model.k, csr.n_rows
    rows = np.repeat(np.arange(m), np.diff(csr.row_ptr))
    i, x = csr.col.astype(np.int64), csr.val
    pred, _, _, dv = runs._loss_grad_fast(model, csr)
    vx = model.V[i] * x[:, None]
    absS = np.zeros((m, k))
    np.add.at(absS, rows, np.abs(vx))
    vv, wx = np.zeros(m), np.zeros(m)
    np.add.at(vv, rows, np.sum(vx * vx, axis=1))
    np.add.at(wx, rows, np.abs(model.w[i] * x))
    Y = (np.abs(csr.label) + wx + 0.5 * (np.sum(absS * absS, axis=1) + vv))[rows]
    r = np.abs(pred - csr.label[rows])
    mag = np.zeros((F, kp + 4))
    np.add.at(mag[:, :k], i, (absS[rows] * np.abs(x)[:, None] + np.abs(vx * x[:, None])) * r[:, None] + np.abs(dv) * Y[:, None])
    np.add.at(mag[:, kp], i, (np.abs(x - 1) + 1) * Y)
    return 4 * 2.0 ** -24 * mag


def _emit(c):
    """The two steps through fm_repl_grad / fm_repl_apply at world 1; before each apply the gradient
    buffer against the NumPy replicated phase (tests/shard_ref_engine.py)."""
    from fm_spark_amd.distributed import HipReplEngine
    from shard_ref_engine import NumpyReplEngine

    eng, ref = HipReplEngine(c.F, c.k), NumpyReplEngine(c.F, c.k)
    for e in (eng, ref):
        e.load_tables(c.keep, c.w[c.keep], c.V[c.keep])
    kp, k = eng.kp, c.k
    grads, stats = [], []
    for t, (csr, step) in enumerate(zip(c.batches, c.steps), start=1):
        b = eng.batch(to_host(csr))
        got = eng.grad_phase(b).cpu().numpy().reshape(c.F, kp + 4).copy()
        want = ref.grad_phase(ref.batch(csr)).numpy().reshape(c.F, kp + 4)
        bound = RTOL * np.abs(want) + ATOL + _fp32_input_slack(R.Model(k=k, w=ref.w, V=ref.V, present=ref.present),
                                                                 csr, c.F, kp)
        touched = np.zeros(c.F, dtype=bool)
        touched[csr.col] = True
        np.testing.assert_array_equal(got[:, kp + 1], touched.astype(np.float32))  # the flags, exactly
        assert not got[~touched].any()  # untouched rows are all zero
        assert not got[:, k:kp].any() and not got[:, kp + 2:].any()
        err = np.abs(got.astype(np.float64) - want)
        assert (err[:, :k] <= bound[:, :k]).all() and (err[:, kp] <= bound[:, kp]).all(), float(err.max())
        for e in (eng, ref):
            e.apply(e.grad, t, step, c.reg, csr.n_rows)
        loss, nl, nu = eng.last_stats()
        stats.append((loss, nu, nl))
        grads.append(got)
        b.close()
    out = eng.export_tables()
    eng.ctx.close()
    return (stats, out), grads


@pytest.mark.parametrize("name,k", CASES)
def test_replicated_emit(gpu, name, k):
    c = _case(name, k)
    res, grads = _emit(c)
    _assert_oracle(c, res, [b.n_rows for b in c.batches])
    again, grads2 = _emit(c)
    _assert_bitwise(res, again)
    for a, b in zip(grads, grads2):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name,k", [(n, k) for n, k in CASES if k in uc.K_SHARDED])
def test_sharded_world1(gpu, name, k):
    """The owner's SegSource: packed records for kp <= 16, S rows of kp floats and a separate {r, yhat}
    above."""
    c = _case(name, k)
    res, n_rows = _sharded(c)
    _assert_oracle(c, res, n_rows)
    _assert_bitwise(res, _sharded(c)[0])


@pytest.mark.parametrize("k", uc.K_SPLIT)
@pytest.mark.parametrize("name", list(uc.SPLIT))
def test_split(gpu, name, k):
    """Layouts over the full view, against the split's chunks (the events are asserted in the builder)."""
    c = _case(name, k)
    fused, n_rows = _single(c, fuse=True, prepare=True)
    _assert_oracle(c, fused, n_rows)
    _assert_same(fused, _single(c, fuse=False, prepare=True)[0])
    _assert_bitwise(fused, _single(c, fuse=True, prepare=True)[0])


def test_split_scan_second_round(gpu):
    """One chunk more than k_split_scan takes in a round: the smallest batch at which its carry across
    rounds exists.  k = 1, one fused step against the oracle (tables, n_unique, loss).  The only test of
    this file above a few seconds: the batch has 12.6 M entries at today's geometry."""
    import update_probe
    from fm_spark_amd.engine import FMContext

    g = update_probe.geometry(1)
    N = g.round_chunks * g.chunk + 1
    cyc = np.asarray([1, 3, 2, 1, 5, 2, 1, 1, 40, 2])
    reps = N // cyc.sum() + 1
    lengths = np.tile(cyc, reps)
    lengths = lengths[: int(np.searchsorted(np.cumsum(lengths), N)) + 1]
    lengths[-1] -= lengths.sum() - N
    assert lengths.sum() == N and lengths.min() >= 1
    F, k, n_rows = len(lengths), 1, 262144
    t0 = time.perf_counter()
    csr, ids, w, V = runs.make_runs(77, lengths, F, k, n_rows=n_rows)
    sp = runs.classify_split(np.repeat(np.arange(F), lengths), g)
    assert sp.nchunks == g.round_chunks + 1 and sp.rounds == 2 and sp.n_multi > 0 and sp.n_single > 0
    model = R.Model.empty(F, k)
    model.load(ids, w, V)
    ro = R.sgd_step_fast(model, csr, 1, 1.5, uc.REG)
    t1 = time.perf_counter()
    ctx = FMContext(F, k, fuse=True)
    assert ctx.fuse_active
    ctx.load_tables(ids, w, V)
    b = ctx.batch(to_host(csr))
    b.prepare()
    o = ctx.step_batch(b, 1, 1.5, uc.REG)
    tables = ctx.export_tables()
    b.close()
    ctx.close()
    print(f"scan second round: N = {N}, build + oracle {t1 - t0:.1f} s, device {time.perf_counter() - t1:.1f} s")
    assert (o.n_unique, o.n_loss_rows, o.n_rows) == (ro.n_unique, ro.n_loss_rows, ro.n_rows)
    assert o.loss_sum == pytest.approx(ro.loss_sum, rel=RTOL)
    assert_tables(model, tables)
