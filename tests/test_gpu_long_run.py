"""GPU: the lazy-L1 row state and the device loss history over a long horizon.

A row header carries {w, t, cum}; a row is brought current by S_{cum[E] - cum} only when something
reads it.  The 48-step problem below keeps rows in every state a long fit produces: id 0 updated at
every step (a multi-entry run), ids 1-255 active, ids 256-319 dormant (in the batches of steps 1 and
40 only), ids 320-447 never in any batch (they see only L1: about a quarter of them cross to exactly
zero), ids 448-511 absent from the loaded model, some of them created by step 30.  The device is
compared with the fp64 oracle (oracle/fm_ref.py) through fm_export_rows with the L1 pending
(k_gather_rows' shrink branch) after steps 1, 2, 10, 29, 30, 39, 40 and 48, and through
fm_export_tables at the end; with a whole-table export (k_flush) in mid-run; with rows loaded and
initialised at epoch > 0; and with transform / calcLossGrad called on the model while it trains.

Budget per element (derived, not measured):
    |dev - ref| <= RTOL |ref| + ATOL + n_upd 2^-22 peak
RTOL / ATOL: the project's 1e-5 / 1e-8 (on the three-rank paths ATOL = max(ATOL, 4 fp32 ulps of the
table's largest value), as tests/test_gpu_fuzz.py); n_upd: the steps so far whose batch held the
row's id (plus one per flush); peak: the largest |w| or |V| the oracle's row has held.  Each update
stores the row rounded to fp32 and the fp32 catch-up adds at most two more fp32 roundings at that
magnitude; a never-touched row has n_upd = 0 and a dormant row at most 2, so where the lazy catch-up
is the thing under test the bound is the project's plain tolerance.

Largest deviation / budget measured on an MI355X (the tests print them), over all rows and, in
parentheses, over the rows with n_upd <= 2 (dormant, never touched, just created):
    48 steps, k = 16: host, fused, unfused 0.044 (0.037); sharded3 0.042 (0.024); replicated3 0.029 (0.028)
    48 steps, k = 4:  fused, unfused 0.044 (0.044);  k = 20: host, prepared 0.191 (0.191)
    flush after step 20, k = 16: fused, unfused 0.043 (0.037); sharded3 0.041 (0.024); replicated3 0.031 (0.028)
    16 steps with table edits, k = 16: fused 0.029, sharded3 0.020, replicated3 0.023
The loss-history test runs 4200 steps on the single table (0.4 s) and 4100 on sharded3, which still
crosses the first capacity of 4096: 5.1 s there against 5.3 s at 4200 (two contexts of three ranks;
every synchronous step reads three ranks' statistics).
"""

import functools

import numpy as np
import pytest

from oracle import fm_ref as R
from problems import f32
from test_gpu_parity import ATOL, RTOL, to_host

gpu_test = pytest.mark.gpu  # per test: the oracle-only guard below runs without a GPU too

F, T, STEP, REG = 512, 48, 0.5, 5e-3
CHECKPOINTS = (1, 2, 10, 29, 30, 39, 40, 48)
ACTIVE, DORMANT, NEVER, ABSENT = (1, 256), (256, 320), (320, 448), (448, 512)
SEED, INIT_SD = 77, 0.05


def make_ctx(path, k, **kw):
    from fm_spark_amd.engine import FMContext

    if path in ("sharded3", "replicated3"):
        return FMContext(F, k, parallel=path[:-1], n_gpus=3, devices=[0] * 3, transport="copy", **kw)
    return FMContext(F, k, fuse={"fused": True, "unfused": False}.get(path), **kw)


@functools.lru_cache(maxsize=None)
def problem(k):
    """(batches[T], ids, w, V): every step 8 rows and one empty row, binary labels, f32(N(0,1)) values."""
    rng = np.random.default_rng(20240 + k)
    batches = []
    for t in range(1, T + 1):
        row_ptr, cols, vals = [0], [], []
        for r in range(9):
            if r == 4:  # the empty row: counted in miniBatchSize, not in the loss
                row_ptr.append(len(cols))
                continue
            ids = [0] + list(rng.choice(np.arange(*ACTIVE), 4, replace=False))
            if t in (1, 40):
                ids += list(rng.choice(np.arange(*DORMANT), 4, replace=False))
            if t == 30:
                ids += list(rng.choice(np.arange(*ABSENT), 2, replace=False))
            ids = np.sort(np.asarray(ids))
            cols.extend(ids.tolist())
            vals.extend(f32(rng.normal(0.0, 1.0, len(ids))).tolist())
            row_ptr.append(len(cols))
        y = (rng.random(9) < 0.25).astype(np.float64)
        batches.append(R.CSR(np.asarray(row_ptr, np.int64), np.asarray(cols, np.int32), np.asarray(vals), y))
    ids = np.arange(ABSENT[0], dtype=np.int32)
    return batches, ids, f32(rng.normal(0.0, 0.1, len(ids))), f32(rng.normal(0.0, 0.1, (len(ids), k)))


class Track:
    """The oracle model with, per row, the number of updates and the largest magnitude it has held."""

    def __init__(self, k, ids, w, V):
        self.model = R.Model.empty(F, k)
        self.model.load(ids, w, V)
        self.n_upd = np.zeros(F)
        self.peak = np.zeros(F)
        self._see(np.arange(F))

    def _see(self, rows):
        m = self.model
        self.peak[rows] = np.maximum(self.peak[rows], np.maximum(np.abs(m.w[rows]), np.max(np.abs(m.V[rows]), axis=1)))

    def step(self, csr, t):
        out = R.sgd_step_fast(self.model, csr, t, STEP, REG)
        if out.executed:
            self.n_upd[np.unique(csr.col)] += 1
            self._see(np.arange(F))
        return out

    def write(self, ids, w, V):
        """Rows written exactly (fm_load_tables / the seeded draw): their rounding history starts over."""
        self.model.load(ids, w, V)
        self.n_upd[ids] = 0
        self.peak[ids] = 0.0
        self._see(np.asarray(ids))

    def snap(self):
        return Snap(self.model.copy(), self.n_upd.copy(), self.peak.copy())


class Snap:
    def __init__(self, model, n_upd, peak):
        self.model, self.n_upd, self.peak = model, n_upd, peak

    def atol3(self):
        m = self.model
        p = np.nonzero(m.present)[0]
        return max(ATOL, 4 * 2.0 ** -24 * max(float(np.max(np.abs(m.V[p]), initial=0.0)),
                                             float(np.max(np.abs(m.w[p]), initial=0.0))))

    def ratio(self, w, V, three_rank, extra_upd=0, rows=None):
        """max over the elements of |dev - ref| / budget, and the row where it is."""
        rows = np.arange(F) if rows is None else np.asarray(rows)
        m = self.model
        atol = self.atol3() if three_rank else ATOL
        slack = ((self.n_upd[rows] + extra_upd * m.present[rows]) * 2.0 ** -22 * self.peak[rows])
        rw = np.abs(w - m.w[rows]) / (RTOL * np.abs(m.w[rows]) + atol + slack)
        rV = np.abs(V - m.V[rows]) / (RTOL * np.abs(m.V[rows]) + atol + slack[:, None])
        per_row = np.maximum(rw, rV.max(axis=1))
        worst = int(np.argmax(per_row))
        return float(per_row[worst]), int(rows[worst])


@functools.lru_cache(maxsize=None)
def oracle_run(k):
    """The 48 oracle steps: per-step results and the snapshots after every step (shared, never changed)."""
    batches, ids, w, V = problem(k)
    tr = Track(k, ids, w, V)
    outs, snaps = [], {0: tr.snap()}
    for t, c in enumerate(batches, start=1):
        outs.append(tr.step(c, t))
        snaps[t] = tr.snap()
    return outs, snaps


def test_oracle_problem_is_not_hollow():
    """The never-touched block ends with both exact zeros and non-zeros (at least 10 % each), the run is
    stable, and the dormant rows were updated exactly twice."""
    for k in (4, 16, 20):
        _, snaps = oracle_run(k)
        m = snaps[T].model
        blk = np.concatenate([m.w[NEVER[0]:NEVER[1], None], m.V[NEVER[0]:NEVER[1]]], axis=1)
        zeros = float(np.mean(blk == 0.0))
        assert 0.10 <= zeros <= 0.90, (k, zeros)
        assert np.all(np.isfinite(m.V)) and max(np.max(np.abs(m.V)), np.max(np.abs(m.w))) < 2.0
        assert np.all(snaps[T].n_upd[NEVER[0]:NEVER[1]] == 0)
        assert np.all(snaps[T].n_upd[DORMANT[0]:DORMANT[1]] <= 2) and snaps[T].n_upd[0] == T
        assert m.present[:ABSENT[0]].all() and 0 < m.present[ABSENT[0]:].sum() < ABSENT[1] - ABSENT[0]


class Runner:
    """One device context stepping the problem's batches on one path."""

    def __init__(self, path, k, batches, **kw):
        self.path, self.k = path, k
        self.ctx = make_ctx(path, k, **kw)
        self.three = path in ("sharded3", "replicated3")
        self.hbs = [to_host(c) for c in batches]
        self.dbs = [] if path == "host" else [self.ctx.batch(h) for h in self.hbs]

    def step(self, t):
        if self.path == "host":
            return self.ctx.step(self.hbs[t - 1], t, STEP, REG)
        self.dbs[t - 1].prepare()
        return self.ctx.step_batch(self.dbs[t - 1], t, STEP, REG)

    def rows(self, ids=None):
        return self.ctx.export_rows(np.arange(F, dtype=np.int32) if ids is None else ids)

    def close(self):
        for b in self.dbs:
            b.close()
        self.ctx.close()


def dev_model(k, w, V, present):
    m = R.Model.empty(F, k)
    p = np.nonzero(present)[0]
    m.load(p, w[p], V[p])
    return m


def check_counts(o, r, what):
    assert o.executed == r.executed, what
    assert (o.n_rows, o.n_loss_rows, o.n_unique) == (r.n_rows, r.n_loss_rows, r.n_unique), what


def check_table_export(run, snap, extra_upd, what):
    gids, gw, gV = run.ctx.export_tables()
    pids = np.nonzero(snap.model.present)[0]
    np.testing.assert_array_equal(gids, pids, err_msg=str(what))
    ratio, row = snap.ratio(gw, gV, run.three, extra_upd, rows=pids)
    assert ratio <= 1.0, (what, "export_tables", ratio, row, snap.n_upd[row])
    return ratio


def long_run(path, k, flush_after=None):
    batches, ids, w, V = problem(k)
    ref_outs, snaps = oracle_run(k)
    run = Runner(path, k, batches)
    run.ctx.load_tables(ids, w, V)
    worst, worst_lazy, extra, pending_loss = 0.0, 0.0, 0, None
    for t in range(1, T + 1):
        o = run.step(t)
        check_counts(o, ref_outs[t - 1], (path, k, t))
        if pending_loss is not None:
            # the step's loss against the oracle's forward on the table read from the device just before it
            assert o.loss_sum == pytest.approx(pending_loss, rel=1e-5), (path, k, t)
            pending_loss = None
        if t in CHECKPOINTS:
            gw, gV, gp = run.rows()  # no flush: the gather applies the pending shrink
            np.testing.assert_array_equal(gp, snaps[t].model.present, err_msg=f"{path} k={k} step {t}")
            ratio, row = snaps[t].ratio(gw, gV, run.three, extra)
            assert ratio <= 1.0, (path, k, t, "export_rows", ratio, row, snaps[t].n_upd[row])
            worst = max(worst, ratio)
            lazy = np.nonzero(snaps[t].n_upd <= 2)[0]  # dormant, never-touched and just-created rows
            worst_lazy = max(worst_lazy, snaps[t].ratio(gw[lazy], gV[lazy], run.three, extra, rows=lazy)[0])
            if t < T:
                pending_loss = R.forward(dev_model(k, gw, gV, gp), batches[t]).loss_sum
        if t == flush_after:
            extra = 1  # the flush rewrites every present row rounded to fp32 once more
            worst = max(worst, check_table_export(run, snaps[t], extra, (path, k, t, "flush")))
    worst = max(worst, check_table_export(run, snaps[T], extra, (path, k, T)))
    assert run.ctx.epoch == T
    run.close()
    print(f"long-run deviation/budget {path} k={k} flush={flush_after}: {worst:.3f} (rows with n_upd <= 2: {worst_lazy:.3f})")
    return worst


LONG_PATHS = [("host", 16), ("fused", 16), ("unfused", 16), ("sharded3", 16), ("replicated3", 16), ("fused", 4),
              ("unfused", 4), ("host", 20), ("prepared", 20)]


@gpu_test
@pytest.mark.parametrize("path,k", LONG_PATHS)
def test_long_run_rows_against_oracle(gpu, path, k):
    """48 steps; counts exact at every step; at the checkpoints fm_export_rows of all 512 ids with the
    L1 pending (present flags exact, values within the budget) and the next step's loss against the
    oracle's forward on the table just read; fm_export_tables at the end."""
    long_run(path, k)


@gpu_test
@pytest.mark.parametrize("path", ["fused", "unfused", "sharded3", "replicated3"])
def test_long_run_with_flush_in_mid_run(gpu, path):
    """The same run with fm_export_tables (k_flush rewrites every header) after step 20: the exported
    table is within the budget there, steps 21-48 continue from the flushed headers, and the
    checkpoints and the final table stay within the budget (one more update per present row)."""
    long_run(path, 16, flush_after=20)


# ------------------------------------------------------------ table edits and inference at epoch > 0
EDIT_STEPS = 16
LOAD_IDS = np.array([17, 260, 330, 400, 450, 460, 470, 480], dtype=np.int32)   # active, dormant, 2 never; 4 absent
DRAW_IDS = np.array([18, 261, 331, 450, 451, 461, 471, 481], dtype=np.int32)   # 4 present (450 since the load); 4 absent
BATCH_PRESENT = np.array([19, 20, 262, 263, 332, 333, 451, 460])
BATCH_ABSENT = np.arange(490, 498)


@functools.lru_cache(maxsize=None)
def edit_inputs(k=16):
    rng = np.random.default_rng(99)
    lw, lV = f32(rng.normal(0.0, 0.1, 8)), f32(rng.normal(0.0, 0.1, (8, k)))
    ids = rng.permutation(np.concatenate([BATCH_PRESENT, BATCH_ABSENT]))
    init_csr = R.CSR(np.arange(0, 17, 4, dtype=np.int64), np.concatenate([np.sort(ids[i:i + 4]) for i in range(0, 16, 4)]).astype(np.int32),
                     f32(rng.normal(0.0, 1.0, 16)), np.zeros(4))
    # the probe of the model in training: 40 rows over present ids, each with a dormant and a never-touched id
    row_ptr, cols = [0], []
    for _ in range(40):
        r = np.concatenate([rng.choice(np.arange(*ACTIVE), 3, replace=False), rng.choice(np.arange(*DORMANT), 1),
                            rng.choice(np.arange(*NEVER), 1), rng.choice(LOAD_IDS[4:], 1)])
        cols.extend(np.sort(r).tolist())
        row_ptr.append(len(cols))
    probe = R.CSR(np.asarray(row_ptr, np.int64), np.asarray(cols, np.int32), f32(rng.normal(0.0, 1.0, len(cols))),
                  (rng.random(40) < 0.25).astype(np.float64))
    return lw, lV, init_csr, probe


@functools.lru_cache(maxsize=None)
def oracle_edit_run(k=16):
    batches, ids, w, V = problem(k)
    lw, lV, init_csr, _ = edit_inputs(k)
    tr = Track(k, ids, w, V)
    outs, after = [], {}
    for t in range(1, EDIT_STEPS + 1):
        outs.append(tr.step(batches[t - 1], t))
        if t == 5:
            tr.write(LOAD_IDS, lw, lV)
            after[t] = tr.snap()
        if t == 8:
            tr.write(DRAW_IDS, *R.init_draw(DRAW_IDS, k, SEED, INIT_SD))
            after[t] = tr.snap()
        if t == 11:
            assert not tr.model.present[BATCH_ABSENT].any() and tr.model.present[BATCH_PRESENT].all()
            tr.write(BATCH_ABSENT, *R.init_draw(BATCH_ABSENT, k, SEED, INIT_SD))
            after[t] = tr.snap()
    return outs, after, tr.snap()


def check_written(run, ids, snap, what):
    """Rows just written: nothing pending on them, so they read back as written (rtol 1e-6)."""
    gw, gV, gp = run.rows(np.asarray(ids, dtype=np.int32))
    assert gp.all(), what
    np.testing.assert_allclose(gw, snap.model.w[ids], rtol=1e-6, atol=0.0, err_msg=str(what))
    np.testing.assert_allclose(gV, snap.model.V[ids], rtol=1e-6, atol=0.0, err_msg=str(what))
    assert run.ctx.num_present() == int(snap.model.present.sum()), what


def check_inference(run, probe, k):
    """transform and calcLossGrad on the model in training (L1 pending on the dormant and never-touched
    rows) against the oracle on the device's own rows at that moment; the table is not written."""
    from test_gpu_fuzz import score_terms

    before = run.rows()
    model = dev_model(k, *before)
    assert model.present[probe.col].all()
    hp = to_host(probe)
    db = run.ctx.batch(hp)
    ref = R.predict(model, probe, -2.0, 3.0, num_features=F)
    for pred in (run.ctx.predict(hp, -2.0, 3.0), run.ctx.predict_batch(db, -2.0, 3.0)):
        if run.three:
            bound = RTOL * np.abs(ref) + np.maximum(1e-7, 8 * 2.0 ** -24 * score_terms(model, probe))
            assert np.all(np.abs(pred - ref) <= bound), (run.path, float(np.max(np.abs(pred - ref) - bound)))
        else:
            np.testing.assert_allclose(pred, ref, rtol=RTOL, atol=1e-7, err_msg=run.path)
    db.close()
    if run.path != "sharded3":  # the per-entry outputs need the whole table on one device
        gp, gl, gdw, gdv = run.ctx.loss_grad(hp)
        rp, rl, rdw, rdv = R.loss_grad(model, probe)
        np.testing.assert_allclose(gp, rp, rtol=1e-6, atol=1e-9, err_msg=run.path)
        np.testing.assert_allclose(gl, rl, rtol=1e-5, atol=1e-9, err_msg=run.path)
        np.testing.assert_array_equal(gdw, rdw)
        np.testing.assert_allclose(gdv, rdv, rtol=1e-5, atol=1e-9, err_msg=run.path)
    after = run.rows()
    for a, b in zip(before, after):
        assert np.array_equal(a, b), (run.path, "inference wrote the table")


@gpu_test
@pytest.mark.parametrize("path", ["fused", "sharded3", "replicated3"])
def test_table_edits_and_inference_at_epoch_gt_0(gpu, path):
    """16 steps at k = 16 with the table edited in mid-run, on the device and the oracle alike:
    fm_load_tables after step 5, fm_init_random after step 8 and fm_init_from_batch after step 11,
    each over present and absent ids (k_load_rows, k_init_random and k_init_entries with epoch > 0 and
    cum[E] > 0).  The written rows read back as written with nothing pending; rows that
    fm_init_from_batch keeps are kept bit for bit; num_present is exact; after step 12 transform and
    calcLossGrad answer from the rows as fm_export_rows shows them and leave them unchanged; the run
    ends within the budget, so each written row's first later shrink started from its epoch's cum."""
    k = 16
    batches, ids, w, V = problem(k)
    lw, lV, init_csr, probe = edit_inputs(k)
    ref_outs, after, final = oracle_edit_run(k)
    run = Runner(path, k, batches[:EDIT_STEPS], seed=SEED, init_sd=INIT_SD)
    run.ctx.load_tables(ids, w, V)
    for t in range(1, EDIT_STEPS + 1):
        o = run.step(t)
        check_counts(o, ref_outs[t - 1], (path, t))
        if t == 5:
            run.ctx.load_tables(LOAD_IDS, lw, lV)
            check_written(run, LOAD_IDS, after[t], (path, "load_tables"))
        if t == 8:
            run.ctx.init_random(DRAW_IDS)
            check_written(run, DRAW_IDS, after[t], (path, "init_random"))
        if t == 11:
            kept = run.rows(BATCH_PRESENT.astype(np.int32))
            ib = run.ctx.batch(to_host(init_csr))
            n = run.ctx.init_from_batch(ib)
            ib.close()
            assert n == int(after[t].model.present.sum()), path
            for a, b in zip(kept, run.rows(BATCH_PRESENT.astype(np.int32))):
                assert np.array_equal(a, b), (path, "init_from_batch changed a present row")
            check_written(run, BATCH_ABSENT, after[t], (path, "init_from_batch"))
        if t == 12:
            check_inference(run, probe, k)
    ratio = check_table_export(run, final, 0, (path, "end"))
    run.close()
    print(f"edit-run deviation/budget {path}: {ratio:.3f}")


# ---------------------------------------------------------- the loss history past its first capacity
HIST_STEPS = {"single": 4200, "sharded3": 4100}


@gpu_test
@pytest.mark.parametrize("path", ["single", "sharded3"])
def test_loss_history_past_first_capacity(gpu, path):
    """The device loss history starts at 4096 steps and is reallocated and copied at step 4097 while
    asynchronous steps are still queued.  4200 steps (4100 on sharded3) enqueued without host
    synchronisation: the history has as many entries, bitwise the per-step return values of the same
    steps run synchronously
    on an identical context (bitwise determinism is an existing invariant); the first 6 match the
    oracle; the reallocation frees what it replaces (live allocations as after step 3)."""
    from test_gpu_lifetime import counters

    Fh, k, step, reg = 8, 2, 0.1, 1e-6
    steps = HIST_STEPS[path]
    rng = np.random.default_rng(4)
    csrs = [R.CSR(np.array([0, 3, 5], np.int64), np.array(c, np.int32), f32(rng.normal(0.0, 1.0, 5)),
                  np.array(y, np.float64)) for c, y in (([0, 2, 5, 1, 2], [1.0, 0.0]), ([1, 3, 7, 2, 6], [0.0, 1.0]))]
    ids = np.arange(Fh, dtype=np.int32)
    w, V = f32(rng.normal(0.0, 0.1, Fh)), f32(rng.normal(0.0, 0.1, (Fh, k)))

    def ctx_of():
        from fm_spark_amd.engine import FMContext

        kw = dict(parallel="sharded", n_gpus=3, devices=[0] * 3, transport="copy") if path == "sharded3" else {}
        c = FMContext(Fh, k, **kw)
        c.load_tables(ids, w, V)
        return c, [c.batch(to_host(x)) for x in csrs]

    a, ab = ctx_of()
    allocs3 = None
    for t in range(1, steps + 1):
        ab[t % 2].prepare()
        a.step_batch(ab[t % 2], t, step, reg, sync=False)
        if t == 3:
            a.sync()
            allocs3 = counters()[1]
    hist = a.loss_history()
    assert a.epoch == steps and len(hist) == steps
    assert counters()[1] == allocs3
    for x in ab:
        x.close()
    a.close()

    b, bb = ctx_of()
    sync_loss = np.zeros(steps)
    for t in range(1, steps + 1):
        bb[t % 2].prepare()
        sync_loss[t - 1] = b.step_batch(bb[t % 2], t, step, reg).loss_sum
    hist_b = b.loss_history()
    for x in bb:
        x.close()
    b.close()
    assert np.all(np.isfinite(sync_loss)) and np.all(sync_loss > 0.0)
    assert np.array_equal(hist, sync_loss), int(np.argmax(hist != sync_loss))
    assert np.array_equal(hist_b, sync_loss)

    model = R.Model.empty(Fh, k)
    model.load(ids, w, V)
    for t in range(1, 7):
        ref = R.sgd_step_fast(model, csrs[t % 2], t, step, reg)
        assert hist[t - 1] == pytest.approx(ref.loss_sum, rel=1e-5), t
