"""GPU: the objective stage of the single-table step (fm_config.loss; fm_objective.hip, k_objective) through
the C-ABI, against the fp64 reference of tests/objective_ref.py with the device's contract
(round_scores=True: the objective reads the score as the forward stored it, rounded to fp32).

Tolerances: the suite's own (tests/test_gpu_parity.py), RTOL 1e-5 / ATOL 1e-8.  Beyond the squared step's
errors the stage adds one fp32 rounding of r (2^-24 relative, as the squared r has) and a few fp64 ulps
of exp / log1p, so nothing is widened.

Shapes sit on the stage's own edges: 256 threads per block and at most 256 blocks (a larger batch
strides the grid: past 65 536 logistic rows); under BPR a team of 1 (g <= 5), 8 (g <= 65) or 64 lanes owns
a group, so the grid is strided past 65 536 / 8 192 / 1 024 groups.  k in {4, 16, 20}: {r, yhat} inside
the S record at both record sizes, and in its own array (kp > 16).  Rows have 0-12 entries.
"""

import ctypes as C
import gc

import numpy as np
import pytest

import objective_ref as O
import pair_ref as P
from fm_spark_amd import _native as N
from oracle import fm_ref as R
from problems import f32, make_rows
from rank_ref import make_rows as rank_rows

pytestmark = pytest.mark.gpu

RTOL = 1e-5  # tests/test_gpu_parity.py
ATOL = 1e-8
KS = [4, 16, 20]
F = 96
STEP = 0.4


def host(csr):
    return N.CSRHost(csr.row_ptr, csr.col, csr.val, csr.label)


def live():
    lib = N.load()
    return int(lib.fm_device_bytes_live()), int(lib.fm_device_allocs_live())


def problem(seed, B, k, max_len=12, F=F):
    lens = np.random.default_rng(1000 + seed).integers(0, max_len + 1, B)
    return make_rows(seed, lens, F, k)


def new_ctx(k, loss, ids, w, V, F=F, w0=0.0, **kw):
    from fm_spark_amd.engine import FMContext

    ctx = FMContext(F, k, loss=loss, w0=w0, **kw)
    ctx.load_tables(ids, w, V)
    return ctx


def ref_model(k, ids, w, V, F=F, w0=0.0):
    m = R.Model.empty(F, k, w0)
    m.load(ids, w, V)
    return m


def assert_tables(model, g):
    gids, gw, gV = g
    pids = np.nonzero(model.present)[0]
    np.testing.assert_array_equal(gids, pids)
    assert np.all(np.isfinite(gw)) and np.all(np.isfinite(gV))
    np.testing.assert_allclose(gw, model.w[pids], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(gV, model.V[pids], rtol=RTOL, atol=ATOL)


def run_both(loss, csr, k, ids, w, V, group=0, steps=1, reg=0.0, w0=0.0, prepare=False, F=F):
    """`steps` steps of one batch on the device and on the reference; every step's loss and counts are
    compared, then the tables.  Returns the device's table."""
    model = ref_model(k, ids, w, V, F, w0)
    ctx = new_ctx(k, loss, ids, w, V, F, w0)
    b = ctx.batch(host(csr))
    if group:
        assert b.set_group(group) is b and b.group == group
    for t in range(1, steps + 1):
        ro = O.step(model, csr, t, STEP, reg, loss, group, round_scores=True, fast=True)
        if prepare:
            b.prepare()
        go = ctx.step_batch(b, t, STEP, reg)
        print(f"{loss} B={csr.n_rows} g={group} k={k} t={t}: loss {go.loss_sum!r} ref {ro.loss_sum!r} rows {go.n_loss_rows}")
        assert np.isfinite(go.loss_sum)
        assert go.loss_sum == pytest.approx(ro.loss_sum, rel=RTOL, abs=ATOL)
        assert (go.n_rows, go.n_loss_rows, go.n_unique) == (ro.n_rows, ro.n_loss_rows, ro.n_unique)
    assert np.array_equal(ctx.loss_history()[-1:], [go.loss_sum])
    tab = ctx.export_tables()
    assert_tables(model, tab)
    b.close()
    ctx.close()
    return tab


# ------------------------------------------------------------------------------------- logistic
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 256, 257, 1025, 4097])
def test_logistic_edge_row_counts(gpu, B, k):
    csr, ids, w, V = problem(B, B, k)
    if B > 1:
        assert (np.diff(csr.row_ptr) == 0).any()  # rows without entries: not counted in n_loss_rows
    run_both("logistic", csr, k, ids, w, V)


@pytest.mark.parametrize("k", [4, 20])
def test_logistic_strides_the_grid(gpu, k):
    B = 70001  # past 256 blocks of 256 threads
    csr, ids, w, V = make_rows(7, np.full(B, 2), F, k)
    run_both("logistic", csr, k, ids, w, V)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("prepare", [False, True])
def test_logistic_three_steps_with_l1(gpu, k, prepare):
    csr, ids, w, V = problem(31, 257, k)
    run_both("logistic", csr, k, ids, w, V, steps=3, reg=2e-2, prepare=prepare)


def test_logistic_fractional_labels(gpu):
    csr, ids, w, V = problem(32, 300, 16)
    csr.label[:] = np.random.default_rng(5).random(300)
    run_both("logistic", csr, 16, ids, w, V)


# ------------------------------------------------------------------------------------------ BPR
GROUPS = [2, 3, 5, 64, 65, 257, 1025]


def crossing(g, edge):
    """The fewest whole groups of g rows beyond `edge` rows: past it by at most one group."""
    return (edge // g + 1) * g


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("g", GROUPS)
@pytest.mark.parametrize("which", ["one", "256"])
def test_bpr_through_set_group(gpu, g, which, k):
    B = g if which == "one" else crossing(g, 256)
    assert which == "one" or 256 < B <= 256 + g
    csr, ids, w, V = problem(g + len(which), B, k)
    run_both("bpr", csr, k, ids, w, V, group=g)


@pytest.mark.parametrize("i,g", list(enumerate(GROUPS)))
def test_bpr_crosses_65536_rows(gpu, i, g):
    B, k = crossing(g, 65536), KS[i % 3]
    assert 65536 < B <= 65536 + g
    csr, ids, w, V = problem(40 + i, B, k, max_len=4)
    run_both("bpr", csr, k, ids, w, V, group=g)


@pytest.mark.parametrize("g,groups,k", [(2, 65537, 4), (5, 65537, 20), (6, 8193, 16), (66, 1025, 20)])
def test_bpr_strides_the_grid(gpu, g, groups, k):
    """More groups than the grid's teams (256 blocks x 256 lanes / team): a team walks several groups."""
    csr, ids, w, V = problem(50 + g, g * groups, k, max_len=2)
    run_both("bpr", csr, k, ids, w, V, group=g)


@pytest.mark.parametrize("k", KS)
def test_bpr_empty_rows_score_w0(gpu, k):
    """Rows without entries in positive and in negative position take part with the score w0."""
    lens = np.random.default_rng(3).integers(1, 9, 12)
    lens[[0, 4, 8, 9, 11]] = 0  # g = 3: row 0 an empty positive, 4 / 8 empty negatives, group 3 all empty
    csr, ids, w, V = make_rows(61, lens, F, k)
    run_both("bpr", csr, k, ids, w, V, group=3, w0=0.75, steps=2, reg=1e-3)


@pytest.mark.parametrize("k", KS)
def test_bpr_negative_repeating_its_positive_cancels(gpu, k):
    """A group whose negative is its positive's row again: d = 0, r = -+ 1/2, and on the rows that only
    those two touch the two contributions cancel."""
    csr, ids, w, V = problem(62, 40, k, F=80)
    own = np.array([90, 91, 92], np.int32)  # ids no other row has (the problem's are below 80)
    xv = f32([0.5, 1.0, -1.25])
    rp = np.concatenate([csr.row_ptr, csr.row_ptr[-1] + [3, 6]])
    twice = R.CSR(rp, np.concatenate([csr.col, own, own]).astype(np.int32), np.concatenate([csr.val, xv, xv]),
                  np.concatenate([csr.label, [1.0, 0.0]]))
    rng = np.random.default_rng(9)
    ids2 = np.arange(F, dtype=np.int32)
    w2, V2 = f32(rng.normal(0, 0.1, F)), f32(rng.normal(0, 0.1, (F, k)))
    gids, gw, gV = run_both("bpr", twice, k, ids2, w2, V2, group=2)
    np.testing.assert_allclose(gw[own], w2[own], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(gV[own], V2[own], rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("n_neg", [1, 4])
def test_bpr_through_sample_pairs_lists(gpu, n_neg):
    """fm_batch_sample_pairs_lists sets the group itself, and the step is the step of the same rows
    uploaded with fm_batch_create + fm_batch_set_group, bit for bit."""
    k = 16
    rng = np.random.default_rng(70)
    u = rank_rows(rng, rng.integers(0, 7, 30), 48)
    rp, col, val = rank_rows(rng, rng.integers(0, 7, 50), 48)
    c = (rp, (col + 48).astype(np.int32), val)
    ids = np.arange(F, dtype=np.int32)
    w, V = f32(rng.normal(0, 0.2, F)), f32(rng.normal(0, 0.2, (F, k)))
    pc, pd = rng.integers(0, 30, 77).astype(np.int32), rng.integers(0, 50, 77).astype(np.int32)
    outs = []
    for device_pairs in (True, False):
        ctx = new_ctx(k, "bpr", ids, w, V)
        zero = lambda rows: N.CSRHost(rows[0], rows[1], rows[2], np.zeros(len(rows[0]) - 1))  # noqa: E731
        bu, bc = ctx.batch(zero(u)), ctx.batch(zero(c))
        if device_pairs:
            ex = ctx.row_lists_from_pairs(pc, pd, 30, 50)
            b, sampled = ctx._sample_pairs(bu, bc, pc, pd, n_neg, ex, 1.0, 0.0, 1234, None, True)
            assert b.group == 1 + n_neg
            ex.close()
        else:
            b = ctx.batch(host(P.concat_pairs(u, c, *P.sampled_pairs(pc, pd, sampled))))
            assert b.group == 0
            b.set_group(1 + n_neg)
        steps = [ctx.step_batch(b, t, STEP, 1e-3) for t in (1, 2)]
        outs.append(([(o.loss_sum, o.n_rows, o.n_loss_rows, o.n_unique) for o in steps], ctx.export_tables()))
        assert steps[0].n_loss_rows == 77 * n_neg and steps[0].n_rows == 77 * (1 + n_neg)
        for x in (b, bu, bc):
            x.close()
        ctx.close()
    assert outs[0][0] == outs[1][0]
    for x, y in zip(outs[0][1], outs[1][1]):
        assert x.tobytes() == y.tobytes()
    # and that step is the reference's
    csr = P.concat_pairs(u, c, *P.sampled_pairs(pc, pd, sampled))
    model = ref_model(k, ids, w, V)
    for t in (1, 2):
        ro = O.step(model, csr, t, STEP, 1e-3, "bpr", 1 + n_neg, round_scores=True, fast=True)
        assert outs[0][0][t - 1][0] == pytest.approx(ro.loss_sum, rel=RTOL, abs=ATOL)
    assert_tables(model, outs[0][1])


# ----------------------------------------------------------------------------- saturated scores
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("scale", [50.0, 1000.0])
@pytest.mark.parametrize("loss,group", [("logistic", 0), ("bpr", 2), ("bpr", 5)])
def test_saturated_scores(gpu, loss, group, scale, k):
    """Every row holds one entry x = 1 of a feature whose w is about +-scale, and entries of small features:
    |yhat| is about scale, sigma and softplus sit in their tails, nothing overflows."""
    B, big = 300, 16
    csr, ids, w, V = problem(80, B, k, max_len=6, F=F - big)
    rng = np.random.default_rng(81)
    pick = (F - big + rng.integers(0, big, B)).astype(np.int32)
    lens = np.diff(csr.row_ptr) + 1
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.insert(csr.col, csr.row_ptr[:-1], pick).astype(np.int32)
    val = np.insert(csr.val, csr.row_ptr[:-1], 1.0)
    sat = R.CSR(rp, col, val, csr.label)
    ids2 = np.arange(F, dtype=np.int32)
    w2 = np.concatenate([w[: F - big], f32(scale * rng.choice([-1.0, 1.0], big) * rng.uniform(0.9, 1.1, big))])
    V2 = f32(np.concatenate([V[: F - big], 0.01 * rng.normal(size=(big, k))]))
    yhat = O.scores(ref_model(k, ids2, w2, V2), sat, fast=True)[0]
    assert np.all(np.abs(yhat) > 0.8 * scale) and (yhat > 0).any() and (yhat < 0).any()
    run_both(loss, sat, k, ids2, w2, V2, group=group, steps=2, reg=1e-3)


# ---------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("loss,group", [("logistic", 0), ("bpr", 5), ("bpr", 65), ("bpr", 257)])
@pytest.mark.parametrize("prepare", [False, True])
def test_equal_runs_give_equal_bits(gpu, loss, group, prepare):
    k = 16
    csr, ids, w, V = problem(90, crossing(max(group, 1), 1500), k)
    runs = []
    for _ in range(2):
        ctx = new_ctx(k, loss, ids, w, V)
        b = ctx.batch(host(csr))
        if group:
            b.set_group(group)
        for t in (1, 2, 3):
            if prepare:
                b.prepare()
            ctx.step_batch(b, t, STEP, 1e-3, sync=False)
        runs.append((ctx.loss_history().tobytes(), [a.tobytes() for a in ctx.export_tables()]))
        b.close()
        ctx.close()
    assert runs[0] == runs[1]


# --------------------------------------------------------------------------- squared is untouched
def raw_create(**fields):
    """fm_create of a zero-initialised fm_config with only `fields` set: (rc, handle, message)."""
    lib = N.load()
    cfg = N.fm_config()
    for name, v in fields.items():
        setattr(cfg, name, v)
    h = C.c_void_p()
    rc = lib.fm_create(C.byref(cfg), C.byref(h))
    msg = lib.fm_last_error()
    return rc, h, msg.decode() if msg else ""


def test_squared_context_is_the_context_without_the_field(gpu):
    from fm_spark_amd.engine import FMContext

    k = 16
    csr, ids, w, V = problem(95, 700, k)
    runs = []
    for explicit in (True, False):
        if explicit:
            ctx = FMContext(F, k, loss="squared")
        else:  # the config as a caller of the earlier header fills it: the field never written
            rc, h, msg = raw_create(num_features=F, k=k, init_sd=0.01, shard_count=1)
            assert rc == 0, msg
            ctx = FMContext.__new__(FMContext)
            ctx._lib, ctx.handle, ctx.num_features, ctx.k = N.load(), h, F, k
        ctx.load_tables(ids, w, V)
        ctx.profile_enable(True)
        b = ctx.batch(host(csr))
        b.set_group(7)  # ignored by a squared context
        outs = [ctx.step_batch(b, t, STEP, 1e-3) for t in (1, 2, 3)]
        prof = ctx.profile_read()
        assert "objective" not in prof and prof["forward"][1] == 3 and prof["update"][1] == 3
        runs.append(([(o.loss_sum, o.n_loss_rows, o.n_unique) for o in outs], ctx.loss_history().tobytes(),
                     [a.tobytes() for a in ctx.export_tables()]))
        b.close()
        ctx.close()
    assert runs[0] == runs[1]
    # ... and it is still the oracle's squared step
    model = ref_model(k, ids, w, V)
    for t in (1, 2, 3):
        ro = R.sgd_step_fast(model, csr, t, STEP, 1e-3)
        assert runs[0][0][t - 1][0] == pytest.approx(ro.loss_sum, rel=RTOL)


def test_objective_profile_entry(gpu):
    k = 4
    csr, ids, w, V = problem(96, 300, k)
    ctx = new_ctx(k, "logistic", ids, w, V)
    ctx.profile_enable(True)
    b = ctx.batch(host(csr))
    for t in (1, 2, 3):
        ctx.step_batch(b, t, STEP, 0.0)
    prof = ctx.profile_read()
    assert prof["objective"][1] == 3 and prof["forward"][1] == 3
    ctx.close()


# -------------------------------------------------------------------------------------- refusals
def test_create_refusals(gpu):
    base = dict(num_features=F, k=4, shard_count=1)
    for message, fields in [
        ("loss must be FM_LOSS_SQUARED, FM_LOSS_LOGISTIC or FM_LOSS_BPR", dict(loss=3)),
        ("loss must be FM_LOSS_SQUARED, FM_LOSS_LOGISTIC or FM_LOSS_BPR", dict(loss=-1)),
        ("loss = FM_LOSS_LOGISTIC cannot take fuse_single = FM_FUSE_ON", dict(loss=N.FM_LOSS_LOGISTIC, fuse_single=N.FM_FUSE_ON)),
        ("loss = FM_LOSS_BPR cannot take fuse_single = FM_FUSE_ON", dict(loss=N.FM_LOSS_BPR, fuse_single=N.FM_FUSE_ON)),
        ("loss = FM_LOSS_LOGISTIC needs parallel == FM_PARALLEL_NONE",
         dict(loss=N.FM_LOSS_LOGISTIC, parallel=N.FM_PARALLEL_SHARDED, n_gpus=1, n_procs=1, transport=N.FM_TRANSPORT_COPY)),
        ("loss = FM_LOSS_BPR needs parallel == FM_PARALLEL_NONE",
         dict(loss=N.FM_LOSS_BPR, parallel=N.FM_PARALLEL_REPLICATED, n_gpus=1, n_procs=1, transport=N.FM_TRANSPORT_COPY)),
        ("loss = FM_LOSS_LOGISTIC needs shard_count == 1", dict(loss=N.FM_LOSS_LOGISTIC, shard_count=2)),
        ("loss = FM_LOSS_BPR needs shard_count == 1", dict(loss=N.FM_LOSS_BPR, shard_count=2, shard_index=1)),
    ]:
        before = live()
        rc, h, msg = raw_create(**{**base, **fields})
        assert rc == -1 and not h.value and message in msg, (fields, rc, msg)
        assert live() == before
    for loss in (N.FM_LOSS_LOGISTIC, N.FM_LOSS_BPR):  # FM_FUSE_OFF and the default are accepted, and never fuse
        for fuse in (N.FM_FUSE_DEFAULT, N.FM_FUSE_OFF):
            rc, h, msg = raw_create(**base, loss=loss, fuse_single=fuse)
            assert rc == 0, msg
            assert N.load().fm_fuse_active(h) == 0
            N.load().fm_destroy(h)


def test_bpr_step_of_an_ungrouped_batch_is_refused(gpu):
    k = 16
    csr, ids, w, V = problem(97, 60, k)
    ctx = new_ctx(k, "bpr", ids, w, V)
    b = ctx.batch(host(csr))
    ctx.reserve(csr.n_rows, csr.nnz)
    tab, before = ctx.export_tables(), live()
    for call in (lambda: ctx.step_batch(b, 1, STEP, 0.0), lambda: ctx.step_batch(b, 1, STEP, 0.0, sync=False),
                 lambda: ctx.step(host(csr), 1, STEP, 0.0)):
        with pytest.raises(N.FMError, match="needs a grouped batch"):
            call()
        assert ctx.epoch == 0 and live() == before and len(ctx.loss_history()) == 0
    for x, y in zip(tab, ctx.export_tables()):
        assert x.tobytes() == y.tobytes()
    b.set_group(4)
    assert ctx.step_batch(b, 1, STEP, 0.0).n_loss_rows == 45 and ctx.epoch == 1
    b.set_group(0)
    with pytest.raises(N.FMError, match="needs a grouped batch"):
        ctx.step_batch(b, 2, STEP, 0.0)
    # the manual replicated phases are the squared step's
    grad = np.zeros(1)
    rc = N.load().fm_repl_grad(ctx.handle, b.handle, grad.ctypes.data_as(C.c_void_p))
    assert rc == -1 and b"fm_repl_grad runs the squared step only" in N.load().fm_last_error()
    rc = N.load().fm_repl_apply(ctx.handle, grad.ctypes.data_as(C.c_void_p), 1, 0.1, 0.0, 10)
    assert rc == -1 and b"fm_repl_apply runs the squared step only" in N.load().fm_last_error()
    rc = N.load().fm_shard_owner_forward(ctx.handle, b.handle, None)
    assert rc == -1 and b"fm_shard_owner_forward runs the squared step only" in N.load().fm_last_error()
    b.close()
    ctx.close()


def test_set_group_refusals_and_bookkeeping(gpu):
    k = 4
    csr, ids, w, V = problem(98, 60, k)
    for loss in ("squared", "logistic", "bpr"):
        ctx = new_ctx(k, loss, ids, w, V)
        if loss != "squared":
            assert ctx.fuse_active is False
        b = ctx.batch(host(csr))
        assert b.group == 0
        for bad, message in [(1, r"group must be 0 or in \[2, 1025\], got 1"), (1026, r"got 1026"), (-2, r"got -2"),
                             (7, "group 7 does not divide the batch's 60 rows"), (1025, "does not divide")]:
            with pytest.raises(N.FMError, match=message):
                b.set_group(bad)
            assert b.group == 0
        assert b.set_group(60).group == 60 and b.set_group(2).group == 2 and b.set_group(0).group == 0
        # a split dataset is not grouped; its views start ungrouped and take a group of their own
        data = ctx.batch_splits(host(csr), [0, 20, 60])
        with pytest.raises(N.FMError, match="fm_batch_create_splits is not grouped"):
            data.set_group(2)
        # every refill resets the group: fm_batch_from_rows, fm_batch_from_pairs, fm_batch_split_view
        src = ctx.batch(host(csr))
        b.set_group(2)
        ctx.batch_from_rows(src, np.arange(10), into=b)
        assert b.group == 0 and b.n_rows == 10
        b.set_group(5)
        ctx.batch_from_pairs(src, src, [0, 1, 2, 3], [4, 5, 6, 7], np.zeros(4), into=b)
        assert b.group == 0
        b.set_group(4)
        b2, sampled = ctx.batch_sample_pairs(src, src, [0, 1, 2], [3, 4, 5], 2, into=b, want_sampled=True)
        assert b2 is b and b.group == 3 and b.n_rows == 9
        ctx.batch_sample_pairs(src, src, [0, 1, 2], [3, 4, 5], 0, into=b)
        assert b.group == 0  # no negatives, no groups
        b.set_group(3)
        ctx.split_view(data, 1, into=b)
        assert b.group == 0 and b.n_rows == 40
        b.set_group(8)
        if loss == "bpr":
            assert ctx.step_batch(b, 1, STEP, 0.0).n_loss_rows == 35
        for x in (b, src, data):
            x.close()
        ctx.close()
    assert N.load().fm_batch_group(None) == -1


# ---------------------------------------------------------------------------------------- memory
@pytest.mark.parametrize("loss,group", [("logistic", 0), ("bpr", 5)])
def test_reserved_steps_allocate_nothing(gpu, loss, group):
    k = 20
    big, ids, w, V = problem(99, 4000, k)
    small = problem(100, 35, k)[0]
    ctx = new_ctx(k, loss, ids, w, V)
    bs = [ctx.batch(host(c)) for c in (small, big)]
    if group:
        for b in bs:
            b.set_group(group)
    ctx.reserve(big.n_rows, big.nnz)
    before = live()
    for t in range(1, 7):
        ctx.step_batch(bs[t % 2], t, STEP, 1e-3, sync=t % 3 == 0)
        assert live() == before
    ctx.sync()
    assert live() == before
    for b in bs:
        b.close()
    ctx.close()
    gc.collect()
