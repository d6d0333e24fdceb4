"""GPU: the binary evaluation through the C-ABI (fm_binary_metrics, fm_evaluate_binary[_batch],
fm_eval_binary_history; fm_binary.hip).

The integers of a record (n_rows, n_pos, tp, fp, two_u) must equal tests/binary_ref.py's, computed from the
call's own returned scores and the labels, with == ; the returned scores must be fm_predict_batch(-inf, inf)'s
bit for bit; the log loss sum must lie within binary_ref's derived budget of the exact sum over those scores.

Shapes sit on the edges of the stage's constants, written out below."""

import ctypes as C
import math

import numpy as np
import pytest

import binary_ref as B
from fm_spark_amd import _native as N
from oracle import fm_ref as R
from problems import f32, make_rows

pytestmark = pytest.mark.gpu
INF = math.inf

K_BLOCK = 256            # kBlock: threads per block of k_binary_rows / _rekey / _flag / _count and of the fold
K_GRID = 1024            # kBinGrid: blocks of those kernels at most; a thread takes several rows past K_BLOCK * K_GRID
K_SORT_TILE = 4096       # kTile: keys per tile of the radix sort (fm_sort.hip)
K_SCAN_CHUNK = 256       # kPairChunk: flags per chunk of the scan (fm_pairs.hip)
K_ROUND_CHUNKS = 1024    # kPairScanNT * kPairScanPer: chunks the one-block scan takes per round
ROUND = K_SCAN_CHUNK * K_ROUND_CHUNKS  # 262 144 rows: one scan round, and the rows one grid takes a thread each
assert ROUND == K_BLOCK * K_GRID

F, K = 300, 16
EDGE_N = [1, 2, K_BLOCK - 1, K_BLOCK, K_BLOCK + 1, K_SORT_TILE - 1, K_SORT_TILE, K_SORT_TILE + 1, 2 * K_SORT_TILE + 1]


def host(csr):
    return N.CSRHost(csr.row_ptr, csr.col, csr.val, csr.label)


def live():
    lib = N.load()
    return int(lib.fm_device_bytes_live()), int(lib.fm_device_allocs_live())


def new_ctx(w0=0.125, scale=0.3, **kw):
    from fm_spark_amd.engine import FMContext

    rng = np.random.default_rng(1)
    ctx = FMContext(F, K, w0=w0, **kw)
    ctx.load_tables(np.arange(F, dtype=np.int32), f32(scale * rng.standard_normal(F)), f32(scale * rng.standard_normal((F, K))))
    return ctx


@pytest.fixture(scope="module")
def ctx(gpu):
    c = new_ctx()
    yield c
    c.close()


def rows(seed, n, max_len=6, labels=None):
    """n rows of 0..max_len entries (some without any: they score w0 and tie with each other), 0/1 labels"""
    rng = np.random.default_rng(5000 + seed)
    csr = make_rows(seed, rng.integers(0, max_len + 1, n), F, K)[0]
    csr.label = (rng.random(n) < 0.3).astype(np.float64) if labels is None else np.asarray(labels, dtype=np.float64)
    return csr


def repeat_rows(csr, counts):
    """row i of csr counts[i] times, in order"""
    counts = np.asarray(counts, dtype=np.int64)
    idx = np.repeat(np.arange(csr.n_rows), counts)
    lens = np.diff(csr.row_ptr)[idx]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ent = np.repeat(csr.row_ptr[idx] - rp[:-1], lens) + np.arange(rp[-1], dtype=np.int64)
    return R.CSR(rp, csr.col[ent], csr.val[ent], csr.label[idx].copy())


def permute_rows(csr, perm):
    lens = np.diff(csr.row_ptr)[perm]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ent = np.repeat(csr.row_ptr[perm] - rp[:-1], lens) + np.arange(rp[-1], dtype=np.int64)
    return R.CSR(rp, csr.col[ent], csr.val[ent], csr.label[perm].copy())


def evaluate_checked(ctx, csr):
    """evaluate_binary_batch of csr, held to predict_batch's bits and the reference; returns (record, scores)"""
    b = ctx.batch(host(csr))
    rec, score = ctx.evaluate_binary_batch(b, want_score=True)
    assert score.tobytes() == ctx.predict_batch(b, -INF, INF).tobytes()
    assert ctx.evaluate_binary_batch(b) == rec  # without the scores: the same record
    b.close()
    B.check(rec, score, csr.label)
    assert rec.executed and rec.epoch == ctx.epoch
    return rec, score


# ----------------------------------------------------------------------------- 1. through a model
@pytest.mark.parametrize("n", EDGE_N)
def test_edge_row_counts_through_a_model(ctx, n):
    csr = rows(n, n)
    rec, score = evaluate_checked(ctx, csr)
    if n > 2:
        assert 0 < rec.n_pos < n and len(np.unique(score)) < n  # both classes, and ties (the rows without entries)
    # the host-CSR call gives the same record
    assert ctx.evaluate_binary(host(csr)) == rec


def test_one_tie_run_covering_everything(ctx):
    n = K_SORT_TILE + K_BLOCK + 1
    rng = np.random.default_rng(3)
    csr = R.CSR(np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), (rng.random(n) < 0.4).astype(np.float64))
    rec, score = evaluate_checked(ctx, csr)
    assert np.all(score == 0.125)
    assert rec.two_u == rec.n_pos * (n - rec.n_pos) and rec.auc == 0.5
    assert (rec.tp, rec.fp) == (rec.n_pos, n - rec.n_pos)


@pytest.mark.parametrize("counts", [(3000, 3000, 3000), (K_BLOCK - 1, 2, K_SORT_TILE - K_BLOCK, 2, 300), (1, K_SORT_TILE, 1)])
def test_tie_runs_straddle_blocks_tiles_and_chunks(ctx, counts):
    """a few distinct rows, each repeated: runs of equal scores that start and end off every boundary, with
    both labels inside each run"""
    base = rows(77, len(counts), max_len=5)
    assert np.all(np.diff(base.row_ptr) >= 0)
    csr = repeat_rows(base, counts)
    n = csr.n_rows
    csr.label = (np.random.default_rng(9).random(n) < 0.5).astype(np.float64)
    rec, score = evaluate_checked(ctx, csr)
    assert len(np.unique(score)) <= len(counts)


@pytest.mark.parametrize("label", [1.0, 0.0])
def test_one_class_only(ctx, label):
    n = K_BLOCK + 3
    csr = rows(21, n, labels=np.full(n, label))
    rec, _ = evaluate_checked(ctx, csr)
    assert rec.two_u == 0 and math.isnan(rec.auc)
    assert rec.n_pos == (n if label else 0)


def test_half_is_negative_and_fractional_labels_enter_the_loss(ctx):
    n = 700
    rng = np.random.default_rng(4)
    lab = rng.choice([0.0, 0.25, 0.5, 0.75, 1.0], n)
    csr = rows(22, n, labels=lab)
    rec, score = evaluate_checked(ctx, csr)
    assert rec.n_pos == int((lab > 0.5).sum()) and (lab == 0.5).sum() > 50
    # the loss is the soft-target one: it differs from the hard labels' by far more than the budget
    hard = B.log_loss(score, (lab > 0.5).astype(np.float64))
    assert abs(hard.value - rec.sum_log_loss) > 1e3 * hard.budget


def test_saturated_scores_keep_the_loss_finite(gpu):
    """|score| of several hundred, right and wrong: softplus stays finite, the loss is about sum |s| over the wrong rows"""
    from fm_spark_amd.engine import FMContext

    ctx = FMContext(F, K, w0=0.0)
    w = np.where(np.arange(F) % 2 == 0, 48.0, -48.0)
    ctx.load_tables(np.arange(F, dtype=np.int32), w, np.zeros((F, K)))
    n = 600
    rng = np.random.default_rng(8)
    sign = rng.integers(0, 2, n)  # the row's ids all even (score +) or all odd (score -)
    per = 10
    col = (2 * rng.integers(0, F // 2, (n, per)) + sign[:, None]).astype(np.int32)
    col = np.sort(col, axis=1)
    for r in range(n):  # distinct ids within a row
        while len(np.unique(col[r])) < per:
            col[r] = np.sort((2 * rng.choice(F // 2, per, replace=False) + sign[r]).astype(np.int32))
    csr = R.CSR(np.arange(0, n * per + 1, per, dtype=np.int64), col.reshape(-1), np.ones(n * per),
                (rng.random(n) < 0.5).astype(np.float64))
    rec, score = evaluate_checked(ctx, csr)
    assert np.all(np.abs(score) == 480.0)
    wrong = (score > 0) != (csr.label > 0.5)
    assert 100 < wrong.sum() < 500
    assert rec.sum_log_loss == pytest.approx(480.0 * wrong.sum(), rel=1e-12)
    ctx.close()


def test_signed_zero_through_a_model(gpu):
    """w0 = -0.0: a row without entries scores w0 = -0.0; a row whose one entry is an explicit zero of a learned
    id (positive w) scores -0.0 + 0.0 = +0.0.  Opposite labels: every pair is a tie."""
    from fm_spark_amd.engine import FMContext

    ctx = FMContext(F, K, w0=-0.0)
    rng = np.random.default_rng(2)
    ctx.load_tables(np.arange(F, dtype=np.int32), f32(0.1 + rng.random(F)), f32(0.1 + rng.random((F, K))))
    n_e, n_z = 300, 217
    rp = np.concatenate([np.zeros(n_e, np.int64), np.arange(n_z + 1, dtype=np.int64)])
    csr = R.CSR(rp, rng.integers(0, F, n_z).astype(np.int32), np.zeros(n_z),
                np.concatenate([np.ones(n_e), np.zeros(n_z)]))
    rec, score = evaluate_checked(ctx, csr)
    assert np.all(score == 0.0)
    signs = np.signbit(score)
    assert signs[:n_e].all() and not signs[n_e:].any()  # both zeros occur: the case shows what it is meant to
    assert rec.two_u == n_e * n_z and rec.auc == 0.5 and rec.tp == 0 and rec.fp == 0
    ctx.close()


def test_lazy_l1_pending_when_evaluated(gpu):
    ctx = new_ctx()
    train = rows(31, 400)
    held = rows(32, 333)
    bt = ctx.batch(host(train))
    for t in (1, 2, 3):
        ctx.step_batch(bt, t, 0.3, 0.05)  # reg_param > 0: every row's shrink is pending until it is next read
    rec, _ = evaluate_checked(ctx, held)
    assert rec.epoch == 3
    bt.close()
    ctx.close()


# ---------------------------------------------------------------------- 2. through fm_binary_metrics
def metrics_checked(ctx, score, label, with_loss=True):
    score = np.asarray(score, dtype=np.float64)
    label = np.asarray(label, dtype=np.float64)
    h0 = len(ctx.eval_binary_history())
    rec = ctx.binary_metrics(score, label)
    B.check(rec, score, label, with_loss=with_loss)
    assert rec.executed and rec.epoch == ctx.epoch
    assert len(ctx.eval_binary_history()) == h0  # nothing appended
    return rec


@pytest.mark.parametrize("n", EDGE_N + [ROUND - 1, ROUND, ROUND + 1])
def test_metrics_edge_counts(ctx, n):
    rng = np.random.default_rng(n)
    score = np.round(rng.normal(0.0, 2.0, n), 3)  # ties once n passes a few thousand
    if n > 4:
        score[rng.integers(0, n, n // 4)] = rng.choice([0.0, -0.0, 1.5], n // 4)
    metrics_checked(ctx, score, (rng.random(n) < 0.3).astype(np.float64))


def test_metrics_isolate_each_sort_pass(ctx):
    rng = np.random.default_rng(6)
    n = K_SORT_TILE + 77
    lab = (rng.random(n) < 0.5).astype(np.float64)
    # the low word only: 1 + j 2^-52, j < 2^32 -- equal high words, the order is the first sort's alone
    low = (np.uint64(0x3FF0000000000000) + rng.integers(0, 2 ** 32, n).astype(np.uint64)).view(np.float64)
    assert len(np.unique(low.view(np.uint64) >> np.uint64(32))) == 1
    metrics_checked(ctx, low, lab)
    # the high word only: low words all zero, both signs -- the second sort's alone
    high = (rng.integers(0, 2 ** 32, n).astype(np.uint64) << np.uint64(32)).view(np.float64)
    high = high[np.isfinite(high)]
    assert np.all(high.view(np.uint64) & np.uint64(0xFFFFFFFF) == 0) and (high < 0).any() and (high > 0).any()
    metrics_checked(ctx, high, lab[: len(high)], with_loss=False)  # (scores up to 1e308: only the order is at stake)
    # equal low words in long runs under distinct high words and the reverse: stability of both
    both = ((rng.integers(0x3FE00000, 0x3FE00004, n).astype(np.uint64) << np.uint64(32)) | rng.integers(0, 3, n).astype(np.uint64)).view(np.float64)
    metrics_checked(ctx, both, lab)


def test_metrics_infinities_denormals_and_signed_zeros(ctx):
    rng = np.random.default_rng(7)
    pool = np.array([-INF, INF, 0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072014e-308, 1.0, -1.0])
    n = 3 * K_BLOCK + 5
    score = rng.choice(pool, n)
    lab = (rng.random(n) < 0.5).astype(np.float64)
    rec = metrics_checked(ctx, score, lab, with_loss=False)  # (an infinite score has no finite loss term)
    assert rec.two_u == B.two_u_quadratic(score, lab)
    # without the infinities the loss is held too
    fin = np.isfinite(score)
    metrics_checked(ctx, score[fin], lab[fin])
    # +0.0 against -0.0 with opposite labels: ties, both ways round
    for pos_zero, neg_zero in ((0.0, -0.0), (-0.0, 0.0)):
        s = np.array([pos_zero] * 5 + [neg_zero] * 7)
        y = np.array([1.0] * 5 + [0.0] * 7)
        rec = metrics_checked(ctx, s, y)
        assert rec.two_u == 35 and rec.auc == 0.5 and (rec.tp, rec.fp) == (0, 0)


# ------------------------------------------------------------------------------- 3. determinism
def test_equal_bytes_twice_and_equal_integers_permuted(ctx):
    n = 2 * K_SORT_TILE + 100
    csr = rows(41, n)
    lib = N.load()
    b = ctx.batch(host(csr))
    outs = [N.fm_binary_out(), N.fm_binary_out()]
    for o in outs:
        N.check(lib.fm_evaluate_binary_batch(ctx.handle, b.handle, None, C.byref(o)), "fm_evaluate_binary_batch")
    assert bytes(outs[0]) == bytes(outs[1])
    rec = ctx.evaluate_binary_batch(b)
    perm = np.random.default_rng(1).permutation(n)
    bp = ctx.batch(host(permute_rows(csr, perm)))
    rec_p, score_p = ctx.evaluate_binary_batch(bp, want_score=True)
    assert B.integers_of(rec_p) == B.integers_of(rec)
    B.check(rec_p, score_p, csr.label[perm])
    # and through fm_binary_metrics with the same scores: the same record but for the history
    m1, m2 = ctx.binary_metrics(score_p, csr.label[perm]), ctx.binary_metrics(score_p, csr.label[perm])
    assert m1 == m2 == rec_p
    b.close()
    bp.close()


# ---------------------------------------------------------------------------------- 4. history
def _last_stats(ctx):
    ls, nl, nu = C.c_double(), C.c_int64(), C.c_int64()
    N.check(N.load().fm_last_stats(ctx.handle, C.byref(ls), C.byref(nl), C.byref(nu)), "fm_last_stats")
    return ls.value, nl.value, nu.value


def test_history_of_enqueued_evaluations_between_steps(gpu):
    data = rows(51, 240)
    held = rows(52, 150)
    recs = {}
    for sync in (False, True):
        ctx = new_ctx(loss="logistic")
        twin = new_ctx(loss="logistic")  # never evaluates
        bt, bh = ctx.batch(host(data)), ctx.batch(host(held))
        tt = twin.batch(host(data))
        ds = ctx.batch_splits(host(held), np.array([0, 50, 150]))
        view = ctx.split_view(ds, 1)
        got = [ctx.evaluate_binary_batch(bh, sync=sync)]           # epoch 0
        for t in (1, 2):
            ctx.step_batch(bt, t, 0.3, 0.02, sync=False)
            twin.step_batch(tt, t, 0.3, 0.02, sync=False)
            got.append(ctx.evaluate_binary_batch(view if t == 1 else bh, sync=sync))  # epochs 1 (a split's view), 2
        before = (ctx.epoch, ctx.loss_history().tobytes(), _last_stats(ctx), len(ctx.eval_history()))
        hist = ctx.eval_binary_history()
        assert [h.epoch for h in hist] == [0, 1, 2] and [h.n_rows for h in hist] == [150, 100, 150]
        assert got == (hist if sync else [None] * 3)
        assert before == (ctx.epoch, ctx.loss_history().tobytes(), _last_stats(ctx), 0)  # regression history untouched
        assert hist[2] != hist[0]  # the table moved between them
        score = ctx.predict_batch(bh, -INF, INF)
        B.check(hist[2], score, held.label)
        for a, b in zip(ctx.export_tables(), twin.export_tables()):  # the evaluations left the table alone
            np.testing.assert_array_equal(a, b)
        recs[sync] = hist
        for x in (view, ds, bt, bh, tt):
            x.close()
        ctx.close()
        twin.close()
    assert recs[False] == recs[True]


def test_history_grows_past_its_first_capacity(gpu):
    ctx = new_ctx()
    bs, bo = ctx.batch(host(rows(61, 8))), ctx.batch(host(rows(62, 9)))
    first = [ctx.evaluate_binary_batch(bo), ctx.evaluate_binary_batch(bs), ctx.evaluate_binary_batch(bo)]
    for _ in range(4100 - 3):
        ctx.evaluate_binary_batch(bs, sync=False)
    hist = ctx.eval_binary_history()
    assert len(hist) == 4100
    assert hist[:3] == first                       # kept across the growth at 4096
    assert all(h == first[1] for h in hist[3:])    # equal inputs, equal bits, before and after it
    bs.close()
    bo.close()
    ctx.close()


# ---------------------------------------------------------------- 5. memory, arguments, refusals
def test_memory_arguments_and_refusals(gpu):
    from fm_spark_amd.engine import FMContext

    lib = N.load()
    start = live()
    ctx = new_ctx()
    other = FMContext(F, K)
    csr = rows(71, 1000)
    b = ctx.batch(host(csr))
    nothing = R.CSR(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0), np.zeros(0))
    empty = ctx.batch(host(nothing))
    ds = ctx.batch_splits(host(csr), np.array([0, 400, 1000]))
    foreign = other.batch(host(csr))
    rec, score = ctx.evaluate_binary_batch(b, want_score=True)  # the scratch grows here
    ctx.binary_metrics(score, csr.label)
    steady = live()
    assert ctx.evaluate_binary_batch(b, want_score=True)[0] == rec
    assert ctx.binary_metrics(score, csr.label) == rec
    assert live() == steady
    n_hist = len(ctx.eval_binary_history())
    out = N.fm_binary_out(n_rows=9, n_pos=9, epoch=9, tp=9, fp=9, two_u=9, sum_log_loss=9.0)
    zeroed = lambda o: (o.n_rows, o.n_pos, o.epoch, o.tp, o.fp, o.two_u, o.sum_log_loss) == (0, 0, 0, 0, 0, 0, 0.0)  # noqa: E731
    dbl = lambda a: N.ptr(a, C.c_double)  # noqa: E731

    def refused(rc, *needles):
        assert rc == -1, rc
        msg = lib.fm_last_error().decode()
        for s in needles:
            assert s in msg, msg

    # zero rows: nothing to do, a zeroed record, nothing appended
    assert lib.fm_evaluate_binary_batch(ctx.handle, empty.handle, None, C.byref(out)) == N.FM_NOTHING_TO_DO and zeroed(out)
    z = ctx.evaluate_binary(host(nothing))
    assert not z.executed and z.n_rows == 0
    z = ctx.binary_metrics(np.zeros(0), np.zeros(0))
    assert not z.executed and z.n_rows == 0
    # a split dataset; its views are accepted
    refused(lib.fm_evaluate_binary_batch(ctx.handle, ds.handle, None, C.byref(out)), "fm_evaluate_binary_batch", "by split")
    # a foreign batch, null batch, null context, null CSR, null out
    refused(lib.fm_evaluate_binary_batch(ctx.handle, foreign.handle, None, C.byref(out)), "fm_evaluate_binary_batch",
            "another context")
    refused(lib.fm_evaluate_binary_batch(ctx.handle, None, None, C.byref(out)), "fm_evaluate_binary_batch")
    refused(lib.fm_evaluate_binary_batch(None, b.handle, None, C.byref(out)), "null fm_ctx")
    refused(lib.fm_evaluate_binary(ctx.handle, None, None, C.byref(out)), "fm_evaluate_binary", "null")
    refused(lib.fm_evaluate_binary(ctx.handle, C.byref(host(csr).c), None, None), "fm_evaluate_binary", "null")
    # out == NULL with score
    buf = np.zeros(1000)
    refused(lib.fm_evaluate_binary_batch(ctx.handle, b.handle, dbl(buf), None), "fm_evaluate_binary_batch", "score needs out")
    # fm_binary_metrics: nulls and n out of range
    refused(lib.fm_binary_metrics(ctx.handle, dbl(buf), dbl(buf), 10, None), "fm_binary_metrics", "null")
    refused(lib.fm_binary_metrics(ctx.handle, None, dbl(buf), 10, C.byref(out)), "fm_binary_metrics", "null")
    refused(lib.fm_binary_metrics(ctx.handle, dbl(buf), None, 10, C.byref(out)), "fm_binary_metrics", "null")
    refused(lib.fm_binary_metrics(ctx.handle, dbl(buf), dbl(buf), -1, C.byref(out)), "fm_binary_metrics", "out of range")
    refused(lib.fm_binary_metrics(ctx.handle, dbl(buf), dbl(buf), 2 ** 31, C.byref(out)), "fm_binary_metrics", "out of range")
    n = C.c_int64()
    refused(lib.fm_eval_binary_history(ctx.handle, None, 0, None), "fm_eval_binary_history", "null")
    refused(lib.fm_eval_binary_history(None, None, 0, C.byref(n)), "null fm_ctx")
    # no refused call appended anything or allocated
    assert len(ctx.eval_binary_history()) == n_hist
    assert live() == steady
    view = ctx.split_view(ds, 1)
    assert ctx.evaluate_binary_batch(view).n_rows == 600
    assert ctx.evaluate_binary_batch(b) == rec
    for x in (view, ds, b, empty, foreign):
        x.close()
    ctx.close()
    other.close()
    assert live() == start


def test_multi_gpu_and_sharded_contexts_are_refused(gpu):
    from fm_spark_amd.engine import FMContext

    lib = N.load()
    csr = rows(81, 64)
    out = N.fm_binary_out()
    s = np.zeros(4)
    for kw in (dict(parallel="replicated", n_gpus=2, devices=[0, 0], transport="copy"),
               dict(parallel="sharded", n_gpus=2, devices=[0, 0], transport="copy"),
               dict(shard_index=0, shard_count=2)):
        ctx = FMContext(F, K, **kw)
        b = ctx.batch(host(csr))
        hc = host(csr)
        for fn, call in ((lambda: lib.fm_evaluate_binary_batch(ctx.handle, b.handle, None, C.byref(out)), "fm_evaluate_binary_batch"),
                         (lambda: lib.fm_evaluate_binary_batch(ctx.handle, b.handle, None, None), "fm_evaluate_binary_batch"),
                         (lambda: lib.fm_evaluate_binary(ctx.handle, C.byref(hc.c), None, C.byref(out)), "fm_evaluate_binary"),
                         (lambda: lib.fm_binary_metrics(ctx.handle, N.ptr(s, C.c_double), N.ptr(s, C.c_double), 4, C.byref(out)),
                          "fm_binary_metrics")):
            assert fn() == -1
            msg = lib.fm_last_error().decode()
            assert msg.startswith(call + " needs a single-table context") and "multi-GPU" in msg, msg
        assert ctx.eval_binary_history() == []
        b.close()
        ctx.close()


def test_profile_names(gpu):
    ctx = new_ctx()
    b = ctx.batch(host(rows(91, 500)))
    ctx.profile_enable(True)
    ctx.evaluate_binary_batch(b)
    prof = ctx.profile_read()
    for name in ("evaluate_binary", "binary_sort", "binary_count"):
        assert name in prof, prof
    b.close()
    ctx.close()
