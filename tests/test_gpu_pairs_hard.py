"""GPU: fm_batch_sample_pairs_hard (include/fm_hip.h) -- n_draw draws per positive, the n_neg the model
scores highest kept in draw order.

Exact yardstick: one rank_batch(n_top = C, -inf, inf) call on the same table returns every pair's device
score; the draws come from tests/pair_ref.py's statement of the draw contract; the expected selection is
the first n_neg under (score descending, j ascending), emitted in ascending j.  `sampled` must equal it
exactly: the sampler's keys are the ranking calls' bits.  Those scores are themselves held to
tests/rank_ref.py's fp64 reference within its reordered-sum bound (tests/test_gpu_rank.py's)."""

import functools

import numpy as np
import pytest

import pair_ref as P
import rank_ref as R
from fm_spark_amd import _native as N
from test_gpu_pairs import F, cand_rows, rows_host

pytestmark = pytest.mark.gpu
INF, W0 = float("inf"), 0.25


def scores(ctx, bu, bc):
    """S [U, C]: the device score of every pair, by one ranking call."""
    idx, sc = ctx.rank_batch(bu, bc, bc.n_rows, -INF, INF)
    S = np.empty_like(sc)
    np.put_along_axis(S, idx.astype(np.int64), sc, axis=1)
    return S


def expected(S, seed, pos_ctx, n_neg, n_draw, ptr, rows):
    draws = P.sample_negatives(seed, pos_ctx, n_draw, ptr, rows, S.shape[1])
    key = S[np.asarray(pos_ctx)[:, None], draws]
    keep = [np.sort(np.lexsort((np.arange(n_draw), -key[i]))[:n_neg]) for i in range(len(draws))]
    return np.take_along_axis(draws, np.asarray(keep, np.int64).reshape(len(draws), n_neg), axis=1)


class World:
    """U = 6 contexts (row 1 empty: no learned entry) against C candidates (every fourth empty) on a table that
    has taken three steps with L1 -- read by catch-up, never flushed; exclude lists: none, three rows, all
    but one row (E = 1), the positives' candidate, half of the rows, one row."""

    def __init__(self, k, C, seed=31):
        from fm_spark_amd.engine import FMContext

        rng = np.random.default_rng(seed + k + C)
        self.k, self.C, self.U = k, C, 6
        self.u, self.c = R.make_rows(rng, [3, 0, 17, 1, 2, 5], 100), cand_rows(rng, np.arange(C) % 4)
        self.ctx = FMContext(F, k, w0=W0)
        self.ctx.load_tables(np.arange(F, dtype=np.int32), R.f32(0.3 * rng.standard_normal(F)),
                             R.f32(0.3 * rng.standard_normal((F, k))))
        self.bu, self.bc = self.ctx.batch(rows_host(self.u)), self.ctx.batch(rows_host(self.c))
        self.lists = [np.zeros(0, np.int64), np.sort(rng.choice(C, 3, replace=False)), np.delete(np.arange(C), C // 2),
                      np.array([C - 3]), np.sort(rng.choice(C, C // 2, replace=False)), np.array([0])]
        self.ptr = np.concatenate([[0], np.cumsum([len(x) for x in self.lists])]).astype(np.int64)
        self.rows = np.concatenate(self.lists).astype(np.int32)
        self.resident = self.ctx.row_lists(self.lists, C)
        for t in range(1, 4):
            self.step(t, 0.05)
        self.S = scores(self.ctx, self.bu, self.bc)

    def step(self, t, size):
        rng = np.random.default_rng(t)
        pc, pd = rng.integers(0, self.U, 40), rng.integers(0, self.C, 40)
        self.ctx.step_batch(self.ctx.batch_from_pairs(self.bu, self.bc, pc, pd, rng.standard_normal(40)), t, size, 1e-3)

    def positives(self, n_pos, seed=5):
        rng = np.random.default_rng(seed)
        pos_ctx = np.concatenate([np.arange(self.U), rng.integers(0, self.U, max(n_pos - self.U, 0))])[:n_pos]
        pos_cand = rng.integers(0, self.C, n_pos)
        pos_cand[pos_ctx == 3] = self.C - 3  # on its context's list
        return pos_ctx, pos_cand

    def sample(self, pos, n_neg, n_draw, resident=False, seed=9, refresh=True, **kw):
        return self.ctx.batch_sample_pairs(self.bu, self.bc, *pos, n_neg, exclude=self.resident if resident else self.lists,
                                           seed=seed, want_sampled=True, n_draw=n_draw, refresh=refresh, **kw)

    def want(self, pos, n_neg, n_draw, seed=9, S=None):
        return expected(self.S if S is None else S, seed, pos[0], n_neg, n_draw, self.ptr, self.rows)


world = functools.lru_cache(maxsize=None)(World)


@pytest.mark.parametrize("k,C", [(4, 8), (16, 1000), (80, 1000)])
def test_scores_lie_within_the_reference_bound(gpu, k, C):
    """the yardstick's own check: every device score against rank_ref, and w0 where nothing is learned"""
    w = world(k, C)
    tw, tV, present = w.ctx.export_rows(np.arange(F))
    ref = R.pair_ref(tw, tV, present, W0, w.u, w.c)
    assert np.all(np.abs(w.S - ref.key) <= ref.bound), float(np.max(np.abs(w.S - ref.key) - ref.bound))
    assert np.all(w.S[1, ::4] == W0) and not ref.learned[1, 0]


@pytest.mark.parametrize("n_draw,n_neg,n_pos,k,C,resident", [
    (1, 1, 1, 4, 1000, False), (2, 1, 5, 16, 1000, True), (2, 2, 257, 80, 1000, False),
    (63, 1, 5, 16, 1000, False), (63, 62, 257, 4, 1000, True), (64, 63, 5, 80, 1000, False),
    (64, 1, 257, 16, 8, True), (64, 64, 5, 4, 8, False), (65, 1, 1, 16, 1000, True),
    (65, 64, 257, 16, 1000, False), (100, 99, 5, 80, 1000, True), (100, 100, 5, 4, 1000, False),
    (100, 1, 257, 16, 8, False), (1024, 1, 5, 16, 1000, False), (1024, 1023, 5, 4, 1000, True),
    (1024, 1024, 1, 80, 1000, False), (1024, 7, 257, 16, 8, True)])
def test_selection_equals_the_ranked_draws(gpu, n_draw, n_neg, n_pos, k, C, resident):
    w = world(k, C)
    pos = w.positives(n_pos)
    b, got = w.sample(pos, n_neg, n_draw, resident)
    want = w.want(pos, n_neg, n_draw)
    np.testing.assert_array_equal(got, want)
    assert (b.n_rows, b.group) == (n_pos * (1 + n_neg), 1 + n_neg)
    for i, u in enumerate(pos[0]):
        assert not np.isin(got[i], w.lists[u]).any()
    if C == 8 and n_draw >= 64 and n_neg < n_draw:  # duplicates and ties, decided by j
        draws = P.sample_negatives(9, pos[0], n_draw, w.ptr, w.rows, C)
        assert any(len(np.unique(draws[i])) < n_draw for i in range(n_pos))
    b.close()


@pytest.mark.parametrize("n_pos,n_neg", [(5, 4), (70, 65)])
def test_all_draws_kept_is_the_uniform_call(gpu, n_pos, n_neg):
    out = []
    for n_draw in (None, n_neg):
        w = World(16, 1000, seed=77)
        pos = w.positives(n_pos)
        b, got = w.sample(pos, n_neg, n_draw, seed=3)
        o = w.ctx.step_batch(b, 4, 0.05, 1e-3)
        tab = w.ctx.export_rows(np.arange(F))
        out.append((got.tobytes(), b.group, o.loss_sum, tab[0].tobytes(), tab[1].tobytes()))
        w.ctx.close()
    assert out[0] == out[1]


def test_batch_is_from_pairs_of_the_selection(gpu):
    w = world(16, 1000)
    pos = w.positives(37)
    b, got = w.sample(pos, 3, 70, pos_label=1.0, neg_label=-0.5)
    pc, pd, y = P.sampled_pairs(*pos, got, 1.0, -0.5)
    rb = w.ctx.batch_from_pairs(w.bu, w.bc, pc, pd, y)
    assert (b.n_rows, b.nnz) == (rb.n_rows, rb.nnz) == (37 * 4, P.concat_pairs(w.u, w.c, pc, pd, y).nnz)
    assert w.ctx.predict_batch(b, -5.0, 5.0).tobytes() == w.ctx.predict_batch(rb, -5.0, 5.0).tobytes()
    assert w.ctx.evaluate_batch(b, -5.0, 5.0) == w.ctx.evaluate_batch(rb, -5.0, 5.0)  # the labels


def test_snapshot_is_read_until_refreshed(gpu):
    w = World(16, 1000, seed=41)
    lib, pos = N.load(), w.positives(40)
    before, (b, first) = w.S, w.sample(pos, 2, 16)
    for t in (4, 5):
        w.step(t, 0.5)  # large enough that the two expected selections differ (asserted below)
    after = scores(w.ctx, w.bu, w.bc)  # (a ranking call between two sampling calls: its scratch is not the snapshot)
    stale, fresh = w.want(pos, 2, 16, S=before), w.want(pos, 2, 16, S=after)
    assert not np.array_equal(stale, fresh)
    np.testing.assert_array_equal(first, stale)
    np.testing.assert_array_equal(w.sample(pos, 2, 16, refresh=False, into=b)[1], stale)
    live = (lib.fm_device_bytes_live(), lib.fm_device_allocs_live())
    np.testing.assert_array_equal(w.sample(pos, 2, 16, refresh=False, into=b)[1], stale)
    np.testing.assert_array_equal(w.sample(pos, 2, 16, into=b)[1], fresh)
    np.testing.assert_array_equal(w.sample(pos, 2, 16, into=b)[1], fresh)
    assert (lib.fm_device_bytes_live(), lib.fm_device_allocs_live()) == live
    w.ctx.close()


def test_deterministic_and_independent_of_the_other_positives(gpu):
    w = world(16, 1000)
    pos = w.positives(9)
    for n_draw in (16, 200):
        b, a = w.sample(pos, 3, n_draw)
        b2, again = w.sample(pos, 3, n_draw)
        assert a.tobytes() == again.tobytes()
        assert w.ctx.predict_batch(b, -5.0, 5.0).tobytes() == w.ctx.predict_batch(b2, -5.0, 5.0).tobytes()
        other = (np.array([5, 0, pos[0][2]]), np.array([1, 2, pos[1][2]]))  # positive 2 again at index 2
        np.testing.assert_array_equal(w.sample(other, 3, n_draw)[1][2], a[2])


def test_refusals_change_nothing(gpu):
    from fm_spark_amd.engine import FMContext

    w = World(4, 8, seed=43)
    ctx, pos = w.ctx, w.positives(6)
    into = ctx.batch_sample_pairs(w.bu, w.bc, *pos, 2, exclude=w.lists, seed=1)
    state = lambda: (ctx.predict_batch(into, -5.0, 5.0).tobytes(), ctx.epoch)
    start = state()
    call = lambda n_neg, n_draw, refresh=True, bu=w.bu, ex=w.lists: ctx.batch_sample_pairs(
        bu, w.bc, *pos, n_neg, exclude=ex, n_draw=n_draw, refresh=refresh, into=into)
    other = ctx.batch(rows_host(R.take_rows(w.u, np.arange(6).repeat(2))))  # twelve context rows
    cases = [("n_draw", lambda: call(3, 2)), ("n_draw", lambda: call(2, 1025)), ("n_draw", lambda: call(-1, 4)),
             (r"\(-5\).*needs the snapshot", lambda: call(2, 4, False))]
    for message, f in cases:
        with pytest.raises(N.FMError, match=message):
            f()
        assert state() == start, message
    call(2, 4)
    start = state()
    with pytest.raises(N.FMError, match=r"\(-5\).*the snapshot is of 6 context and 8 candidate rows"):
        call(2, 4, False, bu=other, ex=None)
    assert state() == start
    ctx.close()
    for mode in ("sharded", "replicated"):
        group = FMContext(F, 4, parallel=mode, n_gpus=2, devices=[0, 0], transport="copy")
        gu, gc_ = group.batch(rows_host(w.u)), group.batch(rows_host(w.c))
        with pytest.raises(N.FMError, match="fm_batch_sample_pairs_hard needs both row sets whole"):
            group.batch_sample_pairs(gu, gc_, *pos, 2, n_draw=4)
        assert group.epoch == 0
        group.close()


def test_fit_interactions_equals_the_hand_driven_loop(gpu):
    """setNegativeCandidates(16), setNegativeRefreshEvery(3), BPR, 7 iterations on the planted problem's first
    contexts: the loss history of fitInteractions' documented loop driven by hand; None is today's fit."""
    from fm_spark_amd.data import splitmix64
    from fm_spark_amd.engine import FMContext
    from fm_spark_amd.linalg import SparseVector
    from fm_spark_amd.ml import DataFrame, FactorizationMachinesSGD

    p = P.planted()
    U, n, iters, n_neg, frac = 4, 96, 7, 3, 0.25
    rows = lambda first, m: (np.arange(m + 1, dtype=np.int64), np.arange(first, first + m, dtype=np.int32), np.ones(m))
    frame = lambda first, m: DataFrame({"features": [SparseVector(p.F, [first + r], [1.0]) for r in range(m)]})
    pc, pd = p.pos_ctx[:n], p.pos_cand[:n]
    inter = DataFrame({"context": [int(v) for v in pc], "candidate": [int(v) for v in pd]})
    est = lambda: (FactorizationMachinesSGD().setDimFactorization(P.K).setInitialSd(P.SD).setStepSize(2.0).setRegParam(1e-4)
                   .setMiniBatchFraction(frac).setMaxIter(iters).setNegativesPerPositive(n_neg).setSeed(3).setLoss("bpr"))
    fit = lambda e: e.fitInteractions(frame(0, U), frame(p.U, p.C), inter)._ctx.loss_history()
    hard = fit(est().setNegativeCandidates(16).setNegativeRefreshEvery(3))
    assert fit(est().setNegativeCandidates(None)).tobytes() == fit(est()).tobytes() != hard.tobytes()

    def loop(n_draw):
        ctx = FMContext(p.F, P.K, seed=3, init_sd=P.SD, w0=0.0, loss="bpr")
        bu, bc = ctx.batch(rows_host(rows(0, U))), ctx.batch(rows_host(rows(p.U, p.C)))
        ex = ctx.row_lists_from_pairs(pc, pd, U, p.C)
        ctx.init_from_batch(bu)
        ctx.init_from_batch(bc)
        seed0, bufs = int(splitmix64(np.uint64(3))), [None, None]

        def sample(t):
            take = P.batch_positives(n, 3, frac, t)
            bufs[t % 2] = ctx.batch_sample_pairs(bu, bc, pc[take], pd[take], n_neg, exclude=ex, seed=seed0 ^ t,
                                                 into=bufs[t % 2], n_draw=n_draw, refresh=(t - 1) % 3 == 0)
            bufs[t % 2].prepare()

        sample(1)
        for t in range(1, iters + 1):
            ctx.step_batch(bufs[t % 2], t, 2.0, 1e-4, sync=False)
            if t < iters:
                sample(t + 1)
        ctx.sync()
        return ctx.loss_history()

    assert loop(16).tobytes() == hard.tobytes()
    for bad in (0, 1025, True, 2.0):
        with pytest.raises(ValueError, match="negativeCandidates"):
            est().setNegativeCandidates(bad)
    with pytest.raises(ValueError, match="negativeRefreshEvery"):
        est().setNegativeRefreshEvery(0)
    assert (est().getNegativeCandidates(), est().getNegativeRefreshEvery()) == (None, 1)
