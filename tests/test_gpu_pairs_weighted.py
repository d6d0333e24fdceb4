"""GPU: popularity-weighted negatives -- fm_row_weights_create / _bind and fm_batch_sample_pairs_weighted
(include/fm_hip.h) against tests/pairs_weighted_ref.py's statement of the draw contract, exactly.

The shapes are the kernels' edges (fm_weights.hip): the cdf search's LDS pivot table holds every
ceil(C / 1024)-th entry, so C = 1023, 1024, 1025 and 4097 sit around its stride 1 -> 2 and a stride of 5;
lists of up to kBindShort = 64 rows are scanned by 16-lane teams and longer ones by a block in tiles of
kBindTile = 1024 rows, so one call holds lists of 0, 1, 63, 64, 65, 255, 256, 257, 1025 and C - 1 rows."""

import functools

import numpy as np
import pytest

import pair_ref as P
import pairs_weighted_ref as W
import rank_ref as R
from fm_spark_amd import _native as N
from test_gpu_pairs import F, cand_rows, new_ctx, rows_host
from test_gpu_pairs_hard import scores

pytestmark = pytest.mark.gpu
LENS = [0, 1, 63, 64, 65, 255, 256, 257, 1025]


def make_weights(rng, C, kind):
    if kind == "ones":
        return np.ones(C, np.int64)
    if kind == "single":  # one row holds all the weight
        w = np.zeros(C, np.int64)
        w[C // 2] = 7
        return w
    if kind == "max":  # W = 2^32 - 1
        w = rng.integers(1, 2**32 // C, C) if C > 1 else np.zeros(1, np.int64)
        w[C // 2] += 2**32 - 1 - w.sum()
        return w
    w = rng.integers(1, 10, C)  # "edge_zeros": zeros at the first and the last row
    w[[0, C - 1]] = 0
    w[C // 3] = 1000
    return w


class World:
    """C candidate rows under `kind` weights; one context per list: LENS rows (at most C - 1) drawn around a
    kept row of non-zero weight, then a list that excludes the heaviest row and one that leaves the kept row
    alone."""

    def __init__(self, C, kind):
        rng = np.random.default_rng(C)
        self.C, self.weight = C, make_weights(rng, C, kind)
        heavy = int(np.argmax(self.weight))
        live = np.flatnonzero(self.weight)
        self.keep = int(live[live != heavy][0]) if len(live) > 1 else heavy
        pool = np.delete(np.arange(C), self.keep)
        self.lists = [np.sort(rng.choice(pool, min(n, C - 1), replace=False)) for n in LENS]
        if heavy != self.keep:
            self.lists.append(np.array([heavy]))
        self.lists.append(pool)
        self.U = len(self.lists)
        self.ptr = np.concatenate([[0], np.cumsum([len(x) for x in self.lists])]).astype(np.int64)
        self.rows = np.concatenate(self.lists).astype(np.int32)
        self.u, self.c = R.make_rows(rng, rng.integers(0, 6, self.U), 100), cand_rows(rng, np.arange(C) % 4)
        self.ctx = new_ctx()
        self.bu, self.bc = self.ctx.batch(rows_host(self.u)), self.ctx.batch(rows_host(self.c))
        self.resident = self.ctx.row_lists(self.lists, C)
        self.rw = self.ctx.row_weights(self.weight).bind(self.resident)
        self.pos = (np.concatenate([np.arange(self.U), rng.integers(0, self.U, 40 - self.U)]), rng.integers(0, C, 40))

    def sample(self, n_neg, excl=True, pos=None, seed=9, **kw):
        pos = self.pos if pos is None else pos
        return self.ctx.batch_sample_pairs(self.bu, self.bc, *pos, n_neg, exclude=self.resident if excl else None, seed=seed,
                                           want_sampled=True, weights=self.rw, **kw)

    def want(self, n_draw, excl=True, pos=None, seed=9):
        pos_ctx = (self.pos if pos is None else pos)[0]
        return W.weighted_negatives(seed, pos_ctx, n_draw, *((self.ptr, self.rows) if excl else (None, None)), self.weight)


world = functools.lru_cache(maxsize=None)(World)
CASES = [(C, kind) for C in (1, 2) for kind in ("ones", "single", "max")] + \
        [(C, kind) for C in (1023, 1024, 1025, 4097) for kind in ("ones", "edge_zeros", "single", "max")]


@pytest.mark.parametrize("C,kind", CASES)
def test_draws_and_batch_equal_the_reference(gpu, C, kind):
    w = world(C, kind)
    assert w.rw.total == int(w.weight.sum()) and w.rw.n_candidates == C
    for n_neg in (0, 1, 4):
        for excl in (True, False):
            b, got = w.sample(n_neg, excl, pos_label=1.0, neg_label=-0.5)
            want = w.want(n_neg, excl)
            np.testing.assert_array_equal(got, want)
            assert np.all(w.weight[got] > 0)
            if excl:
                assert not any(np.isin(got[i], w.lists[u]).any() for i, u in enumerate(w.pos[0]))
                assert np.all(got[w.pos[0] == w.U - 1] == w.keep)  # exactly one eligible row
            rb = w.ctx.batch_from_pairs(w.bu, w.bc, *P.sampled_pairs(*w.pos, want, 1.0, -0.5))
            assert (b.n_rows, b.nnz, b.group) == (rb.n_rows, rb.nnz, 1 + n_neg if n_neg else 0)
            assert w.ctx.predict_batch(b, -5.0, 5.0).tobytes() == w.ctx.predict_batch(rb, -5.0, 5.0).tobytes()
            assert w.ctx.evaluate_batch(b, -5.0, 5.0) == w.ctx.evaluate_batch(rb, -5.0, 5.0)  # the labels
    # equal calls give equal bytes; (seed, i, j) decides a draw whatever n_pos is
    assert w.sample(4)[1].tobytes() == w.sample(4)[1].tobytes()
    prefix = (w.pos[0][:7], w.pos[1][:7])
    np.testing.assert_array_equal(w.sample(4, pos=prefix)[1], w.want(4)[:7])


@pytest.mark.parametrize("C", [1024, 4097])
def test_unit_weights_are_the_uniform_calls(gpu, C):
    w = world(C, "ones")
    for n_neg, n_draw in ((4, None), (3, 70), (2, 16)):
        b, got = w.sample(n_neg, n_draw=n_draw)
        ub, uni = w.ctx.batch_sample_pairs(w.bu, w.bc, *w.pos, n_neg, exclude=w.resident, seed=9, want_sampled=True,
                                           n_draw=n_draw)
        assert got.tobytes() == uni.tobytes()
        assert w.ctx.predict_batch(b, -5.0, 5.0).tobytes() == w.ctx.predict_batch(ub, -5.0, 5.0).tobytes()


@pytest.mark.parametrize("C,kind,n_draw,n_neg", [(1023, "edge_zeros", 16, 3), (1024, "max", 100, 5), (1023, "single", 64, 63)])
def test_selection_keeps_the_best_scored_weighted_draws(gpu, C, kind, n_draw, n_neg):
    """tests/test_gpu_pairs_hard.py's yardstick with the weighted draws: the first n_neg under (rank_batch's own
    score descending, j ascending), in ascending j."""
    w = world(C, kind)
    S = scores(w.ctx, w.bu, w.bc)
    draws = w.want(n_draw)
    key = S[w.pos[0][:, None], draws]
    keep = np.array([np.sort(np.lexsort((np.arange(n_draw), -key[i]))[:n_neg]) for i in range(len(draws))])
    b, got = w.sample(n_neg, n_draw=n_draw)
    np.testing.assert_array_equal(got, np.take_along_axis(draws, keep, axis=1))
    assert (b.n_rows, b.group) == (40 * (1 + n_neg), 1 + n_neg)


def test_refusals_change_nothing(gpu):
    from fm_spark_amd.engine import FMContext

    w = World(1025, "single")
    ctx, lib = w.ctx, N.load()
    into, _ = w.sample(2)
    state = lambda: (ctx.predict_batch(into, -5.0, 5.0).tobytes(), ctx.epoch, lib.fm_device_allocs_live())
    start = state()
    other_c = ctx.row_weights(np.ones(1024, np.int64))
    holds_it = ctx.row_lists([[w.C // 2]] + [[]] * (w.U - 1), w.C)  # context 0 excludes the only weighted row
    call = lambda rw, ex: ctx.batch_sample_pairs(w.bu, w.bc, *w.pos, 2, exclude=ex, weights=rw, into=into)
    unbound = ctx.row_weights(w.weight).bind(holds_it)
    start = state()
    cases = [("W = 0", lambda: ctx.row_weights(np.zeros(5, np.int64))),
             ("W = 4294967296", lambda: ctx.row_weights(np.array([2**31, 2**31]))),
             ("weights of 1024 candidate rows for candidates of 1025", lambda: call(other_c, None)),
             ("context 0 .positive 0. has no eligible candidate row", lambda: call(unbound, holds_it)),
             ("not bound to these exclude lists", lambda: call(w.rw, holds_it)),
             ("n_draw", lambda: ctx.batch_sample_pairs(w.bu, w.bc, *w.pos, 3, weights=w.rw, n_draw=2, into=into))]
    for message, f in cases:
        with pytest.raises(N.FMError, match=r"\(-1\).*" + message):
            f()
        assert state() == start, message
    ctx.close()
    group = FMContext(F, 4, parallel="sharded", n_gpus=2, devices=[0, 0], transport="copy")
    with pytest.raises(N.FMError, match=r"\(-1\).*fm_row_weights_create needs a context of one device"):
        group.row_weights(np.ones(8, np.int64))
    group.close()


def test_live_allocations_are_steady_and_return(gpu):
    w, lib = World(1025, "edge_zeros"), N.load()
    live = lambda: (lib.fm_device_bytes_live(), lib.fm_device_allocs_live())
    w.sample(4)[0].close()  # the context's pair scratch has grown to this call
    start = live()
    rw = w.ctx.row_weights(w.weight).bind(w.resident)
    into = w.ctx.batch_sample_pairs(w.bu, w.bc, *w.pos, 4, exclude=w.resident, weights=rw)
    after_one = live()
    w.ctx.batch_sample_pairs(w.bu, w.bc, *w.pos, 4, exclude=w.resident, weights=rw, into=into)
    rw.bind(w.resident)
    assert live() == after_one
    into.close()
    rw.close()
    assert live() == start
    w.ctx.close()


def test_fit_interactions_with_popularity_negatives(gpu):
    """fitInteractions("popularity") on the planted problem's first contexts equals its documented loop driven by
    hand, whose first batch's negatives are the reference's for popularity_weights' rule restated here."""
    from fm_spark_amd.data import splitmix64
    from fm_spark_amd.engine import FMContext
    from fm_spark_amd.linalg import SparseVector
    from fm_spark_amd.ml import DataFrame, FactorizationMachinesSGD

    p = P.planted()
    U, n, iters, n_neg, frac, power = 4, 96, 5, 3, 0.25, 0.75
    rows = lambda first, m: (np.arange(m + 1, dtype=np.int64), np.arange(first, first + m, dtype=np.int32), np.ones(m))
    frame = lambda first, m: DataFrame({"features": [SparseVector(p.F, [first + r], [1.0]) for r in range(m)]})
    pc, pd = p.pos_ctx[:n], p.pos_cand[:n] // 4 * 4  # repeats: some rows are popular
    inter = DataFrame({"context": [int(v) for v in pc], "candidate": [int(v) for v in pd]})
    est = (FactorizationMachinesSGD().setDimFactorization(P.K).setInitialSd(P.SD).setStepSize(2.0).setRegParam(1e-4)
           .setMiniBatchFraction(frac).setMaxIter(iters).setNegativesPerPositive(n_neg).setSeed(3).setLoss("bpr"))
    assert (est.getNegativeSampling(), est.getNegativePopularityPower()) == ("uniform", 0.75)
    uniform = est.fitInteractions(frame(0, U), frame(p.U, p.C), inter)._ctx.loss_history()
    fitted = est.setNegativeSampling("popularity").fitInteractions(frame(0, U), frame(p.U, p.C), inter)._ctx.loss_history()
    assert len(fitted) == iters and fitted.tobytes() != uniform.tobytes()
    raw = (np.bincount(pd, minlength=p.C) + 1.0) ** power
    weight = np.maximum(1, np.floor(min(2**20, (2**32 - 1) // p.C) * raw / raw.max())).astype(np.int64)
    lists = [np.unique(pd[pc == u]) for u in range(U)]
    ptr, flat = np.concatenate([[0], np.cumsum([len(x) for x in lists])]), np.concatenate(lists)
    ctx = FMContext(p.F, P.K, seed=3, init_sd=P.SD, w0=0.0, loss="bpr")
    bu, bc = ctx.batch(rows_host(rows(0, U))), ctx.batch(rows_host(rows(p.U, p.C)))
    ex = ctx.row_lists_from_pairs(pc, pd, U, p.C)
    rw = ctx.row_weights(weight)
    ctx.init_from_batch(bu)
    ctx.init_from_batch(bc)
    seed0, bufs = int(splitmix64(np.uint64(3))), [None, None]

    def sample(t):
        take = P.batch_positives(n, 3, frac, t)
        bufs[t % 2], got = ctx.batch_sample_pairs(bu, bc, pc[take], pd[take], n_neg, exclude=ex, seed=seed0 ^ t,
                                                  into=bufs[t % 2], weights=rw, want_sampled=True)
        np.testing.assert_array_equal(got, W.weighted_negatives(seed0 ^ t, pc[take], n_neg, ptr, flat, weight))
        bufs[t % 2].prepare()

    sample(1)
    for t in range(1, iters + 1):
        ctx.step_batch(bufs[t % 2], t, 2.0, 1e-4, sync=False)
        if t < iters:
            sample(t + 1)
    ctx.sync()
    assert ctx.loss_history().tobytes() == fitted.tobytes()
    with pytest.raises(ValueError, match="negativeSampling"):
        est.setNegativeSampling("unigram")
