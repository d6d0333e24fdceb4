"""GPU: per-context row lists resident on the device (fm_lists_create / fm_lists_from_pairs) and the calls
that read them (fm_rank_batch_select_lists, fm_rank_positions_batch_lists, fm_batch_sample_pairs_lists).

Every comparison is exact.  A builder's export must be tests/row_lists_ref.py's (ptr, rows) byte for byte,
whatever the order of the pairs; a _lists call's outputs must be the host-list call's with the same lists.

The builder's constants (fm_lists.hip, fm_pairs.hip's scan, fm_sort.hip) whose edges the shapes sit on are
written out below the imports."""

import ctypes as C
import gc
import math

import numpy as np
import pytest

import row_lists_ref as L
from fm_spark_amd import _native as N
from problems import f32
from rank_ref import make_rows

pytestmark = pytest.mark.gpu
INF = math.inf

K_BLOCK = 256            # kBlock: threads per block of k_lists_flag / k_lists_compact (a pair each) and k_lists_ptr (an offset each)
K_SCAN_CHUNK = 256       # kPairChunk: flags per chunk of the scan
K_ROUND_CHUNKS = 1024    # kPairScanNT * kPairScanPer: chunks the one-block scan of the chunk totals takes per round
K_SORT_TILE = 4096       # kTile: keys per tile of the radix sort
ROUND = K_SCAN_CHUNK * K_ROUND_CHUNKS  # 262 144 pairs: one round

F, K = 200, 16           # context ids in [0, 100), candidate ids in [100, 200)
ALL, ONLY, EXCEPT = N.FM_RANK_SELECT_ALL, N.FM_RANK_SELECT_ONLY, N.FM_RANK_SELECT_EXCEPT


def live():
    lib = N.load()
    return lib.fm_device_bytes_live(), lib.fm_device_allocs_live()


def rows_host(rows):
    rp, col, val = rows
    return N.CSRHost(rp, col, val, np.zeros(len(rp) - 1))


def new_ctx(**kw):
    from fm_spark_amd.engine import FMContext

    rng = np.random.default_rng(1)
    ctx = FMContext(F, K, **kw)
    ctx.load_tables(np.arange(F, dtype=np.int32), f32(0.3 * rng.standard_normal(F)), f32(0.3 * rng.standard_normal((F, K))))
    return ctx


@pytest.fixture(scope="module")
def ctx(gpu):
    c = new_ctx()
    yield c
    c.close()


def same_bytes(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() and x.dtype == y.dtype for x, y in zip(a, b))


# ------------------------------------------------------------------------------ 1. fm_lists_from_pairs
def _random_pairs(seed, n, U, Cn):
    rng = np.random.default_rng(seed)
    return rng.integers(0, U, n), rng.integers(0, Cn, n)


def _shapes():
    """name -> (pair_ctx, pair_cand, U, C)"""
    out = {}
    for n in (0, 1, 2, K_BLOCK - 1, K_BLOCK, K_BLOCK + 1, K_SORT_TILE - 1, K_SORT_TILE, K_SORT_TILE + 1):
        out[f"n={n}"] = (*_random_pairs(n, n, 300, 211), 300, 211)  # repeats once n passes a few hundred
    for n in (ROUND - 1, ROUND, ROUND + 1):  # the scan's second round starts past ROUND flags
        out[f"n={n}"] = (*_random_pairs(n, n, 307, 523), 307, 523)  # 160 441 distinct pairs at the most: repeats
    for U in (K_BLOCK - 2, K_BLOCK - 1, K_BLOCK):  # U + 1 offsets = kBlock - 1, kBlock, kBlock + 1 threads of k_lists_ptr
        out[f"U={U}"] = (*_random_pairs(U, 700, U, 40), U, 40)
    out["all pairs equal"] = (np.full(1000, 17), np.full(1000, 123), 300, 211)
    for name, u in (("first", 0), ("last", 299)):
        rng = np.random.default_rng(5)
        out[f"one context, every row: the {name}"] = (np.full(3 * 211, u), rng.permutation(np.tile(np.arange(211), 3)), 300, 211)
    rng = np.random.default_rng(6)  # empty contexts at the front, at the back and for more than a block in the middle
    out["runs of empty contexts"] = (rng.choice([0, 600, 999], 900), rng.integers(0, 50, 900), 1000, 50)
    out["empty front and back"] = (rng.integers(400, 600, 900), rng.integers(0, 50, 900), 1000, 50)
    out["U=1, C=70000"] = (np.zeros(5000, np.int64), rng.integers(0, 70_000, 5000), 1, 70_000)  # 17-bit keys a side
    out["U=70000, C=3"] = (rng.integers(0, 70_000, 5000), rng.integers(0, 3, 5000), 70_000, 3)
    out["U=70000, C=3, one pair at each end"] = (np.array([69_999, 0]), np.array([2, 0]), 70_000, 3)
    return out


SHAPES = _shapes()


@pytest.mark.parametrize("name", list(SHAPES))
def test_from_pairs_export_is_the_reference(ctx, name):
    pc, pd, U, Cn = SHAPES[name]
    ptr, rows = L.lists_from_pairs(pc, pd, U)
    rl = ctx.row_lists_from_pairs(pc, pd, U, Cn)
    got = rl.export()
    assert (rl.n_contexts, rl.n_candidates, rl.total) == (U, Cn, int(ptr[-1]))
    assert rl.longest == (int(np.diff(ptr).max()) if U else 0)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32
    assert got[0].tobytes() == ptr.tobytes() and got[1].tobytes() == rows.tobytes()
    rl.close()


@pytest.mark.parametrize("n,U,Cn", [(K_SORT_TILE + 1, 300, 211), (3000, 1, 70_000), (3000, 70_000, 3)])
def test_from_pairs_any_order_and_twice_equal_bytes(ctx, n, U, Cn):
    pc, pd = _random_pairs(n + U, n, U, Cn)
    pc[: n // 4], pd[: n // 4] = pc[n // 4: 2 * (n // 4)], pd[n // 4: 2 * (n // 4)]  # repeats
    want = L.lists_from_pairs(pc, pd, U)
    order = np.lexsort((pd, pc))
    for perm in (order, order[::-1], np.random.default_rng(9).permutation(n), np.arange(n), np.arange(n)):
        rl = ctx.row_lists_from_pairs(pc[perm], pd[perm], U, Cn)
        assert same_bytes(rl.export(), want)
        rl.close()


def test_from_pairs_refusals(ctx):
    lib = N.load()
    before = live()

    def call(pc, pd, U=5, Cn=7, n=None):
        pc, pd = np.ascontiguousarray(pc, np.int32), np.ascontiguousarray(pd, np.int32)
        h = C.c_void_p(0x5EED)
        rc = lib.fm_lists_from_pairs(ctx.handle, U, Cn, N.ptr(pc, C.c_int32), N.ptr(pd, C.c_int32), len(pc) if n is None else n,
                                     C.byref(h))
        assert h.value == 0x5EED and live() == before
        N.check(rc, "fm_lists_from_pairs")

    for message, args in [(r"pair_ctx index out of \[0, U = 5\)", ([0, 5], [0, 0])),
                          (r"pair_ctx index out of \[0, U = 5\)", ([-1, 1], [0, 9])),  # both lists wrong: pair_ctx is named
                          (r"pair_cand index out of \[0, C = 7\)", ([0, 4], [7, 0])),
                          (r"pair_cand index out of \[0, C = 7\)", ([0, 4], [0, -1])),
                          ("n out of range", ([0], [0], 5, 7, -1)),
                          ("n out of range", ([0], [0], 5, 7, 2**31)),
                          (r"U and C must be in \[0, 2\^31\)", ([0], [0], 2**31, 7)),
                          (r"U and C must be in \[0, 2\^31\)", ([0], [0], 5, -1))]:
        with pytest.raises(N.FMError, match=message):
            call(*args)


# ---------------------------------------------------------------------------------- 2. fm_lists_create
def test_create_round_trips(ctx):
    rng = np.random.default_rng(11)
    Cn = 1100
    lists = [np.sort(rng.choice(Cn, n, replace=False)) for n in (0, 1, Cn, 1023, 1024, 1025, 0, 7)]
    rl = ctx.row_lists(lists, Cn)
    ptr, rows = rl.export()
    assert (rl.n_contexts, rl.n_candidates, rl.total, rl.longest) == (8, Cn, sum(len(x) for x in lists), Cn)
    assert np.array_equal(ptr, np.concatenate([[0], np.cumsum([len(x) for x in lists])]))
    assert rows.dtype == np.int32 and np.array_equal(rows, np.concatenate(lists))
    # duplicates and disorder are the Python layer's to remove, as for rank(only=)
    r2 = ctx.row_lists([[5, 3, 5], [], [2]], 6)
    assert same_bytes(r2.export(), (np.array([0, 2, 2, 3], np.int64), np.array([3, 5, 2], np.int32)))
    # contexts without a row, also over no candidate row
    for lists, n_cand in (([[]], 4), ([[], []], 0)):
        r3 = ctx.row_lists(lists, n_cand)
        assert (r3.n_contexts, r3.total, r3.longest) == (len(lists), 0, 0) and len(r3.export()[1]) == 0
        r3.close()
    rl.close(), r2.close()


def test_create_refuses_what_the_list_rules_refuse(ctx):
    lib = N.load()
    before = live()

    def call(ptr, rows, U, Cn=23):
        ptr = None if ptr is None else np.ascontiguousarray(ptr, np.int64)
        rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
        h = C.c_void_p(0x5EED)
        rc = lib.fm_lists_create(ctx.handle, U, Cn, None if ptr is None else N.ptr(ptr, C.c_int64),
                                 None if rows is None else N.ptr(rows, C.c_int32), C.byref(h))
        assert h.value == 0x5EED and live() == before
        N.check(rc, "fm_lists_create")

    cases = [
        (r"row lists: ptr\[0\] must be 0, got 1", ([1, 2], [0, 1], 1)),
        (r"row lists: ptr must be non-decreasing: ptr\[2\] < ptr\[1\]", ([0, 2, 1], [0, 1], 2)),
        (r"row lists: ptr\[1\] must be < 2\^31", ([0, 2**31], None, 1)),
        ("row lists: null rows with a list that is not empty", ([0, 1], None, 1)),
        (r"row lists: context 0, position 0: row 23 is out of range \[0, 23\)", ([0, 1, 1], [23], 2)),
        (r"row lists: context 1, position 0: row -1 is out of range \[0, 23\)", ([0, 1, 2], [4, -1], 2)),
        ("row lists: context 1, position 1: row 3 after row 5: a list must be strictly ascending", ([0, 0, 2], [5, 3], 2)),
        ("row lists: context 0, position 1: row 5 after row 5: a list must be strictly ascending", ([0, 2], [5, 5], 1)),
        ("row lists: null ptr", (None, [1], 1)),
        (r"row lists: U and C must be in \[0, 2\^31\)", ([0], None, -1)),
        (r"row lists: U and C must be in \[0, 2\^31\)", ([0, 0], None, 1, 2**31)),
    ]
    for message, args in cases:
        with pytest.raises(N.FMError, match=message):
            call(*args)
    # a list may end at one context and the next start with a smaller row
    ok = ctx.row_lists((np.array([0, 2, 4], np.int64), np.array([5, 9, 0, 3], np.int32)), 23)
    assert ok.total == 4
    ok.close()


# --------------------------------------------------------------------------------------- 3. consumers
U_, C_ = 70, 1100  # the 1024-row rank chunk is crossed


@pytest.fixture(scope="module")
def case(ctx):
    """70 contexts, 1100 candidate rows; lists of 0 .. C rows -- nothing, one row, a whole chunk and its
    neighbours, everything but one row (context 3), everything (context 4), and random ones; targets of 0 .. 6
    rows, some of them on their context's list."""
    rng = np.random.default_rng(31)
    u = make_rows(rng, rng.integers(0, 6, U_), 100)
    rp, col, val = make_rows(rng, 1 + np.arange(C_) % 4, 100)
    c = (rp, (col + 100).astype(np.int32), val)
    sizes = [0, 1, 1023, C_ - 1, C_, 1024, 1025] + rng.integers(0, 300, U_ - 7).tolist()
    lists = [np.sort(rng.choice(C_, n, replace=False)) for n in sizes]
    targets = []
    for x in range(U_):
        own = lists[x][: 2] if x % 3 == 0 else np.zeros(0, np.int64)  # excluded targets: -1 / NaN
        targets.append(np.unique(np.concatenate([own, rng.choice(C_, int(rng.integers(0, 5)), replace=False)])))
    bu, bc = ctx.batch(rows_host(u)), ctx.batch(rows_host(c))
    host = lambda ls: (np.concatenate([[0], np.cumsum([len(x) for x in ls])]).astype(np.int64), np.concatenate(ls).astype(np.int32))
    yield dict(u=u, c=c, bu=bu, bc=bc, lists=lists, targets=targets, lists_host=host(lists), targets_host=host(targets))
    bu.close(), bc.close()


def raw_rank(ctx, bu, bc, select, lists, n_top, resident):
    lib = N.load()
    idx, score = np.zeros(bu.n_rows * n_top, np.int32), np.zeros(bu.n_rows * n_top)
    out = (n_top, -5.0, 5.0, N.ptr(idx, C.c_int32), N.ptr(score, C.c_double))
    if resident:
        rc = lib.fm_rank_batch_select_lists(ctx.handle, bu.handle, bc.handle, select, None if lists is None else lists.handle, *out)
    else:
        pp, pr = (None, None) if lists is None else (N.ptr(lists[0], C.c_int64), N.ptr(lists[1], C.c_int32))
        rc = lib.fm_rank_batch_select(ctx.handle, bu.handle, bc.handle, select, pp, pr, *out)
    N.check(rc, "rank")
    return idx, score


def raw_positions(ctx, bu, bc, tgt, ex, resident, n):
    lib = N.load()
    position, score = np.full(max(n, 1), -7, np.int32), np.full(max(n, 1), -7.0)
    out = (-5.0, 5.0, N.ptr(position, C.c_int32), N.ptr(score, C.c_double))
    if resident:
        rc = lib.fm_rank_positions_batch_lists(ctx.handle, bu.handle, bc.handle, None if tgt is None else tgt.handle,
                                               None if ex is None else ex.handle, *out)
    else:
        ep, er = (None, None) if ex is None else (N.ptr(ex[0], C.c_int64), N.ptr(ex[1], C.c_int32))
        rc = lib.fm_rank_positions_batch(ctx.handle, bu.handle, bc.handle, N.ptr(tgt[0], C.c_int64), N.ptr(tgt[1], C.c_int32),
                                         ep, er, *out)
    N.check(rc, "positions")
    return position, score


def raw_sample(ctx, bu, bc, pc, pd, n_neg, ex, resident, seed, handle=None):
    """-> (batch handle, sampled); handle: the batch to refill"""
    lib = N.load()
    pc, pd = np.ascontiguousarray(pc, np.int32), np.ascontiguousarray(pd, np.int32)
    sampled = np.zeros(max(len(pc) * n_neg, 1), np.int32)
    h = handle if handle is not None else C.c_void_p()
    head = (ctx.handle, bu.handle, bc.handle, N.ptr(pc, C.c_int32), N.ptr(pd, C.c_int32), len(pc), n_neg)
    tail = (1.0, -0.5, seed, C.byref(h), N.ptr(sampled, C.c_int32))
    if resident:
        rc = lib.fm_batch_sample_pairs_lists(*head, None if ex is None else ex.handle, *tail)
    else:
        ep, er = (None, None) if ex is None else (N.ptr(ex[0], C.c_int64), N.ptr(ex[1], C.c_int32))
        rc = lib.fm_batch_sample_pairs(*head, ep, er, *tail)
    N.check(rc, "sample")
    return h, sampled


@pytest.mark.parametrize("select", [ONLY, EXCEPT])
@pytest.mark.parametrize("n_top", [1, 100, 1024])
def test_rank_with_resident_lists_is_the_host_call(ctx, case, select, n_top):
    rl = ctx.row_lists(case["lists"], C_)
    want = raw_rank(ctx, case["bu"], case["bc"], select, case["lists_host"], n_top, False)
    got = raw_rank(ctx, case["bu"], case["bc"], select, rl, n_top, True)
    assert same_bytes(got, want)
    idx = want[0].reshape(U_, n_top)
    if select == EXCEPT:
        assert np.all(idx[4] == -1) and idx[3, 0] >= 0 and np.all(idx[3, 1:] == -1)  # nothing / one row eligible
    else:
        assert np.all(idx[0] == -1) and idx[1, 0] == case["lists"][1][0]
    # the Python layer dispatches on the type
    kw = {"only": rl} if select == ONLY else {"exclude": rl}
    py = ctx.rank_batch(case["bu"], case["bc"], n_top, -5.0, 5.0, **kw)
    assert py[0].tobytes() == want[0].tobytes() and py[1].tobytes() == want[1].tobytes()
    rl.close()


def test_rank_all_ignores_the_lists(ctx, case):
    rl = ctx.row_lists(case["lists"], C_)
    want = raw_rank(ctx, case["bu"], case["bc"], ALL, None, 50, False)
    assert same_bytes(raw_rank(ctx, case["bu"], case["bc"], ALL, None, 50, True), want)
    assert same_bytes(raw_rank(ctx, case["bu"], case["bc"], ALL, rl, 50, True), want)
    rl.close()


@pytest.mark.parametrize("with_exclude", [False, True])
def test_positions_with_resident_lists_are_the_host_call(ctx, case, with_exclude):
    n = len(case["targets_host"][1])
    tgt = ctx.row_lists(case["targets"], C_)
    ex = ctx.row_lists(case["lists"], C_) if with_exclude else None
    want = raw_positions(ctx, case["bu"], case["bc"], case["targets_host"], case["lists_host"] if with_exclude else None, False, n)
    got = raw_positions(ctx, case["bu"], case["bc"], tgt, ex, True, n)
    assert same_bytes(got, want)
    if with_exclude:
        assert (want[0][:n] == -1).any() and np.isnan(want[1][:n][want[0][:n] == -1]).all()  # excluded targets
    else:
        assert (want[0][:n] >= 0).all()
    # the Python layer: resident, and one resident with one host list (made resident for the call)
    host_ex = case["lists"] if with_exclude else None
    ref = ctx.rank_positions_batch(case["bu"], case["bc"], case["targets"], -5.0, 5.0, exclude=host_ex)
    before = live()
    for t, e in ((tgt, ex), (tgt, host_ex), (case["targets"], ex)):
        if e is None and t is not tgt:
            continue
        assert same_bytes(ctx.rank_positions_batch(case["bu"], case["bc"], t, -5.0, 5.0, exclude=e), ref)
        assert live() == before
    assert same_bytes(ref[:2], case["targets_host"]) and ref[2].tobytes() == want[0][:n].tobytes()
    tgt.close()
    if ex is not None:
        ex.close()


def _positives(case, rng, n):
    """n positives of contexts other than 4, whose list holds every row"""
    pc = rng.choice(np.delete(np.arange(U_), 4), n)
    pc[:6] = [0, 1, 2, 3, 5, 6]  # no list, one row, a chunk less one, all but one row, a chunk, a chunk and one
    return pc, rng.integers(0, C_, n)


@pytest.mark.parametrize("n_pos,n_neg", [(300, 4), (51, 0), (0, 3)])
def test_sampled_batch_with_resident_lists_is_the_host_call(ctx, case, n_pos, n_neg):
    lib = N.load()
    pc, pd = _positives(case, np.random.default_rng(32), max(n_pos, 6))
    pc, pd = pc[:n_pos], pd[:n_pos]
    rl = ctx.row_lists(case["lists"], C_)
    other = new_ctx()
    ou, oc = other.batch(rows_host(case["u"])), other.batch(rows_host(case["c"]))
    from fm_spark_amd.engine import DeviceBatch

    for ex_host, ex_res in ((case["lists_host"], rl), (None, None)):
        hh, want = raw_sample(other, ou, oc, pc, pd, n_neg, ex_host, False, 77)
        hr, got = raw_sample(ctx, case["bu"], case["bc"], pc, pd, n_neg, ex_res, True, 77)
        assert got.tobytes() == want.tobytes()
        if ex_host is not None and n_pos and n_neg:
            s = got.reshape(n_pos, n_neg)
            assert np.all(s[3] == np.setdiff1d(np.arange(C_), case["lists"][3])[0])  # all but one row excluded
            assert not any(np.isin(s[i], case["lists"][pc[i]]).any() for i in range(n_pos))
        a, b = DeviceBatch(other, None), DeviceBatch(ctx, None)
        a.handle, b.handle = hh, hr
        for x, cx in ((a, other), (b, ctx)):
            x.n_rows, x.nnz = int(lib.fm_batch_rows(x.handle)), int(lib.fm_batch_nnz(x.handle))
        assert (a.n_rows, a.nnz) == (b.n_rows, b.nnz) and a.n_rows == n_pos * (1 + n_neg)
        assert ctx.predict_batch(b, -5.0, 5.0).tobytes() == other.predict_batch(a, -5.0, 5.0).tobytes()
        assert ctx.evaluate_batch(b, -5.0, 5.0) == other.evaluate_batch(a, -5.0, 5.0)  # the labels
        a.close(), b.close()
    # the Python layer, and a step: two fresh contexts, host lists in one and resident ones in the other
    ca, cb = new_ctx(), new_ctx()
    outs = []
    for cx, resident in ((ca, False), (cb, True)):
        xu, xc = cx.batch(rows_host(case["u"])), cx.batch(rows_host(case["c"]))
        ex = cx.row_lists(case["lists"], C_) if resident else case["lists"]
        b, s = cx.batch_sample_pairs(xu, xc, pc, pd, n_neg, exclude=ex, seed=5, want_sampled=True)
        b.prepare()
        o = cx.step_batch(b, 1, 0.3, 1e-3)
        outs.append((s.tobytes(), (o.loss_sum, o.n_rows, o.n_loss_rows, o.n_unique, o.executed), cx.export_tables()))
        if resident:
            ex.close()
    assert outs[0][:2] == outs[1][:2]
    assert same_bytes(outs[0][2], outs[1][2])
    for cx in (ca, cb, other):
        cx.close()
    rl.close()


# --------------------------------------------------------------------------------------- 4. refusals
def test_consumers_refuse_lists_that_do_not_fit(ctx, case):
    from fm_spark_amd.engine import FMContext

    bu, bc = case["bu"], case["bc"]
    rl = ctx.row_lists(case["lists"], C_)
    tgt = ctx.row_lists(case["targets"], C_)
    other = new_ctx()
    foreign = other.row_lists(case["lists"], C_)
    more_ctx = ctx.row_lists(case["lists"] + [[]], C_)
    more_cand = ctx.row_lists(case["lists"], C_ + 1)
    pc, pd = _positives(case, np.random.default_rng(33), 20)
    into, _ = raw_sample(ctx, bu, bc, pc, pd, 2, rl, True, 1)
    from fm_spark_amd.engine import DeviceBatch

    keep = DeviceBatch(ctx, None)
    keep.handle, keep.n_rows = into, 60
    pred = ctx.predict_batch(keep, -5.0, 5.0).tobytes()
    raw_rank(ctx, bu, bc, EXCEPT, rl, 10, True), raw_positions(ctx, bu, bc, tgt, rl, True, tgt.total)  # the scratch is sized
    before = live()
    n_t = tgt.total
    into_value = into.value

    def export_foreign():
        p = np.zeros(U_ + 1, np.int64)
        N.check(N.load().fm_lists_export(ctx.handle, foreign.handle, N.ptr(p, C.c_int64), None, 0), "fm_lists_export")

    sample = lambda ex, pos=(pc, pd): raw_sample(ctx, bu, bc, pos[0], pos[1], 2, ex, True, 1, handle=into)
    cases = [
        ("sel: the lists belong to another context", lambda: raw_rank(ctx, bu, bc, EXCEPT, foreign, 10, True)),
        ("sel: lists of 71 contexts for contexts of 70 rows", lambda: raw_rank(ctx, bu, bc, ONLY, more_ctx, 10, True)),
        ("sel: lists over 1101 candidate rows for candidates of 1100 rows", lambda: raw_rank(ctx, bu, bc, ONLY, more_cand, 10, True)),
        ("null sel with FM_RANK_SELECT_ONLY / _EXCEPT", lambda: raw_rank(ctx, bu, bc, ONLY, None, 10, True)),
        ("null sel with FM_RANK_SELECT_ONLY / _EXCEPT", lambda: raw_rank(ctx, bu, bc, EXCEPT, None, 10, True)),
        ("null tgt: fm_rank_positions needs the target lists", lambda: raw_positions(ctx, bu, bc, None, rl, True, n_t)),
        ("tgt: the lists belong to another context", lambda: raw_positions(ctx, bu, bc, foreign, rl, True, n_t)),
        ("excl: the lists belong to another context", lambda: raw_positions(ctx, bu, bc, tgt, foreign, True, n_t)),
        ("tgt: lists of 71 contexts", lambda: raw_positions(ctx, bu, bc, more_ctx, None, True, n_t)),
        ("excl: lists over 1101 candidate rows", lambda: raw_positions(ctx, bu, bc, tgt, more_cand, True, n_t)),
        ("excl: the lists belong to another context", lambda: sample(foreign)),
        ("excl: lists of 71 contexts", lambda: sample(more_ctx)),
        ("excl: lists over 1101 candidate rows", lambda: sample(more_cand)),
        ("context 4 .* no eligible candidate row", lambda: sample(rl, (np.array([0, 4]), np.array([1, 1])))),
        ("the lists belong to another context", export_foreign),
    ]
    for message, call in cases:
        with pytest.raises(N.FMError, match=message):
            call()
        assert live() == before, message
        assert into.value == into_value and ctx.predict_batch(keep, -5.0, 5.0).tobytes() == pred, message
    # the Python layer keeps host calls and resident lists apart
    with pytest.raises(ValueError, match="RowLists"):
        ctx.rank(rows_host(case["u"]), rows_host(case["c"]), 5, -5.0, 5.0, exclude=rl)
    with pytest.raises(ValueError, match="RowLists"):
        ctx.rank_positions(rows_host(case["u"]), rows_host(case["c"]), tgt, -5.0, 5.0)
    # a multi-GPU context makes no lists
    for mode in ("sharded", "replicated"):
        group = FMContext(F, K, parallel=mode, n_gpus=2, devices=[0, 0], transport="copy")
        at = live()
        with pytest.raises(N.FMError, match="fm_lists_create needs a context of one device"):
            group.row_lists(case["lists"], C_)
        with pytest.raises(N.FMError, match="fm_lists_from_pairs needs a context of one device"):
            group.row_lists_from_pairs(pc, pd, U_, C_)
        assert live() == at
        group.close()
    keep.close()
    for l in (rl, tgt, more_ctx, more_cand, foreign):
        l.close()
    other.close()


# --------------------------------------------------------------------------------------- 5. lifetime
def test_device_memory_is_steady_and_returns(gpu):
    gc.collect()
    start = live()
    ctx = new_ctx()
    rng = np.random.default_rng(41)
    U, Cn = 40, 300
    u = make_rows(rng, rng.integers(0, 5, U), 100)
    rp, col, val = make_rows(rng, 1 + np.arange(Cn) % 3, 100)
    bu, bc = ctx.batch(rows_host(u)), ctx.batch(rows_host((rp, (col + 100).astype(np.int32), val)))
    pc, pd = rng.integers(0, U, 2000), rng.integers(0, Cn // 2, 2000)
    base = live()
    # from_pairs leaves its two buffers and nothing else: ptr 8 (U + 1) bytes, rows 4 bytes a row
    rl = ctx.row_lists_from_pairs(pc, pd, U, Cn)
    assert live() == (base[0] + 8 * (U + 1) + 4 * rl.total, base[1] + 2)
    rl.close()
    assert live() == base
    empty = ctx.row_lists_from_pairs([], [], U, Cn)  # no rows: the smallest allocation, 16 bytes
    assert live() == (base[0] + 8 * (U + 1) + 16, base[1] + 2)
    empty.close()
    for _ in range(3):
        a, b = ctx.row_lists_from_pairs(pc, pd, U, Cn), ctx.row_lists(L.lists_from_pairs(pc, pd, U), Cn)
        assert same_bytes(a.export(), b.export())
        a.close(), b.close()
        assert live() == base
    # two equal calls of every consumer leave both counters equal
    rl = ctx.row_lists_from_pairs(pc, pd, U, Cn)
    tgt = ctx.row_lists([[int(x)] for x in rng.integers(0, Cn, U)], Cn)
    into, marks = None, []
    for _ in range(2):
        ctx.rank_batch(bu, bc, 10, -5.0, 5.0, exclude=rl)
        ctx.rank_batch(bu, bc, 10, -5.0, 5.0, only=rl)
        ctx.rank_positions_batch(bu, bc, tgt, -5.0, 5.0, exclude=rl)
        into = ctx.batch_sample_pairs(bu, bc, pc[:500], pd[:500], 4, exclude=rl, seed=3, into=into)
        ctx.sync()
        marks.append(live())
    assert marks[0] == marks[1]
    # lists may outlive their context
    for b in (into, bu, bc):
        b.close()
    ctx.close()
    assert live() == (8 * (U + 1) + 4 * rl.total + 8 * (U + 1) + 4 * U + start[0], 4 + start[1])
    rl.close(), tgt.close()
    assert live() == start
