"""GPU: exact rank positions (fm_rank_positions / fm_rank_positions_batch; k_rank_position in
fm_rank.hip) against the ranking calls themselves and the reference of tests/rank_position_ref.py.

Three kinds of check, the first two exact:
  slots      the defining property: a target with position p < n_top sits at top_index[u, p] of
             rank(exclude = the same lists, n_top) -- the unrestricted call without lists -- with
             top_score equal to its score bit for bit;
  counting   all rows as targets: each context's eligible targets hold a permutation of 0 .. n_eligible - 1,
             an excluded target -1 / NaN;
  interval   every position lies where the reference allows (an eligible row counts for certain only where
             its reference key beats the target's by more than the smaller of the two bounds of
             rank_ref.pair_ref, and possibly where it is within it).

The constants of fm_rank.hip whose edges the shapes sit on:
  kRankChunk = 1024         rows per chunk, bits per exclusion mask, targets per tile -> C in 1, 1023, 1024,
                            1025, 2049; target lists of 0, 1, 1023, 1024, 1025, 2049 rows;
  kRankTargetBlocks = 512   U = 1 with C = 3000 takes three splits of one chunk; U = 600 one split of three;
  kPosCtxTile = 65535       contexts of one launch (the grid's y extent; no split lists exist whose budget
                            would tile the contexts sooner): U = 65540 takes two launches, the second
                            reading the lists from tgt_ptr + 65535."""

import ctypes as C
import math

import numpy as np
import pytest

import rank_position_ref as P
import rank_ref as R
import rank_select_ref as S
from fm_spark_amd import _native as N
from fm_spark_amd.engine import FMContext
from test_gpu_rank import _small, cand_lens, csr, cut, loaded
from test_gpu_rank_select import edge_lists, live, problem

pytestmark = pytest.mark.gpu
INF = math.inf
F = 4096
CTX_TILE = 65535


def raw(ctx, contexts, candidates, tgt, excl=(None, None), lo=-INF, hi=INF):
    """The C-ABI as it is, without the Python layer's sorting: host rows (CSRHost) or batches; tgt / excl:
    (ptr, rows), each a sequence or None.  Returns (position, score) of len(tgt rows)."""
    lib = N.load()
    arrs = []
    for a, t in zip((*tgt, *excl), (np.int64, np.int32, np.int64, np.int32)):
        arrs.append(None if a is None else np.ascontiguousarray(a, t))
    ptrs = [None if a is None else N.ptr(a, c) for a, c in zip(arrs, (C.c_int64, C.c_int32, C.c_int64, C.c_int32))]
    n = 0 if arrs[1] is None else len(arrs[1])
    position = np.full(max(n, 1), -7, np.int32)
    score = np.full(max(n, 1), -7.0)
    out = (lo, hi, N.ptr(position, C.c_int32), N.ptr(score, C.c_double))
    if isinstance(contexts, N.CSRHost):
        rc = lib.fm_rank_positions(ctx.handle, C.byref(contexts.c), C.byref(candidates.c), *ptrs, *out)
    else:
        rc = lib.fm_rank_positions_batch(ctx.handle, contexts.handle, candidates.handle, *ptrs, *out)
    N.check(rc, "fm_rank_positions")
    return position[:n], score[:n]


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a) == len(b)


def split(ptr, a):
    return [a[ptr[u]:ptr[u + 1]] for u in range(len(ptr) - 1)]


def check_slots(ctx, cu, cc, Cn, got, lists, lo=-INF, hi=INF):
    """The defining property against the ranking call at n_top = min(C, 1024).  Returns the ranking."""
    ptr, rows, pos, score = got
    n_top = min(Cn, N.FM_RANK_MAX_TOP)
    kw = {} if lists is None else {"exclude": lists}
    idx, top = ctx.rank(cu, cc, n_top, lo, hi, **kw)
    seen = 0
    for u, (r, p, s) in enumerate(zip(split(ptr, rows), split(ptr, pos), split(ptr, score))):
        near = (p >= 0) & (p < n_top)
        assert np.array_equal(idx[u, p[near]], r[near]), u
        assert top[u, p[near]].tobytes() == np.ascontiguousarray(s[near]).tobytes(), u
        seen += int(near.sum())
    assert seen > 0 or len(rows) == 0 or np.all(pos < 0)
    return idx, top


def check_interval(ref, got, lists, targets_of=None, contexts=None):
    """Every position within the reference's interval; -1 / NaN exactly for the excluded targets."""
    ptr, rows, pos, score = got
    U, Cn = ref.key.shape
    elig = S.eligible_mask(S.EXCEPT if lists is not None else S.ALL, lists, U, Cn)
    want = ref.score(-INF, INF)
    for u in (range(U) if contexts is None else contexts):
        r, p, s = rows[ptr[u]:ptr[u + 1]], pos[ptr[u]:ptr[u + 1]], score[ptr[u]:ptr[u + 1]]
        ok = elig[u, r]
        assert np.all(p[~ok] == -1) and np.all(np.isnan(s[~ok])) and not np.isnan(s[ok]).any(), u
        if not len(r):
            continue
        pairs = targets_of[u] if targets_of is not None else P.Pairs(ref, u, r)
        assert np.array_equal(pairs.targets, r)
        a, b = pairs.interval(elig[u])
        assert np.all(a[ok] <= p[ok]) and np.all(p[ok] <= b[ok]), (u, r[ok][(p[ok] < a[ok]) | (p[ok] > b[ok])])
        err = np.abs(s[ok] - want[u, r[ok]])
        assert np.all(err <= ref.bound[u, r[ok]]), u


def check_counting(got, lists, U, Cn):
    """All rows as targets: the eligible ones hold a permutation of 0 .. n_eligible - 1."""
    ptr, rows, pos, score = got
    elig = S.eligible_mask(S.EXCEPT if lists is not None else S.ALL, lists, U, Cn)
    for u in range(U):
        assert np.array_equal(rows[ptr[u]:ptr[u + 1]], np.arange(Cn))
        p = pos[ptr[u]:ptr[u + 1]]
        assert np.array_equal(np.sort(p[elig[u]]), np.arange(int(elig[u].sum()))), u
        assert np.all(p[~elig[u]] == -1), u


# ------------------------------------------------------------------------------ 1. chunk edges
@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("Cn", [1, 1023, 1024, 1025, 2049])
def test_chunk_edges_with_all_rows_as_targets(gpu, Cn, k):
    w, V, present, ctxs, cands, w0, ref = problem(k, 3, 2049, 200 + k)
    ref = cut(ref, Cn)
    ctx = loaded(w, V, present, w0=w0)
    cu, cc = csr(ctxs), csr(R.take_rows(cands, np.arange(Cn)))
    every = [np.arange(Cn)] * 3
    pairs = [P.Pairs(ref, u, every[u]) for u in range(3)]
    top = ctx.rank(cu, cc, min(Cn, 100), -INF, INF)[0]
    for name, lists in [("none", None), *edge_lists(Cn, top).items()]:
        got = ctx.rank_positions(cu, cc, every, -INF, INF, exclude=lists)
        assert got[0].tolist() == [0, Cn, 2 * Cn, 3 * Cn] and got[2].dtype == np.int32, name
        check_counting(got, lists, 3, Cn)
        idx, top_score = check_slots(ctx, cu, cc, Cn, got, lists)
        check_interval(ref, got, lists, targets_of=pairs)
        if Cn <= 1024:  # the ranking call returns every row: the positions are its order's inverse, the scores its scores
            for u, (p, s) in enumerate(zip(split(got[0], got[2]), split(got[0], got[3]))):
                m = int((p >= 0).sum())
                order = np.argsort(np.where(p >= 0, p, Cn), kind="stable")[:m]
                assert np.array_equal(idx[u, :m], order) and np.all(idx[u, m:] == -1), (name, u)
                assert top_score[u, :m].tobytes() == s[order].tobytes(), (name, u)
    ctx.close()


# ---------------------------------------------------------------------------- 2. split shapes
def test_one_context_takes_several_splits(gpu):
    w, V, present, ctxs, cands, w0, ref = problem(5, 1, 3000, 301)
    rng = np.random.default_rng(31)
    ctx = loaded(w, V, present, w0=w0)
    cu, cc = csr(ctxs), csr(cands)
    every = [np.arange(3000)]
    pairs = [P.Pairs(ref, 0, every[0])]
    for lists in (None, [np.sort(rng.choice(3000, 300, replace=False))], [np.array([1023, 1024, 2047, 2048, 2999])]):
        got = ctx.rank_positions(cu, cc, every, -INF, INF, exclude=lists)
        check_counting(got, lists, 1, 3000)
        check_slots(ctx, cu, cc, 3000, got, lists)
        check_interval(ref, got, lists, targets_of=pairs)
    ctx.close()


def test_many_contexts_take_one_split_of_several_chunks(gpu):
    U, Cn = 600, 2049
    w, V, present, ctxs, cands, w0, ref = problem(1, U, Cn, 302, centred=False)
    rng = np.random.default_rng(32)
    targets = [np.sort(rng.choice(Cn, n, replace=False)) for n in rng.integers(0, 8, U)]
    targets[7] = np.array([0, 1023, 1024, 2047, 2048])
    lists = [np.sort(rng.choice(Cn, n, replace=False)) for n in rng.integers(0, 60, U)]
    lists[7] = np.array([1, 1024, 2048])
    ctx = loaded(w, V, present)
    cu, cc = csr(ctxs), csr(cands)
    got = ctx.rank_positions(cu, cc, targets, -INF, INF, exclude=lists)
    check_interval(ref, got, lists)
    check_slots(ctx, cu, cc, Cn, got, lists)
    assert got[2][got[0][7]:got[0][8]][[2, 4]].tolist() == [-1, -1]  # rows 1024 and 2048 are on its own exclude list
    for u in (0, 7, 599):  # each context ranked alone: the joint call's bytes
        one = ctx.rank_positions(csr(R.take_rows(ctxs, [u])), cc, [targets[u]], -INF, INF, exclude=[lists[u]])
        assert same(one[1:], [a[got[0][u]:got[0][u + 1]] for a in got[1:]]), u
    ctx.close()


def test_context_tiles_read_their_own_lists(gpu):
    """U = kPosCtxTile + 5: two launches, the second from tgt_ptr + 65535 and excl_ptr + 65535."""
    U, Cn, k = CTX_TILE + 5, 7, 2
    rng = np.random.default_rng(33)
    w, V, present = R.make_table(rng, F, k)
    ctxs, cands = R.make_rows(rng, rng.choice([0, 1, 3], U), F), R.make_rows(rng, np.full(Cn, 3), F)
    ref = R.pair_ref(w, V, present, 0.0, ctxs, cands)
    n_t, n_x = np.arange(U) % 3, (np.arange(U) // 3) % 2  # 0, 1 or 2 targets, 0 or 1 excluded rows: ragged offsets
    tgt_ptr = np.concatenate([[0], np.cumsum(n_t)])
    tgt_rows = np.concatenate([np.sort(rng.choice(Cn, n, replace=False)) for n in n_t]).astype(np.int32)
    ex_ptr = np.concatenate([[0], np.cumsum(n_x)])
    ex_rows = rng.integers(0, Cn, int(n_x.sum())).astype(np.int32)
    ctx = loaded(w, V, present)
    cu, cc = csr(ctxs), csr(cands)
    pos, score = raw(ctx, cu, cc, (tgt_ptr, tgt_rows), (ex_ptr, ex_rows))
    # the reference, vectorised over all targets: exact wherever no other key lies within the bound
    us = np.repeat(np.arange(U), n_t)
    elig = np.ones((U, Cn), bool)
    elig[np.repeat(np.arange(U), n_x), ex_rows] = False
    kt, bt = ref.key[us, tgt_rows], ref.bound[us, tgt_rows]
    diff = ref.key[us] - kt[:, None]
    mb = np.minimum(ref.bound[us], bt[:, None])
    other = np.arange(Cn)[None, :] != tgt_rows[:, None]
    lo_ = np.sum((diff > mb) & other & elig[us], axis=1)
    hi_ = lo_ + np.sum((np.abs(diff) <= mb) & other & elig[us], axis=1)
    ok = elig[us, tgt_rows]
    assert np.all(pos[~ok] == -1) and np.all(np.isnan(score[~ok])) and (~ok).sum() > 100
    assert np.all(lo_[ok] <= pos[ok]) and np.all(pos[ok] <= hi_[ok])
    assert np.mean(lo_ == hi_) > 0.5 and (ok & (us >= CTX_TILE)).sum() >= 2
    assert np.all(np.abs(score[ok] - kt[ok]) <= bt[ok])
    for u in (CTX_TILE - 1, CTX_TILE + 1, CTX_TILE + 2, CTX_TILE + 4):  # either side of the launch edge, alone: the same bytes
        one = raw(ctx, csr(R.take_rows(ctxs, [u])), cc, ([0, n_t[u]], tgt_rows[tgt_ptr[u]:tgt_ptr[u + 1]]),
                  ([0, n_x[u]], ex_rows[ex_ptr[u]:ex_ptr[u + 1]]))
        assert same(one, (pos[tgt_ptr[u]:tgt_ptr[u + 1]], score[tgt_ptr[u]:tgt_ptr[u + 1]])), u
    ctx.close()


# ---------------------------------------------------------------------------- 3. target tiles
def test_target_tiles_of_every_length_in_one_call(gpu):
    U, Cn = 6, 2049
    w, V, present, ctxs, cands, w0, ref = problem(5, U, Cn, 303)
    rng = np.random.default_rng(34)
    lens = [0, 1, 1023, 1024, 1025, 2049]
    targets = [np.sort(rng.choice(Cn, n, replace=False)) for n in lens]
    pairs = [P.Pairs(ref, u, targets[u]) for u in range(U)]
    ctx = loaded(w, V, present, w0=w0)
    cu, cc = csr(ctxs), csr(cands)
    for lists in (None, [np.sort(rng.choice(Cn, 100, replace=False)) for _ in range(U)]):
        got = ctx.rank_positions(cu, cc, targets, -INF, INF, exclude=lists)
        assert np.diff(got[0]).tolist() == lens
        check_interval(ref, got, lists, targets_of=pairs)
        check_slots(ctx, cu, cc, Cn, got, lists)
        p = got[2][got[0][5]:]
        assert np.array_equal(np.sort(p[p >= 0]), np.arange(Cn - (0 if lists is None else 100)))
        for u in (1, 4):  # alone, the other contexts' tiles do not matter
            one = ctx.rank_positions(csr(R.take_rows(ctxs, [u])), cc, [targets[u]], -INF, INF,
                                     exclude=None if lists is None else [lists[u]])
            assert same(one[1:], [a[got[0][u]:got[0][u + 1]] for a in got[1:]]), u
    ctx.close()


# ------------------------------------------------------------------------------------ 4. ties
def test_copies_of_one_row_hold_consecutive_positions_in_row_order(gpu):
    rng = np.random.default_rng(22)
    w, V, present = R.make_table(rng, F, 17)
    ctxs = R.make_rows(rng, [200, 1, 40, 0], F)
    distinct = R.make_rows(rng, np.full(40, 13), F)
    content = rng.integers(0, 40, 2300)  # candidate row -> which distinct row it copies
    cands = R.take_rows(distinct, content)
    lists = [np.sort(rng.choice(2300, n, replace=False)) for n in (700, 1150, 1, 2299)]
    every = [np.arange(2300)] * 4
    ref = R.pair_ref(w, V, present, 0.0, ctxs, cands)
    ctx = loaded(w, V, present)
    cu, cc = csr(ctxs), csr(cands)
    for ex in (None, lists):
        got = ctx.rank_positions(cu, cc, every, -INF, INF, exclude=ex)
        check_counting(got, ex, 4, 2300)  # a permutation of the eligible count: an excluded copy is not counted
        check_slots(ctx, cu, cc, 2300, got, ex)
        check_interval(ref, got, ex)
        elig = S.eligible_mask(S.EXCEPT if ex is not None else S.ALL, ex, 4, 2300)
        groups = 0
        for u, (p, s) in enumerate(zip(split(got[0], got[2]), split(got[0], got[3]))):
            for d in range(40):
                at = np.flatnonzero(elig[u] & (content == d))  # the eligible copies, by ascending row
                if len(at) > 1:
                    groups += 1
                    assert np.array_equal(p[at], p[at[0]] + np.arange(len(at))), (u, d)
                    assert np.all(s[at] == s[at[0]])
        assert groups > 100
    ctx.close()


def test_w0_pairs_and_clamped_ties(gpu):
    rng = np.random.default_rng(31)
    Fm, k, w0 = 500, 5, 5.0
    w, V, present = R.make_table(rng, Fm, k, present_frac=0.6)
    absent = np.flatnonzero(~present)
    ctxs = list(R.make_rows(rng, [0, 3, 60, 2], Fm + 200))  # ids >= F among them
    ctxs[1][ctxs[0][1]:ctxs[0][2]] = absent[:3]            # context 1: absent ids only
    ctxs[1][ctxs[0][3]:ctxs[0][4]] = [Fm + 5, Fm + 100]    # context 3: ids beyond the table only
    ctxs = tuple(ctxs)
    cands = R.make_rows(rng, cand_lens(400), Fm + 200, scale=3.0)
    ref = R.pair_ref(w, V, present, w0, ctxs, cands)
    assert (~ref.learned).sum() >= 3 * 133 and ref.learned[0].any()
    ctx = loaded(w, V, present, w0=w0)
    cu, cc = csr(ctxs), csr(cands)
    every = [np.arange(400)] * 4
    lists = [np.sort(rng.choice(400, 150, replace=False)) for _ in range(4)]
    for ex in (None, lists):
        elig = S.eligible_mask(S.EXCEPT if ex is not None else S.ALL, ex, 4, 400)
        free = ctx.rank_positions(cu, cc, every, -INF, INF, exclude=ex)
        check_counting(free, ex, 4, 400)
        check_slots(ctx, cu, cc, 400, free, ex)
        check_interval(ref, free, ex)
        clamped = ctx.rank_positions(cu, cc, every, 0.0, 1.0, exclude=ex)  # a clamp range that excludes w0
        assert np.array_equal(clamped[2], free[2])  # many scores tie at 0 and 1: the order stays the unclamped key's
        check_slots(ctx, cu, cc, 400, clamped, ex, 0.0, 1.0)
        for u in (0, 1, 3):  # nothing learned on the context's side: its w0 pairs tie, in row order
            p, s, sc = free[2][400 * u:400 * (u + 1)], free[3][400 * u:400 * (u + 1)], clamped[3][400 * u:400 * (u + 1)]
            at = np.flatnonzero(elig[u] & ~ref.learned[u])
            assert len(at) > 50 and np.array_equal(p[at], p[at[0]] + np.arange(len(at))), u
            assert np.all(s[at] == w0) and np.all(sc[at] == w0)  # unclamped, under the clamp too
            rest = elig[u] & ref.learned[u]
            assert np.all((sc[rest] >= 0.0) & (sc[rest] <= 1.0)) and (sc[rest] == 1.0).sum() > 1 and (sc[rest] == 0.0).sum() > 1
    ctx.close()


# ------------------------------------------------------------------------ 5. excluded targets
def test_an_excluded_target_gets_minus_one_and_changes_nothing_else(gpu):
    w, V, present, ctxs, cands, w0, ref = problem(5, 3, 2049, 205)
    Cn = 1100
    rng = np.random.default_rng(5)
    ctx = loaded(w, V, present, w0=w0)
    cu, cc = csr(ctxs), csr(R.take_rows(cands, np.arange(Cn)))
    lists = [np.sort(rng.choice(Cn, n, replace=False)) for n in (200, 0, 1099)]
    lists[0][[0, -1]] = [0, Cn - 1]
    lists[0] = np.unique(lists[0])
    keep = [np.setdiff1d(rng.choice(Cn, 30, replace=False), x) for x in lists]
    both = [np.union1d(a, x[::7]) for a, x in zip(keep, lists)]  # the same targets, and excluded rows among them
    a = ctx.rank_positions(cu, cc, keep, -INF, INF, exclude=lists)
    b = ctx.rank_positions(cu, cc, both, -INF, INF, exclude=lists)
    assert np.all(a[2] >= 0) and (b[2] < 0).sum() == sum(len(x[::7]) for x in lists)
    for u in range(3):
        ra, rb = a[1][a[0][u]:a[0][u + 1]], b[1][b[0][u]:b[0][u + 1]]
        into = np.searchsorted(rb, ra)
        for j in (2, 3):
            xa, xb = a[j][a[0][u]:a[0][u + 1]], b[j][b[0][u]:b[0][u + 1]]
            assert xb[into].tobytes() == xa.tobytes(), (u, j)
            out = np.isin(rb, lists[u])
            assert np.all(xb[out] == -1) if j == 2 else np.all(np.isnan(xb[out]))
    check_interval(cut(ref, Cn), b, lists)
    ctx.close()


# -------------------------------------------------------------------------------- 6. lazy L1
def test_lazy_l1_is_caught_up_on_read(gpu):
    rng = np.random.default_rng(33)
    Fm, k = 256, 8
    w, V, present = R.make_table(rng, Fm, k, present_frac=1.0)
    ctx = loaded(w, V, present)
    # three steps with L1; the first batch's rows (ids < 100) are not touched by the later ones
    for t, (lo_id, hi_id) in enumerate([(0, 100), (100, 200), (100, 200)], start=1):
        rp, col, val = R.make_rows(rng, np.full(64, 6), hi_id - lo_id)
        b = ctx.batch(N.CSRHost(rp, col + lo_id, val, rng.integers(0, 2, 64).astype(np.float64)))
        ctx.step_batch(b, t, 0.05, 0.02)
        b.close()
    ctxs, cands = R.make_rows(rng, [0, 1, 150, 40], Fm), R.make_rows(rng, cand_lens(300), Fm)
    lists = [np.sort(rng.choice(300, n, replace=False)) for n in (10, 290, 150, 0)]
    every = [np.arange(300)] * 4
    cu, cc = csr(ctxs), csr(cands)
    got = {name: ctx.rank_positions(cu, cc, every, -INF, INF, exclude=ex)  # no export in between
           for name, ex in (("none", None), ("lists", lists))}
    ids, w1, V1 = ctx.export_tables()
    assert len(ids) == Fm and not np.array_equal(w1, w)
    ref = R.pair_ref(w1, V1, present, 0.0, ctxs, cands)
    stale = R.pair_ref(w, V, present, 0.0, ctxs, cands)
    for name, ex in (("none", None), ("lists", lists)):
        check_interval(ref, got[name], ex)
        check_slots(ctx, cu, cc, 300, got[name], ex)
        check_counting(got[name], ex, 4, 300)
    with pytest.raises(AssertionError):  # the table as loaded would have ranked otherwise
        check_interval(stale, got["none"], None)
    assert ctx.epoch == 3
    ctx.close()


# ------------------------------------------------------------------ 7. determinism and state
def test_equal_calls_equal_bytes_steady_memory_untouched_state(gpu):
    w, V, present, ctxs, cands = _small(Cn=1100)
    rng = np.random.default_rng(9)
    ctx = loaded(w, V, present)
    cu, cc = csr(ctxs), csr(cands)
    ctx.evaluate(cu, 0.0, 1.0)
    targets = [np.sort(rng.choice(1100, n, replace=False)) for n in (1050, 0, 300)]
    lists = [np.sort(rng.choice(1100, n, replace=False)) for n in (300, 1100, 0)]
    before = ctx.export_tables()
    n_eval = len(ctx.eval_history())
    for ex in (lists, None):
        ctx.rank_positions(cu, cc, targets, 0.0, 1.0, exclude=ex)  # warmed
    mem = live()
    ctx.profile_enable(True)
    for ex in (lists, None):
        first = ctx.rank_positions(cu, cc, targets, 0.0, 1.0, exclude=ex)
        again = ctx.rank_positions(cu, cc, targets, 0.0, 1.0, exclude=ex)
        assert same(first, again)
        assert live() == mem
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    assert {"rank_summary", "rank_position"} <= set(prof) and not {"rank_score", "rank_merge"} & set(prof)
    assert ctx.epoch == 0 and len(ctx.loss_history()) == 0 and len(ctx.eval_history()) == n_eval
    assert same(ctx.export_tables(), before)
    ctx.close()


def test_batch_form_equals_the_host_form(gpu):
    w, V, present, ctxs, cands = _small(Cn=90)
    rng = np.random.default_rng(10)
    ctx = loaded(w, V, present)
    cu, cc = csr(ctxs), csr(cands)
    targets = [np.sort(rng.choice(90, n, replace=False)) for n in (30, 90, 4)]
    lists = [np.sort(rng.choice(90, n, replace=False)) for n in (30, 89, 4)]
    both = R.take_rows(cands, np.concatenate([np.arange(20), np.arange(90)]))
    data = ctx.batch_splits(csr(both), [0, 20, 110])
    view = ctx.split_view(data, 1)  # candidates as split 1 of a split dataset
    bu, src = ctx.batch(cu), ctx.batch(cc)
    sel = ctx.batch_from_rows(src, np.arange(90))  # a batch refilled on the device: the call waits for the gather
    for ex in (None, lists):
        want = ctx.rank_positions(cu, cc, targets, 0.0, 1.0, exclude=ex)
        for bc in (src, view, sel):
            assert same(ctx.rank_positions_batch(bu, bc, targets, 0.0, 1.0, exclude=ex), want)
        with pytest.raises(N.FMError, match="split"):
            ctx.rank_positions_batch(bu, data, targets, 0.0, 1.0, exclude=ex)
    other = loaded(w, V, present)
    with pytest.raises(N.FMError, match="another context"):
        other.rank_positions_batch(bu, sel, targets, 0.0, 1.0, exclude=lists)
    other.close()
    for b in (view, sel, src, data, bu):
        b.close()
    ctx.close()


# -------------------------------------------------------------------------------- 8. refusals
def test_bad_lists_are_refused_and_change_nothing(gpu):
    w, V, present, ctxs, cands = _small(Cn=50)
    ctx = loaded(w, V, present)
    cu, cc = csr(ctxs), csr(cands)
    good = ([0, 2, 2, 5], [3, 7, 0, 1, 49])
    first = raw(ctx, cu, cc, good, good, 0.0, 1.0)
    assert first[0].tolist()[:2] == [-1, -1]  # every target is excluded here
    raw(ctx, cu, cc, good, (None, None), 0.0, 1.0)
    bu, bc = ctx.batch(cu), ctx.batch(cc)
    raw(ctx, bu, bc, good, good, 0.0, 1.0)
    mem = live()
    bad = [
        ("ascending", ([0, 2, 2, 5], [7, 3, 0, 1, 49])),   # unsorted
        ("ascending", ([0, 2, 2, 5], [3, 7, 0, 1, 1])),    # a duplicate
        ("out of range", ([0, 2, 2, 5], [3, 7, 0, 1, 50])),  # row = C
        ("out of range", ([0, 2, 2, 5], [3, 7, -1, 1, 49])),  # row = -1
        ("_ptr", ([1, 2, 2, 5], [3, 7, 0, 1, 49])),        # ptr[0] = 1
        ("_ptr", ([0, 2, 1, 5], [3, 7, 0, 1, 49])),        # decreasing
        ("_ptr", ([0, 2, 2, 2**31], [3, 7, 0, 1, 49])),    # an offset of 2^31
        ("null", ([0, 2, 2, 5], None)),
    ]
    for words, lists in bad:
        for a, b in ((cu, cc), (bu, bc)):
            with pytest.raises(N.FMError, match="target.*" + words):
                raw(ctx, a, b, lists, good, 0.0, 1.0)
            assert live() == mem
            with pytest.raises(N.FMError, match="exclude.*" + words):
                raw(ctx, a, b, good, lists, 0.0, 1.0)
            assert live() == mem
    with pytest.raises(N.FMError, match=r"target.*context 2, position 1"):
        raw(ctx, cu, cc, ([0, 2, 2, 5], [3, 7, 0, 0, 49]), good, 0.0, 1.0)
    with pytest.raises(N.FMError, match=r"exclude.*context 0, position 1: row 50"):
        raw(ctx, cu, cc, good, ([0, 2, 2, 5], [3, 50, 0, 1, 49]), 0.0, 1.0)
    for a, b in ((cu, cc), (bu, bc)):
        with pytest.raises(N.FMError, match="tgt_ptr"):
            raw(ctx, a, b, (None, None), good, 0.0, 1.0)  # a null tgt_ptr
        with pytest.raises(N.FMError, match="tgt_ptr"):
            raw(ctx, a, b, (None, [1]), (None, None), 0.0, 1.0)
        assert live() == mem
    empty = csr((np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0)))
    with pytest.raises(N.FMError, match="candidate"):
        raw(ctx, cu, empty, ([0, 0, 0, 0], []), (None, None), 0.0, 1.0)  # C = 0
    pos, score = raw(ctx, empty, cc, ([0], []), ([0], []), 0.0, 1.0)  # U = 0: nothing to do
    assert pos.shape == score.shape == (0,)
    pos, score = raw(ctx, cu, cc, ([0, 0, 0, 0], [7]), good, 0.0, 1.0)  # no target: nothing written
    assert pos.tolist() == [-7] and score.tolist() == [-7.0]
    lib = N.load()
    nulls = (None,) * 4 + (0.0, 1.0, None, None)
    assert lib.fm_rank_positions(ctx.handle, None, None, *nulls) == -1
    assert lib.fm_rank_positions_batch(ctx.handle, None, None, *nulls) == -1
    tp, tr = np.array([0, 2, 2, 5], np.int64), np.array([3, 7, 0, 1, 49], np.int32)
    assert lib.fm_rank_positions(ctx.handle, C.byref(cu.c), C.byref(cc.c), N.ptr(tp, C.c_int64), N.ptr(tr, C.c_int32), None,
                                 None, 0.0, 1.0, None, None) == -1  # null outputs
    assert live() == mem
    with pytest.raises(ValueError):  # the Python layer: a wrong number of lists
        ctx.rank_positions(cu, cc, [[0]] * 2, 0.0, 1.0)
    with pytest.raises(ValueError):
        ctx.rank_positions(cu, cc, [[0]] * 3, 0.0, 1.0, exclude=[[0]] * 4)
    with pytest.raises(N.FMError, match="target.*out of range"):  # what it leaves to the library
        ctx.rank_positions(cu, cc, [[0], [50], []], 0.0, 1.0)
    again = raw(ctx, cu, cc, good, good, 0.0, 1.0)  # neither the refusals nor the calls changed anything
    assert same(first, again) and live() == mem
    assert ctx.epoch == 0 and len(ctx.loss_history()) == 0
    bu.close(), bc.close()
    ctx.close()


def test_sharded_tables_refuse_and_replicated_answers_host_rows(gpu):
    w, V, present, ctxs, cands = _small()
    cu, cc = csr(ctxs), csr(cands)
    targets, lists = [[0, 7, 49], [3], []], [[1, 5, 9], [], [49]]
    single = loaded(w, V, present)
    want = {name: single.rank_positions(cu, cc, targets, 0.0, 1.0, exclude=ex) for name, ex in (("none", None), ("lists", lists))}
    shard = FMContext(200, 4, shard_count=2)
    group = FMContext(200, 4, parallel="sharded", n_gpus=2, devices=[0, 0])
    for ex in (None, lists):
        for c in (shard, group):
            with pytest.raises(N.FMError, match="shard"):
                c.rank_positions(cu, cc, targets, 0.0, 1.0, exclude=ex)
    shard.close()
    group.close()
    repl = loaded(w, V, present, parallel="replicated", n_gpus=2, devices=[0, 0])
    for name, ex in (("none", None), ("lists", lists)):
        assert same(repl.rank_positions(cu, cc, targets, 0.0, 1.0, exclude=ex), want[name])
    with pytest.raises(N.FMError, match="out of range"):
        repl.rank_positions(cu, cc, targets, 0.0, 1.0, exclude=[[50], [], []])
    bu, bc = repl.batch(cu), repl.batch(cc)
    with pytest.raises(N.FMError, match="whole on one device"):
        repl.rank_positions_batch(bu, bc, targets, 0.0, 1.0, exclude=lists)
    bu.close(), bc.close()
    repl.close()
    single.close()


# ----------------------------------------------------------------------------- 9. model level
def test_rank_positions_and_ranking_evaluator_on_a_movielens_shaped_frame(gpu):
    from fm_spark_amd.linalg import Vectors
    from fm_spark_amd.ml import DataFrame, FactorizationMachinesSGD, _explode
    from fm_spark_amd.tuning import RANKING_METRICS, RankingEvaluator, ranking_metric

    rng = np.random.default_rng(51)
    nf, n_users, n_items = 60, 8, 40  # features: a user one-hot [0, 8), an item one-hot [8, 48), a few tags
    def vec(u, i):
        pairs = ([(u, 1.0)] if u is not None else []) + ([(8 + i, 1.0), (48 + i % 12, 0.5)] if i is not None else [])
        return Vectors.sparse(nf, pairs)
    seen = [(int(rng.integers(n_users)), int(rng.integers(n_items))) for _ in range(400)]
    seen += [(i % n_users, i) for i in range(n_items)]  # every item is trained: no two items score alike
    train = DataFrame.from_rows([(float((u + i) % 3 == 0), vec(u, i)) for u, i in seen], ["label", "features"],
                                num_partitions=2)
    fm = (FactorizationMachinesSGD().setDimFactorization(4).setMaxIter(8).setStepSize(0.3).setRegParam(0.001)
          .setNumFeatures(nf).setSeed(3))
    model = fm.fit(train)
    users = DataFrame.from_rows([(u, vec(u, None)) for u in range(n_users)], ["user", "features"])
    items = DataFrame.from_rows([(i, vec(None, i)) for i in range(n_items)], ["item", "features"])
    seen_by = [sorted({i for v, i in seen if v == u}) for u in range(n_users)]
    seen_by[3] = list(range(n_items))  # a user who has seen everything: no eligible target
    held = [sorted(set(rng.choice(n_items, 6, replace=False).tolist()) - set(s)) for s in seen_by]
    held[5] = []  # and one without a held-out item
    assert sum(len(h) > 0 for h in held) >= 5
    # the reference on the CPU, from the trained table: every interval is a single value
    ids, w, V = model._ctx.export_tables()
    wt, Vt, present = np.zeros(nf), np.zeros((nf, 4)), np.zeros(nf, bool)
    wt[ids], Vt[ids], present[ids] = w, V, True
    ref = R.pair_ref(wt, Vt, present, model.globalBias, _explode(users["features"]), _explode(items["features"]))
    elig = S.eligible_mask(S.EXCEPT, seen_by, n_users, n_items)
    want = []
    for u in range(n_users):
        a, b = P.Pairs(ref, u, held[u]).interval(elig[u])
        assert np.array_equal(a, b), u  # checked on the CPU: the bound separates every key from the targets'
        want.append(P.positions(ref.key[u], elig[u], held[u]))
        assert np.array_equal(a, want[-1])
    ptr = np.concatenate([[0], np.cumsum([len(h) for h in held])])
    want = np.concatenate(want)
    out = model.rankPositions(users, items, held, exclude=seen_by)
    assert out.schema == ["context", "candidate", "position", "score"] and out.count() == ptr[-1]
    assert out["context"] == np.repeat(np.arange(n_users), np.diff(ptr)).tolist()
    assert out["candidate"] == [i for h in held for i in h]
    assert out["position"] == want.tolist()
    recs = model.recommend(users, items, n_items, exclude=seen_by)["recommendations"]
    for u, c, p, s in zip(out["context"], out["candidate"], out["position"], out["score"]):
        assert recs[u][p] == (c, s)  # the same pair, the same float, at that slot of recommend's list
    n_elig = elig.sum(axis=1)
    for name in RANKING_METRICS:
        for k in (1, 5, 100):
            ev = RankingEvaluator().setMetricName(name).setK(k)
            got = ev.evaluateModel(model, users, items, held, exclude=seen_by)
            assert got == ranking_metric(name, k, ptr, want, n_elig)[0], (name, k)
            assert ev.numContextsUsed == sum(len(h) > 0 for h in held) and 0.0 <= got <= 1.0
    free = model.rankPositions(users, items, held)  # nothing excluded: positions among all 40 items
    assert all(p >= q for p, q in zip(free["position"], out["position"]))
    with pytest.raises(ValueError):
        model.rankPositions(users, items, held[:-1])
