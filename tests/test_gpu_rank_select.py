"""GPU: ranking within per-context candidate lists (fm_rank_candidates_select / fm_rank_batch_select;
k_rank_score_sel in fm_rank.hip) against the unrestricted call and the masked reference of
tests/rank_select_ref.py.

Where the unrestricted call can return every row (C <= 1024) the expectation is bitwise: its full
order (n_top = C) filtered on the host by the list and cut to n_top.  Larger C takes the masked
check, with rank_ref's bound for fp64 sums in another order (tests/test_gpu_rank.py has it in full).

The constants of fm_rank.hip whose edges the shapes sit on:
  kRankChunk = 1024        rows per chunk and bits per exclusion mask -> C in 1023, 1024, 1025, 2049; lists
                           of 1023, 1024, 1025, 2049 entries;
  kRankMaxSplits = 64      a list of 65 537 rows takes 65 chunks over 64 splits (one block streams two)
                           and leaves the 3-row list beside it 63 splits without a chunk;
  kRankListBudget = 4 MiB  U = 65 at n_top = 1024 and 8 splits: two passes of 42 and 23 contexts, the
                           second reading sel_ptr + 42."""

import ctypes as C
import functools
import math

import numpy as np
import pytest

import rank_ref as R
import rank_select_ref as S
from fm_spark_amd import _native as N
from fm_spark_amd.engine import FMContext
from test_gpu_rank import _small, cand_lens, csr, ctx_lens, cut, loaded  # the unrestricted call's row sets and helpers

pytestmark = pytest.mark.gpu
INF = math.inf
F = 4096


@functools.lru_cache(maxsize=None)
def problem(k, U, Cmax, seed, centred=True):
    """A table, U contexts, Cmax candidates and their reference, computed once and not changed."""
    rng = np.random.default_rng(seed)
    w, V, present = R.make_table(rng, F, k)
    ctxs, cands = R.make_rows(rng, ctx_lens(U, rng), F), R.make_rows(rng, cand_lens(Cmax), F)
    w0 = 0.0
    if centred:  # a globalBias that puts the middle context's scores on both sides of zero
        key0 = R.pair_ref(w, V, present, 0.0, ctxs, cands).key
        w0 = 0.25 - float(np.median(key0[len(key0) // 2]))
    ref = R.pair_ref(w, V, present, w0, ctxs, cands)
    if centred:
        assert ((ref.key > 0).any(axis=1) & (ref.key < 0).any(axis=1)).any()  # both signs within one context's sort
    return w, V, present, ctxs, cands, w0, ref


def raw(ctx, contexts, candidates, select, ptr, rows, n_top, lo=-INF, hi=INF):
    """The C-ABI as it is, without the Python layer's sorting: host rows (CSRHost) or batches."""
    lib = N.load()
    U = contexts.n_rows
    idx = np.zeros(max(U * n_top, 1), np.int32)
    score = np.zeros(max(U * n_top, 1))
    ptr = None if ptr is None else np.ascontiguousarray(ptr, np.int64)
    rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
    pp = None if ptr is None else N.ptr(ptr, C.c_int64)
    pr = None if rows is None else N.ptr(rows, C.c_int32)
    out = (n_top, lo, hi, N.ptr(idx, C.c_int32), N.ptr(score, C.c_double))
    if isinstance(contexts, N.CSRHost):
        rc = lib.fm_rank_candidates_select(ctx.handle, C.byref(contexts.c), C.byref(candidates.c), select, pp, pr, *out)
    else:
        rc = lib.fm_rank_batch_select(ctx.handle, contexts.handle, candidates.handle, select, pp, pr, *out)
    N.check(rc, "fm_rank_select")
    return idx[: U * n_top].reshape(U, n_top), score[: U * n_top].reshape(U, n_top)


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def live():
    lib = N.load()
    return lib.fm_device_bytes_live(), lib.fm_device_allocs_live()


# ------------------------------------------------------------------------------------ 1. ALL
def test_select_all_with_null_lists_is_the_unrestricted_call(gpu):
    w, V, present, ctxs, cands, w0, ref = problem(5, 3, 2049, 101)
    ctx = loaded(w, V, present, w0=w0)
    cu, cc = csr(ctxs), csr(R.take_rows(cands, np.arange(1025)))
    for n_top in (1, 100, 1024):
        want = ctx.rank(cu, cc, n_top, -INF, INF)
        assert same(raw(ctx, cu, cc, S.ALL, None, None, n_top), want)
        bu, bc = ctx.batch(cu), ctx.batch(cc)
        assert same(raw(ctx, bu, bc, S.ALL, None, None, n_top), want)
        bu.close(), bc.close()
    ctx.close()


# ------------------------------------------------------------------------- 2. EXCEPT, chunk edges
def edge_lists(Cn, top_rows):
    """The issue's exclusion lists, each as U = 3 lists (name -> lists)."""
    U = len(top_rows)
    every = np.arange(Cn)
    kinds = {
        "empty": [[] for _ in range(U)],
        "row 0": [[0]] * U,
        "last row": [[Cn - 1]] * U,
        "first chunk": [np.arange(min(Cn, 1024))] * U,
        "all but one": [np.delete(every, (Cn // 2 + 300 * u) % Cn) for u in range(U)],
        "everything": [every] * U,
        "own top": [np.sort(t) for t in top_rows],
    }
    edge = [r for r in (1023, 1024) if r < Cn]
    if edge:
        kinds["1023, 1024"] = [edge] * U
    return kinds


@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("Cn", [1023, 1024, 1025, 2049])
def test_except_at_the_chunk_edges(gpu, Cn, k):
    w, V, present, ctxs, cands, w0, ref = problem(k, 3, 2049, 200 + k)
    ref = cut(ref, Cn)
    ctx = loaded(w, V, present, w0=w0)
    cu, cc = csr(ctxs), csr(R.take_rows(cands, np.arange(Cn)))
    full = ctx.rank(cu, cc, Cn, -INF, INF) if Cn <= 1024 else None
    for n_top in (1, 100, min(Cn, 1024)):
        top = ctx.rank(cu, cc, n_top, -INF, INF)[0]
        for u in range(3):  # the "own top" really is the top: nothing outside it beats it by more than the bound
            rest = np.ones(Cn, bool)
            rest[top[u]] = False
            if rest.any():
                assert ref.key[u, rest].max() - ref.key[u, top[u]].min() <= ref.bound[u].max()
        for name, lists in edge_lists(Cn, top).items():
            elig = S.eligible_mask(S.EXCEPT, lists, 3, Cn)
            assert np.array_equal(elig.sum(axis=1), [Cn - len(x) for x in lists]), name
            got = ctx.rank(cu, cc, n_top, -INF, INF, exclude=lists)
            if full is not None:
                want = S.filter_full(full[0], full[1], elig, n_top)
                assert same(got, want), (name, n_top)
            else:
                S.check(got[0], got[1], ref, elig)
            if name == "everything":
                assert np.all(got[0] == -1) and np.all(np.isnan(got[1]))
            if name == "all but one":
                assert np.array_equal(got[0][:, 0], [(Cn // 2 + 300 * u) % Cn for u in range(3)])
                assert np.all(got[0][:, 1:] == -1)
            if name == "own top":
                assert not any(set(got[0][u].tolist()) & set(top[u].tolist()) for u in range(3))
    ctx.close()


# ------------------------------------------------------------------ 3. fewer eligible than n_top
def test_fewer_eligible_rows_than_n_top(gpu):
    w, V, present, ctxs, cands, w0, ref = problem(5, 3, 2049, 205)
    Cn, n_top = 1100, 100
    ref = cut(ref, Cn)
    rng = np.random.default_rng(3)
    kept = [np.sort(rng.choice(Cn, 7, replace=False)) for _ in range(3)]
    kept[0][[0, -1]] = [1023, 1024]  # the survivors sit on both sides of the chunk edge
    kept[0].sort()
    lists = [np.delete(np.arange(Cn), x) for x in kept]
    elig = S.eligible_mask(S.EXCEPT, lists, 3, Cn)
    assert np.all(elig.sum(axis=1) == 7)
    ctx = loaded(w, V, present, w0=w0)
    idx, score = ctx.rank(csr(ctxs), csr(R.take_rows(cands, np.arange(Cn))), n_top, -INF, INF, exclude=lists)
    S.check(idx, score, ref, elig)
    for u in range(3):
        assert sorted(idx[u, :7].tolist()) == kept[u].tolist()
        assert np.all(idx[u, 7:] == -1) and np.all(np.isnan(score[u, 7:])) and not np.isnan(score[u, :7]).any()
    ctx.close()


# ----------------------------------------------------------------------------- 4. ONLY, ragged
@pytest.mark.parametrize("n_top", [1, 100])
def test_only_with_ragged_lists(gpu, n_top):
    w, V, present, ctxs, cands, w0, ref = problem(5, 10, 4096, 401)
    Cn = 4096
    rng = np.random.default_rng(40 + n_top)
    lens = [0, 1, n_top - 1, n_top, n_top + 1, 1023, 1024, 1025, 2049, Cn]
    lists = []
    for u, n in enumerate(lens):
        ends = [0, Cn - 1][: n] if u % 2 else [Cn - 1, 0][: n]  # rows 0 and C - 1 are listed
        mid = rng.choice(np.arange(1, Cn - 1), n - len(ends), replace=False)
        lists.append(np.sort(np.concatenate([ends, mid]).astype(np.int64)))
    elig = S.eligible_mask(S.ONLY, lists, 10, Cn)
    assert np.array_equal(elig.sum(axis=1), lens) and elig[-1].all() and elig[1:, [0, Cn - 1]].any(axis=0).all()
    ctx = loaded(w, V, present, w0=w0)
    cu, cc = csr(ctxs), csr(cands)
    idx, score = ctx.rank(cu, cc, n_top, -INF, INF, only=lists)
    S.check(idx, score, ref, elig)
    free = ctx.rank(cu, cc, n_top, -INF, INF)
    assert idx[9].tobytes() == free[0][9].tobytes() and score[9].tobytes() == free[1][9].tobytes()  # the list of all rows
    assert np.all(idx[0] == -1) and np.all(np.isnan(score[0]))
    for u in range(1, 9):
        if not 1 <= len(lists[u]) <= 1024:
            continue
        # the same context against its listed rows as a candidate set of their own
        m = min(n_top, len(lists[u]))
        one_i, one_s = ctx.rank(csr(R.take_rows(ctxs, [u])), csr(R.take_rows(cands, lists[u])), m, -INF, INF)
        assert np.array_equal(lists[u][one_i[0]], idx[u, :m]), u
        assert one_s[0].tobytes() == np.ascontiguousarray(score[u, :m]).tobytes(), u
        assert np.all(idx[u, m:] == -1)
    ctx.close()


# --------------------------------------------------------------------------------- 5. split cap
@functools.lru_cache(maxsize=None)
def split_cap_problem():
    return problem(4, 2, 70000, 501, centred=False)


def test_only_beyond_the_split_cap_beside_a_short_list(gpu):
    w, V, present, ctxs, cands, w0, ref = split_cap_problem()
    Cn, n_top = 70000, 1024
    rng = np.random.default_rng(51)
    long = np.sort(rng.choice(Cn, 65537, replace=False))
    lists = [long, np.array([0, 40000, Cn - 1])]
    elig = S.eligible_mask(S.ONLY, lists, 2, Cn)
    assert elig.sum(axis=1).tolist() == [65537, 3]
    ctx = loaded(w, V, present)
    idx, score = ctx.rank(csr(ctxs), csr(cands), n_top, -INF, INF, only=lists)
    S.check(idx, score, ref, elig)
    assert sorted(idx[1, :3].tolist()) == [0, 40000, Cn - 1] and np.all(idx[1, 3:] == -1)
    ctx.close()


def test_except_every_even_row_beyond_the_split_cap(gpu):
    w, V, present, ctxs, cands, w0, ref = split_cap_problem()
    Cn, n_top = 70000, 1024
    lists = [np.arange(0, Cn, 2)] * 2
    elig = S.eligible_mask(S.EXCEPT, lists, 2, Cn)
    assert len(lists[0]) == 35000 and np.all(elig.sum(axis=1) == 35000)
    ctx = loaded(w, V, present)
    idx, score = ctx.rank(csr(ctxs), csr(cands), n_top, -INF, INF, exclude=lists)
    S.check(idx, score, ref, elig)
    assert np.all(idx % 2 == 1)
    ctx.close()


# ----------------------------------------------------------------------------- 6. context tiles
@pytest.mark.parametrize("mode", [S.ONLY, S.EXCEPT])
def test_context_tiles_read_their_own_lists(gpu, mode):
    w, V, present, ctxs, cands, w0, ref = problem(4, 65, 8193, 601, centred=False)
    U, Cn, n_top = 65, 8193, 1024
    rng = np.random.default_rng(60 + mode)
    # a different list per context; the longest has all 9 chunks, so ONLY takes 8 splits as EXCEPT does
    lens = rng.integers(0, 3000, U)
    lens[[0, 42, 64]] = [Cn, 2500, 1025]
    lists = [np.sort(rng.choice(Cn, n, replace=False)) for n in lens]
    elig = S.eligible_mask(mode, lists, U, Cn)
    assert np.array_equal(elig.sum(axis=1), lens if mode == S.ONLY else Cn - lens)
    kw = {"only": lists} if mode == S.ONLY else {"exclude": lists}
    ctx = loaded(w, V, present)
    cc = csr(cands)
    idx, score = ctx.rank(csr(ctxs), cc, n_top, -INF, INF, **kw)
    S.check(idx, score, ref, elig)
    # the first context of the second pass, alone with its own list: the same bytes
    kw = {name: [lists[42]] for name in kw}
    one = ctx.rank(csr(R.take_rows(ctxs, [42])), cc, n_top, -INF, INF, **kw)
    assert one[0].tobytes() == idx[42].tobytes() and one[1].tobytes() == score[42].tobytes()
    ctx.close()


# -------------------------------------------------------------------------------------- 7. ties
@pytest.mark.parametrize("mode", [S.ONLY, S.EXCEPT])
def test_copies_of_one_row_survive_in_row_order(gpu, mode):
    rng = np.random.default_rng(22)
    w, V, present = R.make_table(rng, F, 17)
    ctxs = R.make_rows(rng, [200, 1, 40, 0], F)
    distinct = R.make_rows(rng, np.full(40, 13), F)
    content = rng.integers(0, 40, 2300)  # candidate row -> which distinct row it copies
    cands = R.take_rows(distinct, content)
    lists = [np.sort(rng.choice(2300, n, replace=False)) for n in (700, 1150, 1, 2299)]
    elig = S.eligible_mask(mode, lists, 4, 2300)
    kw = {"only": lists} if mode == S.ONLY else {"exclude": lists}
    ctx = loaded(w, V, present)
    idx, score = ctx.rank(csr(ctxs), csr(cands), 1024, -INF, INF, **kw)
    S.check(idx, score, R.pair_ref(w, V, present, 0.0, ctxs, cands), elig)
    seen_copies = 0
    for u in range(4):
        m = min(1024, int(elig[u].sum()))
        g = content[idx[u, :m]]
        for d in np.unique(g):
            at = np.flatnonzero(g == d)
            seen_copies += len(at) > 1
            assert np.all(np.diff(idx[u, at]) > 0)          # copies of one row: ascending candidate row
            assert np.all(score[u, at] == score[u, at[0]])  # and the same bits, wherever they sit
            assert np.all(np.diff(at) == 1)                 # equal keys: adjacent in the list
            if m < 1024 or at[-1] < m - 1:                  # every eligible copy is there (the list may cut the last group)
                assert np.array_equal(idx[u, at], np.flatnonzero(elig[u] & (content == d)))
    assert seen_copies > 40
    ctx.close()


# --------------------------------------------------------------------------------- 8. semantics
def test_w0_pairs_and_clamped_ties_under_lists(gpu):
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
    assert ((ref.key < w0) & ref.learned).any() and ((ref.key > w0) & ref.learned).any()
    ctx = loaded(w, V, present, w0=w0)
    cu, cc = csr(ctxs), csr(cands)
    lists = [np.sort(rng.choice(400, 150, replace=False)) for _ in range(4)]
    full_free, full_clamp = ctx.rank(cu, cc, 400, -INF, INF), ctx.rank(cu, cc, 400, 0.0, 1.0)
    for mode, kw in ((S.ONLY, {"only": lists}), (S.EXCEPT, {"exclude": lists})):
        elig = S.eligible_mask(mode, lists, 4, 400)
        m = int(elig[0].sum())
        assert np.all(elig.sum(axis=1) == m) and (elig & ~ref.learned).any(axis=1)[[0, 1, 3]].all()
        free = ctx.rank(cu, cc, m, -INF, INF, **kw)
        S.check(free[0], free[1], ref, elig)
        assert same(free, S.filter_full(full_free[0], full_free[1], elig, m))
        idx, score = ctx.rank(cu, cc, m, 0.0, 1.0, **kw)  # a clamp range that excludes w0
        S.check(idx, score, ref, elig, 0.0, 1.0)
        assert same((idx, score), S.filter_full(full_clamp[0], full_clamp[1], elig, m))
        assert np.array_equal(idx, free[0])  # many scores tie at 0 and 1: the order stays the unclamped key's
        nolearn = ~ref.learned[np.arange(4)[:, None], idx]
        assert nolearn.any() and np.all(score[nolearn] == w0) and np.all(score[~nolearn] <= 1.0)
        assert (np.sum(score == 1.0, axis=1) > 1).any() and (np.sum(score == 0.0, axis=1) > 1).any()
    ctx.close()


def test_lazy_l1_is_caught_up_on_read_under_lists(gpu):
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
    cu, cc = csr(ctxs), csr(cands)
    got = {mode: ctx.rank(cu, cc, 100, -INF, INF, **kw)  # no export in between
           for mode, kw in ((S.ONLY, {"only": lists}), (S.EXCEPT, {"exclude": lists}))}
    full = ctx.rank(cu, cc, 300, -INF, INF)
    ids, w1, V1 = ctx.export_tables()
    assert len(ids) == Fm and not np.array_equal(w1, w)
    ref = R.pair_ref(w1, V1, present, 0.0, ctxs, cands)
    for mode, (idx, score) in got.items():
        elig = S.eligible_mask(mode, lists, 4, 300)
        S.check(idx, score, ref, elig)
        assert same((idx, score), S.filter_full(full[0], full[1], elig, 100))
    assert ctx.epoch == 3
    ctx.close()


# ------------------------------------------------------------------ 9. determinism and lifetime
def test_equal_calls_equal_bytes_steady_memory_untouched_state(gpu):
    w, V, present, ctxs, cands = _small(Cn=1100)
    rng = np.random.default_rng(9)
    ctx = loaded(w, V, present)
    cu, cc = csr(ctxs), csr(cands)
    lists = [np.sort(rng.choice(1100, n, replace=False)) for n in (1050, 0, 300)]
    for kw in ({"only": lists}, {"exclude": lists}):
        ctx.rank(cu, cc, 1024, 0.0, 1.0, **kw)  # warmed
    mem = live()
    ctx.profile_enable(True)
    for kw in ({"only": lists}, {"exclude": lists}):
        first = ctx.rank(cu, cc, 1024, 0.0, 1.0, **kw)
        again = ctx.rank(cu, cc, 1024, 0.0, 1.0, **kw)
        assert same(first, again)
        assert live() == mem
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    assert {"rank_summary", "rank_score", "rank_merge"} <= set(prof)
    assert ctx.epoch == 0 and len(ctx.loss_history()) == 0
    ctx.close()


# ---------------------------------------------------------------------------- 10. the batch form
def test_batch_form_equals_the_host_form(gpu):
    w, V, present, ctxs, cands = _small(Cn=90)
    rng = np.random.default_rng(10)
    ctx = loaded(w, V, present)
    cu, cc = csr(ctxs), csr(cands)
    lists = [np.sort(rng.choice(90, n, replace=False)) for n in (30, 89, 4)]
    both = R.take_rows(cands, np.concatenate([np.arange(20), np.arange(90)]))
    data = ctx.batch_splits(csr(both), [0, 20, 110])
    view = ctx.split_view(data, 1)  # candidates as split 1 of a split dataset
    bu, src = ctx.batch(cu), ctx.batch(cc)
    sel = ctx.batch_from_rows(src, np.arange(90))  # a batch refilled on the device: the call waits for the gather
    for kw in ({"only": lists}, {"exclude": lists}):
        want = ctx.rank(cu, cc, 7, 0.0, 1.0, **kw)
        for bc in (src, view, sel):
            assert same(ctx.rank_batch(bu, bc, 7, 0.0, 1.0, **kw), want)
        with pytest.raises(N.FMError, match="split"):
            ctx.rank_batch(bu, data, 7, 0.0, 1.0, **kw)
    other = loaded(w, V, present)
    with pytest.raises(N.FMError, match="another context"):
        other.rank_batch(bu, sel, 7, 0.0, 1.0, exclude=lists)
    other.close()
    for b in (view, sel, src, data, bu):
        b.close()
    ctx.close()


# -------------------------------------------------------------------------------- 11. refusals
def test_bad_lists_are_refused_and_change_nothing(gpu):
    w, V, present, ctxs, cands = _small(Cn=50)
    ctx = loaded(w, V, present)
    cu, cc = csr(ctxs), csr(cands)
    good = ([0, 2, 2, 5], [3, 7, 0, 1, 49])
    first = raw(ctx, cu, cc, S.EXCEPT, *good, 10, 0.0, 1.0)
    raw(ctx, cu, cc, S.ONLY, *good, 10, 0.0, 1.0)
    bu, bc = ctx.batch(cu), ctx.batch(cc)
    raw(ctx, bu, bc, S.EXCEPT, *good, 10, 0.0, 1.0)
    mem = live()
    bad = [
        ("ascending", ([0, 2, 2, 5], [7, 3, 0, 1, 49])),   # unsorted
        ("ascending", ([0, 2, 2, 5], [3, 7, 0, 1, 1])),    # a duplicate
        ("out of range", ([0, 2, 2, 5], [3, 7, 0, 1, 50])),  # row = C
        ("out of range", ([0, 2, 2, 5], [3, 7, -1, 1, 49])),  # row = -1
        ("sel_ptr", ([1, 2, 2, 5], [3, 7, 0, 1, 49])),     # sel_ptr[0] = 1
        ("sel_ptr", ([0, 2, 1, 5], [3, 7, 0, 1, 49])),     # decreasing
        ("null", (None, None)),
        ("null", ([0, 2, 2, 5], None)),
    ]
    for select in (S.ONLY, S.EXCEPT):
        for words, (ptr, rows) in bad:
            for a, b in ((cu, cc), (bu, bc)):
                with pytest.raises(N.FMError, match=words):
                    raw(ctx, a, b, select, ptr, rows, 10, 0.0, 1.0)
                assert live() == mem
    with pytest.raises(N.FMError, match=r"context 2, position 1"):
        raw(ctx, cu, cc, S.ONLY, [0, 2, 2, 5], [3, 7, 0, 0, 49], 10, 0.0, 1.0)
    for a, b in ((cu, cc), (bu, bc)):
        with pytest.raises(N.FMError, match="select"):
            raw(ctx, a, b, 3, *good, 10, 0.0, 1.0)
        with pytest.raises(N.FMError, match="n_top"):
            raw(ctx, a, b, S.EXCEPT, *good, 51, 0.0, 1.0)
        assert live() == mem
    empty = csr((np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0)))
    with pytest.raises(N.FMError, match="candidate"):
        raw(ctx, cu, empty, S.EXCEPT, [0, 0, 0, 0], [], 1, 0.0, 1.0)
    idx, score = raw(ctx, empty, cc, S.EXCEPT, [0], [], 5, 0.0, 1.0)  # U = 0: nothing to do
    assert idx.shape == score.shape == (0, 5)
    lib = N.load()
    assert lib.fm_rank_candidates_select(ctx.handle, None, None, S.ONLY, None, None, 1, 0.0, 1.0, None, None) == -1
    assert lib.fm_rank_batch_select(ctx.handle, None, None, S.ONLY, None, None, 1, 0.0, 1.0, None, None) == -1
    assert live() == mem
    with pytest.raises(ValueError):  # the Python layer: both arguments, a wrong number of lists
        ctx.rank(cu, cc, 10, 0.0, 1.0, only=[[0]] * 3, exclude=[[0]] * 3)
    with pytest.raises(ValueError):
        ctx.rank(cu, cc, 10, 0.0, 1.0, exclude=[[0]] * 2)
    with pytest.raises(N.FMError, match="out of range"):  # what it leaves to the library
        ctx.rank(cu, cc, 10, 0.0, 1.0, exclude=[[0], [50], []])
    again = raw(ctx, cu, cc, S.EXCEPT, *good, 10, 0.0, 1.0)  # neither the refusals nor the calls changed anything
    assert same(first, again) and live() == mem
    assert ctx.epoch == 0 and len(ctx.loss_history()) == 0
    bu.close(), bc.close()
    ctx.close()


def test_sharded_tables_refuse_and_replicated_answers_host_rows(gpu):
    w, V, present, ctxs, cands = _small()
    cu, cc = csr(ctxs), csr(cands)
    lists = [[1, 5, 9], [], [49]]
    single = loaded(w, V, present)
    want = {name: single.rank(cu, cc, 10, 0.0, 1.0, **{name: lists}) for name in ("only", "exclude")}
    shard = FMContext(200, 4, shard_count=2)
    group = FMContext(200, 4, parallel="sharded", n_gpus=2, devices=[0, 0])
    for name in want:
        for c in (shard, group):
            with pytest.raises(N.FMError, match="shard"):
                c.rank(cu, cc, 10, 0.0, 1.0, **{name: lists})
    shard.close()
    group.close()
    repl = loaded(w, V, present, parallel="replicated", n_gpus=2, devices=[0, 0])
    for name in want:
        assert same(repl.rank(cu, cc, 10, 0.0, 1.0, **{name: lists}), want[name])
    with pytest.raises(N.FMError, match="out of range"):
        repl.rank(cu, cc, 10, 0.0, 1.0, exclude=[[50], [], []])
    bu, bc = repl.batch(cu), repl.batch(cc)
    with pytest.raises(N.FMError, match="whole on one device"):
        repl.rank_batch(bu, bc, 10, 0.0, 1.0, exclude=lists)
    bu.close(), bc.close()
    repl.close()
    single.close()


# -------------------------------------------------------------------------------- 12. recommend
def test_recommend_excludes_each_users_seen_items(gpu):
    from fm_spark_amd.linalg import Vectors
    from fm_spark_amd.ml import DataFrame, FactorizationMachinesSGD

    rng = np.random.default_rng(51)
    nf, n_users, n_items = 60, 8, 40  # features: a user one-hot [0, 8), an item one-hot [8, 48), a few tags
    def vec(u, i):
        pairs = ([(u, 1.0)] if u is not None else []) + ([(8 + i, 1.0), (48 + i % 12, 0.5)] if i is not None else [])
        return Vectors.sparse(nf, pairs)
    seen = [(int(rng.integers(n_users)), int(rng.integers(n_items))) for _ in range(400)]
    train = DataFrame.from_rows([(float((u + i) % 3 == 0), vec(u, i)) for u, i in seen], ["label", "features"],
                                num_partitions=2)
    fm = (FactorizationMachinesSGD().setDimFactorization(4).setMaxIter(8).setStepSize(0.3).setRegParam(0.001)
          .setNumFeatures(nf).setSeed(3))
    model = fm.fit(train)
    users = DataFrame.from_rows([(u, vec(u, None)) for u in range(n_users)], ["user", "features"])
    items = DataFrame.from_rows([(i, vec(None, i)) for i in range(n_items)], ["item", "features"])
    seen_by = [sorted({i for v, i in seen if v == u}) for u in range(n_users)]
    seen_by[3] = [i for i in range(n_items) if i not in (11, 29)]  # a user who has seen all but two items
    assert all(0 < len(s) < n_items for s in seen_by) and sum(n_items - len(s) < 6 for s in seen_by) == 1
    free = model.recommend(users, items, n_items)["recommendations"]
    plain = model.recommend(users, items, 6)["recommendations"]
    assert [r[:6] for r in free] == plain  # without the arguments: today's result
    out = model.recommend(users, items, 6, exclude=seen_by)
    assert out.count() == n_users and out["user"] == list(range(n_users))
    for u, recs in enumerate(out["recommendations"]):
        assert not {c for c, _ in recs} & set(seen_by[u])
        assert recs == [(c, p) for c, p in free[u] if c not in seen_by[u]][:6]  # exactly: the same pairs, the same floats
        assert len(recs) == min(6, n_items - len(seen_by[u]))
    assert sorted(c for c, _ in out["recommendations"][3]) == [11, 29]
    only = model.recommend(users, items, 6, only=seen_by)["recommendations"]
    for u, recs in enumerate(only):
        assert recs == [(c, p) for c, p in free[u] if c in seen_by[u]][:6]
    with pytest.raises(ValueError):
        model.recommend(users, items, 6, exclude=seen_by, only=seen_by)
    with pytest.raises(ValueError):
        model.recommend(users, items, 6, exclude=seen_by[:-1])
