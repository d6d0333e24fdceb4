"""CPU: the masked ranking reference (tests/rank_select_ref.py) against brute force over
rank_ref.pair_ref on tiny shapes, and the Python layer's normalisation of the row lists
(engine.normalize_row_lists, rank(only=, exclude=))."""

import numpy as np
import pytest

import rank_ref as R
import rank_select_ref as S
from fm_spark_amd.engine import FMContext, normalize_row_lists


def tiny(seed=1, U=4, C=9, k=3, F=40):
    rng = np.random.default_rng(seed)
    w, V, present = R.make_table(rng, F, k)
    ctxs = R.make_rows(rng, [5, 0, 2, 7][:U], F)
    distinct = R.make_rows(rng, [3, 0, 1, 4], F)
    cands = R.take_rows(distinct, np.arange(C) % 4)  # copies: exact ties, broken by the row
    return R.pair_ref(w, V, present, 0.25, ctxs, cands)


def lists_for(rng, U, C):
    out = [np.zeros(0, np.int64), np.arange(C), np.array([0, C - 1])]
    out += [np.sort(rng.choice(C, rng.integers(1, C), replace=False)) for _ in range(U - 3)]
    return out[:U]


@pytest.mark.parametrize("mode", [S.ALL, S.ONLY, S.EXCEPT])
def test_mask_and_order_against_brute_force(mode):
    ref = tiny()
    U, C = ref.key.shape
    lists = lists_for(np.random.default_rng(2), U, C)
    elig = S.eligible_mask(mode, lists, U, C)
    for u in range(U):
        for c in range(C):
            listed = c in set(lists[u].tolist())
            assert elig[u, c] == (True if mode == S.ALL else listed if mode == S.ONLY else not listed)
    assert len(np.unique(ref.key[0])) < C  # the problem has exact ties
    for n_top in (1, 4, C):
        for u in range(U):
            pairs = sorted((-ref.key[u, c], c) for c in range(C) if elig[u, c])[:n_top]
            want = [c for _, c in pairs] + [-1] * (n_top - len(pairs))
            assert S.expected_order(ref.key[u], elig[u], n_top).tolist() == want


def result_of(ref, elig, n_top, lo=-np.inf, hi=np.inf):
    U = ref.key.shape[0]
    idx = np.stack([S.expected_order(ref.key[u], elig[u], n_top) for u in range(U)])
    score = np.where(idx >= 0, ref.score(lo, hi)[np.arange(U)[:, None], np.maximum(idx, 0)], np.nan)
    return idx, score


def test_filter_full_equals_expected_order():
    ref = tiny(seed=3)
    U, C = ref.key.shape
    elig = S.eligible_mask(S.EXCEPT, lists_for(np.random.default_rng(4), U, C), U, C)
    full_i, full_s = result_of(ref, np.ones((U, C), bool), C)
    for n_top in (1, 5, C):
        got_i, got_s = S.filter_full(full_i, full_s, elig, n_top)
        want_i, want_s = result_of(ref, elig, n_top)
        assert got_i.tobytes() == want_i.tobytes() and got_s.tobytes() == want_s.tobytes()


def test_check_accepts_the_reference_and_refuses_each_fault():
    ref = tiny(seed=5)
    U, C = ref.key.shape
    lists = lists_for(np.random.default_rng(6), U, C)
    for mode in (S.ONLY, S.EXCEPT):
        elig = S.eligible_mask(mode, lists, U, C)
        for n_top in (1, 4, C):
            S.check(*result_of(ref, elig, n_top), ref, elig)
        S.check(*result_of(ref, elig, 4, 0.0, 0.5), ref, elig, 0.0, 0.5)
    elig = S.eligible_mask(S.EXCEPT, lists, U, C)  # context 2: all but rows 0 and C - 1
    idx, score = result_of(ref, elig, 4)

    def refused(i, s):
        with pytest.raises(AssertionError):
            S.check(i, s, ref, elig)

    bad = idx.copy()
    bad[2, 0] = 0  # an excluded row
    refused(bad, score)
    bad = idx.copy()
    bad[2, [0, 3]] = bad[2, [3, 0]]  # out of order (scores follow their rows)
    bs = score.copy()
    bs[2, [0, 3]] = bs[2, [3, 0]]
    if ref.key[2, idx[2, 0]] - ref.key[2, idx[2, 3]] > ref.bound[2].max():
        refused(bad, bs)
    bad, bs = idx.copy(), score.copy()
    bad[2, 3], bs[2, 3] = -1, np.nan  # a real entry missing
    refused(bad, bs)
    bad, bs = idx.copy(), score.copy()
    bad[0, 0], bs[0, 0] = 1, ref.key[0, 1]  # context 0 excludes nothing here; context 1 everything:
    S.check(idx, score, ref, elig)
    assert np.all(idx[1] == -1) and np.all(np.isnan(score[1]))
    bad, bs = idx.copy(), score.copy()
    bad[1, 0], bs[1, 0] = 3, ref.key[1, 3]  # an entry where nothing is eligible
    refused(bad, bs)
    bs = score.copy()
    bs[2, 1] += 1e-6  # a score off by more than the bound
    refused(idx, bs)


# ------------------------------------------------------------------- the Python layer's lists
def test_lists_are_sorted_and_deduplicated():
    ptr, rows = normalize_row_lists([[5, 1, 3, 1], [], np.array([2, 2, 2]), (7, 0)], 4)
    assert ptr.dtype == np.int64 and rows.dtype == np.int32
    assert ptr.tolist() == [0, 3, 3, 4, 6] and rows.tolist() == [1, 3, 5, 2, 0, 7]
    ptr, rows = normalize_row_lists([], 0)
    assert ptr.tolist() == [0] and rows.size == 0
    ptr, rows = normalize_row_lists([[], []], 2)
    assert ptr.tolist() == [0, 0, 0] and rows.size == 0 and rows.dtype == np.int32


def test_a_ptr_rows_pair_is_read_as_csr():
    pair = (np.array([0, 2, 2, 5]), np.array([9, 4, 3, 3, 1]))
    ptr, rows = normalize_row_lists(pair, 3)
    assert ptr.tolist() == [0, 2, 2, 4] and rows.tolist() == [4, 9, 1, 3]
    with pytest.raises(ValueError):
        normalize_row_lists((np.array([0, 2, 1, 5]), np.arange(5)), 3)
    with pytest.raises(ValueError):
        normalize_row_lists((np.array([0, 2, 2, 4]), np.arange(5)), 3)
    with pytest.raises(ValueError):
        normalize_row_lists((np.array([1, 2, 2, 5]), np.arange(5)), 3)


def test_wrong_length_and_wrong_types_are_refused():
    with pytest.raises(ValueError, match="per context"):
        normalize_row_lists([[1], [2]], 3)
    with pytest.raises(ValueError, match="per context"):
        normalize_row_lists([[1], [2], [3], [4]], 3)
    with pytest.raises(ValueError, match="integers"):
        normalize_row_lists([[1.5], [2]], 2)
    with pytest.raises(ValueError, match="integers"):
        normalize_row_lists([[[1, 2]], [2]], 2)
    with pytest.raises(ValueError, match="int32"):
        normalize_row_lists([[2**31]], 1)
    ptr, rows = normalize_row_lists([[-1, 4]], 1)  # whether a row is a candidate row is the library's check
    assert rows.tolist() == [-1, 4]


def test_both_arguments_given_is_refused_before_anything_else():
    with pytest.raises(ValueError, match="not both"):
        FMContext._rank(None, None, None, "fm_rank_candidates", None, None, 1, 1, 0.0, 1.0, [[0]], [[0]])
