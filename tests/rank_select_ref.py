"""Reference of fm_rank_candidates_select / fm_rank_batch_select (include/fm_hip.h): the eligibility
mask of per-context row lists, the expected order under it, and test_gpu_rank.check's conditions
restricted to the eligible rows.  Keys, bounds and the unrestricted order come from rank_ref."""

import numpy as np

import rank_ref as R

ALL, ONLY, EXCEPT = 0, 1, 2


def eligible_mask(mode, lists, U, C):
    """[U, C] bool: context u may be given candidate row c.  lists: U integer sequences (ignored for ALL)."""
    if mode == ALL:
        return np.ones((U, C), bool)
    assert len(lists) == U
    listed = np.zeros((U, C), bool)
    for u, rows in enumerate(lists):
        listed[u, np.asarray(rows, np.int64)] = True
    return listed if mode == ONLY else ~listed


def expected_order(key_row, eligible, n_top):
    """One context's expected top_index: its eligible rows by key descending, row ascending, cut to
    n_top and filled up with -1."""
    order = R.ref_order(key_row)
    order = order[np.asarray(eligible, bool)[order]][:n_top]
    return np.concatenate([order, np.full(n_top - len(order), -1)]).astype(np.int32)


def filter_full(full_idx, full_score, eligible, n_top):
    """The bitwise expectation where the unrestricted call can return every row (C <= 1024): its
    full order ([U, C] from n_top = C) filtered by the mask, cut to n_top, filled with -1 / NaN."""
    U = full_idx.shape[0]
    idx = np.full((U, n_top), -1, np.int32)
    score = np.full((U, n_top), np.nan)
    for u in range(U):
        keep = eligible[u, full_idx[u]]
        m = min(n_top, int(keep.sum()))
        idx[u, :m] = full_idx[u, keep][:m]
        score[u, :m] = full_score[u, keep][:m]
    return idx, score


def check(idx, score, ref, eligible, lo=-np.inf, hi=np.inf):
    """test_gpu_rank.check's conditions on one call's result, among the eligible rows; ref: rank_ref.PairRef."""
    U, Cn = ref.key.shape
    n = idx.shape[1]
    assert idx.shape == score.shape == (U, n) and idx.dtype == np.int32
    assert eligible.shape == (U, Cn)
    want_all = ref.score(lo, hi)
    tri = np.triu(np.ones((n, n), bool), 1)
    for u in range(U):
        m = min(n, int(eligible[u].sum()))
        # exactly min(n_top, eligible) real entries, then -1 / NaN
        assert np.all(idx[u, m:] == -1) and np.all(np.isnan(score[u, m:])), u
        i, s = idx[u, :m], score[u, :m]
        if m == 0:
            continue
        assert i.min() >= 0 and i.max() < Cn and len(np.unique(i)) == m, u
        assert np.all(eligible[u, i]), (u, i[~eligible[u, i]])  # no ineligible row returned
        key, bnd, learned = ref.key[u, i], ref.bound[u, i], ref.learned[u, i]
        # scores: within the bound of the reference, exactly w0 where nothing is learned
        err = np.abs(s - want_all[u, i])
        assert np.all(err <= bnd), (u, float(np.max(err - bnd)))
        assert np.all(s[~learned] == ref.w0), u
        # the returned keys are non-increasing (a clamp keeps that; w0 pairs rank at w0, return it unclamped)
        shown = np.where(learned, s, min(max(ref.w0, lo), hi))
        assert np.all(np.diff(shown) <= 0), u
        # no eligible row left out beats the list's last key by more than the bound
        out = eligible[u].copy()
        out[i] = False
        assert m == n or not out.any(), u  # a list shorter than n_top leaves no eligible row out
        over = ref.key[u, out] - key[-1]
        assert np.all(over <= np.minimum(ref.bound[u, out], bnd[-1])), (u, float(over.max()))
        # where two reference keys differ by more than the bound, the order is the reference's
        rise = key[None, :] - key[:, None]  # [j, l] = key_l - key_j, a violation where j < l
        assert not np.any(tri[:m, :m] & (rise > np.minimum(bnd[None, :], bnd[:, None]))), u
