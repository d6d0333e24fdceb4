"""fm_batch_sample_pairs_weighted's draw contract (include/fm_hip.h) in NumPy, and its brute-force statement."""

import numpy as np

from pair_ref import draw_ranks


def weighted_negatives(seed, pos_ctx, n_draw, excl_ptr, excl_rows, weight):
    """c [n_pos, n_draw] by the contract's formulas; excl_ptr None: nothing excluded."""
    weight = np.asarray(weight, np.int64)
    cdf = np.concatenate([[0], np.cumsum(weight)])
    pos_ctx = np.asarray(pos_ctx, np.int64)
    lists = [np.zeros(0, np.int64) if excl_ptr is None else np.asarray(excl_rows[excl_ptr[u]:excl_ptr[u + 1]], np.int64)
             for u in pos_ctx]
    X = [np.concatenate([[0], np.cumsum(weight[e])]) for e in lists]  # X_0 .. X_L
    r = draw_ranks(seed, len(pos_ctx), n_draw, [cdf[-1] - x[-1] for x in X])
    out = np.zeros((len(pos_ctx), n_draw), np.int64)
    for i, (e, x) in enumerate(zip(lists, X)):
        t = np.searchsorted(cdf[e] - x[:-1], r[i], side="right")
        out[i] = np.searchsorted(cdf, r[i] + x[t], side="right") - 1
    return out


def eligible_expanded(excl, weight):
    """The ascending list of eligible rows, each repeated weight times: element r is the draw of rank r."""
    w = np.array(weight, np.int64)
    w[np.asarray(excl, np.int64)] = 0
    return np.repeat(np.arange(len(w)), w)
