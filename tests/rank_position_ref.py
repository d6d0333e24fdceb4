"""Reference of fm_rank_positions / fm_rank_positions_batch (include/fm_hip.h), from rank_ref.pair_ref's
keys and bounds.

The position of target row t of context u among u's eligible rows is
    pos(u, t) = #{eligible c : key(u, c) > key(u, t), or key(u, c) == key(u, t) and c < t}
(rank_ref.ref_order's order).  ``positions`` gives it exactly on the reference keys.  The device sums its
keys in another order, so its position may differ wherever two reference keys are closer than their
bound: an eligible row c != t counts for certain only where key_c - key_t > min(bound_c, bound_t), and
possibly where |key_c - key_t| <= min(bound_c, bound_t).  ``Pairs.interval`` gives the [lo, hi] a device
position may lie in."""

import numpy as np

import rank_ref as R


def positions(key_row, eligible, targets):
    """Exact positions of `targets` (candidate rows) among the eligible rows of one context; -1 for a
    target that is not eligible.  O(C log C): the inverse of the eligible rows' order."""
    eligible = np.asarray(eligible, bool)
    order = R.ref_order(key_row)
    order = order[eligible[order]]
    pos = np.full(len(key_row), -1, np.int64)
    pos[order] = np.arange(len(order))
    return pos[np.asarray(targets, np.int64)]


class Pairs:
    """One context's targets against all candidate rows: which rows rank before a target for certain,
    which possibly.  Built once per (context, target list) and shared by the exclude lists tried."""

    def __init__(self, ref: R.PairRef, u: int, targets):
        self.targets = np.asarray(targets, np.int64)
        key, bnd = ref.key[u], ref.bound[u]
        diff = key[None, :] - key[self.targets][:, None]           # [t, c] = key_c - key_t
        mb = np.minimum(bnd[None, :], bnd[self.targets][:, None])
        other = np.arange(len(key))[None, :] != self.targets[:, None]
        self.certain = (diff > mb) & other
        self.possible = (np.abs(diff) <= mb) & other

    def interval(self, eligible):
        """(lo, hi) per target among the eligible rows (the target's own eligibility is the caller's)."""
        e = np.asarray(eligible, bool).astype(np.int64)
        lo = self.certain.astype(np.int64) @ e
        return lo, lo + self.possible.astype(np.int64) @ e
