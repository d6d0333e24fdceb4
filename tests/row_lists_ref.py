"""Host reference of fm_lists_from_pairs: per-context lists of the distinct candidate rows its pairs name,
ascending, as (ptr int64 [U + 1], rows int32)."""

import numpy as np


def lists_from_pairs(pair_ctx, pair_cand, U):
    """Vectorised: the pairs sorted by (context, candidate), the first of every run of equal pairs kept,
    the contexts' counts summed into offsets."""
    pc = np.asarray(pair_ctx, dtype=np.int64)
    pd = np.asarray(pair_cand, dtype=np.int64)
    order = np.lexsort((pd, pc))
    sc, sd = pc[order], pd[order]
    head = np.ones(len(sc), dtype=bool)
    head[1:] = (sc[1:] != sc[:-1]) | (sd[1:] != sd[:-1])
    ptr = np.zeros(U + 1, dtype=np.int64)
    np.cumsum(np.bincount(sc[head], minlength=U), out=ptr[1:])
    return ptr, sd[head].astype(np.int32)


def lists_brute(pair_ctx, pair_cand, U):
    """One context at a time, straight from the definition."""
    lists = [sorted({int(c) for u2, c in zip(pair_ctx, pair_cand) if u2 == u}) for u in range(U)]
    ptr = np.zeros(U + 1, dtype=np.int64)
    for u, l in enumerate(lists):
        ptr[u + 1] = ptr[u] + len(l)
    return ptr, np.asarray([c for l in lists for c in l], dtype=np.int32)
