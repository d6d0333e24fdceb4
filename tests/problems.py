"""Seeded test problems shared by the CPU and GPU suites (inputs rounded to fp32 so the
device's fp32 tables start from exactly the oracle's values)."""

import numpy as np

from oracle import fm_ref as R


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def make_rows(seed, lengths, F, k, *, kinds=None, pool=None, x_scale=True, labels="binary"):
    """A problem whose rows have exactly the given lengths, built without a Python loop over rows
    (make_problem draws row by row, and its draws are what seeds elsewhere depend on).

    lengths: int [n] -- entries per row -- or int [n, R]: row i holds lengths[i, r] entries whose id is
    r modulo R (the entries a sharded context routes to owner r), owner after owner.
    kinds: None, or int [nnz] per entry in row order: 0 = an id of the shared pool (ids [0, pool),
    each row a window of a random permutation of it, so distinct within the row and repeated across
    rows), 1 = an id no other entry of the batch has (drawn from a permutation of [pool, F)).
    pool: the pool's size (default F; a multiple of R, at least R times the longest run of pool ids).
    x_scale: values shrunk by 4 / sqrt(row length) on long rows, so a score stays O(1).
    Ids within a row are distinct and in no particular order.  Returns (csr, ids, w, V) as make_problem."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    n = lengths.shape[0]
    Rr = 1 if lengths.ndim == 1 else lengths.shape[1]
    seg_len = lengths.reshape(-1)
    row_len = lengths.reshape(n, Rr).sum(axis=1)
    row_ptr = np.concatenate([[0], np.cumsum(row_len)]).astype(np.int64)
    nnz = int(row_ptr[-1])
    pool = F if pool is None else int(pool)
    assert pool % Rr == 0 and 0 < pool <= F
    Q = pool // Rr
    seg_start = np.concatenate([[0], np.cumsum(seg_len)])[:-1]
    seg_of = np.repeat(np.arange(n * Rr), seg_len)
    pos = np.arange(nnz) - seg_start[seg_of]  # the entry's place in its (row, residue) segment
    kinds = np.zeros(nnz, dtype=np.int64) if kinds is None else np.asarray(kinds, dtype=np.int64)
    assert kinds.shape == (nnz,) and (Rr == 1 or not kinds.any())
    assert seg_len.max(initial=0) <= Q, "a row's pool ids must fit the pool to stay distinct"
    perm = rng.permutation(Q)
    off = rng.integers(0, Q, size=n * Rr)
    col = Rr * perm[(off[seg_of] + pos) % Q] + seg_of % Rr
    uniq = np.nonzero(kinds == 1)[0]
    assert len(uniq) <= F - pool, "not enough ids outside the pool for the batch-unique entries"
    col[uniq] = pool + rng.permutation(F - pool)[: len(uniq)]
    x = rng.normal(0.0, 1.0, size=nnz)
    if x_scale:
        x *= np.minimum(1.0, 4.0 / np.sqrt(np.maximum(np.repeat(row_len, row_len), 1)))
    x = f32(x)
    u = rng.random(nnz)
    x[u < 0.05] = 0.0  # explicit zeros stay active
    x[u > 0.7] = 1.0  # unit values travel elided (test_upload_unit_values_elided)
    if labels == "binary":
        y = (rng.random(n) < 0.25).astype(np.float64)
    else:
        y = f32(rng.normal(0.0, 1.0, n))
    csr = R.CSR(row_ptr=row_ptr, col=col.astype(np.int32), val=x.astype(np.float64), label=y)
    ids = np.arange(F, dtype=np.int32)
    w = f32(rng.normal(0.0, 0.1, F))
    V = f32(rng.normal(0.0, 0.1, (F, k)))
    return csr, ids, w, V


def make_problem(seed, n_rows, F, k, mean_nnz, *, empty_frac=0.1, zero_frac=0.05, hot=None, labels="binary"):
    rng = np.random.default_rng(seed)
    row_ptr = [0]
    cols, vals = [], []
    for _ in range(n_rows):
        if rng.random() < empty_frac:
            row_ptr.append(len(cols))
            continue
        z = int(rng.integers(1, 2 * mean_nnz))
        z = min(z, F)
        ids = rng.choice(F, size=z, replace=False)
        if hot is not None and rng.random() < 0.9 and hot not in ids:
            ids[0] = hot
        ids = np.sort(ids)
        v = f32(rng.normal(0.0, 1.0, size=z))
        v[rng.random(z) < zero_frac] = 0.0  # explicit zeros stay active
        cols.extend(ids.tolist())
        vals.extend(v.tolist())
        row_ptr.append(len(cols))
    if labels == "binary":
        y = (rng.random(n_rows) < 0.25).astype(np.float64)
    else:
        y = f32(rng.normal(0.0, 1.0, n_rows))
    csr = R.CSR(row_ptr=np.asarray(row_ptr, np.int64), col=np.asarray(cols, np.int32),
                val=np.asarray(vals, np.float64), label=y)
    ids = np.arange(F, dtype=np.int32)
    w = f32(rng.normal(0.0, 0.1, F))
    V = f32(rng.normal(0.0, 0.1, (F, k)))
    return csr, ids, w, V
