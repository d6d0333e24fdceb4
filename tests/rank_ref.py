"""fp64 NumPy reference of fm_rank_candidates (include/fm_hip.h), vectorised from row summaries.

Over the learned entries e of a row r (ids below F and present in the table; the others are dropped):
    S_r = sum v_e x_e    Q_r = sum |v_e|^2 x_e^2    L_r = sum w_e x_e    a_r = L_r + (|S_r|^2 - Q_r) / 2
    yhat(u, c) = w0 + a_u + a_c + <S_u, S_c>
which is FactorizationMachinesModel.predict's score of the row made of u's entries followed by c's
(tests/test_rank_cpu.py pins it to oracle.fm_ref.predict on the explicitly concatenated rows).  A pair
without a learned entry on either side has the key w0 and scores w0 unclamped.

The bound of a pair for sums taken in another order (the tests' tolerance):
    (nnz_u + nnz_c + kp + 16) 2^-52 M,   kp = roundup(k, 4)
    M = |w0| + sum |w x| + (sum_f (sum_e |v_ef x_e|)^2 + sum_e |v_e|^2 x_e^2) / 2   over both rows' learned entries
"""

from dataclasses import dataclass

import numpy as np


@dataclass
class RowSums:
    S: np.ndarray      # [n, k]
    Q: np.ndarray      # [n]
    L: np.ndarray      # [n]
    A: np.ndarray      # [n, k]  sum |v x|
    Labs: np.ndarray   # [n]     sum |w x|
    learned: np.ndarray  # [n] learned entries
    nnz: np.ndarray    # [n] entries, dropped ones included


def row_sums(w, V, present, row_ptr, col, val) -> RowSums:
    w, V, present = np.asarray(w, np.float64), np.asarray(V, np.float64), np.asarray(present, bool)
    F, k = V.shape
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)
    val = np.asarray(val, np.float64)
    n = len(row_ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    ok = (col >= 0) & (col < F)
    ok[ok] &= present[col[ok]]
    r, c, x = rows[ok], col[ok], val[ok]
    vx = V[c] * x[:, None]
    S, A = np.zeros((n, k)), np.zeros((n, k))
    Q, L, Labs = np.zeros(n), np.zeros(n), np.zeros(n)
    np.add.at(S, r, vx)
    np.add.at(A, r, np.abs(vx))
    np.add.at(Q, r, np.sum(V[c] * V[c], axis=1) * x * x)
    np.add.at(L, r, w[c] * x)
    np.add.at(Labs, r, np.abs(w[c] * x))
    return RowSums(S, Q, L, A, Labs, np.bincount(r, minlength=n), np.diff(row_ptr))


@dataclass
class PairRef:
    key: np.ndarray      # [U, C] the order's key: unclamped yhat, w0 for a pair without a learned entry
    learned: np.ndarray  # [U, C] bool: the pair has a learned entry
    bound: np.ndarray    # [U, C] the reordered-sum bound
    w0: float

    def score(self, lo, hi):
        """What top_score holds: the clamped key, w0 unclamped where nothing is learned."""
        return np.where(self.learned, np.clip(self.key, lo, hi), self.w0)


def pair_ref(w, V, present, w0, contexts, candidates) -> PairRef:
    """contexts / candidates: (row_ptr, col, val)."""
    u = row_sums(w, V, present, *contexts)
    c = row_sums(w, V, present, *candidates)
    k = np.asarray(V).shape[1]
    kp = (k + 3) // 4 * 4
    a_u = u.L + 0.5 * (np.sum(u.S * u.S, axis=1) - u.Q)
    a_c = c.L + 0.5 * (np.sum(c.S * c.S, axis=1) - c.Q)
    y = w0 + a_u[:, None] + a_c[None, :] + u.S @ c.S.T
    learned = (u.learned[:, None] + c.learned[None, :]) > 0
    key = np.where(learned, y, w0)
    # sum_f (A_u + A_c)^2 = |A_u|^2 + |A_c|^2 + 2 <A_u, A_c>
    sq = np.sum(u.A * u.A, axis=1)[:, None] + np.sum(c.A * c.A, axis=1)[None, :] + 2.0 * (u.A @ c.A.T)
    M = abs(w0) + u.Labs[:, None] + c.Labs[None, :] + 0.5 * (sq + u.Q[:, None] + c.Q[None, :])
    bound = (u.nnz[:, None] + c.nnz[None, :] + kp + 16) * 2.0 ** -52 * M
    return PairRef(key, learned, bound, float(w0))


def ref_order(key_row, n_top=None):
    """Candidate rows of one context in rank order: key descending, row ascending."""
    order = np.lexsort((np.arange(len(key_row)), -np.asarray(key_row)))
    return order if n_top is None else order[:n_top]


def concat_rows(contexts, candidates):
    """The U * C materialised rows (row u * C + c = u's entries, then c's) as (row_ptr, col, val)."""
    (rpu, cu, vu), (rpc, cc, vc) = contexts, candidates
    U, C = len(rpu) - 1, len(rpc) - 1
    cols, vals, rp = [], [], [0]
    for a in range(U):
        for b in range(C):
            cols.append(np.concatenate([cu[rpu[a]:rpu[a + 1]], cc[rpc[b]:rpc[b + 1]]]))
            vals.append(np.concatenate([vu[rpu[a]:rpu[a + 1]], vc[rpc[b]:rpc[b + 1]]]))
            rp.append(rp[-1] + len(cols[-1]))
    col = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, np.int32)
    val = np.concatenate(vals).astype(np.float64) if vals else np.zeros(0)
    return np.asarray(rp, np.int64), col, val


def f32(a):
    """Values a fp32 table holds exactly."""
    return np.asarray(a, np.float32).astype(np.float64)


def make_rows(rng, lens, id_hi, scale=1.0):
    """A CSR row set (row_ptr, col, val): row i has lens[i] distinct ids below id_hi (a run of
    consecutive ids from a random start, wrapping), fp32-exact values."""
    lens = np.asarray(lens, np.int64)
    assert lens.size == 0 or lens.max() <= id_hi
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = np.repeat(np.arange(len(lens)), lens)
    start = rng.integers(0, id_hi, len(lens))
    col = ((start[rows] + np.arange(len(rows)) - rp[rows]) % id_hi).astype(np.int32)
    val = f32(scale * rng.standard_normal(len(col)))
    return rp, col, val


def take_rows(rows, sel):
    """Rows sel (any order) of a row set."""
    rp, col, val = rows
    sel = np.asarray(sel, np.int64)
    lens = rp[sel + 1] - rp[sel]
    nrp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    src = np.repeat(rp[sel], lens) + np.arange(int(nrp[-1])) - np.repeat(nrp[:-1], lens)
    return nrp, col[src], val[src]


def make_table(rng, F, k, present_frac=0.85, scale=0.5):
    present = rng.random(F) < present_frac
    w = f32(scale * rng.standard_normal(F)) * present
    V = f32(scale * rng.standard_normal((F, k))) * present[:, None]
    return w, V, present
