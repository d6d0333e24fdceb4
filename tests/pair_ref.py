"""NumPy references of fm_batch_from_pairs / fm_batch_sample_pairs (include/fm_hip.h), and the planted
recommender problem the pair tests train on.

concat_pairs       the host CSR whose row i is context row pair_ctx[i] followed by candidate row pair_cand[i]
sample_negatives   the counter-based draw of the header, per (seed, positive i, negative j):
                       h = splitmix64(seed ^ splitmix64((i << 20) | j));  r = ((h >> 32) * E) >> 32
                       c = r + #{t : excl[t] - t <= r}        E = C - len(excl), excl the context's sorted list
sampled_pairs      the (pair_ctx, pair_cand, labels) of a sampled batch: each positive, then its negatives
planted()          U = 64 one-hot contexts (ids 0 .. 63), C = 256 one-hot candidates (ids 64 .. 319); context u
                   likes the 32 candidates with c % 8 == u % 8, split per context by one
                   default_rng(7) (a permutation per context, in context order) into 24 training positives and 8
                   held-out rows: 1536 interactions
oracle_fit         fitInteractions' loop on the fp64 oracle (oracle.fm_ref.sgd_step_fast) over these batches
"""

import functools
from dataclasses import dataclass

import numpy as np

from fm_spark_amd.data import splitmix64
from oracle import fm_ref as R

U64 = np.uint64


def concat_pairs(ctx_rows, cand_rows, pair_ctx, pair_cand, labels) -> R.CSR:
    """ctx_rows / cand_rows: (row_ptr, col, val)."""
    (rpu, cu, vu), (rpc, cc, vc) = ctx_rows, cand_rows
    rpu, rpc = np.asarray(rpu, np.int64), np.asarray(rpc, np.int64)
    pc, pd = np.asarray(pair_ctx, np.int64), np.asarray(pair_cand, np.int64)
    lu, lc = rpu[pc + 1] - rpu[pc], rpc[pd + 1] - rpc[pd]
    rp = np.concatenate([[0], np.cumsum(lu + lc)]).astype(np.int64)
    n = int(rp[-1])
    row = np.repeat(np.arange(len(pc)), lu + lc)
    j = np.arange(n) - rp[row]
    from_u = j < lu[row]
    col, val = np.zeros(n, np.int32), np.zeros(n)
    su = rpu[pc[row[from_u]]] + j[from_u]
    sc = rpc[pd[row[~from_u]]] + j[~from_u] - lu[row[~from_u]]
    col[from_u], val[from_u] = np.asarray(cu)[su], np.asarray(vu)[su]
    col[~from_u], val[~from_u] = np.asarray(cc)[sc], np.asarray(vc)[sc]
    return R.CSR(rp, col, val, np.asarray(labels, np.float64))


def draw_ranks(seed, n_pos, n_neg, E):
    """r [n_pos, n_neg]: the rank of every draw among its context's E[i] eligible rows."""
    i = np.arange(n_pos, dtype=U64)[:, None]
    j = np.arange(n_neg, dtype=U64)[None, :]
    h = splitmix64(U64(int(seed) & (2**64 - 1)) ^ splitmix64((i << U64(20)) | j))
    return (((h >> U64(32)) * np.asarray(E, U64)[:, None]) >> U64(32)).astype(np.int64)


def sample_negatives(seed, pos_ctx, n_neg, excl_ptr, excl_rows, C):
    """c [n_pos, n_neg]; excl_ptr None: nothing excluded."""
    pos_ctx = np.asarray(pos_ctx, np.int64)
    n_pos = len(pos_ctx)
    if excl_ptr is None:
        return draw_ranks(seed, n_pos, n_neg, np.full(n_pos, C))
    excl_ptr = np.asarray(excl_ptr, np.int64)
    L = excl_ptr[pos_ctx + 1] - excl_ptr[pos_ctx]
    r = draw_ranks(seed, n_pos, n_neg, C - L)
    out = np.zeros((n_pos, n_neg), np.int64)
    for i, u in enumerate(pos_ctx):
        excl = np.asarray(excl_rows[excl_ptr[u]:excl_ptr[u + 1]], np.int64)
        out[i] = r[i] + np.searchsorted(excl - np.arange(len(excl)), r[i], side="right")
    return out


def sampled_pairs(pos_ctx, pos_cand, negatives, pos_label=1.0, neg_label=0.0):
    """The sampled batch's rows: positive i at i (1 + n_neg), its negatives behind it."""
    negatives = np.asarray(negatives, np.int64)
    n_pos, n_neg = negatives.shape
    pc = np.repeat(np.asarray(pos_ctx, np.int64), 1 + n_neg)
    pd = np.concatenate([np.asarray(pos_cand, np.int64)[:, None], negatives], axis=1).reshape(-1)
    y = np.tile(np.concatenate([[pos_label], np.full(n_neg, neg_label)]), n_pos)
    return pc, pd, y


# ------------------------------------------------------------------------ planted problem
@dataclass
class Planted:
    U: int
    C: int
    F: int
    contexts: tuple      # (row_ptr, col, val)
    candidates: tuple
    pos_ctx: np.ndarray  # the 1536 training interactions, context after context
    pos_cand: np.ndarray
    train: list          # per context: its training rows, sorted (the exclude lists)
    held: list           # per context: its held-out rows, sorted
    excl_ptr: np.ndarray
    excl_rows: np.ndarray


K, SD, STEP, REG, FRAC, ITERS, NEG, SEED = 8, 0.1, 200.0, 0.0, 0.25, 300, 4, 0


@functools.lru_cache(maxsize=None)
def planted() -> Planted:
    U, C = 64, 256
    rng = np.random.default_rng(7)
    pc, pd, train, held = [], [], [], []
    for u in range(U):
        liked = rng.permutation(np.flatnonzero(np.arange(C) % 8 == u % 8))
        pc += [u] * 24
        pd += liked[:24].tolist()
        train.append(np.sort(liked[:24]))
        held.append(np.sort(liked[24:]))
    one_hot = lambda n, first: (np.arange(n + 1, dtype=np.int64), np.arange(first, first + n, dtype=np.int32), np.ones(n))
    ptr = np.arange(0, 24 * U + 1, 24, dtype=np.int64)
    return Planted(U, C, U + C, one_hot(U, 0), one_hot(C, U), np.asarray(pc), np.asarray(pd), train, held, ptr,
                   np.concatenate(train).astype(np.int32))


def batch_positives(n, seed, frac, t):
    """The positives (indices into the interactions) of iteration t = 1 ..: fitInteractions' rule."""
    m = max(1, int(round(frac * n)))
    perm = np.random.default_rng(seed).permutation(n)
    return perm[((t - 1) * m + np.arange(m)) % n]


def iteration_batch(p: Planted, t, seed=SEED, frac=FRAC, n_neg=NEG) -> R.CSR:
    take = batch_positives(len(p.pos_ctx), seed, frac, t)
    neg = sample_negatives(int(splitmix64(U64(seed))) ^ t, p.pos_ctx[take], n_neg, p.excl_ptr, p.excl_rows, p.C)
    return concat_pairs(p.contexts, p.candidates, *sampled_pairs(p.pos_ctx[take], p.pos_cand[take], neg))


def initial_model(p: Planted, seed=SEED) -> R.Model:
    m = R.Model.empty(p.F, K)
    ids = np.arange(p.F)
    m.load(ids, *R.init_draw(ids, K, seed, SD))
    return m


@functools.lru_cache(maxsize=None)
def oracle_fit(n_iter: int):
    """(model after n_iter iterations, [batches]) of the planted configuration on the oracle."""
    p = planted()
    m = initial_model(p)
    batches = [iteration_batch(p, t) for t in range(1, n_iter + 1)]
    for t, b in enumerate(batches, start=1):
        R.sgd_step_fast(m, b, t, STEP, REG)
    return m, batches


def held_out_metric(name, k, model: R.Model, p: Planted):
    """A RankingMetrics figure of the held-out rows among each context's rows outside its training list."""
    from fm_spark_amd.tuning import ranking_metric
    from rank_ref import pair_ref

    key = pair_ref(model.w, model.V, model.present, model.w0, p.contexts, p.candidates).key
    pos = []
    for u in range(p.U):
        ok = np.ones(p.C, bool)
        ok[p.train[u]] = False
        for c in p.held[u]:
            ahead = (key[u] > key[u, c]) | ((key[u] == key[u, c]) & (np.arange(p.C) < c))
            pos.append(int(np.sum(ahead & ok)))
    return ranking_metric(name, k, np.arange(0, 8 * p.U + 1, 8), np.asarray(pos), np.full(p.U, p.C - 24))[0]
