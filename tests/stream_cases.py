"""Inputs of the stream-order scenarios (tests/test_gpu_stream_order.py), NumPy only, and the fp64
oracle's statement that every scenario can see a lost wait (tests/test_stream_cases_cpu.py).

One dataset of N_SEL * ROWS rows over F features, every row of exactly LEN entries, so every selection
of ROWS rows, every split, and every pair batch (a context row of CTX_LEN entries followed by a
candidate row of CAND_LEN = LEN - CTX_LEN) holds ROWS rows and ROWS * LEN entries.  That gives the GPU
scenarios two guarantees: no call of a measured round grows a device buffer (a growth drains the
device and would hide the held-back lane), and a lost wait can only read valid, in-range, stale data
of the same shape -- a failure is a wrong bit, never a fault.

A scenario's contents are named by keys: "S<i>" selection i of the dataset, "V<s>" its split s (rows
[s * ROWS, (s + 1) * ROWS)), "P<j>" pair batch j.  SCENARIOS names, per scenario family, the contents
its steps read in program order and the contents they would read were the wait under test lost: the
step reading the batch's previous contents (a reader that runs before the refill, or before the sort
of the new contents), or the refill landing before the step.
"""

from __future__ import annotations

from functools import lru_cache

import numpy as np

from oracle import fm_ref as R
from problems import make_rows

F = 300
ROWS = 200
LEN = 7
KS = (8, 16)
STEP, REG = 0.2, 1e-4
N_SEL = 6
SEED_DATA, SEED_SEL, SEED_PAIR = 300, 301, 302
CTX_LEN, CAND_LEN = 3, 4
N_CTX, N_CAND = 64, 96
N_POS, N_NEG = 50, 3  # N_POS * (1 + N_NEG) == ROWS
RTOL, ATOL = 1e-5, 1e-8  # tests/test_gpu_parity.py
SEPARATION = 10.0  # a lost wait moves a word by more than this many tolerances

assert LEN == CTX_LEN + CAND_LEN and N_POS * (1 + N_NEG) == ROWS


@lru_cache(maxsize=None)
def dataset(k):
    """(csr, ids, w, V): the dataset and the tables every scenario starts from."""
    return make_rows(SEED_DATA, np.full(N_SEL * ROWS, LEN), F, k)


def take(csr, rows):
    rows = np.asarray(rows, dtype=np.int64)
    lens = np.diff(csr.row_ptr)[rows]
    idx = np.concatenate([np.arange(csr.row_ptr[r], csr.row_ptr[r + 1]) for r in rows]) if len(rows) else np.zeros(0, np.int64)
    return R.CSR(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), csr.col[idx], csr.val[idx], csr.label[rows])


@lru_cache(maxsize=None)
def selection(i):
    """Selection i: ROWS rows of the dataset, drawn from all of it, in no particular order."""
    return np.random.default_rng(SEED_SEL + i).permutation(N_SEL * ROWS)[:ROWS].astype(np.int64)


def split_rows():
    return np.arange(N_SEL + 1, dtype=np.int64) * ROWS


@lru_cache(maxsize=None)
def pair_sources():
    """(contexts, candidates): rows of CTX_LEN entries over ids [0, F / 2) and of CAND_LEN entries over
    [F / 2, F), so a pair row's ids are distinct."""
    u = make_rows(SEED_PAIR, np.full(N_CTX, CTX_LEN), F // 2, 1)[0]
    c = make_rows(SEED_PAIR + 1, np.full(N_CAND, CAND_LEN), F // 2, 1)[0]
    c = R.CSR(c.row_ptr, (c.col + F // 2).astype(np.int32), c.val, c.label)
    return u, c


@lru_cache(maxsize=None)
def pair_list(j):
    """(pair_ctx, pair_cand, labels) of pair batch j: ROWS pairs."""
    rng = np.random.default_rng(SEED_PAIR + 10 + j)
    return (rng.integers(0, N_CTX, ROWS).astype(np.int32), rng.integers(0, N_CAND, ROWS).astype(np.int32),
            (rng.random(ROWS) < 0.25).astype(np.float64))


@lru_cache(maxsize=None)
def positives(j):
    """(pos_ctx, pos_cand, exclude lists) of sampled pair batch j: N_POS positives, each context's
    exclude list its own positives' candidate rows."""
    rng = np.random.default_rng(SEED_PAIR + 20 + j)
    pc = rng.integers(0, N_CTX, N_POS).astype(np.int32)
    pd = rng.integers(0, N_CAND, N_POS).astype(np.int32)
    lists = [sorted({int(d) for c, d in zip(pc, pd) if c == u}) for u in range(N_CTX)]
    return pc, pd, lists


def pair_batch(j):
    """Pair batch j as fm_batch_from_pairs builds it: row i = the context row's entries, then the
    candidate row's."""
    u, c = pair_sources()
    pc, pd, y = pair_list(j)
    col = np.concatenate([np.concatenate([u.col[u.row_ptr[a]:u.row_ptr[a + 1]], c.col[c.row_ptr[b]:c.row_ptr[b + 1]]])
                          for a, b in zip(pc, pd)])
    val = np.concatenate([np.concatenate([u.val[u.row_ptr[a]:u.row_ptr[a + 1]], c.val[c.row_ptr[b]:c.row_ptr[b + 1]]])
                          for a, b in zip(pc, pd)])
    return R.CSR(np.arange(ROWS + 1, dtype=np.int64) * LEN, col.astype(np.int32), val, y.copy())


@lru_cache(maxsize=None)
def contents(k, key):
    """The CSR a key names."""
    csr = dataset(k)[0]
    kind, n = key[0], int(key[1:])
    if kind == "S":
        return take(csr, selection(n))
    if kind == "V":
        return take(csr, np.arange(n * ROWS, (n + 1) * ROWS))
    if kind == "P":
        return pair_batch(n)
    raise KeyError(key)


# family -> (what the steps read in program order, what they read when the wait under test is lost)
SCENARIOS = {
    # two batches stepped in turn: the second step's sort (or its refill) lands before the first step's
    # update has read -> the first update works on the second batch's view
    "two_batches": (["S0", "S1"], ["S1", "S1"]),
    # a batch refilled, then read: the reader runs first and sees the previous contents
    "refill_then_read": (["S0", "S1"], ["S0", "S0"]),
    # a batch stepped, then refilled: the refill lands first and the step reads the new contents
    "read_then_refill": (["S0", "S1"], ["S1", "S1"]),
    # the same through split views (a re-pointed view's new sort lands in the view the step reads)
    "views": (["V0", "V1"], ["V1", "V1"]),
    # the same through pair batches
    "pairs": (["P0", "P1"], ["P1", "P1"]),
    # fm_step's two upload slots, five host batches: the third upload lands in slot 0 before the
    # first step has read it
    "host_slots": (["S0", "S1", "S2", "S3", "S4"], ["S2", "S1", "S2", "S3", "S4"]),
    # the fit's loop: six iterations over two batches; a lost wait anywhere makes one iteration read
    # its batch's previous or next contents (here: iteration 3 reads what iteration 1 read)
    "fit_loop": (["S0", "S1", "S2", "S3", "S4", "S5"], ["S0", "S1", "S0", "S3", "S4", "S5"]),
}


def oracle_run(k, keys, t0=1, model=None):
    """sgd_step_fast over the keys' contents from the scenario tables (or `model`, in place):
    (loss sums, model)."""
    _, ids, w, V = dataset(k)
    if model is None:
        model = R.Model.empty(F, k)
        model.load(ids, w, V)
    losses = []
    for i, key in enumerate(keys):
        losses.append(R.sgd_step_fast(model, contents(k, key), t0 + i, STEP, REG).loss_sum)
    return np.asarray(losses), model


def separation(k, family):
    """The largest |program - lost| / (ATOL + RTOL |program|) over the loss sums and the table words."""
    program, lost = SCENARIOS[family]
    la, ma = oracle_run(k, program)
    lb, mb = oracle_run(k, lost)
    worst = 0.0
    for a, b in ((la, lb), (ma.w, mb.w), (ma.V, mb.V)):
        worst = max(worst, float(np.max(np.abs(a - b) / (ATOL + RTOL * np.abs(a)))))
    return worst


def prediction_separation(k, a, b):
    """The same for the unclamped predictions of contents a and b under the scenario tables (the readers
    that do not step: predict, evaluate, rank)."""
    _, ids, w, V = dataset(k)
    model = R.Model.empty(F, k)
    model.load(ids, w, V)
    pa = R.predict(model, contents(k, a), -np.inf, np.inf)
    pb = R.predict(model, contents(k, b), -np.inf, np.inf)
    return float(np.max(np.abs(pa - pb) / (ATOL + RTOL * np.abs(pa))))
