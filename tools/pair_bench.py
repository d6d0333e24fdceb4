"""Measurement tool (not product): what building a recommender's mini-batch on the device costs, against
the host route it replaces and against the split-view fit loop.

Shape: c5's table (1M features, k = 16); 65 536 context rows of about 20 entries, 16 384 candidate rows of
13; 200 excluded rows per context; 52 429 positives x (1 + 4) = 262 145 rows per batch.

  (a) the device build per batch: fm_batch_sample_pairs' draw + scan and its gather by HIP events (the
      library's profile), and the call through ctx.sync() by the host clock;
  (b) the route it replaces: a NumPy draw + concatenation + fm_batch_create of the same rows, host clock;
  (c) ms per iteration of the pipelined loop (sample, prepare, step; two batches in turn) against the same
      loop over split views of a resident dataset of the same rows -- the fit's own fastest path -- with the
      exclude lists as host arrays at every call, resident (a RowLists made once), and absent;
  (d) building those lists on the device from their 13.1M (context, row) pairs (fm_lists_from_pairs), by HIP
      events (the sorts through the compaction) and through the call by the host clock, beside a vectorised
      NumPy build (lexsort + unique + bincount) of the same lists.

Runs on the GPU only: without one the context constructor raises.  Writes profiles/pairs/pair_bench.json.
  python tools/pair_bench.py [iters] [reps]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from fm_spark_amd._native import CSRHost  # noqa: E402
from fm_spark_amd.engine import FMContext  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 32
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
F, k = bench.CONFIGS["c5"][:2]
U, C, N_EXCL, N_POS, N_NEG, N_SETS = 65_536, 16_384, 200, 52_429, 4, 4
rng = np.random.default_rng(20261021)


def rows(n, lens, lo, hi):
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = rng.integers(lo, hi, int(rp[-1])).astype(np.int32)
    val = np.where(rng.random(len(col)) < 0.7, 1.0, rng.standard_normal(len(col))).astype(np.float32).astype(np.float64)
    return rp, col, val


ctx_rows = rows(U, rng.integers(16, 25, U), 0, F // 2)
cand_rows = rows(C, np.full(C, 13), F // 2, F)
# 200 distinct rows per context: a random start and an odd stride below C / 200, sorted
start, stride = rng.integers(0, C, U), 2 * rng.integers(0, C // N_EXCL // 2, U) + 1
excl = np.sort((start[:, None] + stride[:, None] * np.arange(N_EXCL)[None, :]) % C, axis=1)
ex = (np.arange(0, U * N_EXCL + 1, N_EXCL, dtype=np.int64), np.ascontiguousarray(excl.reshape(-1), dtype=np.int32))
pos = [(rng.integers(0, U, N_POS).astype(np.int32), rng.integers(0, C, N_POS).astype(np.int32)) for _ in range(N_SETS)]

ctx = FMContext(F, k, seed=20261015, init_sd=bench.INIT_SD)  # no GPU: raises here
ctx.init_random_range(0, F)
bu = ctx.batch(CSRHost(*ctx_rows, np.zeros(U)))
bc = ctx.batch(CSRHost(*cand_rows, np.zeros(C)))
res = {"shape": {"features": F, "k": k, "contexts": U, "candidates": C, "excluded_per_context": N_EXCL, "positives": N_POS,
                 "negatives_per_positive": N_NEG, "rows_per_batch": N_POS * (1 + N_NEG)}, "iters": iters, "reps": reps}


resident = ctx._row_lists(ex, C)  # (ex is normalised as built)


def sample(j, into, lists=True):
    """lists: True -- the host arrays at every call; "resident" -- the RowLists; False -- none"""
    pc, pd = pos[j % N_SETS]
    given = resident if lists == "resident" else ex if lists else (None, None)
    return ctx._sample_pairs(bu, bc, pc, pd, N_NEG, given, 1.0, 0.0, j, into, False)


def host_rows(j):
    """(b)'s host part: the draw (uniform over each context's rows outside its list) and the concatenated CSR."""
    pc, pd = pos[j % N_SETS]
    r = rng.integers(0, C - N_EXCL, (N_POS, N_NEG))
    key = excl[pc] - np.arange(N_EXCL)[None, :]                       # [n_pos, 200], non-decreasing per row
    neg = r + np.sum(key[:, None, :] <= r[:, :, None], axis=2)        # the r-th eligible row
    qc = np.repeat(pc.astype(np.int64), 1 + N_NEG)
    qd = np.concatenate([pd[:, None].astype(np.int64), neg], axis=1).reshape(-1)
    y = np.tile(np.concatenate([[1.0], np.zeros(N_NEG)]), N_POS)
    (rpu, cu, vu), (rpc, cc, vc) = ctx_rows, cand_rows
    lu, lc = rpu[qc + 1] - rpu[qc], rpc[qd + 1] - rpc[qd]
    rp = np.concatenate([[0], np.cumsum(lu + lc)]).astype(np.int64)
    row = np.repeat(np.arange(len(qc)), lu + lc)
    jj = np.arange(int(rp[-1])) - rp[row]
    fu = jj < lu[row]
    su, sc = (rpu[qc[row]] + jj)[fu], (rpc[qd[row]] + jj - lu[row])[~fu]
    col, val = np.empty(len(row), np.int32), np.empty(len(row))
    col[fu], val[fu] = cu[su], vu[su]
    col[~fu], val[~fu] = cc[sc], vc[sc]
    return rp, col, val, y, neg


def host_build(j):
    """(b): host_rows, then fm_batch_create of them."""
    csr = CSRHost(*host_rows(j)[:4])
    return csr, ctx.batch(csr)


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": len(v)}


# ---- (a) the device build alone
into = sample(0, None)
ctx.sync()
for j in range(3):  # warm-up: scratch and the batch grown
    into = sample(j, into)
ctx.sync()
ctx.profile_enable(True)
ctx.profile_reset()
host_ms = []
for j in range(4 * reps):
    t0 = time.perf_counter()
    into = sample(j, into)
    ctx.sync()
    host_ms.append(1e3 * (time.perf_counter() - t0))
prof = ctx.profile_read()
ctx.profile_enable(False)
res["a_device_build"] = {
    "rows": into.n_rows, "entries": into.nnz,
    "draw_scan_ms_hip_events": prof["pair_draw"][0] / prof["pair_draw"][1],
    "gather_ms_hip_events": prof["pair_gather"][0] / prof["pair_gather"][1],
    "call_to_sync_ms_host_clock": spread(host_ms),
    # the exclude lists' share of the call: the host's check and staging copy (host clock inside the library), the upload
    "lists_check_ms_host": prof["pair_lists_check"][0] / prof["pair_lists_check"][1],
    "lists_stage_ms_host": prof["pair_lists_stage"][0] / prof["pair_lists_stage"][1],
    "lists_upload_ms_hip_events": prof["pair_lists_upload"][0] / prof["pair_lists_upload"][1],
}

# ---- (b) the host route, and the split dataset of its rows for (c)
host_ms, csrs = [], []
for j in range(N_SETS + 1):
    t0 = time.perf_counter()
    csr, b = host_build(j)
    ctx.sync()
    dt = 1e3 * (time.perf_counter() - t0)
    b.close()
    if j:  # the first is warm-up
        host_ms.append(dt)
        csrs.append(csr)
res["b_host_route"] = {"numpy_draw_concat_and_fm_batch_create_ms_host_clock": spread(host_ms)}
split_rows = np.concatenate([[0], np.cumsum([c.n_rows for c in csrs])])
off = np.cumsum([0] + [c.nnz for c in csrs])
data = ctx.batch_splits(CSRHost(np.concatenate([csrs[0].row_ptr] + [c.row_ptr[1:] + o for c, o in zip(csrs[1:], off[1:])]),
                                np.concatenate([c.col for c in csrs]), np.concatenate([c.val for c in csrs]),
                                np.concatenate([c.label for c in csrs])), split_rows)
res["c_split_dataset"] = {"rows_per_split": [int(c.n_rows) for c in csrs], "entries_per_split": [int(c.nnz) for c in csrs]}
del csrs


# ---- (c) the pipelined loops
def loop_pairs(bufs, lists=True):
    t0 = time.perf_counter()
    bufs[1] = sample(1, bufs[1], lists)
    bufs[1].prepare()
    for t in range(1, iters + 1):
        ctx.step_batch(bufs[t % 2], t, bench.STEP_SIZE, bench.REG_PARAM, sync=False)
        if t < iters:
            bufs[(t + 1) % 2] = sample(t + 1, bufs[(t + 1) % 2], lists)
            bufs[(t + 1) % 2].prepare()
    ctx.sync()
    return 1e3 * (time.perf_counter() - t0) / iters


def loop_views(bufs):
    t0 = time.perf_counter()
    bufs[1] = ctx.split_view(data, 1 % N_SETS, into=bufs[1])
    bufs[1].prepare()
    for t in range(1, iters + 1):
        ctx.step_batch(bufs[t % 2], t, bench.STEP_SIZE, bench.REG_PARAM, sync=False)
        if t < iters:
            bufs[(t + 1) % 2] = ctx.split_view(data, (t + 1) % N_SETS, into=bufs[(t + 1) % 2])
            bufs[(t + 1) % 2].prepare()
    ctx.sync()
    return 1e3 * (time.perf_counter() - t0) / iters


pb, vb = [None, None], [None, None]
loop_pairs(pb)  # warm-up: both loops' buffers grown
loop_views(vb)
loop_pairs(pb, lists=False)
loop_pairs(pb, lists="resident")
pairs_ms, views_ms, free_ms, resident_ms = [], [], [], []
for _ in range(reps):  # alternating
    pairs_ms.append(loop_pairs(pb))
    resident_ms.append(loop_pairs(pb, lists="resident"))
    views_ms.append(loop_views(vb))
    free_ms.append(loop_pairs(pb, lists=False))
# where the pair loop's host time goes: the sample call alone on an idle device, with the exclude lists (13.1M
# rows checked, staged and uploaded by every call) and without them (excl_ptr = NULL)
t_call, t_free, t_res = [], [], []
for t in range(1, 25):
    t0 = time.perf_counter()
    pb[t % 2] = sample(t, pb[t % 2], lists=(True, False, "resident")[t % 3])
    (t_call, t_free, t_res)[t % 3].append(1e3 * (time.perf_counter() - t0))
    ctx.sync()
res["c_pipelined_loop"] = {
    "pairs_ms_per_iter": spread(pairs_ms), "split_views_ms_per_iter": spread(views_ms),
    "ratio_of_medians": float(np.median(pairs_ms) / np.median(views_ms)),
    "pairs_without_exclude_lists_ms_per_iter": spread(free_ms),
    "ratio_without_exclude_lists": float(np.median(free_ms) / np.median(views_ms)),
    "sample_call_host_ms_idle_device": spread(t_call),
    "sample_call_without_exclude_lists_host_ms_idle_device": spread(t_free),
    # the same loop with the lists resident (fm_batch_sample_pairs_lists): no check, staging or upload per call
    "pairs_resident_lists_ms_per_iter": spread(resident_ms),
    "ratio_resident_to_host_lists": float(np.median(resident_ms) / np.median(pairs_ms)),
    "ratio_resident_to_without_exclude_lists": float(np.median(resident_ms) / np.median(free_ms)),
    "ratio_resident_to_split_views": float(np.median(resident_ms) / np.median(views_ms)),
    "sample_call_resident_lists_host_ms_idle_device": spread(t_res),
}


# ---- (d) the lists built on the device from their pairs, beside a vectorised NumPy build
def numpy_lists(pc, pd, n_ctx):
    order = np.lexsort((pd, pc))
    sc, sd = pc[order], pd[order]
    head = np.ones(len(sc), dtype=bool)
    head[1:] = (sc[1:] != sc[:-1]) | (sd[1:] != sd[:-1])
    ptr = np.zeros(n_ctx + 1, dtype=np.int64)
    np.cumsum(np.bincount(sc[head], minlength=n_ctx), out=ptr[1:])
    return ptr, sd[head].astype(np.int32)


shuffle = rng.permutation(U * N_EXCL)  # the lists' own pairs, in no order
lp_ctx = np.repeat(np.arange(U, dtype=np.int32), N_EXCL)[shuffle]
lp_cand = ex[1][shuffle]
ctx.row_lists_from_pairs(lp_ctx, lp_cand, U, C).close()  # warm-up
ctx.profile_enable(True)
ctx.profile_reset()
build_ms = []
for _ in range(reps):
    t0 = time.perf_counter()
    built = ctx.row_lists_from_pairs(lp_ctx, lp_cand, U, C)
    build_ms.append(1e3 * (time.perf_counter() - t0))
    got = built.export()
    built.close()
prof = ctx.profile_read()
ctx.profile_enable(False)
assert got[0].tobytes() == ex[0].tobytes() and got[1].tobytes() == ex[1].tobytes()  # the lists the loops used
numpy_ms = []
for _ in range(2):
    t0 = time.perf_counter()
    want = numpy_lists(lp_ctx, lp_cand, U)
    numpy_ms.append(1e3 * (time.perf_counter() - t0))
assert want[0].tobytes() == ex[0].tobytes() and want[1].tobytes() == ex[1].tobytes()
res["d_lists_from_pairs"] = {
    "pairs": int(U * N_EXCL), "list_rows": int(ex[0][-1]),
    "device_ms_hip_events": prof["lists_build"][0] / prof["lists_build"][1],
    "call_ms_host_clock": spread(build_ms),
    "numpy_lexsort_unique_bincount_ms_host_clock": spread(numpy_ms),
}
out = os.path.join(ROOT, "profiles", "pairs")
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, "pair_bench.json"), "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res, indent=1))
