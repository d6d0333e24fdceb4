"""Measurement tool (not product): what popularity-weighted negatives cost beside uniform ones, at
tools/pair_bench.py's shape (c5's table; 65 536 contexts, 16 384 candidate rows, 200 excluded rows per
context resident as a RowLists; 52 429 positives x (1 + 4) rows per batch).

  (a) fm_row_weights_create and fm_row_weights_bind by HIP events (the library's profile: "weights_cdf",
      "weights_bind") and through the calls by the host clock;
  (b) the draw + scan alone by HIP events ("pair_draw"), uniform and weighted;
  (c) ms per iteration of the pipelined loop (sample, prepare, step; two batches in turn) with uniform and
      with weighted draws, in alternating repetitions, min - max.

--uniform-only measures the uniform halves of (b) and (c) alone and touches no weighted entry point: the same
file copied into a checkout of the parent commit gives the parent's uniform loop for the comparison.
Weights: a Zipf-like popularity (rank^-1 counts over a permutation of the rows) through popularity_weights.

Runs on the GPU only.  Writes profiles/weighted_neg/<name>.json.
  python tools/weighted_neg_bench.py [--uniform-only] [--name NAME] [iters] [reps]"""
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

args = sys.argv[1:]
uniform_only = "--uniform-only" in args
name = args[args.index("--name") + 1] if "--name" in args else "weighted_neg_bench"
nums = [int(a) for a in args if a.isdigit()]
iters, reps = (nums[0] if nums else 32), (nums[1] if len(nums) > 1 else 5)
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
start, stride = rng.integers(0, C, U), 2 * rng.integers(0, C // N_EXCL // 2, U) + 1
excl = np.sort((start[:, None] + stride[:, None] * np.arange(N_EXCL)[None, :]) % C, axis=1)
ex = (np.arange(0, U * N_EXCL + 1, N_EXCL, dtype=np.int64), np.ascontiguousarray(excl.reshape(-1), dtype=np.int32))
pos = [(rng.integers(0, U, N_POS).astype(np.int32), rng.integers(0, C, N_POS).astype(np.int32)) for _ in range(N_SETS)]
counts = np.zeros(C, np.int64)
counts[rng.permutation(C)] = (U * N_EXCL / np.arange(1, C + 1) / np.log(C)).astype(np.int64)

ctx = FMContext(F, k, seed=20261015, init_sd=bench.INIT_SD)  # no GPU: raises here
ctx.init_random_range(0, F)
bu = ctx.batch(CSRHost(*ctx_rows, np.zeros(U)))
bc = ctx.batch(CSRHost(*cand_rows, np.zeros(C)))
resident = ctx._row_lists(ex, C)
res = {"shape": {"features": F, "k": k, "contexts": U, "candidates": C, "excluded_per_context": N_EXCL, "positives": N_POS,
                 "negatives_per_positive": N_NEG, "rows_per_batch": N_POS * (1 + N_NEG)}, "iters": iters, "reps": reps}


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": len(v)}


def per_call(prof, key):
    return prof[key][0] / prof[key][1]


# ---- (a) the weights made resident and bound
rw = None
if not uniform_only:
    from fm_spark_amd.ml import popularity_weights

    weight = popularity_weights(counts, 0.75)
    ctx.row_weights(weight).bind(resident).close()  # warm-up
    ctx.profile_enable(True)
    ctx.profile_reset()
    create_ms, bind_ms = [], []
    for _ in range(reps):
        if rw is not None:
            rw.close()
        t0 = time.perf_counter()
        rw = ctx.row_weights(weight)
        t1 = time.perf_counter()
        rw.bind(resident)
        create_ms.append(1e3 * (t1 - t0))
        bind_ms.append(1e3 * (time.perf_counter() - t1))
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    res["a_weights"] = {"W": int(weight.sum()), "heaviest": int(weight.max()), "lightest": int(weight.min()),
                        "list_rows_bound": int(ex[0][-1]),
                        "cdf_scan_ms_hip_events": per_call(prof, "weights_cdf"),
                        "bind_ms_hip_events": per_call(prof, "weights_bind"),
                        "create_call_ms_host_clock": spread(create_ms), "bind_call_ms_host_clock": spread(bind_ms)}


def sample(j, into, weighted):
    pc, pd = pos[j % N_SETS]
    if weighted:
        return ctx._sample_pairs(bu, bc, pc, pd, N_NEG, resident, 1.0, 0.0, j, into, False, N_NEG, True, rw)
    return ctx._sample_pairs(bu, bc, pc, pd, N_NEG, resident, 1.0, 0.0, j, into, False)


def loop(bufs, weighted):
    t0 = time.perf_counter()
    bufs[1] = sample(1, bufs[1], weighted)
    bufs[1].prepare()
    for t in range(1, iters + 1):
        ctx.step_batch(bufs[t % 2], t, bench.STEP_SIZE, bench.REG_PARAM, sync=False)
        if t < iters:
            bufs[(t + 1) % 2] = sample(t + 1, bufs[(t + 1) % 2], weighted)
            bufs[(t + 1) % 2].prepare()
    ctx.sync()
    return 1e3 * (time.perf_counter() - t0) / iters


kinds = [False] if uniform_only else [False, True]
label = {False: "uniform", True: "weighted"}

# ---- (b) the draw + scan alone
res["b_draw_scan_ms_hip_events"] = {}
for weighted in kinds:
    into = None
    for j in range(3):  # warm-up
        into = sample(j, into, weighted)
    ctx.sync()
    ctx.profile_enable(True)
    ctx.profile_reset()
    for j in range(4 * reps):
        into = sample(j, into, weighted)
        ctx.sync()
    res["b_draw_scan_ms_hip_events"][label[weighted]] = per_call(ctx.profile_read(), "pair_draw")
    ctx.profile_enable(False)
    into.close()

# ---- (c) the pipelined loops, alternating
bufs = [None, None]
for weighted in kinds:
    loop(bufs, weighted)  # warm-up
ms = {w: [] for w in kinds}
for _ in range(reps):
    for weighted in kinds:
        ms[weighted].append(loop(bufs, weighted))
res["c_pipelined_loop_ms_per_iter"] = {label[w]: spread(v) for w, v in ms.items()}
if not uniform_only:
    res["c_pipelined_loop_ms_per_iter"]["ratio_of_medians_weighted_to_uniform"] = float(np.median(ms[True]) / np.median(ms[False]))

out = os.path.join(ROOT, "profiles", "weighted_neg")
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, name + ".json"), "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res, indent=1))
