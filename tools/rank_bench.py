"""Measurement tool (not product): top-N ranking on the device against the only route without it.
c5's table (F = 1M, k = 16, random init), U = 64 contexts of 26 entries, C = 16384 candidates of 13
entries, n_top = 100.  In one process, warmed, three repetitions alternating:
  subject   FMContext.rank_batch on the two resident row sets (host clock around `calls` calls, each of
            which ends in a stream synchronise and the copy of its U x n_top results);
  baseline  FMContext.predict_batch over the resident U * C materialised rows (row u C + c = u's
            entries, then c's): the device time of its forward alone (the library's event profile,
            taken in a pass of its own after the timed windows), with the host clock of the whole
            call beside it.  What the route costs besides -- building the rows on the host, uploading
            them, the NumPy top-N of the U * C scores -- is timed once each and reported separately.
The two results are compared: the materialised route's top-N by (score descending, row ascending)
against rank_batch's rows, and the scores.  Bytes and operations are counted from the shapes.
Prints one JSON object (and writes it to --out).
  python tools/rank_bench.py [--out FILE] [--calls N] [--reps N] [--rank-only]
--rank-only: the subject's calls alone, for a kernel trace (rocprofv3 --kernel-trace --stats -- python ...)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from fm_spark_amd._native import CSRHost  # noqa: E402
from fm_spark_amd.engine import FMContext  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rank-only", action="store_true")
args = ap.parse_args()

F, k, _, _, _ = bench.CONFIGS["c5"]
U, ZU, C, ZC, N_TOP = 64, 26, 16384, 13, 100
CHUNK, MAX_SPLITS, TARGET_BLOCKS = 1024, 64, 512  # fm_rank.hip: kRankChunk, kRankMaxSplits, kRankTargetBlocks
INF = float("inf")


def log(msg):
    print(msg, file=sys.stderr, flush=True)


rng = np.random.default_rng(20261020)
# contexts draw their ids below F / 2 (a user and their history), candidates above (an item and its tags)
cu_col = rng.integers(0, F // 2, (U, ZU)).astype(np.int32)
cc_col = rng.integers(F // 2, F, (C, ZC)).astype(np.int32)
cu_val = rng.standard_normal((U, ZU)).astype(np.float32).astype(np.float64)
cc_val = rng.standard_normal((C, ZC)).astype(np.float32).astype(np.float64)
contexts = CSRHost(np.arange(U + 1, dtype=np.int64) * ZU, cu_col.ravel(), cu_val.ravel(), np.zeros(U))
candidates = CSRHost(np.arange(C + 1, dtype=np.int64) * ZC, cc_col.ravel(), cc_val.ravel(), np.zeros(C))

ctx = FMContext(F, k, seed=20261015, init_sd=bench.INIT_SD)
ctx.init_random_range(0, F)
ctx.sync()
bu, bc = ctx.batch(contexts), ctx.batch(candidates)


def rank_window(calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        out = ctx.rank_batch(bu, bc, N_TOP, -INF, INF)
    return (time.perf_counter() - t0) / calls, out


if args.rank_only:
    rank_window(3)
    per_call, _ = rank_window(args.calls)
    print(json.dumps({"rank_batch_s_per_call_under_trace": per_call, "calls": args.calls}), flush=True)
    sys.exit(0)

# ---- the materialised route's host work, once
t0 = time.perf_counter()
Z = ZU + ZC
m_col = np.empty((U, C, Z), dtype=np.int32)
m_val = np.empty((U, C, Z), dtype=np.float64)
m_col[:, :, :ZU], m_col[:, :, ZU:] = cu_col[:, None, :], cc_col[None, :, :]
m_val[:, :, :ZU], m_val[:, :, ZU:] = cu_val[:, None, :], cc_val[None, :, :]
pairs = CSRHost(np.arange(U * C + 1, dtype=np.int64) * Z, m_col.ravel(), m_val.ravel(), np.zeros(U * C))
t_build = time.perf_counter() - t0
t0 = time.perf_counter()
bp = ctx.batch(pairs)
ctx.sync()
t_upload = time.perf_counter() - t0
del m_col, m_val
log(f"materialised {U * C} rows, {U * C * Z} entries: host build {t_build:.3f} s, upload {t_upload:.3f} s")

# ---- warm, then alternate
rank_window(3)
ctx.predict_batch(bp, -INF, INF)
rank_s, pred_call_s = [], []
for rep in range(args.reps):
    per_call, (r_idx, r_score) = rank_window(args.calls)
    t0 = time.perf_counter()
    pred = ctx.predict_batch(bp, -INF, INF)
    t1 = time.perf_counter()
    rank_s.append(per_call)
    pred_call_s.append(t1 - t0)
    log(f"rep {rep}: rank_batch {per_call * 1e3:.3f} ms per call ({args.calls} calls)   predict_batch call {(t1 - t0) * 1e3:.3f} ms")

# ---- device times by the library's events, a pass of its own
ctx.profile_enable(True)
ctx.profile_reset()
for rep in range(args.reps):
    rank_window(args.calls)
    ctx.predict_batch(bp, -INF, INF)
prof = ctx.profile_read()
ctx.profile_enable(False)
dev_ms = {name: ms / n for name, (ms, n) in prof.items()}

# ---- the materialised route's host top-N, and the comparison
t0 = time.perf_counter()
scores = pred.reshape(U, C)
part = np.argpartition(-scores, N_TOP - 1, axis=1)[:, :N_TOP]
m_idx = np.empty((U, N_TOP), dtype=np.int64)
for u in range(U):
    p = part[u]
    m_idx[u] = p[np.lexsort((p, -scores[u, p]))]
t_sort = time.perf_counter() - t0
rows = np.arange(U)[:, None]
same_rows = int(np.sum(m_idx == r_idx))
max_diff = float(np.max(np.abs(r_score - scores[rows, r_idx])))

kp = (k + 3) // 4 * 4
line = 128  # bytes of one table record at k = 16 (fm_internal.h record_stride)
nch = -(-C // CHUNK)
splits = min(nch, MAX_SPLITS, -(-TARGET_BLOCKS // U))  # fm_rank.hip rank_splits
stages = sum(range(1, CHUNK.bit_length()))  # compare-exchange stages of one chunk sort: 55
width = 1 << (N_TOP - 1).bit_length()       # a list's width in LDS: the power of two that holds n_top
fold = width.bit_length()                   # stages of one fold: the elementwise best, then log2(width) merges
counted = {
    "rank_summary": {"table_rows_gathered": U * ZU + C * ZC, "table_bytes": (U * ZU + C * ZC) * line,
                     "entry_bytes": (U * ZU + C * ZC) * 8, "summary_bytes_written": (U + C) * ((kp + 2) * 8 + 4)},
    "rank_score": {"fp64_flops": 2 * kp * U * C + 3 * U * C, "summary_bytes_read_per_context": C * (kp + 1) * 8 + C * 4,
                   "summary_bytes_read_all_contexts": U * (C * (kp + 1) * 8 + C * 4),
                   "summary_bytes_distinct": C * (kp + 1) * 8 + C * 4, "blocks": U * splits, "chunk_sorts": U * nch,
                   "compare_exchanges": U * nch * stages * CHUNK // 2 + U * (nch - splits) * fold * width // 2,
                   "barrier_stages_per_block": -(-nch // splits) * stages + (-(-nch // splits) - 1) * fold,
                   "list_bytes_written": U * splits * N_TOP * 12},
    "rank_merge": {"list_bytes_read": U * splits * N_TOP * 12, "compare_exchanges": U * (splits - 1) * fold * width // 2,
                   "barrier_stages_per_block": (splits - 1) * fold,
                   "result_bytes": U * N_TOP * 12},
    "materialised_predict": {"table_rows_gathered": U * C * Z, "table_bytes": U * C * Z * line,
                             "entry_bytes": U * C * Z * 8, "result_bytes": U * C * 8},
}
rank_dev_ms = sum(dev_ms.get(n, 0.0) for n in ("rank_summary", "rank_score", "rank_merge"))
res = {
    "config": "c5 table", "F": F, "k": k, "contexts": U, "context_entries": ZU, "candidates": C, "candidate_entries": ZC,
    "n_top": N_TOP, "calls_per_window": args.calls, "reps": args.reps,
    "rank_batch_s_per_call": rank_s, "rank_batch_spread_s": max(rank_s) - min(rank_s),
    "device_ms_per_call": dev_ms, "rank_device_ms_per_call": rank_dev_ms,
    "materialised": {"predict_device_ms": dev_ms.get("predict"), "predict_batch_call_s": pred_call_s,
                     "host_build_s": t_build, "upload_s": t_upload, "host_top_n_s": t_sort},
    "predict_device_over_rank_call": dev_ms.get("predict", 0.0) * 1e-3 / max(rank_s),
    "agreement": {"equal_rows": same_rows, "of": U * N_TOP, "max_abs_score_diff": max_diff,
                  "max_abs_score": float(np.max(np.abs(r_score)))},
    "counted_from_shapes": counted,
    "what": "host clock per rank_batch call (stream synchronise and result copy inside) over windows of `calls` calls, "
            "alternating with one predict_batch over the resident materialised rows; device_ms_per_call: the library's "
            "event profile in a later pass of the same process",
}
text = json.dumps(res, indent=1)
print(text, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
assert max_diff <= 1e-12 * (1.0 + res["agreement"]["max_abs_score"]), "the two routes' scores differ"
