"""Measurement tool (not product): the binary evaluation on the device (fm_evaluate_binary_batch) against the
route it replaces and against its neighbours.  Two workloads on one GPU, eval_bench's: c5's table and batch
(F = 1M, k = 16, 65,536 rows) and a c3-shaped resident batch (F = 100M, k = 16, 262,144 rows), click labels,
tables random-initialised.  In one process, warmed, `--reps` repetitions alternating, min-max reported:
  1. device time by the library's event profile (a pass of its own per call kind): "evaluate_binary" (the score
     pass, the per-row pass, the two sorts, the scan, the pair count, the fold) with "binary_sort" and
     "binary_count" inside it, against "evaluate" (fm_evaluate_batch) and "predict" (fm_predict_batch) on the
     same batch;
  2. host wall time per call, windows of `--calls` calls: evaluate_binary_batch synchronous (one 56-byte
     record back), evaluate_binary_batch enqueue-only (the window ends in one sync, reported per call both
     with and without it), and the route it replaces: predict_batch(-inf, inf) (B doubles back) + NumPy log
     loss + a stable-argsort AUC (tuning.binary_sums).
The two routes' integers must be equal and their log loss agree to 1e-12 relative.  Prints one JSON object (and
writes it to --out).
  python tools/binary_eval_bench.py [--out FILE, default profiles/binary_eval/binary_eval_bench.json] [--calls N] [--reps N] [--configs c5,c3]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from fm_spark_amd._native import CSRHost  # noqa: E402
from fm_spark_amd.data import synthetic_batch  # noqa: E402
from fm_spark_amd.engine import FMContext  # noqa: E402
from fm_spark_amd.tuning import binary_sums  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "binary_eval",
                                              "binary_eval_bench.json"))
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--configs", default="c5,c3")
args = ap.parse_args()
INF = math.inf


def log(msg):
    print(msg, file=sys.stderr, flush=True)


def span(v):
    return {"min": min(v), "max": max(v), "all": v}


def run(name):
    F, k, B, zipf_s, _ = bench.CONFIGS[name]
    t0 = time.perf_counter()
    hb = synthetic_batch(B, F, batch_index=7000, zipf_s=zipf_s)
    ctx = FMContext(F, k, seed=20261021, init_sd=bench.INIT_SD)
    ctx.init_random_range(0, F)
    b = ctx.batch(CSRHost(hb.row_ptr, hb.col, hb.val, hb.label))
    ctx.sync()
    log(f"{name}: {B} rows, {len(hb.col)} entries, table of {F} rows ready in {time.perf_counter() - t0:.1f} s")
    y = np.asarray(hb.label, dtype=np.float64)

    def sync_window(calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            s = ctx.evaluate_binary_batch(b)
        return (time.perf_counter() - t0) / calls, s

    def enqueue_window(calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            ctx.evaluate_binary_batch(b, sync=False)
        t1 = time.perf_counter()
        ctx.sync()
        return (t1 - t0) / calls, (time.perf_counter() - t0) / calls

    def numpy_window(calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            s = binary_sums(ctx.predict_batch(b, -INF, INF), y)
        return (time.perf_counter() - t0) / calls, s

    sync_window(3)
    enqueue_window(3)
    numpy_window(1)
    host = {"evaluate_binary_batch_sync": [], "evaluate_binary_batch_enqueue": [], "evaluate_binary_batch_enqueue_with_final_sync": [],
            "predict_batch_plus_numpy": []}
    for rep in range(args.reps):
        ts, rec_d = sync_window(args.calls)
        te, tes = enqueue_window(args.calls)
        tn, rec_h = numpy_window(max(args.calls // 4, 1))
        host["evaluate_binary_batch_sync"].append(ts)
        host["evaluate_binary_batch_enqueue"].append(te)
        host["evaluate_binary_batch_enqueue_with_final_sync"].append(tes)
        host["predict_batch_plus_numpy"].append(tn)
        log(f"{name} rep {rep}: sync {ts * 1e3:.3f} ms  enqueue {te * 1e3:.3f} ms ({tes * 1e3:.3f} with the final sync)  "
            f"predict_batch + numpy {tn * 1e3:.3f} ms per call")
    ints = lambda r: (r.n_rows, r.n_pos, r.tp, r.fp, r.two_u)  # noqa: E731
    assert ints(rec_d) == ints(rec_h), "the two routes' integers differ"
    assert abs(rec_d.sum_log_loss - rec_h.sum_log_loss) <= 1e-12 * abs(rec_h.sum_log_loss), "the two routes' log loss differ"
    # device times: one profiled window per call kind and repetition, alternating
    ctx.profile_enable(True)
    kinds = {"evaluate_binary": ("evaluate_binary", "binary_sort", "binary_count"), "evaluate": ("evaluate",), "predict": ("predict",)}
    dev = {nm: [] for names in kinds.values() for nm in names}
    for rep in range(args.reps):
        for which, names in kinds.items():
            ctx.profile_reset()
            for _ in range(args.calls):
                if which == "evaluate_binary":
                    ctx.evaluate_binary_batch(b)
                elif which == "evaluate":
                    ctx.evaluate_batch(b, 0.0, 1.0)
                else:
                    ctx.predict_batch(b, -INF, INF)
            prof = ctx.profile_read()
            for nm in names:
                ms, n = prof[nm]
                dev[nm].append(ms / n)
    ctx.profile_enable(False)
    res = {
        "F": F, "k": k, "rows": B, "entries": int(len(hb.col)),
        "device_ms_per_call": {nm: span(v) for nm, v in dev.items()},
        "host_s_per_call": {nm: span(v) for nm, v in host.items()},
        "record": {"n_rows": rec_d.n_rows, "n_pos": rec_d.n_pos, "tp": rec_d.tp, "fp": rec_d.fp, "two_u": rec_d.two_u,
                   "logLoss": rec_d.logLoss, "auc": rec_d.auc, "logLoss_numpy": rec_h.logLoss},
        "bytes_back_per_call": {"evaluate_binary_batch": 56, "predict_batch": 8 * B},
        "device_slower_than_numpy_route": min(host["evaluate_binary_batch_sync"]) > max(host["predict_batch_plus_numpy"]),
    }
    b.close()
    ctx.close()
    return res


out = {"calls_per_window": args.calls, "reps": args.reps,
       "what": "device: the library's event profile per call, one window per call kind and repetition, alternating; host: "
               "perf_counter around windows of calls (a synchronous call ends in a stream synchronise; the NumPy route's "
               "windows are a quarter as long)",
       "configs": {name: run(name) for name in args.configs.split(",")}}
text = json.dumps(out, indent=1)
print(text, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
