"""Measurement tool (not product): the evaluation on the device (fm_evaluate_batch) against predict.
Two workloads on one GPU: c5's table and batch (F = 1M, k = 16, 65,536 rows, regression labels) and a
c3-shaped resident batch (F = 100M, k = 16, 262,144 rows); tables random-initialised.  In one process,
warmed, `--reps` repetitions alternating:
  1. device time by the library's event profile (a pass of its own): "evaluate" (the kEvaluate forward
     and the fold; "eval_fold" is the fold alone, inside it) against "predict", fm_predict_batch's
     forward -- the unchanged yardstick;
  2. host wall time of one validation metric (mae): evaluate_batch (synchronous: one 40-byte record
     back) against predict_batch + the NumPy metric (B doubles back), windows of `--calls` calls; and,
     on c5, today's transform + RegressionEvaluator.evaluate over the same rows as a frame (once: it
     explodes the frame's vectors in Python and re-uploads them).
The two routes' mae are compared.  Prints one JSON object (and writes it to --out).
  python tools/eval_bench.py [--out FILE, default profiles/eval/eval_bench.json] [--calls N] [--reps N] [--configs c5,c3] [--no-frame]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from fm_spark_amd._native import CSRHost  # noqa: E402
from fm_spark_amd.data import synthetic_batch  # noqa: E402
from fm_spark_amd.engine import FMContext  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "eval", "eval_bench.json"))
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--configs", default="c5,c3")
ap.add_argument("--no-frame", action="store_true")
args = ap.parse_args()
LO, HI = 0.0, 1.0


def log(msg):
    print(msg, file=sys.stderr, flush=True)


def frame_route(ctx, k, b):
    """today's route over the same rows as a frame: transform + RegressionEvaluator.evaluate"""
    from fm_spark_amd.linalg import SparseVector
    from fm_spark_amd.ml import DataFrame, FactorizationMachinesModel
    from fm_spark_amd.tuning import RegressionEvaluator

    vecs = [SparseVector(ctx.num_features, b.col[b.row_ptr[i]:b.row_ptr[i + 1]], b.val[b.row_ptr[i]:b.row_ptr[i + 1]])
            for i in range(b.n_rows)]
    df = DataFrame({"label": [float(y) for y in b.label], "features": vecs})
    model = FactorizationMachinesModel("bench", k, 0.0, ctx=ctx).setMinLabel(LO).setMaxLabel(HI)
    ev = RegressionEvaluator().setMetricName("mae")
    t0 = time.perf_counter()
    out = model.transform(df)
    t1 = time.perf_counter()
    mae = ev.evaluate(out)
    t2 = time.perf_counter()
    return {"transform_s": t1 - t0, "evaluator_s": t2 - t1, "total_s": t2 - t0, "mae": mae}


def run(name):
    F, k, B, zipf_s, _ = bench.CONFIGS[name]
    lab = {}
    if name == "c5":
        lab = dict(labels="regression", w_star=np.random.default_rng(20261015).normal(0.0, 0.1, F))
    t0 = time.perf_counter()
    hb = synthetic_batch(B, F, batch_index=7000, zipf_s=zipf_s, **lab)
    ctx = FMContext(F, k, seed=20261015, init_sd=bench.INIT_SD)
    ctx.init_random_range(0, F)
    b = ctx.batch(CSRHost(hb.row_ptr, hb.col, hb.val, hb.label))
    ctx.sync()
    log(f"{name}: {B} rows, {len(hb.col)} entries, table of {F} rows ready in {time.perf_counter() - t0:.1f} s")
    y = np.asarray(hb.label, dtype=np.float64)

    def eval_window(calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            s = ctx.evaluate_batch(b, LO, HI)
            mae = s.mae
        return (time.perf_counter() - t0) / calls, mae

    def pred_window(calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            p = ctx.predict_batch(b, LO, HI)
            mae = float(np.mean(np.abs(y - p)))
        return (time.perf_counter() - t0) / calls, mae

    eval_window(3)
    pred_window(3)
    ev_s, pr_s = [], []
    for rep in range(args.reps):
        te, mae_e = eval_window(args.calls)
        tp, mae_p = pred_window(args.calls)
        ev_s.append(te)
        pr_s.append(tp)
        log(f"{name} rep {rep}: evaluate_batch {te * 1e3:.3f} ms   predict_batch + numpy {tp * 1e3:.3f} ms per call")
    # device times: one profiled pass per repetition, alternating, each read on its own
    ctx.profile_enable(True)
    dev = {"evaluate": [], "eval_fold": [], "predict": []}
    for rep in range(args.reps):
        for which in ("evaluate", "predict"):
            ctx.profile_reset()
            for _ in range(args.calls):
                if which == "evaluate":
                    ctx.evaluate_batch(b, LO, HI)
                else:
                    ctx.predict_batch(b, LO, HI)
            prof = ctx.profile_read()
            for nm in (("evaluate", "eval_fold") if which == "evaluate" else ("predict",)):
                ms, n = prof[nm]
                dev[nm].append(ms / n)
    ctx.profile_enable(False)
    med = {nm: statistics.median(v) for nm, v in dev.items()}
    res = {
        "F": F, "k": k, "rows": B, "entries": int(len(hb.col)),
        "device_ms_per_call": dev, "device_ms_median": med,
        "evaluate_over_predict": med["evaluate"] / med["predict"],
        "accepted": med["evaluate"] <= 1.04 * med["predict"] + med["eval_fold"],
        "host_s_per_call": {"evaluate_batch": ev_s, "predict_batch_plus_numpy": pr_s},
        "host_s_median": {"evaluate_batch": statistics.median(ev_s), "predict_batch_plus_numpy": statistics.median(pr_s)},
        "mae": {"evaluate_batch": mae_e, "predict_batch_plus_numpy": mae_p},
        "bytes_back_per_call": {"evaluate_batch": 40, "predict_batch": 8 * B},
    }
    if name == "c5" and not args.no_frame:
        res["frame_route"] = frame_route(ctx, k, hb)
        log(f"{name}: transform + RegressionEvaluator {res['frame_route']['total_s']:.3f} s")
    assert abs(mae_e - mae_p) <= 1e-12 * max(1.0, abs(mae_p)), "the two routes' mae differ"
    b.close()
    ctx.close()
    return res


out = {"calls_per_window": args.calls, "reps": args.reps, "clamp": [LO, HI],
       "what": "device: the library's event profile per call, one window per repetition, evaluate and predict "
               "alternating; host: perf_counter around windows of synchronous calls (each ends in a stream synchronise)",
       "configs": {name: run(name) for name in args.configs.split(",")}}
text = json.dumps(out, indent=1)
print(text, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
