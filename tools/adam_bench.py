"""Measurement tool (not product): what the lazy AdamW rule of the window stage (fm_config.optimizer = FM_OPT_ADAM;
fm_adam.hip on fm_window.h) costs in the recommender's training loop against the SGD update and against FTRL's rule
on the same stage, at tools/ftrl_bench.py's shape (the pair bench's: c5's table, 262 145 rows and about 8.65M
entries per batch, k = 16, squared loss, fuse_single = FM_FUSE_OFF).  Adam moves FTRL's bytes per touched row, so
FTRL's stage time in the same run is the yardstick.

One context per process: the driver starts a fresh child process per leg (--only), the legs sgd, ftrl, adam
alternating, `reps` rounds.  A leg reports
  (a) ms per iteration of the pipelined loop (sample, prepare, step; two batches in turn), host clock around a
      loop that ends in a sync;
  (b) its stage's own time from the "update" / "ftrl" / "adam" profile entry (HIP events) in a profiled loop of
      its own, after (a).
The driver reports both as min - max over the rounds, and the ratio of Adam's stage to FTRL's.  --tree PATH imports
the package and bench.py from another checkout (legs without "adam" only).
Runs on the GPU only.  Writes profiles/adam/adam_bench.json (or --out).
  python tools/adam_bench.py [--iters 32] [--reps 3] [--only adam] [--tree PATH] [--out JSON]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=32)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--only", default=None, help="one leg in this process: sgd | ftrl | adam")
ap.add_argument("--legs", default="sgd,ftrl,adam")
ap.add_argument("--tree", default=None, help="checkout to import fm_spark_amd and bench from (default: this one)")
ap.add_argument("--out", default=None)
args = ap.parse_args()

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(args.tree) if args.tree else HERE
STAGE = {"sgd": "update", "ftrl": "ftrl", "adam": "adam"}


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": len(v)}


def leg(opt):
    sys.path.insert(0, ROOT)
    import bench
    from fm_spark_amd._native import CSRHost
    from fm_spark_amd.engine import FMContext

    F, k = bench.CONFIGS["c5"][:2]
    U, C, N_EXCL, N_POS, N_NEG, N_SETS = 65_536, 16_384, 200, 52_429, 4, 4
    rng = np.random.default_rng(20261126)

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
    # "ftrl" at tools/ftrl_bench.py's beta; "adam" at its defaults (eps 1e-8, 0.9 / 0.999)
    kw = {"sgd": {}, "ftrl": {"optimizer": "ftrl", "opt_init": 0.1}, "adam": {"optimizer": "adam"}}[opt]
    ctx = FMContext(F, k, seed=20261015, init_sd=bench.INIT_SD, fuse=False, **kw)  # no GPU: raises here
    ctx.init_random_range(0, F)
    bu, bc = ctx.batch(CSRHost(*ctx_rows, np.zeros(U))), ctx.batch(CSRHost(*cand_rows, np.zeros(C)))
    lists = ctx._row_lists(ex, C)
    bufs, t = [None, None], [0]

    def sample(j):
        pc, pd = pos[j % N_SETS]
        bufs[j % 2] = ctx._sample_pairs(bu, bc, pc, pd, N_NEG, lists, 1.0, 0.0, j, bufs[j % 2], False)
        bufs[j % 2].prepare()

    def loop(n):
        t0 = time.perf_counter()
        sample(t[0] + 1)
        for _ in range(n):
            t[0] += 1
            ctx.step_batch(bufs[t[0] % 2], t[0], bench.STEP_SIZE, bench.REG_PARAM, sync=False)
            sample(t[0] + 1)  # (one batch more than is stepped: the same in every loop)
        ctx.sync()
        return 1e3 * (time.perf_counter() - t0) / n

    loop(4)  # warm-up: scratch and both batches grown
    ms = loop(args.iters)
    ctx.profile_enable(True)
    ctx.profile_reset()
    loop(16)
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    fin = float(ctx.loss_history()[-1])
    assert np.isfinite(fin), (opt, fin)
    return {"opt": opt, "loop_ms_per_iter": ms, "last_loss_sum": fin, "rows_per_batch": bufs[0].n_rows,
            "entries_per_batch": bufs[0].nnz,
            "ms_per_launch": {name: prof[name][0] / prof[name][1] for name in ("forward", "sort", STAGE[opt]) if name in prof}}


if args.only:
    print("LEG " + json.dumps(leg(args.only)), flush=True)
    sys.exit(0)

legs = args.legs.split(",")
recs = {opt: [] for opt in legs}
for _ in range(args.reps):  # alternating, a fresh process (one context) per leg
    for opt in legs:
        cmd = [sys.executable, os.path.abspath(__file__), "--only", opt, "--iters", str(args.iters)]
        cmd += ["--tree", args.tree] if args.tree else []
        out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300).stdout
        recs[opt].append(json.loads(next(line for line in out.splitlines() if line.startswith("LEG "))[4:]))
res = {"shape": {"config": "c5", "k": 16, "rows_per_batch": recs[legs[0]][0]["rows_per_batch"],
                 "entries_per_batch": recs[legs[0]][0]["entries_per_batch"], "fuse_single": "FM_FUSE_OFF"},
       "iters": args.iters, "reps": args.reps, "tree": os.path.relpath(ROOT, HERE),
       "a_pipelined_loop_ms_per_iter_host_clock": {opt: spread([r["loop_ms_per_iter"] for r in v]) for opt, v in recs.items()},
       "b_stage_ms_per_launch_hip_events": {opt: spread([r["ms_per_launch"][STAGE[opt]] for r in v]) for opt, v in recs.items()},
       "b_forward_ms_per_launch_hip_events": {opt: spread([r["ms_per_launch"]["forward"] for r in v]) for opt, v in recs.items()},
       "last_loss_sum": {opt: sorted({r["last_loss_sum"] for r in v}) for opt, v in recs.items()}}
stage = res["b_stage_ms_per_launch_hip_events"]
if "adam" in stage and "ftrl" in stage:
    res["adam_stage_over_ftrl_stage_ratio_of_medians"] = stage["adam"]["median"] / stage["ftrl"]["median"]
out = args.out or os.path.join(HERE, "profiles", "adam", "adam_bench.json")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res, indent=1))
