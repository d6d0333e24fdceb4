"""Measurement tool (not product): what the objective stage (fm_config.loss; fm_objective.hip) costs in the
recommender's training loop, squared against logistic against BPR.

Shape: tools/pair_bench.py's -- c5's table (1M features, k = 16); 65 536 context rows of about 20 entries,
16 384 candidate rows of 13; 200 excluded rows per context, resident (fm_lists); 52 429 positives x (1 + 4) =
262 145 rows, about 8.66M entries per batch.  fuse_single = FM_FUSE_OFF on all three contexts, so the three
loops differ by the stage alone.

  (a) ms per iteration of the pipelined loop (sample, prepare, step; two batches in turn) for each loss, the
      three loops alternating, `reps` repetitions, min - max reported;
  (b) the stage's own time from the "objective" profile entry (HIP events), beside the forward's and the
      update's, in a short profiled loop of its own (the events are not in (a)'s loops).

--only squared runs the squared loop alone and --tree PATH imports the package and bench.py from another
checkout: together they measure the parent commit's squared loop with this same script (the parent has no
fm_config.loss, so nothing but defaults is passed for "squared").  --parent JSON (repeatable) embeds such
results in this run's output: the squared path launches nothing new, so the two must agree within the
repetitions' spread.

Runs on the GPU only: without one the context constructor raises.  Writes profiles/objective/objective_bench.json
(or --out).
  python tools/objective_bench.py [--iters 32] [--reps 5] [--only squared] [--tree PATH] [--parent JSON] [--out JSON]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=32)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only", default=None, help="one loss: squared | logistic | bpr")
ap.add_argument("--tree", default=None, help="checkout to import fm_spark_amd and bench from (default: this one)")
ap.add_argument("--parent", action="append", default=[], help="a --only squared result of the parent commit to embed")
ap.add_argument("--out", default=None)
args = ap.parse_args()

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(args.tree) if args.tree else HERE
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from fm_spark_amd._native import CSRHost  # noqa: E402
from fm_spark_amd.engine import FMContext  # noqa: E402

iters, reps = args.iters, args.reps
LOSSES = [args.only] if args.only else ["squared", "logistic", "bpr"]
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


class Run:
    """One context of a loss with its resident sources and lists, and the loop over them."""

    def __init__(self, loss):
        kw = {} if loss == "squared" else {"loss": loss}  # (the parent's constructor has no such argument)
        self.loss = loss
        self.ctx = FMContext(F, k, seed=20261015, init_sd=bench.INIT_SD, fuse=False, **kw)  # no GPU: raises here
        self.ctx.init_random_range(0, F)
        self.bu = self.ctx.batch(CSRHost(*ctx_rows, np.zeros(U)))
        self.bc = self.ctx.batch(CSRHost(*cand_rows, np.zeros(C)))
        self.lists = self.ctx._row_lists(ex, C)
        self.bufs = [None, None]
        self.t = 0  # the iteration index runs on across the loops: eta = step / sqrt(t)

    def sample(self, j):
        pc, pd = pos[j % N_SETS]
        b = self.ctx._sample_pairs(self.bu, self.bc, pc, pd, N_NEG, self.lists, 1.0, 0.0, j, self.bufs[j % 2], False)
        self.bufs[j % 2] = b
        b.prepare()

    def loop(self, n):
        ctx, t0 = self.ctx, time.perf_counter()
        self.sample(self.t + 1)
        for _ in range(n):
            self.t += 1
            ctx.step_batch(self.bufs[self.t % 2], self.t, bench.STEP_SIZE, bench.REG_PARAM, sync=False)
            self.sample(self.t + 1)  # (one batch more than is stepped: the same in every loop)
        ctx.sync()
        return 1e3 * (time.perf_counter() - t0) / n


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": len(v)}


runs = [Run(loss) for loss in LOSSES]
for r in runs:  # warm-up: scratch and both batches grown
    r.loop(4)
ms = {r.loss: [] for r in runs}
for _ in range(reps):  # alternating
    for r in runs:
        ms[r.loss].append(r.loop(iters))
res = {"shape": {"features": F, "k": k, "contexts": U, "candidates": C, "excluded_per_context": N_EXCL, "positives": N_POS,
                 "negatives_per_positive": N_NEG, "rows_per_batch": runs[0].bufs[0].n_rows,
                 "entries_per_batch": runs[0].bufs[0].nnz, "fuse_single": "FM_FUSE_OFF", "exclude_lists": "resident"},
       "iters": iters, "reps": reps, "tree": os.path.relpath(ROOT, HERE),
       "a_pipelined_loop_ms_per_iter_host_clock": {loss: spread(v) for loss, v in ms.items()}}
if "squared" in ms:
    res["a_ratio_of_medians_to_squared"] = {loss: float(np.median(v) / np.median(ms["squared"])) for loss, v in ms.items()}
# ---- (b) the stage itself, by HIP events
stage = {}
for r in runs:
    r.ctx.profile_enable(True)
    r.ctx.profile_reset()
    r.loop(16)
    prof = r.ctx.profile_read()
    r.ctx.profile_enable(False)
    stage[r.loss] = {name: {"ms_per_launch": prof[name][0] / prof[name][1], "launches": prof[name][1]}
                     for name in ("forward", "objective", "update", "sort") if name in prof}
    fin = r.ctx.loss_history()[-1]
    assert np.isfinite(fin), (r.loss, fin)
    stage[r.loss]["last_loss_sum"] = float(fin)
res["b_profiled_loop_hip_events"] = stage
res["b_stage_bytes_each_way"] = 8 * runs[0].bufs[0].n_rows
for path in args.parent:
    with open(path) as f:
        pj = json.load(f)
    res.setdefault("parent_commit_squared_loop", []).append(
        {"file": os.path.basename(path), "ms_per_iter": pj["a_pipelined_loop_ms_per_iter_host_clock"]["squared"],
         "profiled": pj["b_profiled_loop_hip_events"]["squared"]})
out = args.out or os.path.join(HERE, "profiles", "objective", "objective_bench.json")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res, indent=1))
