"""What the fp64 partial-sum wire (fm_config.wire = FM_WIRE_FP64) costs against the fp32 wire.

One process, COPY transport, R ranks on device 0, the c3 shape of `bench.py --copy-ranks 8`
(100M hashed features, k = 16, 256K rows per rank, the same synthetic batches).  Two contexts
with the same seed, one per wire, stepped in alternating reps inside one call; per rep and wire
one JSON line with

  ms_per_iter        wall time of the timed steps (enqueue only, batches prepared two steps
                     ahead, as bench.py times a group), profiling off
  owner_forward_ms   per launch, fm_profile_read of rank 0 (HIP events) over a few extra steps:
  combine_ms         the owners' partial pass (all chunks) and the requester's combine
  bytes              per rank and step, rank 0's batch: what crosses to other ranks in each
                     direction, (kp + 2) words per remote (sample, owner) pair

then a summary line with the medians and the fp64 / fp32 ratio.  COPY on one device shows what
the kernels and the device copies cost; it says nothing about xGMI, where the partial direction's
bytes double (both directions together 1.5x).

    python tools/wire_bench.py [--ranks 8] [--steps 12] [--reps 3] [--out profiles/wire_fp64/wire_bench.jsonl]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # as bench.py: main, side and exchange streams on queues of their own

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F, K, B, ZIPF = 100_000_000, 16, 262_144, 1.05  # bench.py's c3
STEP_SIZE, REG_PARAM, INIT_SD, SEED = 0.1, 1e-6, 0.01, 20261015
DEPTH = 2  # batches prepared this many steps ahead (bench.py's group default)


def concat(parts):
    from fm_spark_amd.data import Batch

    offs = np.cumsum([0] + [p.nnz for p in parts])
    row_ptr = np.concatenate([parts[0].row_ptr[:1]] + [p.row_ptr[1:] + o for p, o in zip(parts, offs[:-1])])
    return Batch(row_ptr=row_ptr.astype(np.int64), col=np.concatenate([p.col for p in parts]),
                 val=np.concatenate([p.val for p in parts]), label=np.concatenate([p.label for p in parts]))


def remote_pairs(b, R, r):
    """(sample, owner) pairs of rank r's batch b whose owner is another rank, and all of its pairs."""
    owner = b.col.astype(np.int64) % R
    sample = np.repeat(np.arange(b.n_rows, dtype=np.int64), np.diff(b.row_ptr))
    pairs = np.unique(sample * R + owner)
    return int(np.count_nonzero(pairs % R != r)), int(len(pairs))


class Job:
    def __init__(self, wire, R, host_batches):
        from fm_spark_amd._native import CSRHost
        from fm_spark_amd.engine import FMContext

        self.wire = wire
        self.ctx = FMContext(F, K, seed=SEED, init_sd=INIT_SD, parallel="sharded", n_gpus=R, devices=[0] * R,
                             transport="copy", wire=wire)
        self.ctx.init_random_range(0, F)
        self.batches = [self.ctx.batch(CSRHost(b.row_ptr, b.col, b.val, b.label)) for b in host_batches]
        self.t = 0

    def run(self, steps):
        """`steps` iterations, each preparing the batch DEPTH steps ahead (none left pending at the
        end); returns wall seconds."""
        nb = len(self.batches)
        depth = max(1, min(DEPTH, nb - 1))
        for j in range(depth):
            self.batches[j % nb].prepare()
        self.ctx.sync()
        t0 = time.perf_counter()
        for i in range(steps):
            self.t += 1
            self.ctx.step_batch(self.batches[i % nb], self.t, STEP_SIZE, REG_PARAM, sync=False)
            if i + depth < steps:
                self.batches[(i + depth) % nb].prepare()
        self.ctx.sync()
        return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--steps", type=int, default=12, help="timed iterations per rep and wire")
    ap.add_argument("--profile-steps", type=int, default=4, help="extra iterations per rep and wire under fm_profile")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", type=int, default=3, help="distinct resident mini-batches cycled through")
    ap.add_argument("--rows", type=int, default=B, help="rows per rank and batch (c3: 262144)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "wire_bench needs a GPU"
    from fm_spark_amd.data import synthetic_batch

    R, kp = args.ranks, (K + 3) // 4 * 4
    t0 = time.perf_counter()
    rank_batches = [[synthetic_batch(args.rows, F, batch_index=g * 1000 + i, zipf_s=ZIPF) for i in range(args.batches)]
                    for g in range(R)]
    host_batches = [concat([rb[i] for rb in rank_batches]) for i in range(args.batches)]
    print(f"generated {args.batches} batches of {R} x {args.rows} rows in {time.perf_counter() - t0:.1f}s", file=sys.stderr)
    remote, allp = remote_pairs(rank_batches[0][0], R, 0)
    jobs = {w: Job(w, R, host_batches) for w in ("fp32", "fp64")}
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for j in jobs.values():
        j.run(max(args.warmup, args.batches))
    recs = []
    for rep in range(args.reps):
        for wire, j in jobs.items():  # alternating: fp32, fp64, fp32, ...
            word = 8 if wire == "fp64" else 4
            sec = j.run(args.steps)
            j.ctx.profile_reset()
            j.ctx.profile_enable(True)
            j.run(args.profile_steps)
            prof = j.ctx.profile_read()
            j.ctx.profile_enable(False)
            per = {n: prof[n][0] / max(prof[n][1], 1) for n in ("owner_forward", "combine", "owner_update") if n in prof}
            rec = {"what": "wire_bench rep", "rep": rep, "wire": wire, "ranks": R, "transport": "copy, one device",
                   "rows_per_rank": args.rows, "k": K, "num_features": F, "steps": args.steps,
                   "ms_per_iter": 1e3 * sec / args.steps,
                   "owner_forward_ms": per.get("owner_forward"), "combine_ms": per.get("combine"),
                   "owner_update_ms": per.get("owner_update"),
                   "bytes": {"partials_B": word * (kp + 2) * remote, "s_rows_B": 4 * (kp + 2) * remote,
                             "remote_pairs": remote, "pairs": allp, "partial_word_B": word}}
            recs.append(rec)
            emit(rec)
    losses = {w: j.ctx.loss_history() for w, j in jobs.items()}
    assert all(np.all(np.isfinite(v)) for v in losses.values()), "non-finite loss"

    def med(wire, key):
        v = [r[key] for r in recs if r["wire"] == wire and r[key] is not None]
        return float(np.median(v)) if v else None

    m = {w: {k: med(w, k) for k in ("ms_per_iter", "owner_forward_ms", "combine_ms")} for w in jobs}
    b32 = next(r["bytes"] for r in recs if r["wire"] == "fp32")
    b64 = next(r["bytes"] for r in recs if r["wire"] == "fp64")
    emit({"what": "wire_bench summary", "ranks": R, "reps": args.reps, "median": m,
          "ratio_fp64_over_fp32": {k: (m["fp64"][k] / m["fp32"][k] if m["fp32"][k] else None) for k in m["fp32"]},
          "bytes_both_directions_ratio": (b64["partials_B"] + b64["s_rows_B"]) / max(b32["partials_B"] + b32["s_rows_B"], 1),
          "loss_rel_diff_last_step": float(abs(losses["fp64"][-1] - losses["fp32"][-1]) / abs(losses["fp32"][-1])),
          "note": "COPY transport, every rank on one device: the kernels' and the device copies' cost, not xGMI's"})
    for j in jobs.values():
        for b in j.batches:
            b.close()
        j.ctx.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
