"""Measurement tool (not product): what score-aware negatives (fm_batch_sample_pairs_hard) cost in the
pipelined BPR loop, against the uniform loop on this tree and on the parent commit.

Shape: tools/pair_bench.py's -- c5's table (1M features, k = 16); 65 536 context rows of about 20 entries,
16 384 candidate rows of 13; 200 excluded rows per context, resident; 52 429 positives x (1 + 4) rows per
batch; loss "bpr".

Legs, each in a process of its own (one context per process), the repetitions alternating over the legs:
  uniform           the loop with fm_batch_sample_pairs_lists, on this tree
  parent_uniform    the same loop on the tree given with --parent (a built checkout of the parent commit)
  hard{16,64}_r{1,8}  n_draw = 16 / 64, the snapshot refreshed every iteration / every eighth
A hard leg also reports pair_snapshot and pair_draw by HIP events (the library's profile, a loop of its own).
The only bar: uniform's median <= parent_uniform's median + (its max - its min).

Runs on the GPU only.  Writes profiles/hard_neg/hard_neg_bench.json.
  python tools/hard_neg_bench.py [--parent DIR] [iters] [reps]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {"uniform": (None, 1), "hard16_r1": (16, 1), "hard64_r1": (64, 1), "hard16_r8": (16, 8), "hard64_r8": (64, 8)}


def leg(name, tree, iters):
    """One leg in this process: ms per iteration of three loops after a warm-up one, and the phases."""
    sys.path.insert(0, tree)
    import numpy as np

    import bench
    from fm_spark_amd._native import CSRHost
    from fm_spark_amd.engine import FMContext

    n_draw, every = LEGS.get(name, (None, 1))
    F, k = bench.CONFIGS["c5"][:2]
    U, C, N_EXCL, N_POS, N_NEG, N_SETS = 65_536, 16_384, 200, 52_429, 4, 4
    rng = np.random.default_rng(20261021)

    def rows(n, lens, lo, hi):
        rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        col = rng.integers(lo, hi, int(rp[-1])).astype(np.int32)
        val = np.where(rng.random(len(col)) < 0.7, 1.0, rng.standard_normal(len(col))).astype(np.float32).astype(np.float64)
        return rp, col, val

    ctx_rows, cand_rows = rows(U, rng.integers(16, 25, U), 0, F // 2), rows(C, np.full(C, 13), F // 2, F)
    start, stride = rng.integers(0, C, U), 2 * rng.integers(0, C // N_EXCL // 2, U) + 1
    excl = np.sort((start[:, None] + stride[:, None] * np.arange(N_EXCL)[None, :]) % C, axis=1)
    ex = (np.arange(0, U * N_EXCL + 1, N_EXCL, dtype=np.int64), np.ascontiguousarray(excl.reshape(-1), dtype=np.int32))
    pos = [(rng.integers(0, U, N_POS).astype(np.int32), rng.integers(0, C, N_POS).astype(np.int32)) for _ in range(N_SETS)]
    ctx = FMContext(F, k, seed=20261015, init_sd=bench.INIT_SD, loss="bpr")  # no GPU: raises here
    ctx.init_random_range(0, F)
    bu, bc = ctx.batch(CSRHost(*ctx_rows, np.zeros(U))), ctx.batch(CSRHost(*cand_rows, np.zeros(C)))
    resident = ctx._row_lists(ex, C)
    extra = lambda t: () if n_draw is None else (n_draw, (t - 1) % every == 0)

    def loop(bufs):
        t0 = time.perf_counter()
        sample = lambda t: ctx._sample_pairs(bu, bc, *pos[t % N_SETS], N_NEG, resident, 1.0, 0.0, t, bufs[t % 2], False, *extra(t))
        bufs[1] = sample(1)
        bufs[1].prepare()
        for t in range(1, iters + 1):
            ctx.step_batch(bufs[t % 2], t, bench.STEP_SIZE, bench.REG_PARAM, sync=False)
            if t < iters:
                bufs[(t + 1) % 2] = sample(t + 1)
                bufs[(t + 1) % 2].prepare()
        ctx.sync()
        return 1e3 * (time.perf_counter() - t0) / iters

    bufs = [None, None]
    loop(bufs)
    out = {"ms_per_iter": [loop(bufs) for _ in range(3)]}
    if n_draw is not None:
        ctx.profile_enable(True)
        ctx.profile_reset()
        loop(bufs)
        prof = ctx.profile_read()
        ctx.profile_enable(False)
        out["phases_ms_hip_events"] = {n: prof[n][0] / prof[n][1] for n in ("pair_snapshot", "pair_draw", "pair_gather") if n in prof}
    print("LEG " + json.dumps(out))


def main(argv):
    import numpy as np

    parent = None
    if "--parent" in argv:
        i = argv.index("--parent")
        parent = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    iters = int(argv[0]) if argv else 32
    reps = int(argv[1]) if len(argv) > 1 else 3
    names = ["uniform"] + (["parent_uniform"] if parent else []) + list(LEGS)[1:]
    runs = {n: [] for n in names}
    phases = {}
    for _ in range(reps):  # alternating
        for n in names:
            tree = parent if n == "parent_uniform" else ROOT
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", n, tree, str(iters)], capture_output=True,
                               text=True, timeout=600)
            line = [l for l in p.stdout.splitlines() if l.startswith("LEG ")]
            if p.returncode != 0 or not line:
                sys.exit(f"leg {n} failed ({p.returncode}):\n{p.stderr[-2000:]}")
            got = json.loads(line[0][4:])
            runs[n] += got["ms_per_iter"]
            if "phases_ms_hip_events" in got:
                phases[n] = got["phases_ms_hip_events"]
    spread = lambda v: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "n": len(v)}
    res = {"iters": iters, "reps": reps, "ms_per_iter": {n: spread(v) for n, v in runs.items()}, "phases_ms_hip_events": phases}
    med = {n: res["ms_per_iter"][n]["median"] for n in names}
    res["ratio_to_uniform"] = {n: med[n] / med["uniform"] for n in names if n != "uniform"}
    if parent:
        pu = res["ms_per_iter"]["parent_uniform"]
        res["bar_uniform_vs_parent"] = {"limit_ms": pu["median"] + pu["max"] - pu["min"], "holds": med["uniform"] <= pu["median"] + pu["max"] - pu["min"]}
    out = os.path.join(ROOT, "profiles", "hard_neg")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "hard_neg_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        leg(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    else:
        main(sys.argv[1:])
