"""Measurement tool (not product): exact rank positions (fm_rank_positions_batch) beside the top-N call on
the same rows and beside the only route to the same numbers a caller had without it.
The shape of tools/rank_bench.py: c5's table (F = 1M, k = 16, random init), U = 64 contexts of 26
entries, C = 16384 candidates of 13 entries; 20 targets and 200 exclusions per context.  One process,
warmed, three repetitions alternating over the first two routes, then three calls of the third:
  positions  fm_rank_positions_batch on the two resident row sets, lists normalised once;
  except     fm_rank_batch_select, FM_RANK_SELECT_EXCEPT with the same exclusions, n_top = 100;
  predict    what `positions` replaces: FMContext.predict_batch over the U * C materialised rows (built
             and uploaded once, timed apart) and a NumPy count per target over the downloaded scores.
The host clock is taken around windows of `calls` calls (every call ends in a stream synchronise and the
copy of its results).  The predict route runs behind the alternation, not inside it: its call leaves
23 ms of host work (the NumPy count over U x T x C) between device calls, and the 50-call window that
followed it in the rotation (the positions route's) read 0.22 to 0.66 ms per call on the host clock where
it reads 0.15 ms with the predict route left out; why was not looked into.  The library's event profile per
pass is read in a later pass of the same process, route by route.  The positions are compared with the
predict route's counts (equal wherever no other score lies within 1e-9 of the target's: the two routes
sum in different orders) and, for targets ranked below 100, with the slot of the `except` call bit for
bit.  Prints one JSON object (and writes it to --out).
  python tools/rank_position_bench.py [--out FILE] [--calls N] [--reps N] [--no-predict]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from fm_spark_amd import _native as N  # noqa: E402
from fm_spark_amd.engine import FMContext, normalize_row_lists  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--no-predict", action="store_true")
args = ap.parse_args()

F, k, _, _, _ = bench.CONFIGS["c5"]
U, ZU, Cn, ZC, N_TOP = 64, 26, 16384, 13, 100
N_TARGET, N_EXCEPT = 20, 200
INF = float("inf")


def log(msg):
    print(msg, file=sys.stderr, flush=True)


rng = np.random.default_rng(20261020)
cu_col = rng.integers(0, F // 2, (U, ZU)).astype(np.int32)
cc_col = rng.integers(F // 2, F, (Cn, ZC)).astype(np.int32)
cu_val = rng.standard_normal((U, ZU)).astype(np.float32).astype(np.float64)
cc_val = rng.standard_normal((Cn, ZC)).astype(np.float32).astype(np.float64)
contexts = N.CSRHost(np.arange(U + 1, dtype=np.int64) * ZU, cu_col.ravel(), cu_val.ravel(), np.zeros(U))
candidates = N.CSRHost(np.arange(Cn + 1, dtype=np.int64) * ZC, cc_col.ravel(), cc_val.ravel(), np.zeros(Cn))

ctx = FMContext(F, k, seed=20261015, init_sd=bench.INIT_SD)
ctx.init_random_range(0, F)
ctx.sync()
bu, bc = ctx.batch(contexts), ctx.batch(candidates)
lib = N.load()

# per context: 220 distinct rows, the first 20 its targets (held-out), the rest what it has seen
picks = [rng.choice(Cn, N_TARGET + N_EXCEPT, replace=False) for _ in range(U)]
tg_ptr, tg_rows = normalize_row_lists([p[:N_TARGET] for p in picks], U)
ex_ptr, ex_rows = normalize_row_lists([p[N_TARGET:] for p in picks], U)
position = np.zeros(U * N_TARGET, np.int32)
pscore = np.zeros(U * N_TARGET)
idx = np.zeros(U * N_TOP, np.int32)
score = np.zeros(U * N_TOP)


def route_positions():
    N.check(lib.fm_rank_positions_batch(ctx.handle, bu.handle, bc.handle, N.ptr(tg_ptr, C.c_int64), N.ptr(tg_rows, C.c_int32),
                                        N.ptr(ex_ptr, C.c_int64), N.ptr(ex_rows, C.c_int32), -INF, INF,
                                        N.ptr(position, C.c_int32), N.ptr(pscore, C.c_double)), "fm_rank_positions_batch")
    return position.copy(), pscore.copy()


def route_except():
    N.check(lib.fm_rank_batch_select(ctx.handle, bu.handle, bc.handle, N.FM_RANK_SELECT_EXCEPT, N.ptr(ex_ptr, C.c_int64),
                                     N.ptr(ex_rows, C.c_int32), N_TOP, -INF, INF, N.ptr(idx, C.c_int32),
                                     N.ptr(score, C.c_double)), "fm_rank_batch_select")
    return idx.reshape(U, N_TOP).copy(), score.reshape(U, N_TOP).copy()


def window(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        out = fn()
    return (time.perf_counter() - t0) / calls, out


routes = {"positions": route_positions, "except": route_except}
calls_of = {name: args.calls for name in routes}
if not args.no_predict:
    # ---- the materialised route's host work, once (tools/rank_bench.py's)
    t0 = time.perf_counter()
    Z = ZU + ZC
    m_col = np.empty((U, Cn, Z), dtype=np.int32)
    m_val = np.empty((U, Cn, Z), dtype=np.float64)
    m_col[:, :, :ZU], m_col[:, :, ZU:] = cu_col[:, None, :], cc_col[None, :, :]
    m_val[:, :, :ZU], m_val[:, :, ZU:] = cu_val[:, None, :], cc_val[None, :, :]
    pairs = N.CSRHost(np.arange(U * Cn + 1, dtype=np.int64) * Z, m_col.ravel(), m_val.ravel(), np.zeros(U * Cn))
    t_build = time.perf_counter() - t0
    t0 = time.perf_counter()
    bp = ctx.batch(pairs)
    ctx.sync()
    t_upload = time.perf_counter() - t0
    del m_col, m_val
    log(f"materialised {U * Cn} rows, {U * Cn * Z} entries: host build {t_build:.3f} s, upload {t_upload:.3f} s")
    elig = np.ones((U, Cn), bool)
    elig[np.repeat(np.arange(U), N_EXCEPT), ex_rows] = False
    rows_of = tg_rows.reshape(U, N_TARGET)
    t_count = []

    def route_predict():
        s = ctx.predict_batch(bp, -INF, INF).reshape(U, Cn)
        t0 = time.perf_counter()
        st = s[np.arange(U)[:, None], rows_of]                                  # [U, T]
        ahead = (s[:, None, :] > st[:, :, None]) | ((s[:, None, :] == st[:, :, None]) &
                                                    (np.arange(Cn)[None, None, :] < rows_of[:, :, None]))
        pos = np.sum(ahead & elig[:, None, :], axis=2)
        t_count.append(time.perf_counter() - t0)
        return pos, s

    routes["predict"] = route_predict
    calls_of["predict"] = 1

for name in ("positions", "except"):  # warm
    window(routes[name], 3)
host_s = {name: [] for name in routes}
last = {}
for rep in range(args.reps):
    for name in ("positions", "except"):
        per_call, last[name] = window(routes[name], calls_of[name])
        host_s[name].append(per_call)
    log(f"rep {rep}: " + "   ".join(f"{n} {host_s[n][-1] * 1e3:.3f} ms" for n in ("positions", "except")))
if "predict" in routes:
    window(routes["predict"], 1)  # warm
    for rep in range(args.reps):
        per_call, last["predict"] = window(routes["predict"], 1)
        host_s["predict"].append(per_call)
    log("predict route: " + "   ".join(f"{t * 1e3:.3f} ms" for t in host_s["predict"]))

# ---- device times by the library's events, route by route
dev_ms = {}
ctx.profile_enable(True)
for name, fn in routes.items():
    ctx.profile_reset()
    window(fn, calls_of[name])
    prof = ctx.profile_read()
    dev_ms[name] = {p: ms / calls_of[name] for p, (ms, n) in prof.items()}
ctx.profile_enable(False)

pos, ps = last["positions"]
e_i, e_s = last["except"]
near = 0
slots_agree = True
for u in range(U):
    p, r, s = (a[u * N_TARGET:(u + 1) * N_TARGET] for a in (pos, tg_rows, ps))
    m = p < N_TOP
    near += int(m.sum())
    slots_agree &= np.array_equal(e_i[u, p[m]], r[m]) and e_s[u, p[m]].tobytes() == np.ascontiguousarray(s[m]).tobytes()
mean = {n: float(np.mean(v)) for n, v in host_s.items()}
res = {
    "config": "c5 table", "F": F, "k": k, "contexts": U, "context_entries": ZU, "candidates": Cn, "candidate_entries": ZC,
    "targets_per_context": N_TARGET, "exclusions_per_context": N_EXCEPT, "n_top_of_except": N_TOP,
    "calls_per_window": calls_of, "reps": args.reps,
    "host_s_per_call": host_s, "host_spread_s": {n: max(v) - min(v) for n, v in host_s.items()},
    "device_ms_per_call": dev_ms,
    "ratio_positions_over_except": {"call": mean["positions"] / mean["except"],
                                    "rank_position_over_rank_score": dev_ms["positions"]["rank_position"] /
                                    dev_ms["except"]["rank_score"]},
    "agreement": {"targets_below_n_top": near, "their_slots_of_except_equal_bytes": bool(slots_agree)},
    "what": "host clock per call (stream synchronise and result copy inside) over windows of calls, the routes "
            "alternating (the predict route behind them); device_ms_per_call: the library's event profile per pass, in a later pass of the same process",
}
if not args.no_predict:
    m_pos, s = last["predict"]
    st = s[np.arange(U)[:, None], rows_of]
    gap = np.abs(s[:, None, :] - st[:, :, None])
    gap[np.arange(U)[:, None], np.arange(N_TARGET)[None, :], rows_of] = np.inf
    clear = gap.min(axis=2) > 1e-9
    agree = bool(np.array_equal(m_pos[clear], pos.reshape(U, N_TARGET)[clear]))
    res["materialised"] = {"rows": U * Cn, "entries": U * Cn * Z, "host_build_s": t_build, "upload_s": t_upload,
                           "numpy_count_s": t_count[-args.reps:], "predict_plus_count_s_per_call": host_s["predict"]}
    res["ratio_positions_over_predict_route"] = {"call": mean["positions"] / mean["predict"],
                                                 "with_build_and_upload": mean["positions"] / (mean["predict"] + t_build + t_upload)}
    res["agreement"].update({"targets_without_a_score_within_1e-9": int(clear.sum()),
                             "their_positions_equal_the_predict_routes": agree})
text = json.dumps(res, indent=1)
print(text, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
assert slots_agree, "a position disagrees with the slot of the select call"
if not args.no_predict:
    assert agree, "a position disagrees with the materialised route's count"
