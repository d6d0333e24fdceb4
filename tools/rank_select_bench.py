"""Measurement tool (not product): ranking within per-context candidate lists (fm_rank_batch_select)
beside the unrestricted call and beside the only route a caller had without it.
The shape of tools/rank_bench.py: c5's table (F = 1M, k = 16, random init), U = 64 contexts of 26
entries, C = 16384 candidates of 13 entries, n_top = 100.  One process, warmed, three repetitions
alternating over the routes:
  all       FMContext.rank_batch on the two resident row sets (the unrestricted call);
  except    fm_rank_batch_select, FM_RANK_SELECT_EXCEPT, 200 random exclusions per context;
  only      fm_rank_batch_select, FM_RANK_SELECT_ONLY, 512 listed rows per context;
  per_ctx   what `only` replaces: 64 rank_batch calls, one per context, each on a resident one-row
            context batch and a resident batch of that context's 512 candidates (built before the clock).
The host clock is taken around windows of `calls` calls (every call ends in a stream synchronise and
the copy of its results); the select routes go through the C-ABI with lists normalised once, and the
Python layer's normalisation (np.unique per list) is timed separately.  The library's event profile
per pass is read in a later pass of the same process, route by route.  `only` is compared with
`per_ctx` bit for bit, `except` with the unrestricted call's first 1024 filtered on the host.
Prints one JSON object (and writes it to --out).
  python tools/rank_select_bench.py [--out FILE] [--calls N] [--reps N] [--unrestricted-only] [--k K]
--k: another factor count on the same rows (default c5's 16); at k = 128 a pair's dot product is eight
times as long.
--unrestricted-only: the `all` route alone; runs on a tree without the select calls (the parent commit),
for the check that the unrestricted call's time did not move."""
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
from fm_spark_amd.engine import FMContext  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--unrestricted-only", action="store_true")
ap.add_argument("--k", type=int, default=None)
args = ap.parse_args()

F, k, _, _, _ = bench.CONFIGS["c5"]
k = args.k or k
U, ZU, Cn, ZC, N_TOP = 64, 26, 16384, 13, 100
N_EXCEPT, N_ONLY = 200, 512
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


def window(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        out = fn()
    return (time.perf_counter() - t0) / calls, out


def route_all():
    return ctx.rank_batch(bu, bc, N_TOP, -INF, INF)


routes = {"all": route_all}
if not args.unrestricted_only:
    from fm_spark_amd.engine import normalize_row_lists  # noqa: E402

    excl = [rng.choice(Cn, N_EXCEPT, replace=False) for _ in range(U)]
    only = [rng.choice(Cn, N_ONLY, replace=False) for _ in range(U)]
    t0 = time.perf_counter()
    ex_ptr, ex_rows = normalize_row_lists(excl, U)
    t_norm_except = time.perf_counter() - t0
    t0 = time.perf_counter()
    on_ptr, on_rows = normalize_row_lists(only, U)
    t_norm_only = time.perf_counter() - t0
    idx = np.zeros(U * N_TOP, np.int32)
    score = np.zeros(U * N_TOP)

    def select(mode, ptr, rows):
        N.check(lib.fm_rank_batch_select(ctx.handle, bu.handle, bc.handle, mode, N.ptr(ptr, C.c_int64), N.ptr(rows, C.c_int32),
                                         N_TOP, -INF, INF, N.ptr(idx, C.c_int32), N.ptr(score, C.c_double)),
                "fm_rank_batch_select")
        return idx.reshape(U, N_TOP).copy(), score.reshape(U, N_TOP).copy()

    # the per-context route's resident batches
    one_u = [ctx.batch(N.CSRHost(np.array([0, ZU], np.int64), cu_col[u], cu_val[u], np.zeros(1))) for u in range(U)]
    sub_c = []
    for u in range(U):
        r = on_rows[on_ptr[u]:on_ptr[u + 1]]
        sub_c.append(ctx.batch(N.CSRHost(np.arange(len(r) + 1, dtype=np.int64) * ZC, cc_col[r].ravel(), cc_val[r].ravel(),
                                         np.zeros(len(r)))))
    ctx.sync()

    def route_per_ctx():
        return [ctx.rank_batch(one_u[u], sub_c[u], N_TOP, -INF, INF) for u in range(U)]

    routes["except"] = lambda: select(N.FM_RANK_SELECT_EXCEPT, ex_ptr, ex_rows)
    routes["only"] = lambda: select(N.FM_RANK_SELECT_ONLY, on_ptr, on_rows)
    routes["per_ctx"] = route_per_ctx

calls_of = {name: (max(args.calls // 10, 1) if name == "per_ctx" else args.calls) for name in routes}
for name, fn in routes.items():  # warm
    window(fn, 3)
host_s = {name: [] for name in routes}
last = {}
for rep in range(args.reps):
    for name, fn in routes.items():
        per_call, last[name] = window(fn, calls_of[name])
        host_s[name].append(per_call)
    log(f"rep {rep}: " + "   ".join(f"{n} {host_s[n][-1] * 1e3:.3f} ms" for n in routes))

# ---- device times by the library's events, route by route
dev_ms = {}
ctx.profile_enable(True)
for name, fn in routes.items():
    ctx.profile_reset()
    window(fn, calls_of[name])
    prof = ctx.profile_read()
    per = calls_of[name]  # passes of a route's call: per_ctx launches each 64 times per call
    dev_ms[name] = {p: ms / per for p, (ms, n) in prof.items() if p.startswith("rank_")}
    dev_ms[name]["passes_per_call"] = {p: n / per for p, (ms, n) in prof.items() if p.startswith("rank_")}
ctx.profile_enable(False)

res = {
    "config": "c5 table", "F": F, "k": k, "contexts": U, "context_entries": ZU, "candidates": Cn, "candidate_entries": ZC,
    "n_top": N_TOP, "calls_per_window": calls_of, "reps": args.reps,
    "host_s_per_call": host_s, "host_spread_s": {n: max(v) - min(v) for n, v in host_s.items()},
    "device_ms_per_call": dev_ms,
    "what": "host clock per call (stream synchronise and result copy inside) over windows of calls, the routes "
            "alternating; device_ms_per_call: the library's event profile per pass, summed over a call's launches, in a "
            "later pass of the same process",
}
if not args.unrestricted_only:
    a_i, a_s = ctx.rank_batch(bu, bc, 1024, -INF, INF)
    e_i, e_s = last["except"]
    o_i, o_s = last["only"]
    agree_except = agree_only = True
    for u in range(U):
        keep = ~np.isin(a_i[u], ex_rows[ex_ptr[u]:ex_ptr[u + 1]])
        agree_except &= a_i[u, keep][:N_TOP].tobytes() == e_i[u].tobytes() and a_s[u, keep][:N_TOP].tobytes() == e_s[u].tobytes()
        p_i, p_s = last["per_ctx"][u]
        agree_only &= (np.array_equal(on_rows[on_ptr[u]:on_ptr[u + 1]][p_i[0]], o_i[u]) and p_s[0].tobytes() == o_s[u].tobytes())
    mean = {n: float(np.mean(v)) for n, v in host_s.items()}
    res.update({
        "exclusions_per_context": N_EXCEPT, "listed_per_context": N_ONLY,
        "python_normalise_s": {"except": t_norm_except, "only": t_norm_only},
        "ratio_except_over_all": {"call": mean["except"] / mean["all"],
                                  "rank_score": dev_ms["except"]["rank_score"] / dev_ms["all"]["rank_score"]},
        "ratio_only_over_per_ctx": {"call": mean["only"] / mean["per_ctx"]},
        "ratio_only_over_all": {"call": mean["only"] / mean["all"],
                                "rank_score": dev_ms["only"]["rank_score"] / dev_ms["all"]["rank_score"]},
        "agreement": {"except_equals_filtered_unrestricted_bytes": bool(agree_except),
                      "only_equals_per_context_route_bytes": bool(agree_only)},
    })
text = json.dumps(res, indent=1)
print(text, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
if not args.unrestricted_only:
    assert agree_except and agree_only, "a select route disagrees with its reference route"
