"""Measurement tool (not product): what it costs to make fit's resident dataset at c3, by either path.
Builds bench.py's fit-leg dataset and splits (16 x 256K rows, 16 partitions, F = 100M, k = 16), then
in one process, three reps of each path, alternating (host clock around calls that end in a device
synchronise):
  (a) the host layout: ml._select_csr (the permuted host copy) + batch_splits + sync, the two timed
      separately -- what bench.py's fit.setup_s.layout / upload_once time;
  (b) batch_layout_splits + sync: the source uploaded in its own row order, laid out on the device.
After the last rep the mini-batch loop runs once over each dataset from identically seeded tables and
the loss histories must be equal bit for bit.  Prints one JSON object; bench.py does not report (b).
  python tools/fit_layout_bench.py [iters] [reps]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from fm_spark_amd._native import CSRHost  # noqa: E402
from fm_spark_amd.data import synthetic_batch  # noqa: E402
from fm_spark_amd.engine import FMContext  # noqa: E402
from fm_spark_amd.ml import _select_csr, run_minibatch_sgd_splits  # noqa: E402
from fm_spark_amd.sampler import random_split_csr  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 16
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
parts = 16
F, k, B, zs, _ = bench.CONFIGS["c3"]


def log(msg):
    print(msg, file=sys.stderr, flush=True)


def context():
    c = FMContext(F, k, seed=20261015, init_sd=bench.INIT_SD)
    c.init_random_range(0, F)
    c.sync()
    return c


t0 = time.perf_counter()
ds = bench.concat_batches([synthetic_batch(B, F, batch_index=7000 + i, zipf_s=zs) for i in range(iters)])
n = ds.n_rows
sizes = [n * (i + 1) // parts - n * i // parts for i in range(parts)]
log(f"generated {n} rows, {ds.nnz} entries in {time.perf_counter() - t0:.1f} s")
split_of, _, order = random_split_csr(sizes, ds.label, ds.row_ptr, ds.col, ds.val, F, [0.1] * iters, 1234)
splits = [order[split_of[order] == i] for i in range(iters)]
rest = order[split_of[order] < 0]
lay = np.concatenate(splits + [rest]).astype(np.int64)
split_rows = np.concatenate([[0], np.cumsum([len(r) for r in splits] + [len(rest)])])
src = CSRHost(ds.row_ptr, ds.col, ds.val, ds.label)

ctx_a, ctx_b = context(), context()
a_layout, a_upload, b_total = [], [], []
da = db = None
for rep in range(reps):
    for d in (da, db):
        if d is not None:
            d.close()
    t0 = time.perf_counter()
    host = _select_csr(ds.row_ptr, ds.col, ds.val, ds.label, lay)
    t1 = time.perf_counter()
    da = ctx_a.batch_splits(host, split_rows)
    ctx_a.sync()
    t2 = time.perf_counter()
    del host
    db = ctx_b.batch_layout_splits(src, split_rows, lay)
    ctx_b.sync()
    t3 = time.perf_counter()
    a_layout.append(t1 - t0)
    a_upload.append(t2 - t1)
    b_total.append(t3 - t2)
    log(f"rep {rep}: (a) layout {t1 - t0:.3f} s + upload {t2 - t1:.3f} s = {t2 - t0:.3f} s   (b) {t3 - t2:.3f} s")

assert (da.n_rows, da.nnz) == (db.n_rows, db.nnz)
la = run_minibatch_sgd_splits(ctx_a, da, bench.STEP_SIZE, bench.REG_PARAM, n_iter=iters)
lb = run_minibatch_sgd_splits(ctx_b, db, bench.STEP_SIZE, bench.REG_PARAM, n_iter=iters)
same = len(la) == len(lb) and all(x == y for x, y in zip(la, lb)) and bool(np.all(np.isfinite(la)))
a_total = [x + y for x, y in zip(a_layout, a_upload)]
res = {"config": "c3", "dataset_rows": int(n), "dataset_nnz": int(ds.nnz), "iterations": iters, "partitions": parts,
       "host_layout_s": {"layout": a_layout, "upload": a_upload, "total": a_total,
                         "spread": max(a_total) - min(a_total)},
       "device_layout_s": {"total": b_total, "spread": max(b_total) - min(b_total)},
       "device_below_host_by_s": min(a_total) - max(b_total),
       "loss_histories_bitwise_equal": bool(same), "losses": len(la),
       "what": "host clock; (a) ml._select_csr + FMContext.batch_splits + sync, (b) FMContext.batch_layout_splits + sync, "
               "alternating in one process; bench.py's fit.setup_s.layout keeps timing (a)'s host gather"}
print(json.dumps(res, indent=1), flush=True)
assert same, "the loss histories of the two datasets differ"
assert min(a_total) - max(b_total) > res["host_layout_s"]["spread"], "(b) is not below (a) by more than (a)'s spread"
