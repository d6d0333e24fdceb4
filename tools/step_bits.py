"""Bit-level pin of the step's update paths (tests/golden/step_bits.json, tests/test_gpu_step_bits.py).

A fixed set of small problems goes through fm_step_batch; per case the tool records the loss history
as hex floats and a SHA-256 of the fm_export_tables bytes (ids, w, V).  A sharded case runs the same
problem through a sharded context of R ranks on one device (the group path: route, owner forward,
fm_shard_combine, owner update) and adds a SHA-256 of fm_predict over batch 0 on the trained tables
(the sharded predict's combine, present counts included).  A refactor of the forward, the segmented
update, its combine, the replicated apply, or the sharded requester's combine and predict must
reproduce every digest.

    python tools/step_bits.py --out tests/golden/step_bits.json     # record (GPU)
    python tools/step_bits.py --check tests/golden/step_bits.json   # compare (GPU)

The recorded bits depend on the compiler as well as on the code (fma contraction, the order of a
reduction the optimiser is free to pick): after a toolchain change, regenerate the fixture from a
known-good commit's library (FM_HIP_LIB=<that build> python tools/step_bits.py --out ...), never from
the code under test.

Every problem: 768 rows + 2 empty ones over 4,096 features (make_problem of tests/problems.py, then)
  * id 3 in every non-empty row (one run of 768 entries: the long-run combine),
  * id 7 in 300 rows (a run that crosses one 256-entry update wave: the two-range combine and beyond),
  * id 11 in exactly two adjacent rows, besides the many natural runs of two (group-boundary pieces),
  * one row of 230 entries, 200 of them ids no other row holds (more singletons than any lane group
    keeps in LDS at every k the fused forward serves: the overflow walk),
  * a third of the ids absent from the loaded model,
three steps over two alternating batches with regParam > 0, so rows are re-read with L1 pending.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

F = 4096
N_ROWS = 768
STEPS = 3
STEP_SIZE = 0.3
REG = 0.01
_SPECIAL = 16   # ids [0, 16): placed by hand
_OWN = 256      # ids [F - 256, F): the long row's own


def _batch(seed, k):
    from oracle import fm_ref as R
    from problems import f32, make_problem

    c = make_problem(seed, N_ROWS, F - _SPECIAL - _OWN, k, 8, empty_frac=0.0)[0]
    rng = np.random.default_rng(seed + 1)
    in7 = set(rng.choice(N_ROWS, size=300, replace=False).tolist())
    own = np.sort(rng.choice(_OWN, size=200, replace=False)) + (F - _OWN)
    rows = []
    for r in range(N_ROWS):
        ids = (c.col[c.row_ptr[r]:c.row_ptr[r + 1]] + _SPECIAL).tolist()
        val = c.val[c.row_ptr[r]:c.row_ptr[r + 1]].tolist()
        head = [3] + ([7] if r in in7 else []) + ([11] if r in (400, 401) else [])
        hval = f32(rng.normal(0.0, 1.0, size=len(head))).tolist()
        if r == 100:  # the long row
            extra = np.setdiff1d(rng.choice(F - _SPECIAL - _OWN, size=30, replace=False) + _SPECIAL, ids)
            ids = np.concatenate([ids, extra, own])
            val = np.concatenate([val, f32(rng.normal(0.0, 1.0, size=len(extra) + len(own)))])
            o = np.argsort(ids, kind="stable")
            ids, val = ids[o].tolist(), val[o].tolist()
        rows.append((head + ids, hval + val))
    rows.insert(5, ([], []))  # an empty row inside the batch and one at its end
    rows.append(([], []))
    rp = np.cumsum([0] + [len(i) for i, _ in rows]).astype(np.int64)
    col = np.asarray([x for i, _ in rows for x in i], np.int32)
    val = np.asarray([x for _, v in rows for x in v], np.float64)
    label = np.insert(np.append(c.label, 0.0), 5, 1.0)
    return R.CSR(row_ptr=rp, col=col, val=val, label=label)


_problems = {}


def problem(k):
    """(the two batches, ids, w, V of the loaded model) for k factors, built once."""
    if k not in _problems:
        from problems import make_problem

        _, ids, w, V = make_problem(4200 + k, 1, F, k, 1)
        keep = ids[ids % 3 != 1]  # a third of the rows absent
        _problems[k] = ([_batch(4300 + 10 * k + i, k) for i in range(2)], keep, w[keep], V[keep])
    return _problems[k]


# name -> (k, fuse, prepared steps); "repl": the replicated emit through fm_repl_grad / fm_repl_apply
CASES = {}
for _k in (3, 8, 12, 16):
    CASES[f"k{_k}_fused"] = (_k, True, (1, 2, 3))
    CASES[f"k{_k}_unfused"] = (_k, False, (1, 2, 3))
    CASES[f"k{_k}_unprepared"] = (_k, True, ())
for _k in (32, 80):
    CASES[f"k{_k}_prepared"] = (_k, True, (1, 2, 3))
    CASES[f"k{_k}_unprepared"] = (_k, True, ())
CASES["k16_mixed"] = (16, True, (1, 3))  # an unprepared step between fused ones
CASES["k8_repl"] = (8, None, ())
CASES["k16_repl"] = (16, None, ())
# sharded: fuse = (R, wire); batch 1 is prepared (routed ahead) behind step 1, steps 1 and 3 route
# inline.  The smallest shapes that reach every requester kernel family: teams of 1 .. 16 lanes
# (k = 3, 8, 16, 32, 80; at k = 80 the 20 quads take two trips of the team, the second partly idle),
# the pair slots in registers (R <= 8, all eight at R = 8) and owner by owner (R = 12), both wires,
# and one owner alone.
for _k, _r, _w in ((3, 3, "fp32"), (8, 3, "fp64"), (16, 3, "fp32"), (16, 3, "fp64"), (32, 8, "fp32"),
                   (80, 2, "fp64"), (16, 12, "fp32"), (16, 12, "fp64"), (80, 12, "fp32"), (8, 1, "fp32")):
    CASES[f"k{_k}_shard{_r}_{_w}"] = (_k, (_r, _w), (2,))


def _sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _digest(loss, tables):
    return {"loss": [float(x).hex() for x in loss], "tables": _sha(tables)}


def run_case(name):
    from fm_spark_amd._native import CSRHost
    from fm_spark_amd.distributed import HipReplEngine
    from fm_spark_amd.engine import FMContext

    k, fuse, prepared = CASES[name]
    csrs, ids, w, V = problem(k)
    hosts = [CSRHost(c.row_ptr, c.col, c.val, c.label) for c in csrs]
    if fuse is None:
        eng = HipReplEngine(F, k)
        eng.load_tables(ids, w, V)
        bs = [eng.batch(h) for h in hosts]
        loss = []
        for t in range(1, STEPS + 1):
            b = bs[(t - 1) % 2]
            eng.apply(eng.grad_phase(b), t, STEP_SIZE, REG, b.n_rows)
            loss.append(eng.last_stats()[0])
        out = _digest(loss, eng.export_tables())
        eng.ctx.close()
        return out
    sharded = isinstance(fuse, tuple)
    if sharded:
        R, wire = fuse
        ctx = FMContext(F, k, parallel="sharded", n_gpus=R, devices=[0] * R, transport="copy", wire=wire)
    else:
        ctx = FMContext(F, k, fuse=fuse)
    ctx.load_tables(ids, w, V)
    bs = [ctx.batch(h) for h in hosts]
    for t in range(1, STEPS + 1):
        b = bs[(t - 1) % 2]
        if t in prepared:
            b.prepare()
        ctx.step_batch(b, t, STEP_SIZE, REG)
    out = _digest(ctx.loss_history(), ctx.export_tables())
    if sharded:
        out["predict"] = _sha([ctx.predict(hosts[0], 0.0, 1.0)])
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="write the digests of every case to this file")
    ap.add_argument("--check", help="compare every case against this file; exit 1 on a difference")
    args = ap.parse_args()
    res = {name: run_case(name) for name in CASES}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    if args.check:
        with open(args.check) as f:
            want = json.load(f)
        bad = [n for n in CASES if want.get(n) != res[n]]
        print(json.dumps({"cases": len(CASES), "differ": bad}))
        return 1 if bad else 0
    if not args.out:
        print(json.dumps(res, indent=1, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
