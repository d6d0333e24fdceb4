"""Bit-level pin of the ranking calls (tests/golden/rank_bits.json, tests/test_gpu_rank_bits.py).

A fixed set of small problems goes through fm_rank_candidates / fm_rank_batch, their _select forms and
fm_rank_positions / fm_rank_positions_batch; per case the tool records a SHA-256 of the index bytes and
one of the score bytes (for the positions calls: of the position bytes and of the score bytes).  A
refactor of the summaries, the score kernels, the exclude mask, the merge, the counting pass or the
host code that tiles and uploads for them must reproduce every digest.

    python tools/rank_bits.py --out tests/golden/rank_bits.json     # record (GPU)
    python tools/rank_bits.py --check tests/golden/rank_bits.json   # compare (GPU)

The recorded bits depend on the compiler as well as on the code (fma contraction, the order of a
reduction the optimiser is free to pick): after a toolchain change, regenerate the fixture from a
known-good commit's library (FM_HIP_LIB=<that build> python tools/rank_bits.py --out ...), never from
the code under test.

Every problem: one single-table context over 4,096 features with globalBias 0.125 and a third of the
ids absent from the loaded model; rows of 1 .. 12 entries, of which
  * a few context and candidate rows hold absent ids alone or nothing at all (no learned entry: such a
    pair ranks at globalBias, unclamped),
  * candidate rows 900, 1030 and 2048 repeat the content of rows 17, 17 and 3 (ties, within a chunk
    and across two, broken by the row),
3 contexts (the second without a learned entry) or 600, and up to 2,049 candidates: two chunks of
1,024 rows and one row.
"""
from __future__ import annotations

import argparse
import functools
import hashlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F = 4096
C_MAX = 2049
W0 = 0.125
INF = math.inf
_UNLEARNED_CAND = (5, 700, 1024, 2047)  # candidate rows without a learned entry (700: no entry at all)
_COPIES = ((900, 17), (1030, 17), (2048, 3))  # (row, the row whose content it repeats)


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _rows(rng, n, unlearned, empty=()):
    """n rows as lists of (ids, values): ids distinct and ascending; a row of `unlearned` holds ids the
    model lacks (id % 3 == 1) alone, a row of `empty` nothing."""
    absent = np.arange(1, F, 3)
    rows = []
    for r in range(n):
        z = int(rng.integers(1, 13))
        ids = np.sort(rng.choice(absent if r in unlearned else F, size=z, replace=False))
        val = _f32(rng.normal(0.0, 1.0, size=z))
        if r in empty:
            ids, val = ids[:0], val[:0]
        rows.append((ids, val))
    return rows


def _csr(rows):
    from fm_spark_amd._native import CSRHost

    rp = np.cumsum([0] + [len(i) for i, _ in rows]).astype(np.int64)
    col = np.concatenate([i for i, _ in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    val = np.concatenate([v for _, v in rows] + [np.zeros(0)])
    return CSRHost(rp, col, val, np.zeros(len(rows)))


@functools.lru_cache(maxsize=None)
def problem(k):
    """(ids, w, V of the loaded model, the 3 contexts, the 600 contexts, the candidates as row lists)
    for k factors, built once."""
    rng = np.random.default_rng(5200 + k)
    ids = np.arange(F, dtype=np.int32)
    keep = ids[ids % 3 != 1]  # a third of the ids absent
    w = _f32(rng.normal(0.0, 0.1, F))[keep]
    V = _f32(rng.normal(0.0, 0.1, (F, k)))[keep]
    ctx3 = _rows(rng, 3, unlearned={1})
    ctx600 = _rows(rng, 600, unlearned={0, 340, 341, 599}, empty={341})
    cands = _rows(rng, C_MAX, unlearned=set(_UNLEARNED_CAND), empty={700})
    for r, src in _COPIES:
        cands[r] = cands[src]
    return keep, w, V, ctx3, ctx600, cands


def _lists(name):
    """The per-context row lists of the 3-context cases, over the 2,049 candidates."""
    e = np.zeros(0, np.int64)
    return {
        # EXCEPT
        "empty": [e, e, e],
        "straddle": [np.arange(1020, 1030), np.arange(1000, 1100), np.concatenate([[0, 1023, 1024], np.arange(2040, C_MAX)])],
        "chunk": [np.arange(1024), np.arange(1024, 2048), np.arange(C_MAX)],  # the last: nothing eligible
        "mixed": [e, np.arange(1023, 1026), np.arange(1024)],
        # ONLY: an empty list, one longer than a chunk, a short one with the tied and the unlearned rows
        "ragged": [e, np.arange(C_MAX)[np.arange(C_MAX) % 4 != 1], np.array([3, 5, 17, 700, 900, 1030, 2047, 2048])],
        # positions: more than 1,024 targets; the tied and the unlearned rows; two rows
        "targets": [np.arange(C_MAX)[np.arange(C_MAX) % 4 != 0], np.array([5, 17, 700, 900, 1030]), np.array([3, 2048])],
        # ... and exclude lists that hold targets of their own context (rows 1001 .. 1099; row 17)
        "excluded": [np.arange(1000, 1100), np.concatenate([[17], np.arange(1024, 2048)]), e],
    }[name]


# name -> (call, k, contexts, C, n_top, list name or None, exclude list name or None, batch form, lo, hi)
CASES = {}
for _k in (4, 16, 80):
    for _c in (1023, 1025, 2049):
        for _n in (1, 100):
            CASES[f"all_k{_k}_C{_c}_n{_n}"] = ("rank", _k, 3, _c, _n, None, None, False, -INF, INF)
CASES["all_k16_C2049_n100_clamped"] = ("rank", 16, 3, 2049, 100, None, None, False, 0.0, 0.25)
CASES["all_k16_C1025_n100_batch"] = ("rank", 16, 3, 1025, 100, None, None, True, -INF, INF)
for _l in ("empty", "straddle", "chunk", "mixed"):
    CASES[f"except_{_l}_k16"] = ("rank", 16, 3, 2049, 100, None, _l, False, -INF, INF)
CASES["except_straddle_k80_n1"] = ("rank", 80, 3, 2049, 1, None, "straddle", False, -INF, INF)
CASES["except_mixed_k16_batch"] = ("rank", 16, 3, 2049, 100, None, "mixed", True, -INF, INF)
CASES["only_ragged_k16"] = ("rank", 16, 3, 2049, 100, "ragged", None, False, -INF, INF)
CASES["only_ragged_k80_n1"] = ("rank", 80, 3, 2049, 1, "ragged", None, False, -INF, INF)
CASES["only_ragged_k4_batch_clamped"] = ("rank", 4, 3, 2049, 100, "ragged", None, True, 0.0, 0.25)
# 600 contexts at n_top = 1024: one split, 341 contexts per pass of the score kernel -> two passes
CASES["all_k4_U600_n1024"] = ("rank", 4, 600, 2049, 1024, None, None, False, -INF, INF)
CASES["positions_k16"] = ("positions", 16, 3, 2049, 0, "targets", None, False, -INF, INF)
CASES["positions_k16_excluded"] = ("positions", 16, 3, 2049, 0, "targets", "excluded", False, -INF, INF)
CASES["positions_k80_excluded_batch"] = ("positions", 80, 3, 2049, 0, "targets", "excluded", True, -INF, INF)
CASES["positions_k4_clamped"] = ("positions", 4, 3, 2049, 0, "targets", None, False, 0.0, 0.25)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(name):
    from fm_spark_amd.engine import FMContext

    call, k, U, Cn, n_top, lst, excl, batch, lo, hi = CASES[name]
    ids, w, V, ctx3, ctx600, cands = problem(k)
    ctx = FMContext(F, k, w0=W0)
    ctx.load_tables(ids, w, V)
    cu, cc = _csr(ctx3 if U == 3 else ctx600), _csr(cands[:Cn])
    held = [ctx.batch(cu), ctx.batch(cc)] if batch else []
    rows = held or [cu, cc]
    exclude = None if excl is None else _lists(excl)
    if call == "rank":
        fn = ctx.rank_batch if batch else ctx.rank
        idx, score = fn(*rows, n_top, lo, hi, only=None if lst is None else _lists(lst), exclude=exclude)
        out = {"index": _sha(idx), "score": _sha(score)}
    else:
        fn = ctx.rank_positions_batch if batch else ctx.rank_positions
        _, _, position, score = fn(*rows, _lists(lst), lo, hi, exclude=exclude)
        out = {"position": _sha(position), "score": _sha(score)}
    for b in held:
        b.close()
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
