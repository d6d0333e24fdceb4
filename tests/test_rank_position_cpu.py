"""CPU: the reference of fm_rank_positions (tests/rank_position_ref.py) against an O(C^2) loop, every
RankingEvaluator metric against a literal restatement on hand cases whose values are written out, the
binding of the two new entry points, and the Python layer's argument errors.  No GPU."""

import ctypes as C
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rank_position_ref as P
import rank_ref as R
from fm_spark_amd import _native as N
from fm_spark_amd.engine import FMContext
from fm_spark_amd.tuning import RANKING_METRICS, RankingEvaluator, ranking_metric

HEADER = Path(__file__).resolve().parents[1] / "include" / "fm_hip.h"
_I32P, _I64P, _DP, _P = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.c_void_p


# ---------------------------------------------------------------------------- the reference
def tiny(seed=1, U=4, Cn=37, distinct=6):
    rng = np.random.default_rng(seed)
    w, V, present = R.make_table(rng, 64, 3)
    ctxs = R.make_rows(rng, [5, 0, 1, 9][:U], 64)
    rows = R.make_rows(rng, np.array([4, 0, 1, 7, 2, 3])[np.arange(distinct) % 6], 64)
    cands = R.take_rows(rows, rng.integers(0, distinct, Cn))  # copies: exact ties, also at w0 (context 1, the empty rows)
    return R.pair_ref(w, V, present, 0.5, ctxs, cands)


def test_positions_against_the_quadratic_loop():
    ref = tiny()
    U, Cn = ref.key.shape
    rng = np.random.default_rng(2)
    ties = 0
    for u in range(U):
        elig = rng.random(Cn) < 0.7
        targets = np.sort(rng.choice(Cn, 20, replace=False))
        got = P.positions(ref.key[u], elig, targets)
        for t, g in zip(targets, got):
            if not elig[t]:
                assert g == -1
                continue
            want = 0
            for c in range(Cn):
                if elig[c] and (ref.key[u, c] > ref.key[u, t] or (ref.key[u, c] == ref.key[u, t] and c < t)):
                    want += 1
            assert g == want
            ties += int(np.sum(elig & (ref.key[u] == ref.key[u, t])) > 1)
        # all eligible rows as targets: a permutation
        every = P.positions(ref.key[u], elig, np.arange(Cn))
        assert sorted(every[elig].tolist()) == list(range(int(elig.sum()))) and np.all(every[~elig] == -1)
    assert ties > 10


def test_interval_holds_the_exact_position_and_is_it_without_near_ties():
    ref = tiny(seed=3, distinct=30)
    U, Cn = ref.key.shape
    rng = np.random.default_rng(4)
    single = wide = 0
    for u in range(U):
        elig = rng.random(Cn) < 0.8
        targets = np.flatnonzero(elig)
        lo, hi = P.Pairs(ref, u, targets).interval(elig)
        pos = P.positions(ref.key[u], elig, targets)
        assert np.all(lo <= pos) and np.all(pos <= hi)
        for t, a, b in zip(targets, lo, hi):
            near = elig & (np.abs(ref.key[u] - ref.key[u, t]) <= np.minimum(ref.bound[u], ref.bound[u, t]))
            near[t] = False
            assert b - a == near.sum()  # as wide as the rows within the bound, literally
            single += a == b
            wide += a < b
    assert single > 10 and wide > 10


# ------------------------------------------------------------------------------ the metrics
def literal(name, k, ranked, relevant):
    """Spark's RankingMetrics on one context, restated on the ranked list itself: `ranked` the eligible
    rows in order, `relevant` the set of target rows (all of them eligible)."""
    rel = [r in relevant for r in ranked]
    T = len(relevant)
    if name == "precisionAtK":
        return sum(rel[:k]) / k
    if name == "recallAtK":
        return sum(rel[:k]) / T
    if name == "hitRateAtK":
        return float(any(rel[:k]))
    if name == "ndcgAtK":
        dcg = sum(1.0 / math.log2(i + 2) for i, r in enumerate(rel[:k]) if r)
        return dcg / sum(1.0 / math.log2(i + 2) for i in range(min(k, T)))
    if name == "meanAveragePrecision":
        hits, total = 0, 0.0
        for i, r in enumerate(rel):
            if r:
                hits += 1
                total += hits / (i + 1)
        return total / T
    if name == "meanReciprocalRank":
        return next(1.0 / (i + 1) for i, r in enumerate(rel) if r)
    pairs = [(i, j) for i, r in enumerate(rel) if r for j, q in enumerate(rel) if not q]  # auc
    return sum(i < j for i, j in pairs) / len(pairs)


# name -> (ranked rows, relevant rows).  Eight rows at most.
HAND = {
    "perfect": ([3, 1, 4, 0, 2, 5], {3, 1}),
    "reversed": ([3, 1, 4, 0, 2, 5], {2, 5}),
    "mixed": ([7, 6, 5, 4, 3, 2, 1, 0], {6, 3, 0}),
    "one target": ([0, 1, 2], {1}),
}
# the values, written out: metric -> case -> k -> value
L2 = math.log2
WRITTEN = {
    "precisionAtK": {"perfect": {1: 1.0, 2: 1.0, 10: 0.2}, "reversed": {2: 0.0, 5: 0.2, 10: 0.2},
                     "mixed": {2: 0.5, 5: 0.4}, "one target": {1: 0.0, 10: 0.1}},
    "recallAtK": {"perfect": {1: 0.5, 2: 1.0, 10: 1.0}, "reversed": {2: 0.0, 5: 0.5, 10: 1.0},
                  "mixed": {2: 1 / 3, 5: 2 / 3, 10: 1.0}, "one target": {1: 0.0, 2: 1.0}},
    "hitRateAtK": {"perfect": {1: 1.0}, "reversed": {4: 0.0, 5: 1.0}, "mixed": {1: 0.0, 2: 1.0}, "one target": {1: 0.0, 10: 1.0}},
    "ndcgAtK": {"perfect": {1: 1.0, 2: 1.0, 10: 1.0},
                "reversed": {4: 0.0, 5: (1 / L2(6)) / (1 + 1 / L2(3)), 10: (1 / L2(6) + 1 / L2(7)) / (1 + 1 / L2(3))},
                "mixed": {2: (1 / L2(3)) / (1 + 1 / L2(3)), 10: (1 / L2(3) + 1 / L2(6) + 1 / L2(9)) / (1 + 1 / L2(3) + 0.5)},
                "one target": {1: 0.0, 10: 1 / L2(3)}},
    "meanAveragePrecision": {"perfect": {10: 1.0}, "reversed": {10: (1 / 5 + 2 / 6) / 2}, "mixed": {1: (1 / 2 + 2 / 5 + 3 / 8) / 3},
                             "one target": {10: 0.5}},
    "meanReciprocalRank": {"perfect": {10: 1.0}, "reversed": {10: 0.2}, "mixed": {1: 0.5}, "one target": {10: 0.5}},
    "auc": {"perfect": {10: 1.0}, "reversed": {10: 0.0}, "mixed": {10: (4 + 2 + 0) / 15}, "one target": {10: 0.5}},
}


def as_positions(cases):
    """(ptr, position, n_eligible) of hand cases, the targets of a context in ascending row order."""
    ptr, pos, n = [0], [], []
    for ranked, relevant in cases:
        pos += [ranked.index(r) for r in sorted(relevant)]
        ptr.append(len(pos))
        n.append(len(ranked))
    return np.array(ptr), np.array(pos, np.int32), np.array(n)


@pytest.mark.parametrize("name", RANKING_METRICS)
def test_every_metric_on_the_hand_cases(name):
    assert set(WRITTEN) == set(RANKING_METRICS)
    for case, by_k in WRITTEN[name].items():
        ranked, relevant = HAND[case]
        for k, want in by_k.items():
            ev = RankingEvaluator().setMetricName(name).setK(k)
            got = ev.evaluatePositions(*as_positions([HAND[case]]))
            assert got == pytest.approx(want, rel=1e-14, abs=0), (case, k)
            assert got == pytest.approx(literal(name, k, ranked, relevant), rel=1e-14, abs=0), (case, k)
            assert ev.numContextsUsed == 1 and ev.isLargerBetter()
    # k larger than the list is in the table above (k = 10 against 3 to 8 rows); the mean over contexts:
    k = 2
    cases = list(HAND.values())
    value, used = ranking_metric(name, k, *as_positions(cases))
    assert used == 4
    assert value == pytest.approx(sum(literal(name, k, r, t) for r, t in cases) / 4, rel=1e-14)


@pytest.mark.parametrize("name", RANKING_METRICS)
def test_contexts_without_a_target_are_left_out(name):
    ptr, pos, n = as_positions([HAND["mixed"], ([0, 1, 2], set()), HAND["reversed"]])
    alone = [ranking_metric(name, 3, *as_positions([HAND[c]]))[0] for c in ("mixed", "reversed")]
    value, used = ranking_metric(name, 3, ptr, pos, n)
    assert used == 2 and value == pytest.approx(sum(alone) / 2, rel=1e-14)
    # a target that is not eligible (-1) does not count as one: the context is as without it
    ptr2, pos2 = np.array([0, 4, 5, 7]), np.concatenate([pos[:3], [-1], [-1], pos[3:]]).astype(np.int32)
    assert ranking_metric(name, 3, ptr2, pos2, n) == (value, used)
    # nothing to average: NaN and 0 contexts; auc also leaves out a context whose eligible rows are all targets
    value, used = ranking_metric(name, 3, np.array([0, 0]), np.zeros(0, np.int32), np.array([5]))
    assert math.isnan(value) and used == 0
    value, used = ranking_metric(name, 3, np.array([0, 2]), np.array([1, 0], np.int32), np.array([2]))
    assert used == (0 if name == "auc" else 1)


def test_ties_rank_by_row_in_the_reference_and_the_metrics_follow():
    """Tied keys: the positions are those of the (key, row) order, and each metric is the literal one of
    that ranked list."""
    key = np.array([0.5, 2.0, 0.5, 2.0, 0.5, -1.0, 2.0, 0.5])  # three rows tie at 2.0, four at 0.5
    elig = np.ones(8, bool)
    elig[3] = False
    ranked = [1, 6, 0, 2, 4, 7, 5]
    targets = [2, 3, 6, 7]
    pos = P.positions(key, elig, targets)
    assert pos.tolist() == [3, -1, 1, 5]
    for name in RANKING_METRICS:
        for k in (1, 2, 4, 10):
            got, used = ranking_metric(name, k, [0, 4], pos, [7])
            assert used == 1 and got == pytest.approx(literal(name, k, ranked, {2, 6, 7}), rel=1e-14), (name, k)


# ------------------------------------------------------------------------------- the binding
def test_header_binding_and_exports():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in ("fm_rank_positions", "fm_rank_positions_batch"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text)
    csrp = C.POINTER(N.fm_csr)
    tail = [_I64P, _I32P, _I64P, _I32P, C.c_double, C.c_double, _I32P, _DP]
    assert N.SIGNATURES["fm_rank_positions"] == (C.c_int, [_P, csrp, csrp] + tail)
    assert N.SIGNATURES["fm_rank_positions_batch"] == (C.c_int, [_P, _P, _P] + tail)
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.lib_path())], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (fm_\w+)$", out, flags=re.M))
    assert {"fm_rank_positions", "fm_rank_positions_batch"} <= exported


def test_null_context_is_an_error_with_a_message():
    lib = N.load()
    for fn in (lib.fm_rank_positions, lib.fm_rank_positions_batch):
        lib.fm_create(None, None)  # leaves another message behind
        assert fn(None, None, None, None, None, None, None, 0.0, 1.0, None, None) == -1
        assert b"null fm_ctx" in lib.fm_last_error()


# ------------------------------------------------------------------------ the Python layer
def test_python_level_argument_errors():
    call = lambda targets, exclude=None: FMContext._rank_positions(None, None, "fm_rank_positions", None, None, 3, targets,
                                                                   0.0, 1.0, exclude)
    with pytest.raises(ValueError, match="targets"):
        call(None)
    with pytest.raises(ValueError, match="per context"):
        call([[0], [1]])
    with pytest.raises(ValueError, match="per context"):
        call([[0], [1], [2]], exclude=[[0]])
    with pytest.raises(ValueError, match="integers"):
        call([[0.5], [1], [2]])
    ev = RankingEvaluator()
    assert ev.getMetricName() == "ndcgAtK" and ev.getK() == 10
    with pytest.raises(ValueError, match="unsupported"):
        ev.setMetricName("rmse")
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            ev.setK(bad)
    with pytest.raises(ValueError, match="unsupported"):
        ranking_metric("ndcg", 1, [0], [], [])
    with pytest.raises(ValueError):
        ranking_metric("auc", 0, [0], [], [])
    with pytest.raises(ValueError, match="ptr"):
        ev.evaluatePositions([0, 2], [1], [5])          # ptr ends beyond the positions
    with pytest.raises(ValueError, match="ptr"):
        ev.evaluatePositions([0, 1], [1], [5, 5])       # one n_eligible too many
