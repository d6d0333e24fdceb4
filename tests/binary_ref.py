"""The binary evaluation's reference (fm_binary_metrics / fm_evaluate_binary*, include/fm_hip.h): the
integers of a record computed exactly, the log loss sum formed term by term as the kernel forms it and
summed with math.fsum, and the error budget of the device's sum.

Integers.  positive = label > 0.5, predicted positive = score > 0.  two_u (twice the Mann-Whitney U of the
positives over the negatives: 2 per pair the positive wins, 1 per tie) comes from the sorted formula the
device uses -- over the ascending scores, with cp[i] positives and A(i) = i - cp[i] negatives before position
i, a run [s, e) of equal scores adds (cp[e] - cp[s]) (A(s) + A(e)) -- in Python integers; `two_u_quadratic`
is the definition itself, a loop over all pairs, and tests/test_binary_cpu.py holds the first to the second.
Scores compare as IEEE doubles: -0.0 == +0.0.  The device must give these integers exactly.

Log loss.  A row's term is t = (max(s, 0) + log1p(exp(-|s|))) - y s, every operation in fp64 (fm_device.h,
softplus_d).  The reference forms the same expression with NumPy and sums with math.fsum.  The device's sum
may differ for two reasons, and the budget is the sum of both bounds (U = 2^-53, the unit roundoff):

 1. It adds its terms in another order: at most (n + 1) U fsum(|t_i|), eval_ref.budget's bound for a
    reordered fp64 sum.
 2. Its terms are not bit for bit the host's.  Per row, with e = exp(-|s|) in (0, 1], L = log1p(e) in
    (0, ln 2], m = max(s, 0):
      - exp and log1p.  The HIP math API reference lists both within 1 ulp in double precision; where that
        document is not at hand the limits the device library is specified to are the OpenCL C ones, which
        are looser and therefore safe to budget with: exp <= 3 ulp, log1p <= 2 ulp (K_EXP, K_LOG1P below).
        The host's libm (glibc: both within 1 ulp) is no better than K_HOST = 1 either.  An error of k ulp
        in e moves L by at most k 2^-52 e (|d log1p / de| <= 1); log1p's own error is at most k 2^-52 L.
        So the two sides' L differ by at most  2^-52 ((K_EXP + K_HOST) e + (K_LOG1P + K_HOST) L).
      - m + L is rounded on each side: 2 U (m + L).
      - y s: the host rounds the product, the device may contract it into the subtraction (an fma keeps it
        unrounded): U |y s|.  The subtraction itself is rounded on each side: 2 U |t|.
    At y = 1 and large s, m + L and y s are both about s and t is tiny: the allowance is then absolute in
    |s| (about 3 U s per row), not relative to t -- that is the cancellation, and it is in the formula, not
    added by hand.
It is derived from the formats and the libraries' stated limits, not tuned to what the kernel returns.
"""

from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

import eval_ref

U = eval_ref.U
K_EXP, K_LOG1P, K_HOST = 3, 2, 1


def positives(label) -> np.ndarray:
    return np.asarray(label, dtype=np.float64) > 0.5


def two_u_sorted(score, label) -> int:
    s = np.asarray(score, dtype=np.float64) + 0.0
    pos = positives(label)
    order = np.argsort(s, kind="stable")
    ss, sp = s[order], pos[order]
    n = len(ss)
    cp = [0] * (n + 1)
    for i in range(n):
        cp[i + 1] = cp[i] + int(sp[i])
    total, b = 0, 0
    while b < n:
        e = b + 1
        while e < n and ss[e] == ss[b]:
            e += 1
        total += (cp[e] - cp[b]) * ((b - cp[b]) + (e - cp[e]))
        b = e
    return total


def two_u_fast(score, label) -> int:
    """two_u_sorted vectorised (the GPU tests' larger shapes); exact: int64 throughout, n < 2^31"""
    s = np.asarray(score, dtype=np.float64) + 0.0
    pos = positives(label)
    n = len(s)
    if n == 0:
        return 0
    order = np.argsort(s, kind="stable")
    ss, sp = s[order], pos[order]
    cp = np.concatenate([[0], np.cumsum(sp, dtype=np.int64)])
    heads = np.flatnonzero(np.concatenate([[True], ss[1:] != ss[:-1]])).astype(np.int64)
    ends = np.concatenate([heads[1:], [n]]).astype(np.int64)
    terms = (cp[ends] - cp[heads]) * ((heads - cp[heads]) + (ends - cp[ends]))
    return int(sum(int(t) for t in terms.tolist()))


def two_u_quadratic(score, label) -> int:
    """the definition: every (positive, negative) pair, 2 for a win, 1 for a tie"""
    s = np.asarray(score, dtype=np.float64)
    pos = positives(label)
    total = 0
    for i in np.flatnonzero(pos):
        for j in np.flatnonzero(~pos):
            total += 2 if s[i] > s[j] else 1 if s[i] == s[j] else 0
    return total


def loss_terms(score, label) -> np.ndarray:
    """softplus(s) - y s per row, every operation as the kernel's"""
    s = np.asarray(score, dtype=np.float64)
    y = np.asarray(label, dtype=np.float64)
    return (np.maximum(s, 0.0) + np.log1p(np.exp(-np.abs(s)))) - y * s


def term_allowance(score, label) -> np.ndarray:
    """bound 2 of the module text, per row"""
    s = np.asarray(score, dtype=np.float64)
    y = np.asarray(label, dtype=np.float64)
    e = np.exp(-np.abs(s))
    L = np.log1p(e)
    m = np.maximum(s, 0.0)
    t = (m + L) - y * s
    return 2.0 * U * ((K_EXP + K_HOST) * e + (K_LOG1P + K_HOST) * L) + 2.0 * U * (m + L) + U * np.abs(y * s) + 2.0 * U * np.abs(t)


def log_loss(score, label) -> eval_ref.Sum:
    t = loss_terms(score, label)
    return eval_ref.Sum(math.fsum(t.tolist()), eval_ref.budget(t) + math.fsum(term_allowance(score, label).tolist()))


@dataclass(frozen=True)
class Ref:
    n_rows: int
    n_pos: int
    tp: int
    fp: int
    two_u: int
    loss: eval_ref.Sum

    @property
    def integers(self):
        return (self.n_rows, self.n_pos, self.tp, self.fp, self.two_u)


def record(score, label, two_u=two_u_fast, with_loss=True) -> Ref:
    s = np.asarray(score, dtype=np.float64)
    pos = positives(label)
    hit = s > 0.0
    loss = log_loss(s, label) if with_loss else eval_ref.Sum(math.nan, math.inf)
    return Ref(len(s), int(pos.sum()), int((pos & hit).sum()), int((~pos & hit).sum()), two_u(s, label), loss)


def integers_of(rec):
    """the integers of a BinarySums"""
    return (rec.n_rows, rec.n_pos, rec.tp, rec.fp, rec.two_u)


def check(rec, score, label, loss_budgets: float = 1.0, with_loss=True) -> Ref:
    """rec (a BinarySums) against the record of (score, label): integers with ==, the log loss within
    loss_budgets times the budget; returns the reference."""
    ref = record(score, label, with_loss=with_loss)
    assert integers_of(rec) == ref.integers, (integers_of(rec), ref.integers)
    if with_loss:
        off = abs(rec.sum_log_loss - ref.loss.value)
        print(f"log loss {rec.sum_log_loss!r} exact {ref.loss.value!r} off {off:.3e} budget {loss_budgets * ref.loss.budget:.3e}")
        assert math.isfinite(rec.sum_log_loss)
        assert off <= loss_budgets * ref.loss.budget, "sum_log_loss: " + ref.loss.miss(rec.sum_log_loss)
    return ref
