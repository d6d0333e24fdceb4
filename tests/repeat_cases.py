"""Batches in which a row holds one feature id more than once, for tests/test_gpu_repeated_ids.py.

The library takes such rows (include/fm_hip.h: each occurrence is an entry of its own), and the oracle
states the rule: S sums v x of every entry, sum v^2 x^2 takes every entry, g_w takes its -y once per
entry.  runs.make_runs cannot build them (a run's entries lie in distinct rows), so make_repeat_runs
stands beside it: a batch whose sorted view is a prescribed list of runs, with a prescribed sample for
every entry of the runs it is told about.  Layouts are written in the units of update_probe.Geometry
and placed with runs.layout, as tests/update_cases.py does; every case follows its two-step protocol
(reg_param > 0, every other designated id absent from the loaded table, a first batch that touches none
of the second's rows).

For every designated (repeated) id the case asserts on the oracle alone that two wrong readings of a
repeat -- *merged*: a row's repeats become one entry with x summed; *first-only*: only the first
occurrence is kept -- each move the id's w or some column of its V by at least 8 times what the
comparison tolerates (margin >= 1).  No GPU here: tests/test_repeat_cases_cpu.py runs every case.
"""

from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import runs
import update_cases as uc
from oracle import fm_ref as R
from problems import f32

RTOL, ATOL, REG, SEEDS = uc.RTOL, uc.ATOL, uc.REG, uc.SEEDS
FACTOR = 8.0  # a wrong reading must move a designated row by this many tolerances

K_CASES = (1, 8, 16, 24, 72)  # one quad, the fused cap's neighbours, a multi-quad row (of uc.K_ALL)
K_ONE = (1, 8, 64)  # uc.K_LONG's
ONE_M = {"G": lambda g: g.group, "G+1": lambda g: g.group + 1, "Wv-1": lambda g: g.wave - 1, "Wv": lambda g: g.wave,
         "Wv+1": lambda g: g.wave + 1, "2Wv+1": lambda g: 2 * g.wave + 1}
# the positions of the repeated id in `spread`'s row of SPREAD_LEN entries: the first, the last and three
# inner ones.  A forward team takes rpp = TEAM / GS entries per pass, entry j in pass j // rpp by lane
# group j % rpp; for every power of two rpp up to 64 these five lie in five passes and in min(5, rpp)
# lane groups (spread_ok), so no table of the forward's shapes is needed
SPREAD_POS = (0, 65, 130, 195, 260)
SPREAD_LEN = 261


def spread_ok(rpp):
    p = np.asarray(SPREAD_POS)
    return len(set((p // rpp).tolist())) == len(p) and len(set((p % rpp).tolist())) == min(len(p), rpp)


# ------------------------------------------------------------------------------------- the builder
def make_repeat_runs(seed, run_lengths, F, k, *, n_rows, samples, designated=(), n_reserved=0, x_at=None,
                     place=None, big_y=10.0):
    """A batch whose sorted view is the runs ``run_lengths`` in id order (run i is feature i), as
    runs.make_runs, but with the rows of run i's entries given by samples[i] wherever i is in
    ``samples`` -- a row may repeat.  The other runs' entries go to row p mod (n_rows - n_reserved) for
    the sorted position p, so the last n_reserved rows hold only what ``samples`` puts there.  The
    stable sort orders a run by row and, within a row, by place in the row: a non-decreasing samples[i]
    (required of the ``designated`` runs) is the run's samples in view order.

    Values as make_runs.  The entries of the designated runs take |x| in [1/2, 1] (times the same
    shrink on rows of more than 16 entries), their rows a label of magnitude big_y, and in a row of up
    to 16 entries the others |x| >= 1/2.  x_at: {(run, j): x} sets single entries.  place: {row: (run,
    positions)} puts the run's entries at those places of the row (ids are otherwise ascending in a
    row).  Returns (csr, ids, w, V)."""
    rng = np.random.default_rng(seed)
    c = np.asarray(run_lengths, dtype=np.int64)
    assert c.ndim == 1 and len(c) > 0 and (c >= 1).all() and len(c) <= F
    N = int(c.sum())
    n_free = n_rows - n_reserved
    assert n_free >= 1
    starts = np.concatenate([[0], np.cumsum(c)])[:-1]
    key = np.repeat(np.arange(len(c), dtype=np.int64), c)
    row = np.arange(N, dtype=np.int64) % n_free
    for i, rows_i in samples.items():
        rows_i = np.asarray(rows_i, dtype=np.int64)
        assert rows_i.shape == (c[i],) and rows_i.min() >= 0 and rows_i.max() < n_rows, (i, rows_i, c[i])
        row[starts[i]:starts[i] + c[i]] = rows_i
    for i in designated:
        assert i in samples and (np.diff(samples[i]) >= 0).all(), "a designated run's samples must not decrease"
    free_runs = np.setdiff1d(np.arange(len(c)), list(samples))
    assert len(free_runs) == 0 or c[free_runs].max() <= n_free, "a free run's entries need distinct rows"
    order = np.lexsort((np.arange(N), key, row))  # CSR order: by row, ids ascending, repeats in view order
    row_len = np.bincount(row, minlength=n_rows)
    row_ptr = np.concatenate([[0], np.cumsum(row_len)]).astype(np.int64)
    for r, (i, at) in (place or {}).items():
        seg = order[row_ptr[r]:row_ptr[r + 1]]
        mine, rest = seg[key[seg] == i], seg[key[seg] != i]
        assert len(mine) == len(at) and max(at) < len(seg)
        out = np.full(len(seg), -1, dtype=np.int64)
        out[list(at)] = mine
        out[out < 0] = rest
        order[row_ptr[r]:row_ptr[r + 1]] = out
    col = key[order]
    row_of = np.repeat(np.arange(n_rows), row_len)
    shrink = np.minimum(1.0, 4.0 / np.sqrt(np.maximum(row_len, 1)))[row_of]
    x = f32(rng.normal(0.0, 1.0, size=N) * shrink)
    u = rng.random(N)
    x[u < 0.05] = 0.0
    x[u > 0.7] = 1.0
    y = f32(rng.normal(0.0, 1.0, n_rows))
    pos_of = np.empty(N, dtype=np.int64)  # sorted position -> CSR entry
    pos_of[:] = np.argsort(col, kind="stable")
    des = np.asarray(sorted(designated), dtype=np.int64)
    if len(des):
        e = np.concatenate([pos_of[starts[i]:starts[i] + c[i]] for i in des])
        rows_des = np.unique(row_of[e])
        y[rows_des] = big_y * np.where(rng.random(len(rows_des)) < 0.5, -1.0, 1.0)
        near = np.isin(row_of, rows_des) & (row_len[row_of] <= 16) & (np.abs(x) < 0.5)
        x[near] = 1.0
        x[e] = f32(rng.uniform(0.5, 1.0, len(e)) * np.where(rng.random(len(e)) < 0.5, -1.0, 1.0) * shrink[e])
    for (i, j), v in (x_at or {}).items():
        x[pos_of[starts[i] + j]] = v
    csr = R.CSR(row_ptr=row_ptr, col=col.astype(np.int32), val=f32(x).astype(np.float64), label=y)
    w = f32(rng.normal(0.0, 0.1, F))
    V = f32(rng.normal(0.0, 0.1, (F, k)))
    return csr, np.arange(F, dtype=np.int32), w, V


def run_samples(csr, i):
    """The rows of feature i's entries in view order."""
    rows = np.repeat(np.arange(csr.n_rows), np.diff(csr.row_ptr))
    return rows[np.nonzero(csr.col == i)[0]]


# ------------------------------------------------------------------------------------- wrong readings
def merged(csr):
    """Every row's repeats of an id as one entry with x summed (at the first occurrence's place)."""
    return _reread(csr, True)


def first_only(csr):
    """Every row's repeats of an id dropped but the first."""
    return _reread(csr, False)


def _reread(csr, add):
    rows = np.repeat(np.arange(csr.n_rows), np.diff(csr.row_ptr))
    pair = rows * (int(csr.col.max()) + 1) + csr.col
    _, first, inv = np.unique(pair, return_index=True, return_inverse=True)
    keep = np.sort(first)
    val = csr.val.copy()
    if add:
        tot = np.zeros(len(first))
        np.add.at(tot, inv, csr.val)
        val[first] = tot
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=csr.n_rows))]).astype(np.int64)
    return R.CSR(row_ptr=ptr, col=csr.col[keep], val=val[keep], label=csr.label)


def discriminators(before, after, csr, ids, step):
    """(merged, first-only): min over the designated ids of the largest |change| of the id's w or of a
    column of its V, in units of FACTOR tolerances of the true value, when the second step reads the
    batch the wrong way."""
    ids = np.asarray(ids, dtype=np.int64)
    out = []
    for wrong in (merged(csr), first_only(csr)):
        m = before.copy()
        R.sgd_step_fast(m, wrong, 2, step, REG)
        dv = np.abs(m.V[ids] - after.V[ids]) / (RTOL * np.abs(after.V[ids]) + ATOL)
        dw = np.abs(m.w[ids] - after.w[ids]) / (RTOL * np.abs(after.w[ids]) + ATOL)
        out.append(float(np.maximum(dv.max(axis=1), dw).min() / FACTOR))
    return tuple(out)


# ------------------------------------------------------------------------------------- layouts
# Each returns SimpleNamespace(N, spans, fill_spec(lengths, idx_of) -> builder arguments, check(ev)) over
# the view the segmented update consumes; idx_of(first) is the run that starts at sorted position first.
def _idx(lengths):
    starts = np.concatenate([[0], np.cumsum(lengths)])[:-1]
    at = {int(s): i for i, s in enumerate(starts)}
    return lambda first: at[first]


def _others(lengths, taken, n):
    """The first n runs not in ``taken``."""
    out = [i for i in range(len(lengths)) if i not in taken][:n]
    assert len(out) == n, "the layout holds too few free runs"
    return out


def _also_in(lengths, starts, n_free, runs_, row):
    """samples that put the last entry of each of runs_ into ``row`` (a reserved one: above every free row)."""
    s = {}
    for i in runs_:
        rows_i = np.sort((starts[i] + np.arange(lengths[i])) % n_free)
        rows_i[-1] = row
        s[i] = rows_i
    return s


def lay_pair_only(g):
    G, Wv = g.group, g.wave
    assert G >= 4 and Wv >= 4 * G
    N = Wv + 37
    spans = [(G - 1, G), (2 * G + 2, 2 * G + 3), (Wv - 1, Wv), (N - 2, N - 1)]  # astride a group and a wave, at N
    n_free = 60

    def spec(lengths, idx):
        des = [idx(a) for a, _ in spans]
        return dict(n_rows=n_free + len(des), n_reserved=len(des), designated=des,
                    samples={i: [n_free + j] * 2 for j, i in enumerate(des)})

    def check(ev, c):
        uc._need(ev, "run2_astride_group", "run2_astride_wave", "last_run_multi_ends_at_N")
        for i in c.des:
            rows = run_samples(c.batches[1], i)
            assert len(rows) == 2 and rows[0] == rows[1] and np.diff(c.batches[1].row_ptr)[rows[0]] == 2

    return SimpleNamespace(N=N, spans=spans, spec=spec, check=check)


def lay_cancel(g):
    n, n_free = 4, 40
    spans = []
    for j in range(n):
        spans += [(8 * j + 2, 8 * j + 4), (8 * j + 5, 8 * j + 6)]  # b: 3 entries, c: 2
    N = g.wave // 2 + 29

    def spec(lengths, idx):
        b = [idx(a) for a, _ in spans[0::2]]
        c_ = [idx(a) for a, _ in spans[1::2]]
        samples, x_at, place = {}, {}, {}
        for j, (ib, ic) in enumerate(zip(b, c_)):
            row = n_free + j
            samples[ib] = [2 * j + 1, row, row]  # b once in another row, then b(+3) .. b(-3)
            samples[ic] = [2 * j + 2, row]
            x_at[(ib, 1)], x_at[(ib, 2)] = 3.0, -3.0
            place[row] = (ib, (0, 2))
        return dict(n_rows=n_free + n, n_reserved=n, designated=b, samples=samples, x_at=x_at, place=place)

    def check(ev, c):
        csr = c.batches[1]
        for i in c.des:
            row = run_samples(csr, i)[-1]
            a, b = csr.row_ptr[row], csr.row_ptr[row + 1]
            assert csr.col[a:b].tolist()[::2] == [i, i] and b - a == 3 and csr.val[a] + csr.val[a + 2] == 0
            assert abs(csr.val[a]) == 3.0 and (csr.col == i).sum() == 3

    return SimpleNamespace(N=N, spans=spans, spec=spec, check=check)


def lay_spread(g):
    Wv = g.wave
    spans = [(Wv - 2, Wv + 2), (2 * Wv + 4, 2 * Wv + 8)]  # astride a wave, and inside one
    n_free = 200
    n_fill = SPREAD_LEN - len(SPREAD_POS)
    N = 2 * Wv + 20 + 4 * n_fill  # room for 2 n_fill other runs of two entries

    def spec(lengths, idx):
        des = [idx(a) for a, _ in spans]
        starts = np.concatenate([[0], np.cumsum(lengths)])[:-1]
        free = _others(lengths, set(des), 2 * n_fill)
        samples, place = {}, {}
        for j, i in enumerate(des):
            row = n_free + j
            samples[i] = [row] * len(SPREAD_POS)
            samples.update(_also_in(lengths, starts, n_free, free[j * n_fill:(j + 1) * n_fill], row))
            place[row] = (i, SPREAD_POS)
        return dict(n_rows=n_free + 2, n_reserved=2, designated=des, samples=samples, place=place)

    def check(ev, c):
        csr = c.batches[1]
        for i in c.des:
            row = run_samples(csr, i)[0]
            a, b = csr.row_ptr[row], csr.row_ptr[row + 1]
            assert b - a == SPREAD_LEN >= 40 and tuple(np.nonzero(csr.col[a:b] == i)[0]) == SPREAD_POS
        assert SPREAD_POS[0] == 0 and SPREAD_POS[-1] == SPREAD_LEN - 1

    return SimpleNamespace(N=N, spans=spans, spec=spec, check=check)


def lay_one(name, g):
    """One id m times in one row, twice: a run from a wave's first entry, and one astride a wave boundary."""
    Wv = g.wave
    m = ONE_M[name](g)
    assert 2 <= m <= 2 * Wv + 1
    a0 = Wv
    c0 = (a0 + m - 1) // Wv + 2
    s0 = c0 * Wv + Wv // 2 if m > Wv else (c0 + 1) * Wv - m // 2
    spans = [(a0, a0 + m - 1), (s0, s0 + m - 1)]
    N = s0 + m + Wv // 2 + 3
    n_free = max(40, N // 6)

    def spec(lengths, idx):
        des = [idx(a) for a, _ in spans]
        starts = np.concatenate([[0], np.cumsum(lengths)])[:-1]
        free = _others(lengths, set(des), 10)
        samples = {}
        for j, i in enumerate(des):
            samples[i] = [n_free + j] * m
            samples.update(_also_in(lengths, starts, n_free, free[5 * j:5 * j + 5], n_free + j))  # five other ids beside it
        return dict(n_rows=n_free + 2, n_reserved=2, designated=des, samples=samples)

    def check(ev, c):
        two = {(r.first, r.last) for r in ev.owners_two}
        long_ = {(r.first, r.last) for r in ev.owners_long}
        inside = {tuple(s) for s in spans} - two - long_  # runs that stay inside one range
        if m <= Wv:
            assert inside == {spans[0]} and spans[1] in two, (m, two, long_)
            if m == Wv:
                assert a0 // Wv in ev.run_is_wave
        elif m == Wv + 1:
            assert set(spans) <= two and "owner_starts_on_p0_later" in ev.flags, (m, two, long_)
        else:
            assert set(spans) <= long_ and "long_ends_on_first_of_c2" in ev.flags, (m, two, long_)
        for i in c.des:
            assert len(set(run_samples(c.batches[1], i).tolist())) == 1 and (c.batches[1].col == i).sum() == m

    return SimpleNamespace(N=N, spans=spans, spec=spec, check=check, absent_from=1 if m % 2 else 0)


def lay_mixed(g):
    Wv = g.wave
    h = Wv // 2 + 3  # rows that hold the hot id twice: about a third of them
    n_free = 3 * h
    hot = (2 * Wv - 2, 2 * Wv - 3 + 2 * h)  # two entries of range 1, all of range 2, into range 3
    assert Wv >= 64
    a = g.group + 15
    assert a + 8 < Wv - 3
    spans = [(4, 9), (a, a + 5), (Wv - 3, Wv + 2), hot]  # runs of 6 (one astride a wave), then the hot run
    N = hot[1] + 1 + Wv // 2 + 5

    def spec(lengths, idx):
        six = [idx(a) for a, b in spans if b - a == 5]
        ih = idx(hot[0])
        samples = {ih: np.repeat(np.arange(0, n_free, 3), 2)}
        for j, i in enumerate(six):
            s0 = 7 * j + 1
            samples[i] = [s0, s0, s0 + 1, s0 + 3, s0 + 3, s0 + 3]
        return dict(n_rows=n_free, n_reserved=0, designated=[ih] + six, samples=samples)

    def check(ev, c):
        assert hot in {(r.first, r.last) for r in ev.owners_long}, [(r.first, r.last) for r in ev.owners_long]
        csr = c.batches[1]
        rows = run_samples(csr, c.des[0])
        assert len(rows) == 2 * h and (rows[0::2] == rows[1::2]).all()
        assert abs(len(set(rows.tolist())) / csr.n_rows - 1 / 3) < 0.01
        for i in c.des[1:]:
            assert np.diff(run_samples(csr, i)).tolist() == [0, 1, 2, 0, 0]

    return SimpleNamespace(N=N, spans=spans, spec=spec, check=check)


LAYOUTS = {"pair-only": lay_pair_only, "cancel": lay_cancel, "spread": lay_spread, "mixed": lay_mixed}
ONE = {f"one-sample-run-{n}": functools.partial(lay_one, n) for n in ONE_M}
NAMES = list(LAYOUTS) + ["self-pair"] + list(ONE)
SMALL = ("pair-only", "cancel")  # the two oracles are compared bit for bit on these


def ks_of(name):
    return K_ONE if name in ONE else K_CASES


def fusable(k):
    return k <= uc.K_FUSED_MAX


# ------------------------------------------------------------------------------------- cases
def _finish(name, k, geom, fused, seed0, make, lengths, des, n_rows, absent_from=1):
    """The two-step protocol over the batch make(seed) -> (csr, ids, w, V) whose designated ids are des."""
    n_runs = len(lengths)
    F = n_runs + uc.N_EXTRA
    assert F <= 4096 and n_rows <= 700
    keys = np.repeat(np.arange(n_runs), lengths)
    ev = runs.classify(keys, geom, fused=fused)
    free = np.setdiff1d(np.arange(n_runs), des)
    absent = set(des[absent_from::2]) | {F - 1} | set(free[np.random.default_rng(n_runs).random(len(free)) < 0.1].tolist())
    keep = np.asarray([i for i in range(F) if i not in absent], dtype=np.int32)
    step = uc.step_size_for(n_rows)
    for seed in range(seed0, seed0 + SEEDS):
        csr, ids, w, V = make(seed)
        first = uc._first_batch(seed + 1000, n_runs, F, k)
        model = R.Model.empty(F, k)
        model.load(keep, w[keep], V[keep])
        o1 = R.sgd_step_fast(model, first, 1, step, REG)
        before = model.copy()
        o2 = R.sgd_step_fast(model, csr, 2, step, REG)
        margins = discriminators(before, model, csr, des, step)
        if min(margins) >= 1.0:
            break
    return SimpleNamespace(name=name, k=k, geom=geom, fused=fused, F=F, keep=keep, w=w, V=V, batches=[first, csr],
                           steps=[step, step], reg=REG, model=model, outs=[o1, o2], events=ev, keys=keys, before=before,
                           des=list(des), margins=margins, absent=absent)


def _build(name, k, geom, fused, lay, seed0):
    compact_lengths = runs.layout(lay.N, lay.spans, 2 if fused else 1)
    spec = lay.spec(compact_lengths, _idx(compact_lengths))
    if fused:  # the layout is the compacted view: true singletons go into the full one
        lengths, at = runs.sprinkle(compact_lengths)
        re = lambda i: int(at[i])  # noqa: E731
        spec["samples"] = {re(i): v for i, v in spec["samples"].items()}
        spec["designated"] = [re(i) for i in spec["designated"]]
        spec["x_at"] = {(re(i), j): v for (i, j), v in spec.get("x_at", {}).items()}
        spec["place"] = {r: (re(i), p) for r, (i, p) in spec.get("place", {}).items()}
    else:
        lengths = compact_lengths
    n_rows = spec["n_rows"]
    F = len(lengths) + uc.N_EXTRA
    c = _finish(name, k, geom, fused, seed0, lambda seed: make_repeat_runs(seed, lengths, F, k, **spec), lengths,
                spec["designated"], n_rows, getattr(lay, "absent_from", 1))
    c.lay = lay
    return c


def _build_self_pair(k, geom, fused, seed0):
    """Every row concatenated with itself: all ids twice, all runs even."""
    rng = np.random.default_rng(5)
    base = rng.integers(1, 6, 150)
    base[40] = 40
    n_rows = 120
    big = np.concatenate([[0], np.cumsum(base)])[:-1][::7]  # the first entry of every seventh run
    lengths = 2 * base
    F = len(lengths) + uc.N_EXTRA

    def make(seed):
        one, ids, w, V = runs.make_runs(seed, base, F, k, n_rows=n_rows, big=big)
        n = np.diff(one.row_ptr)
        take = np.concatenate([np.tile(np.arange(a, b), 2) for a, b in zip(one.row_ptr[:-1], one.row_ptr[1:])])
        ptr = np.concatenate([[0], np.cumsum(2 * n)]).astype(np.int64)
        return R.CSR(row_ptr=ptr, col=one.col[take], val=one.val[take], label=one.label), ids, w, V

    c = _finish("self-pair", k, geom, fused, seed0, make, lengths, list(range(0, len(base), 7)), n_rows)
    c.lay = None
    return c


@functools.lru_cache(maxsize=None)
def case(name, k, geom, fused=False):
    """The case ``name`` at k factors: two batches, the tables, the oracle's two steps (computed once,
    shared by every mode that runs the case), the second batch's events and both discriminators."""
    seed0 = 6000 + 17 * k
    if name == "self-pair":
        return _build_self_pair(k, geom, fused, seed0)
    return _build(name, k, geom, fused, {**LAYOUTS, **ONE}[name](geom), seed0)


def assert_case(c):
    """What every test of a case asserts before it runs anything on the device: the second batch's
    sorted view is the layout, it holds the event the case is named for, a repeated id counts once in
    n_unique, and both wrong readings of a repeat would be seen."""
    csr = c.batches[1]
    _, keys = runs.sorted_view(csr)
    np.testing.assert_array_equal(keys, c.keys)
    rows = np.repeat(np.arange(csr.n_rows), np.diff(csr.row_ptr))
    n_pairs = len(np.unique(rows * c.F + csr.col))
    assert c.outs[1].n_unique == len(np.unique(csr.col)) == len(np.unique(c.keys)) <= n_pairs < csr.nnz
    for i in c.des:
        r = rows[csr.col == i]
        assert len(r) > len(set(r.tolist())), f"designated id {i} repeats in no row"
    ev = c.events.update
    if c.lay is not None:
        assert ev.N == c.lay.N
        c.lay.check(ev, c)
    else:
        assert ev.N == csr.nnz and (np.diff(np.nonzero(np.diff(c.keys, prepend=-1))[0], append=len(c.keys)) % 2 == 0).all()
    if c.fused:
        sp = c.events.split
        assert sp.n_multi == ev.N and (sp.n_single > 0) == (c.lay is not None)
    assert min(c.margins) >= 1.0, f"{c.name} k={c.k}: discriminators (merged, first-only) {c.margins} of {FACTOR} tolerances"
