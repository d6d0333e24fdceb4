"""The layouts of tests/test_gpu_update_edges.py, written in the units of the update side's geometry
(update_probe.Geometry: G = entries per lane group, Wv = per wave, B = per block, the combine's
ranges, the split's chunk), with, for each, the structural events it must contain (runs.classify)
and the entries whose loss no comparison may miss (the designated boundary entries).

No GPU here: tests/test_runs_cpu.py builds every case, checks its events and its sensitivity on the
oracle alone; the GPU tests build the same cases and run them.
"""

from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np

import runs
from oracle import fm_ref as R

RTOL, ATOL = 1e-5, 1e-8  # the project's tolerance (test_gpu_parity)
REG = 1e-3  # reg_param > 0: rows untouched by step 1 reach step 2 with an L1 catch-up pending
N_EXTRA = 8  # features only the first step's batch touches
STEP1 = 0.3  # the first step's step_size
SEEDS = 12  # draws tried, in order, for one that meets the sensitivity condition

K_ALL = (1, 5, 8, 9, 16, 24, 32, 40, 64, 72, 128, 136, 256)
K_LONG = (1, 8, 12, 64, 72, 256)
K_SHARDED = (8, 16, 24, 72)
K_SPLIT = (3, 16)
K_FUSED_MAX = 16  # the fused step serves k <= 16
LONG_FOLLOW = (64, 65, 66, 128, 129, 130)
LONG_START = (0, 3)


# ------------------------------------------------------------------------------------- layouts
# Each returns SimpleNamespace(N, spans, check): the designated runs at absolute positions of the
# view the segmented update consumes, and the assertion on runs.classify_update's events.
def _need(ev, *flags):
    missing = [f for f in flags if f not in ev.flags]
    assert not missing, f"layout lacks {missing}: has {sorted(ev.flags)}"


def lay_groups(g):
    G, Wv = g.group, g.wave
    NG, h = Wv // G, g.group // 2
    assert G >= 4 and NG >= 4
    nwh = min(3, NG - 2)  # whole groups a tail piece can pass inside one wave and still close mid-group
    spans = [
        (Wv, Wv + G - 1),  # fills group 0 of wave 1
        (Wv + G + h, Wv + 2 * G - 1),  # from mid-group to the group's last entry
        (Wv + 2 * G, Wv + 2 * G + h - 1),  # from the group's first entry to mid-group
        (2 * Wv + G - 1, 2 * Wv + G),  # 2 astride a group boundary
        (3 * Wv + h, 3 * Wv + (nwh + 1) * G + h - 1),  # a tail through nwh whole groups, closing mid-group
        (5 * Wv - h, 5 * Wv + 3 * G + h - 1),  # a wave's first piece through 3 whole groups, closing mid-group
    ]

    def check(ev):
        _need(ev, "run_fills_group", "run_ends_on_group_last", "run_starts_on_group_first", "run2_astride_group",
              "tail_open_from_last_group", "last_wave_partial", "inplace_close")
        assert (nwh, True) in ev.tail_chains, ev.tail_chains
        assert (3, True) in ev.head_chains, ev.head_chains
        # the paired stores' layouts: both groups of a pair close in one entry step, either alone, and
        # an even group whose partner lies past N
        assert {"both_close", "even_closes_alone", "odd_closes_alone", "even_closes_partner_empty"} <= ev.pair, ev.pair

    return SimpleNamespace(N=7 * Wv + 3, spans=spans, check=check)


def lay_singletons(g):
    def check(ev):
        _need(ev, "all_singletons", "last_wave_partial")
        assert "both_close" in ev.pair and ev.n_runs == ev.N

    return SimpleNamespace(N=g.block + g.wave + 5, spans=[], check=check)


def lay_waves(g):
    Wv, B = g.wave, g.block
    assert B >= 2 * Wv
    later = 3 * B // Wv
    spans = [
        (0, Wv - 1),  # exactly one wave, at range 0
        (B - 1, B),  # 2 astride a block boundary
        (B + Wv - 1, B + Wv),  # 2 astride a wave boundary inside a block
        (2 * B + Wv - 4, 2 * B + Wv - 1),  # ends on a wave's last entry ...
        (2 * B + Wv, 2 * B + Wv + 2),  # ... and a new run follows
        (later * Wv, (later + 1) * Wv - 1),  # exactly one wave, at a later range
        (4 * B + Wv - 1, 4 * B + Wv + 1),  # opens on a wave's last entry
    ]

    def check(ev):
        _need(ev, "run2_astride_wave", "run2_astride_block", "run_ends_on_wave_last_then_new",
              "run_opens_on_wave_last", "tail_open_from_wave_last_entry", "last_wave_partial")
        assert {0, later} <= set(ev.run_is_wave), ev.run_is_wave

    return SimpleNamespace(N=4 * B + 2 * Wv + 7, spans=spans, check=check)


def lay_combine(g):
    L = g.wave
    per_wave = 64 // g.comb_lanes
    assert per_wave >= 3 and L >= 32
    base = per_wave * -(-16 // per_wave)  # the first range of a combine wave, past the spans before it
    spans = [
        (0, L + 4),  # owner starting exactly on p0 = 0
        (3 * L - 1, 3 * L),  # tail of 1 + head of 1
        (4 * L - 7, 5 * L - 1),  # tail + a head that is the whole next wave; the range after starts a new key
        (6 * L, 7 * L + 4),  # owner starting exactly on p0 > 0
        (8 * L + L // 2, 10 * L),  # the shortest long run: mid-range c, all of c + 1, the first entry of c + 2
        (12 * L + 5, 15 * L + L // 2),  # ranges 13 and 14 lie wholly inside the run: they must not own
        (base * L + 3, (base + 2) * L),  # two long runs whose owner ranges (base, base + 2) share
        ((base + 2) * L + 9, (base + 4) * L + 2),  # one combine wave
    ]

    def check(ev):
        _need(ev, "owner_starts_on_p0_range0", "owner_starts_on_p0_later", "two_tail1_head1", "two_head_is_whole_wave",
              "long_ends_on_first_of_c2", "two_longs_in_one_combine_wave", "wave_inside_run_full")
        assert {13, 14} <= set(ev.nonowners_inside), ev.nonowners_inside
        assert {base, base + 2} <= {r.c for r in ev.owners_long}

    return SimpleNamespace(N=(base + 5) * L + 11, spans=spans, check=check)


TAIL_N = {"1": lambda g: 1, "Wv-1": lambda g: g.wave - 1, "Wv": lambda g: g.wave, "Wv+1": lambda g: g.wave + 1,
          "B-1": lambda g: g.block - 1, "B": lambda g: g.block, "B+1": lambda g: g.block + 1,
          "2B+1": lambda g: 2 * g.block + 1}
TAIL_OWN = ("1", "Wv+1", "B+1", "2B+1")  # N - 1 a multiple of the wave: the last entry can open a new wave alone


def lay_tail(name, own, g):
    """N entries; the last run ends at N (own: the last entry is a run of its own, alone in a new wave)."""
    N = TAIL_N[name](g)
    if own or N == 1:
        spans = [(N - 1, N - 1)]
    else:
        spans = [(N - 3, N - 1)]

    def check(ev):
        assert ev.N == N
        if own:
            _need(ev, "last_entry_own_run_at_wave_start")
        elif N > 1:
            _need(ev, "last_run_multi_ends_at_N")
        if N % g.wave:
            _need(ev, "last_wave_partial")

    return SimpleNamespace(N=N, spans=spans, check=check)


def lay_long(follow, c0, g):
    """One run from the middle of range c0 into the middle of range c0 + follow: ``follow`` ranges after
    its owner begin with its key."""
    L = g.wave
    first, last = c0 * L + L // 2, (c0 + follow) * L + L // 3
    rounds = [64] * (follow // 64) + [follow % 64]

    def check(ev):
        rec = [r for r in ev.owners_long if r.c == c0]
        assert len(rec) == 1 and rec[0].follow == follow and rec[0].rounds == rounds, (rec, rounds)
        _need(ev, "wave_inside_run_full")

    n_rows = last + 38  # the run does not wrap: the first and the last entry of N share their rows with fillers
    # rows of two entries: the run's own and a filler's, which must be a present row for the run's
    # entry to have a g_V at all, so only the run's row itself is absent here (when it starts in range 3)
    return SimpleNamespace(N=2 * n_rows, spans=[(first, last)], check=check, n_rows=n_rows, fill=40, rounds=rounds,
                           absent="run" if c0 else "none")


STRUCT = {"groups": lay_groups, "singletons": lay_singletons, "waves": lay_waves, "combine": lay_combine}
for _n in TAIL_N:
    STRUCT[f"tail-{_n}"] = functools.partial(lay_tail, _n, False)
for _n in TAIL_OWN:
    STRUCT[f"tail-{_n}-own"] = functools.partial(lay_tail, _n, True)
LONG = {f"long-{n}-from-{c0}": functools.partial(lay_long, n, c0) for n in LONG_FOLLOW for c0 in LONG_START}
LAYOUTS = {**STRUCT, **LONG}
# a compacted view holds no run of 1: the layouts that are about one stay with the unfused step
UNFUSED_ONLY = {"singletons", "tail-1"} | {f"tail-{n}-own" for n in TAIL_OWN}


def ks_of(name):
    return K_LONG if name in LONG else K_ALL


def fusable(name, k):
    return k <= K_FUSED_MAX and name not in UNFUSED_ONLY


# the split's layouts: over the FULL view of a fused batch (singletons are spans of one entry)
def split_chunks(g):
    C = g.chunk
    spans = [(C + i, C + i) for i in range(C)] + [(3 * C - 1, 3 * C), (4 * C, 4 * C), (5 * C - 1, 5 * C - 1)]

    def check(sp):
        assert (sp.nm[1], sp.ns[1]) == (0, C) and sp.ns[0] == 0 and sp.ns[2] == 0  # only singletons between only multi
        assert sp.after[2] and sp.before[3]  # 2 astride a chunk: each half is multi by the key across the boundary alone
        assert not sp.multi[4 * C] and not sp.multi[5 * C - 1]  # a singleton as a chunk's first and last entry

    return SimpleNamespace(N=5 * C + 7, spans=spans, check=check)


def split_even(g):
    C = g.chunk
    N = 2 * C

    def check(sp):
        assert sp.N % C == 0 and sp.multi[N - 1] and sp.multi[N - 2] and not sp.multi[N - 3]

    return SimpleNamespace(N=N, spans=[(7, 7), (C, C), (N - 3, N - 3), (N - 2, N - 1)], check=check)


def split_odd(g):
    C = g.chunk
    N = 2 * C + 1

    def check(sp):
        assert sp.size[2] == 1 and sp.before[2] and sp.after[1] and (sp.nm[2], sp.ns[2]) == (1, 0)

    return SimpleNamespace(N=N, spans=[(7, 7), (C, C), (N - 2, N - 1)], check=check)


def split_none(g):
    N = 4 * g.block + 3

    def check(sp):
        assert sp.n_multi == 0 and sp.n_single == N

    return SimpleNamespace(N=N, spans=[(i, i) for i in range(N)], check=check)


def split_count(delta, g):
    """A compacted count of Wv + delta under a grid sized by nnz >= 4 B."""
    want = g.wave + delta
    N = 4 * g.block + 5
    lens = ([3] if want % 2 else []) + [2] * ((want - (3 if want % 2 else 0)) // 2)
    stride = (N - 8) // len(lens)
    assert stride >= 5
    multi, spans = [], []
    for i, n in enumerate(lens):
        multi.append((4 + i * stride, 4 + i * stride + n - 1))
    at = 0
    for a, b in multi:
        spans += [(p, p) for p in range(at, a)] + [(a, b)]
        at = b + 1
    spans += [(p, p) for p in range(at, N)]

    def check(sp):
        assert sp.n_multi == want and sp.N >= 4 * g.block

    return SimpleNamespace(N=N, spans=spans, check=check)


SPLIT = {"chunks": split_chunks, "N=2C": split_even, "N=2C+1": split_odd, "none": split_none,
         "count-Wv-1": functools.partial(split_count, -1), "count-Wv": functools.partial(split_count, 0),
         "count-Wv+1": functools.partial(split_count, 1)}


# ------------------------------------------------------------------------------------- cases
def _marks(spans, N, g, chunked=False):
    """The designated boundary entries: the first and last entry of N and of every designated run, and
    inside a run both sides of its wave boundaries and of its group boundaries (the first two and the last
    two of each) and the first entries of the ranges at which the combine's end search starts a round; for
    the split, both sides of every chunk boundary."""
    m = {0, N - 1}
    for a, b in spans:
        if a == b and chunked:
            continue
        m |= {a, b}
        wb = [p for p in range((a // g.wave + 1) * g.wave, b + 1, g.wave)]
        for p in wb[:2] + wb[-2:]:
            m |= {p - 1, p}
        gb = [p for p in range((a // g.group + 1) * g.group, b + 1, g.group)]
        for p in gb[:2] + gb[-2:]:
            m |= {p - 1, p}
        rb = [p for p in range((a // g.wave + 1) * g.wave, b + 1, 64 * g.wave)]  # the end search's rounds
        for p in rb:
            m |= {p, min(p + g.wave, b)}
    if chunked:
        for p in range(g.chunk, N, g.chunk):
            m |= {p - 1, p}
    return np.asarray(sorted(p for p in m if 0 <= p < N), dtype=np.int64)


def _first_batch(seed, n_runs, F, k):
    """The first step's batch: entries of the N_EXTRA last features only, so every row of the second
    batch is untouched by it."""
    lens = np.asarray([3, 1, 2, 5, 1, 2, 4, 1][:N_EXTRA])
    return runs.make_runs(seed, lens, F, k, n_rows=7, ids=np.arange(n_runs, n_runs + N_EXTRA))[0]


def step_size_for(m):
    """eta / m about 1e-4 for a batch of up to ten thousand rows, and step_size 1.5 beyond.  An entry's
    share of its row's update stays above the comparison's tolerance (asserted per case, not assumed:
    sensitivity below) while a whole run's update stays below 0.1 or so: the device forms it from fp32
    inputs (relative error 1e-7), and where the new value lands next to the L1 threshold that error must
    still sit under the absolute floor ATOL."""
    return min(max(0.03, 1.5e-4 * m), 1.5)


def _build(name, k, geom, fused, lay, kind, seed0):
    g = geom
    fill = getattr(lay, "fill", None) or (2 if fused and kind == "update" else 1)
    if kind == "split":
        lengths = runs.layout(lay.N, lay.spans, 2)
        consumed_idx = None
    elif fused:
        compact_lengths = runs.layout(lay.N, lay.spans, fill)
        lengths, consumed_idx = runs.sprinkle(compact_lengths)
    else:
        lengths = runs.layout(lay.N, lay.spans, fill)
    n_runs = len(lengths)
    keys = np.repeat(np.arange(n_runs), lengths)
    ev = runs.classify(keys, g, fused=fused)
    if kind == "split":
        lay.check(ev.split)
        marks = _marks(lay.spans, lay.N, g, chunked=True)
    else:
        lay.check(ev.update)
        in_view = _marks(lay.spans, lay.N, g)
        marks = runs.compact(keys)[1][in_view] if fused else in_view  # positions in the full view
    F = n_runs + N_EXTRA
    # absent from the model: every other designated run ...
    starts = np.concatenate([[0], np.cumsum(lengths)])[:-1]
    pos_of = {int(s): i for i, s in enumerate(starts)}
    if fused and kind == "update":
        cstarts = np.concatenate([[0], np.cumsum(compact_lengths)])[:-1]
        des = [int(consumed_idx[np.searchsorted(cstarts, a)]) for a, _ in lay.spans]
    else:
        des = [pos_of[a] for a, _ in lay.spans][:64]
    n_rows = getattr(lay, "n_rows", None)
    m = n_rows or max(int(lengths.max()), -(-int(lengths.sum()) // 6))
    # ... and a fifth of the features that share no row with a designated entry, at random: at k = 1 an
    # entry's g_V is the sum of its row's OTHER present entries, and must not vanish with their rows
    rowpos = runs.rows_of_view(lengths, m)
    shares = np.add.reduceat(np.isin(rowpos, rowpos[marks]).astype(np.int64), starts) > 0
    free = np.nonzero(~shares & (np.random.default_rng(n_runs).random(n_runs) < 0.2))[0].tolist()
    how = getattr(lay, "absent", "mixed")
    absent = {"mixed": set(des[1::2]) | set(free), "run": set(des), "none": set()}[how] | {F - 1}
    keep = np.asarray([i for i in range(F) if i not in absent], dtype=np.int32)
    step = step_size_for(m)
    last = None
    for seed in range(seed0, seed0 + SEEDS):
        csr, ids, w, V = runs.make_runs(seed, lengths, F, k, n_rows=m, big=marks)
        first = _first_batch(seed + 1000, n_runs, F, k)
        model = R.Model.empty(F, k)
        model.load(keep, w[keep], V[keep])
        o1 = R.sgd_step_fast(model, first, 1, STEP1, REG)
        before = model.copy()
        o2 = R.sgd_step_fast(model, csr, 2, step, REG)
        margin = sensitivity(before, model, csr, marks, step)
        last = margin
        if margin >= 1.0:
            break
    return SimpleNamespace(name=name, k=k, geom=g, fused=fused, kind=kind, F=F, keep=keep, w=w, V=V, batches=[first, csr],
                           steps=[STEP1, step], reg=REG, model=model, outs=[o1, o2], events=ev, marks=marks, margin=last,
                           keys=keys, before=before)


def sensitivity(before, after, csr, marks, step_size, t=2):
    """min over the designated entries e (of row i) of  (eta / m) max_f |g_V,e[f]| / (8 (RTOL max|V_i| + ATOL))
    and of the same for g_w: >= 1 means a single dropped or doubled designated entry moves its row by at
    least eight times what the comparison tolerates.  max|V_i| covers the row before and after the step."""
    order, _ = runs.sorted_view(csr)
    e = order[marks]
    dv, dw = runs.entry_update_sizes(before, csr, t, step_size)
    i = csr.col[e].astype(np.int64)
    vmax = np.maximum(np.abs(before.V[i]).max(axis=1), np.abs(after.V[i]).max(axis=1))
    wmax = np.maximum(np.abs(before.w[i]), np.abs(after.w[i]))
    # an entry alone in its row has g_V = 0 identically (S x - v x^2 with S = v x): nothing of V hangs on it
    alone = np.diff(csr.row_ptr)[np.repeat(np.arange(csr.n_rows), np.diff(csr.row_ptr))[e]] == 1
    mv = np.where(alone, np.inf, dv[e] / (8 * (RTOL * vmax + ATOL)))
    return float(min(mv.min(), (dw[e] / (8 * (RTOL * wmax + ATOL))).min()))


@functools.lru_cache(maxsize=None)
def case(name, k, geom, fused=False):
    """The case ``name`` at k factors: two batches, the tables, the oracle's two steps (computed once,
    shared by every mode that runs the case) and the events of the second batch."""
    if name in SPLIT:
        return _build(name, k, geom, True, SPLIT[name](geom), "split", 4000 + 17 * k)
    return _build(name, k, geom, fused, LAYOUTS[name](geom), "update", 2000 + 17 * k)


def assert_case(c):
    """What every test of a case asserts before it runs anything on the device: the second batch's sorted
    view is the layout (the builder against a stable host sort), and the designated entries are felt."""
    _, keys = runs.sorted_view(c.batches[1])
    np.testing.assert_array_equal(keys, c.keys)
    assert c.margin >= 1.0, f"{c.name} k={c.k}: sensitivity margin {c.margin:.3g} < 1 for every seed tried"
