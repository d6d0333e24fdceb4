"""Batches with a prescribed run structure, and what that structure means to the update kernels.

The step's sorted view is the batch's entries stably sorted by feature id, so a batch in which
feature i has c_i entries has a sorted view of exactly the runs c_0, c_1, ... in id order.
make_runs builds such a batch; layout places designated runs at absolute sorted positions and fills
the gaps; sprinkle adds singleton features to a view (the fused step's split removes them again);
classify computes, from the key array a kernel consumes and the geometry the library reports
(tests/update_probe.py), which structural events of k_segment_update, k_segment_combine and
k_split_* occur -- a model of their control flow, not of their arithmetic.  tests/test_runs_cpu.py
checks all of it without a GPU; tests/test_gpu_update_edges.py asserts through classify that each of
its batches holds the event it is named for.
"""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from oracle import fm_ref as R
from problems import f32


# ------------------------------------------------------------------------------------- builders
def make_runs(seed, run_lengths, F, k, *, n_rows=None, ids=None, big=(), big_x=6.0, big_y=10.0):
    """A batch whose sorted view is the runs ``run_lengths`` in id order (feature ids ``ids``,
    strictly increasing, default 0, 1, ...).  Entry j of run i, whose run starts at sorted position
    start_i, goes to row (start_i + j) mod n_rows, so a run's rows are distinct (n_rows >= the longest
    run) and rows fill evenly; the stable sort orders a run by row, so where a run wraps past the last
    row its entry at sorted position p is not the one in row p mod n_rows.  Values and labels
    as problems.make_rows: fp32-rounded, some explicit zeros and unit values, values shrunk on long
    rows, regression labels (so r = yhat - y is not tiny).  ``big``: sorted positions whose entry
    takes |x| = big_x; its row takes a label of magnitude big_y and its row's other entries
    |x| >= 1/2 (a unit value otherwise), so that the entry's own gradient is large whatever was
    drawn around it.  Returns (csr, ids, w, V) as make_problem."""
    rng = np.random.default_rng(seed)
    c = np.asarray(run_lengths, dtype=np.int64)
    assert c.ndim == 1 and len(c) > 0 and (c >= 1).all()
    N = int(c.sum())
    fid = np.arange(len(c), dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    assert fid.shape == c.shape and (np.diff(fid) > 0).all() and 0 <= fid[0] and fid[-1] < F
    if n_rows is None:
        n_rows = max(int(c.max()), -(-N // 6))
    assert n_rows >= c.max(), "a run's entries need distinct rows"
    key = np.repeat(fid, c)  # the sorted view's keys
    row = np.arange(N, dtype=np.int64) % n_rows
    order = np.lexsort((key, row))  # CSR order: by row, ids ascending within a row
    col = key[order]
    row_len = np.bincount(row, minlength=n_rows)
    row_ptr = np.concatenate([[0], np.cumsum(row_len)]).astype(np.int64)
    x = rng.normal(0.0, 1.0, size=N)
    x *= np.minimum(1.0, 4.0 / np.sqrt(np.maximum(np.repeat(row_len, row_len), 1)))
    x = f32(x)
    u = rng.random(N)
    x[u < 0.05] = 0.0  # explicit zeros stay active
    x[u > 0.7] = 1.0  # unit values travel elided
    y = f32(rng.normal(0.0, 1.0, n_rows))
    big = np.asarray(big, dtype=np.int64)
    if len(big):
        assert big.min() >= 0 and big.max() < N
        view = np.argsort(col, kind="stable")  # view[p]: the entry at sorted position p
        row_of = np.repeat(np.arange(n_rows), row_len)  # CSR order (a run that wraps past the last row is
        rows_big = np.unique(row_of[view[big]])         # sorted by row again: position p need not lie in row p mod n_rows)
        y[rows_big] = big_y * np.where(rng.random(len(rows_big)) < 0.5, -1.0, 1.0)
        in_big = np.isin(row_of, rows_big)
        x[in_big & (np.abs(x) < 0.5)] = 1.0
        x[view[big]] = big_x * np.where(rng.random(len(big)) < 0.5, -1.0, 1.0)
    csr = R.CSR(row_ptr=row_ptr, col=col.astype(np.int32), val=x.astype(np.float64), label=y)
    ids_all = np.arange(F, dtype=np.int32)
    w = f32(rng.normal(0.0, 0.1, F))
    V = f32(rng.normal(0.0, 0.1, (F, k)))
    return csr, ids_all, w, V


def rows_of_view(run_lengths, n_rows):
    """The row of the entry at each sorted position of make_runs' batch (the stable sort orders a run's
    entries by row)."""
    c = np.asarray(run_lengths, dtype=np.int64)
    rid = np.repeat(np.arange(len(c)), c)
    row = np.arange(int(c.sum()), dtype=np.int64) % n_rows
    return row[np.lexsort((row, rid))]


def sorted_view(csr):
    """(order, keys): the entries stably sorted by id, as the step's sort leaves them."""
    order = np.argsort(csr.col, kind="stable")
    return order, csr.col[order].astype(np.int64)


def layout(N, spans, fill=1):
    """Run lengths, summing to N, that put a run at each of the absolute sorted positions
    ``spans`` = [(first, last), ...] (inclusive, ascending, disjoint) and fill every gap with runs
    of ``fill`` entries; a gap that is no multiple of ``fill`` ends in one longer run (a run of 3 in
    an odd gap at fill = 2), and a gap shorter than ``fill`` is one run (refused where that would be
    a run of 1 at fill >= 2: a singleton does not survive the fused step's compaction)."""
    out = []

    def gap(n):
        if n <= 0:
            assert n == 0, "spans overlap or run past N"
            return
        q = max(n // fill, 1)
        last = n - (q - 1) * fill
        assert fill == 1 or last >= 2, f"a gap of {n} cannot be filled with runs of {fill} or more"
        out.extend([fill] * (q - 1) + [last])

    at = 0
    for first, last in spans:
        assert first <= last
        gap(first - at)
        out.append(last - first + 1)
        at = last + 1
    gap(N - at)
    return np.asarray(out, dtype=np.int64)


def sprinkle(run_lengths, every=3, lead=1):
    """The full view of a fused batch: ``run_lengths`` (the compacted view: every run 2 or more) with
    a singleton run put before every ``every``-th run and ``lead`` at the front.  Returns (lengths of
    the full view, the index in it of each run of the compacted view)."""
    c = np.asarray(run_lengths, dtype=np.int64)
    assert (c >= 2).all()
    out, idx = [1] * lead, []
    for i, n in enumerate(c):
        if i and i % every == 0:
            out.append(1)
        idx.append(len(out))
        out.append(int(n))
    return np.asarray(out, dtype=np.int64), np.asarray(idx, dtype=np.int64)


def compact(keys):
    """(keys, positions) of the entries the fused step's split keeps: the runs of two or more."""
    keys = np.asarray(keys)
    n = len(keys)
    prev = np.zeros(n, dtype=bool)
    prev[1:] = keys[1:] == keys[:-1]
    nxt = np.zeros(n, dtype=bool)
    nxt[:-1] = prev[1:]
    pos = np.nonzero(prev | nxt)[0]
    return keys[pos], pos


# ------------------------------------------------------------------------------------- classify
def _runs(keys):
    keys = np.asarray(keys, dtype=np.int64)
    n = len(keys)
    st = np.ones(n, dtype=bool)
    st[1:] = keys[1:] != keys[:-1]
    first_of = np.nonzero(st)[0]
    last_of = np.concatenate([first_of[1:] - 1, [n - 1]]) if n else first_of
    rid = np.cumsum(st) - 1
    end = np.zeros(n, dtype=bool)
    end[last_of] = True
    return st, end, first_of, last_of, rid


def classify_update(keys, geom):
    """The events of k_segment_update and k_segment_combine over the key array they consume (the
    sorted view; for a fused step the compacted one).  geom: update_probe.Geometry."""
    keys = np.asarray(keys, dtype=np.int64)
    N = len(keys)
    G, Wv, B = geom.group, geom.wave, geom.block
    NG = Wv // G
    ev = SimpleNamespace(N=N, n_runs=0, flags=set(), tail_chains=set(), head_chains=set(), pair=set(),
                         run_is_wave=[], owners_two=[], owners_long=[], nonowners_inside=[], longs=[])
    if N == 0:
        return ev
    st, end, first_of, last_of, rid = _runs(keys)
    ev.n_runs = len(first_of)
    f, l = first_of, last_of
    ln = l - f + 1
    F = ev.flags

    def flag(name, cond):
        if np.any(cond):
            F.add(name)

    same_grp, same_wave = f // G == l // G, f // Wv == l // Wv
    flag("run_fills_group", (f % G == 0) & (ln == G))
    flag("run_ends_on_group_last", (l % G == G - 1) & (ln >= 2) & (f % G != 0) & same_grp)
    flag("run_starts_on_group_first", (f % G == 0) & (ln >= 2) & (l % G != G - 1) & same_grp)
    flag("run2_astride_group", (ln == 2) & (f % G == G - 1) & same_wave)
    flag("run2_astride_wave", (ln == 2) & (f % Wv == Wv - 1) & (l % B != 0))
    flag("run2_astride_block", (ln == 2) & (f % B == B - 1))
    flag("run_ends_on_wave_last_then_new", (l % Wv == Wv - 1) & (ln >= 2) & (l + 1 < N))
    flag("run_opens_on_wave_last", (f % Wv == Wv - 1) & (ln >= 2))
    flag("all_singletons", [bool((ln == 1).all())])
    flag("last_wave_partial", [N % Wv != 0])
    flag("last_run_multi_ends_at_N", [ln[-1] >= 2])
    flag("last_entry_own_run_at_wave_start", [ln[-1] == 1 and (N - 1) % Wv == 0])
    ev.run_is_wave = sorted((f[(f % Wv == 0) & (ln == Wv)] // Wv).tolist())

    # ---- the lane groups' pieces (phase 2 -> phase 3)
    gb = np.arange(0, N, G, dtype=np.int64)  # a group's first entry (groups with a valid entry)
    gl = np.minimum(gb + G, N) - 1  # its last valid entry
    gw = gb % Wv // G  # its index in the wave
    hst = np.where(st[gb], 0, np.where(l[rid[gb]] <= gl, 2, 1))
    tail = ~end[gl] & (f[rid[gl]] >= gb)
    ev.hst = hst
    # a tail piece extends through the whole groups after it until a head piece closes (in the wave)
    t_last = l[rid[gl]]
    closes = tail & (t_last // Wv == gb // Wv)
    whole = t_last // G - gb // G - 1  # head pieces with hst == 1 passed before the closing one
    ev.tail_chains = set(zip(whole[closes].tolist(), (t_last[closes] % G != G - 1).tolist()))  # (whole, mid-group)
    flag("tail_open_at_wave_end", tail & ~closes)
    flag("tail_open_from_last_group", tail & ~closes & (gw == NG - 1))  # extend(.., NG): no iteration
    flag("tail_open_from_wave_last_entry", tail & ~closes & (gw == NG - 1) & (f[rid[gl]] == gl) & (gl % Wv == Wv - 1))
    # the wave's first piece: its run began in an earlier wave
    w0 = (gw == 0) & (hst > 0)
    h_last = l[rid[gb]]
    h_in = w0 & (h_last // Wv == gb // Wv)
    ev.head_chains = set(zip((h_last[h_in] // G - gb[h_in] // G).tolist(), (h_last[h_in] % G != G - 1).tolist()))
    flag("head_closed_in_first_group", w0 & (hst == 2))
    flag("wave_inside_run", w0 & (hst == 1) & (h_last // Wv > gb // Wv))  # every group hst == 1: extend to the last
    flag("wave_inside_run_full", w0 & (hst == 1) & (h_last // Wv > gb // Wv) & (gb + Wv <= N))
    flag("inplace_close", same_grp)

    # ---- paired row stores: runs closed in phase 2 (begun and ended in one group), per entry step
    cl = l[same_grp]
    closed_at = set(zip((cl // G).tolist(), (cl % G).tolist()))  # (global group, entry step)
    n_groups = len(gb)
    for (g, j) in closed_at:
        if g % 2 == 0:
            if g + 1 >= n_groups and (g + 1) % NG != 0:
                ev.pair.add("even_closes_partner_empty")  # the partner group lies past N
            elif (g + 1, j) in closed_at:
                ev.pair.add("both_close")
            else:
                ev.pair.add("even_closes_alone")
        elif (g - 1, j) not in closed_at:
            ev.pair.add("odd_closes_alone")

    # ---- k_segment_combine: the owner predicate per range, as the kernel evaluates it
    L = Wv
    nr = -(-N // L)
    per_wave = 64 // geom.comb_lanes  # ranges per combine wave
    for c in range(nr):
        p0 = c * L
        p1 = min(p0 + L, N)
        if p1 >= N:
            continue
        p2 = (c + 2) * L
        kl, kn, kf = keys[p1 - 1], keys[p1], keys[p0]
        kb = keys[p0 - 1 if p0 > 0 else 0]
        k2 = keys[p2 if p2 < N else N - 1]
        if kn != kl:
            continue
        if kf == kl and p0 > 0 and kb == kl:
            ev.nonowners_inside.append(c)
            continue
        r = rid[p1 - 1]
        at_p0 = bool(kf == kl)
        two = not (p2 < N and k2 == kl)
        rec = SimpleNamespace(c=c, first=int(f[r]), last=int(l[r]), tail=int(p1 - f[r]), at_p0=at_p0)
        if at_p0:
            F.add("owner_starts_on_p0_range0" if p0 == 0 else "owner_starts_on_p0_later")
        if two:
            rec.head = int(l[r] - p1 + 1)
            ev.owners_two.append(rec)
            if rec.tail == 1 and rec.head == 1:
                F.add("two_tail1_head1")
            if rec.head == L and p2 < N:
                F.add("two_head_is_whole_wave")  # ends on the next range's last entry: k2 starts a new key
        else:
            # the end search: ballots over 64 ranges at a time from c + 1
            cend, rounds = c + 1, []
            while True:
                cont = [(cc < nr and keys[cc * L] == kl) for cc in range(cend, cend + 64)]
                if all(cont):
                    rounds.append(64)
                    cend += 64
                    continue
                rounds.append(cont.index(False))
                cend += rounds[-1]
                break
            rec.follow, rec.rounds = cend - c - 1, rounds
            ev.owners_long.append(rec)
            if rec.last == p2:
                F.add("long_ends_on_first_of_c2")
    by_wave = {}
    for rec in ev.owners_long:
        by_wave.setdefault(rec.c // per_wave, []).append(rec.c)
    flag("two_longs_in_one_combine_wave", [any(len(v) >= 2 for v in by_wave.values())])
    return ev


def classify_split(keys, geom):
    """The events of k_split_count / _scatter over the full sorted view: per chunk (nm, ns), and
    whether the key before / after the chunk alone decides its first / last entry to be multi."""
    keys = np.asarray(keys, dtype=np.int64)
    N, C = len(keys), geom.chunk
    prev = np.zeros(N, dtype=bool)
    prev[1:] = keys[1:] == keys[:-1]
    nxt = np.zeros(N, dtype=bool)
    nxt[:-1] = prev[1:]
    multi = prev | nxt
    nch = -(-N // C)
    pad = np.zeros(nch * C, dtype=np.int64)
    pad[:N] = multi
    nm = pad.reshape(nch, C).sum(axis=1)
    size = np.minimum(C, N - C * np.arange(nch))
    b = C * np.arange(1, nch)  # first entries of chunks 1..
    before = np.zeros(nch, dtype=bool)
    before[1:] = prev[b] & ~nxt[b]
    e = C * np.arange(1, nch) - 1  # last entries of chunks 0..nch-2
    after = np.zeros(nch, dtype=bool)
    after[:-1] = nxt[e] & ~prev[e]
    return SimpleNamespace(N=N, nchunks=nch, nm=nm, ns=size - nm, before=before, after=after, size=size,
                           n_multi=int(multi.sum()), n_single=int(N - multi.sum()),
                           rounds=-(-nch // geom.round_chunks), multi=multi)


def classify(keys, geom, fused=False):
    """Events of a step over the sorted view ``keys``: .split (the full view, fused steps only) and
    .update (the view the segmented update consumes: ``keys`` without its runs of 1 when fused)."""
    keys = np.asarray(keys, dtype=np.int64)
    seen = compact(keys)[0] if fused else keys
    return SimpleNamespace(update=classify_update(seen, geom), split=classify_split(keys, geom) if fused else None,
                           consumed=seen)


# ------------------------------------------------------------------------------------- sensitivity
def entry_update_sizes(model, csr, t, step_size):
    """Per entry of csr (CSR order), what that entry alone moves its row by in the oracle's step from
    ``model``: (eta / m) max_f |g_V,e[f]| and (eta / m) |g_w,e| (SGD.scala:145-154)."""
    import math

    m = csr.n_rows
    eta = step_size / math.sqrt(t)
    pred, _, dw, dv = _loss_grad_fast(model, csr)
    rows = np.repeat(np.arange(m), np.diff(csr.row_ptr))
    r = pred - csr.label[rows]
    g_v = np.abs(dv * r[:, None]).max(axis=1)
    g_w = np.abs(dw * pred - csr.label[rows])
    return g_v * eta / m, g_w * eta / m


def _loss_grad_fast(model, csr):
    """R.loss_grad's columns with numpy reductions (the same arithmetic per entry)."""
    m = csr.n_rows
    rows = np.repeat(np.arange(m), np.diff(csr.row_ptr))
    i = csr.col.astype(np.int64)
    x = csr.val
    vfxi = model.V[i] * x[:, None]
    S = np.zeros((m, model.k))
    np.add.at(S, rows, vfxi)
    ws = np.zeros(m)
    np.add.at(ws, rows, model.w[i] * x)
    vv = np.zeros(m)
    np.add.at(vv, rows, np.sum(model.V[i] ** 2, axis=1) * x * x)
    yhat = 0.5 * (np.sum(S * S, axis=1) - vv) + ws + model.w0
    pred = yhat[rows]
    d = pred - csr.label[rows]
    return pred, d * d, x.copy(), S[rows] * x[:, None] - vfxi * x[:, None]
