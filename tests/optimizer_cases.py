"""A structural model of the two optimizer update stages (fm_ftrl.hip, fm_adagrad.hip) and the named cases of
tests/test_gpu_optimizer_edges.py: to those stages what runs.classify is to k_segment_update -- their control
flow, never their arithmetic.  NumPy only; tests/test_optimizer_cases_cpu.py checks all of it without a GPU.

ftrl_events / ada_events say, per run of the sorted view, where the run is applied, from how many pieces it
is summed and which global slots its partials pass through.  The cases are written in the stages' own units
(W, stretch, L: the seams fm_seam_ftrl_window, fm_seam_ftrl_stretch, fm_seam_adagrad_piece), placed with
runs.layout by absolute sorted position, and each asserts through the model that it holds the event it is named
for.  build() turns a case into the three-step protocol of the GPU test: the case's batch, the same layout
behind a lead of 7 entries, the case's batch again -- so every designated row is updated with live state on its
second and third touch -- with a large entry (make_runs' big) in every piece of every designated run.
"""

from __future__ import annotations

import copy
import functools
from types import SimpleNamespace

import numpy as np

import adagrad_ref as A
import ftrl_ref as Fr
import runs
from oracle import fm_ref as R
from problems import f32

FACTOR = 8.0  # an omitted piece must move its run's row by more than this many budgets (repeat_cases.FACTOR)
LEAD = 7  # the second batch's layout is the first's behind a run of this many entries
BIG_X, BIG_Y = 4.0, 10.0  # make_runs' big entries
# Every batch is padded with empty rows to M_MIN rows.  The references' budgets follow a row's own roundings through
# a step, not another row's through the next forward; that holds while a step's gain on such a deviation stays under
# 1.  For FTRL the gain is about (1 / den) x x' |r| / m with 1 / den up to alpha / beta = 100, so a batch of a few dozen
# rows with |x| = 4 beside labels of 10 multiplies a rounding tenfold per step (conditioning() measured 52 budgets
# after three steps at m = 45) and one of M_MIN rows does not.  m cannot grow at will: an absent row leaves 0 only
# once its |sum g| / m exceeds lambda1, and until then an omitted piece would not show.
M_MIN = 2048
ROW_LEN = 6  # entries per row of a case's batches
OWNERS = 48  # the fan-out cases: owners of a fold beyond the second block of 16 lane groups


def _bounds(keys):
    keys = np.asarray(keys, dtype=np.int64)
    if len(keys) == 0:
        return keys, keys
    _, _, first, last, _ = runs._runs(keys)
    return first, last


# ------------------------------------------------------------------------------------- the model
def ftrl_events(keys, W, stretch):
    """Where k_ftrl_window / k_ftrl_fold apply each run of the sorted view ``keys`` (windows of W entries,
    lane-group stretches of ``stretch`` entries, W a multiple of stretch).  For a run [first, last]:

    site (line numbers of fm_ftrl.hip):
      "stretch"  first and last lie in one stretch: the walk sees the run's head and its end and applies the
                 row there (336-338: kFEnd with ``started``).
      "close"    stretch boundaries cut the run and first and last lie in one window: the group holding the
                 last entry has a closed head piece of a run that began inside the window (360: head_row =
                 hst == 2 && head_key != lead_key) and folds the LDS pieces in stretch order (376-383).
      "fold"     last lies in a later window than first: window first // W owns the run (448-452) and
                 k_ftrl_fold adds the partials in window order (459-467).
    pieces     the stretch pieces the run is summed from, per window it touches (one walk accumulator each:
               297-298, reset at 345-347); their total is ``n_pieces``.
    slots      "fold" runs only: the global slot of each window partial, in the order the fold adds them.  The
               window the run begins in writes its open tail to 2 w + 1 (384 with g0 >= 0, or 387 where the tail
               begins in the last stretch); every later window writes its leading or whole-window piece to 2 w
               (384 with g0 == -1), and the fold reads 2 w + 1 (459) and then 2 w' (464).
    Returns SimpleNamespace(first, last, site, pieces, n_pieces, slots, owners, n_windows): arrays / lists
    indexed by run; owners are the windows whose lane group does fold work."""
    assert W % stretch == 0 and stretch >= 1
    first, last = _bounds(keys)
    N = len(np.asarray(keys))
    site, pieces, slots, owners = [], [], [], []
    for f, l in zip(first.tolist(), last.tolist()):
        w0, w1 = f // W, l // W
        per = []
        for w in range(w0, w1 + 1):
            lo, hi = max(f, w * W), min(l, w * W + W - 1)
            per.append(hi // stretch - lo // stretch + 1)
        pieces.append(per)
        if w0 != w1:
            site.append("fold")
            slots.append([2 * w0 + 1] + [2 * w for w in range(w0 + 1, w1 + 1)])
            owners.append(w0)
        else:
            site.append("stretch" if f // stretch == l // stretch else "close")
            slots.append([])
    return SimpleNamespace(first=first, last=last, site=np.asarray(site, dtype=object), pieces=pieces,
                           n_pieces=np.asarray([sum(p) for p in pieces], dtype=np.int64), slots=slots,
                           owners=sorted(owners), n_windows=-(-N // W), N=N)


def ftrl_events_brute(keys, W, stretch):
    """ftrl_events restated entry by entry: one walk over the view that tracks the stretch and the window of
    every entry, as the kernel's waves and lane groups meet them."""
    keys = np.asarray(keys, dtype=np.int64)
    out = []
    cur = None
    for p, key in enumerate(keys.tolist()):
        s, w = p // stretch, p // W
        if cur is None or cur["key"] != key:
            cur = dict(key=key, first=p, stretches=[s], windows=[w], per={w: 1}, began=w)
            out.append(cur)
        else:
            if w != cur["windows"][-1]:
                cur["windows"].append(w)
                cur["per"][w] = 0
            if s != cur["stretches"][-1]:
                cur["stretches"].append(s)
                cur["per"][w] += 1
        cur["last"] = p
    res = []
    for r in out:
        if len(r["windows"]) > 1:
            site = "fold"
            slots = [2 * w + 1 if w == r["began"] else 2 * w for w in r["windows"]]
        else:
            site, slots = ("stretch" if len(r["stretches"]) == 1 else "close"), []
        res.append((r["first"], r["last"], site, [r["per"][w] for w in r["windows"]], slots))
    return res


def ada_events(keys, L):
    """Where k_ada_piece / k_ada_fold apply each run (fm_adagrad.hip).  A run is cut into pieces of L entries
    counted from its first entry (k_ada_flag, 102); a run of one piece is applied by k_ada_piece ("piece":
    209, 262-263), a longer one is listed hot (103) and applied by k_ada_fold ("fold": 333-375) from the
    partials its pieces left in slot 2 (piece's first entry // L) + (the piece heads the run) (186, 265).
    Returns SimpleNamespace(first, last, site, n_pieces, slots, hot): slots per run in piece order."""
    first, last = _bounds(keys)
    n = (last - first) // L + 1
    site = np.where(n == 1, "piece", "fold").astype(object)
    slots = [[2 * ((f + m * L) // L) + (m == 0) for m in range(c)] if c > 1 else []
             for f, c in zip(first.tolist(), n.tolist())]
    return SimpleNamespace(first=first, last=last, site=site, n_pieces=n.astype(np.int64), slots=slots,
                           hot=first[n > 1], N=len(np.asarray(keys)))


def ada_events_brute(keys, L):
    keys = np.asarray(keys, dtype=np.int64)
    res, cur = [], None
    for p, key in enumerate(keys.tolist()):
        if cur is None or cur[0] != key:
            cur = [key, p, p, [p]]  # key, first, last, the pieces' first entries
            res.append(cur)
        else:
            if p - cur[3][-1] == L:
                cur[3].append(p)
            cur[2] = p
    out = []
    for key, f, l, heads in res:
        many = len(heads) > 1
        out.append((f, l, "fold" if many else "piece", len(heads),
                    [2 * (h // L) + (1 if h == f else 0) for h in heads] if many else []))
    return out


# ------------------------------------------------------------------------------------- the cases
# A case: SimpleNamespace(N, spans, des, holds) -- the view's length, the placed runs, which of them the case is
# about (indices into spans) and holds(ev, runs_of): asserts the named event on the events of the view, runs_of
# mapping a span to its run index.
def _case(N, spans, holds, des=None):
    return SimpleNamespace(N=N, spans=spans, des=list(range(len(spans))) if des is None else des, holds=holds)


def ftrl_cases(W, g):
    """The named FTRL cases for windows of W and stretches of g entries."""
    assert W % g == 0 and W // g >= 4 and g >= 12
    c = {}

    def ends(ev, ix):
        a, b = ix
        assert ev.last[a] % g == g - 1 and ev.last[a] % W != W - 1 and ev.site[a] == "close"
        assert ev.last[b] % W == W - 1 and ev.site[b] == "close" and ev.first[b + 1] % W == 0

    c["ends-on-stretch-and-window-last"] = _case(W + 9, [(g - 3, 2 * g - 1), (W - g - 2, W - 1)], ends)

    def opens(ev, ix):
        (a,) = ix
        assert ev.first[a] % W == W - 1 and ev.site[a] == "fold" and ev.pieces[a][0] == 1
        assert ev.slots[a] == [2 * (ev.first[a] // W) + 1, 2 * (ev.first[a] // W) + 2]

    c["opens-on-window-last"] = _case(W + 2 * g, [(W - 1, W + g + 2)], opens)

    def closes_first(ev, ix):
        (a,) = ix
        assert ev.last[a] % W == 0 and ev.first[a] < ev.last[a] and ev.site[a] == "fold" and ev.pieces[a][-1] == 1

    c["ends-on-window-first"] = _case(W + g, [(W - g - 3, W)], closes_first)

    def whole(ev, ix):
        (a,) = ix
        w0, w1 = ev.first[a] // W, ev.last[a] // W
        assert w1 - w0 == 2 and ev.site[a] == "fold" and ev.pieces[a][1] == W // g
        assert ev.slots[a] == [2 * w0 + 1, 2 * w0 + 2, 2 * w0 + 4]

    c["covers-one-whole-window"] = _case(3 * W + 5, [(W - g - 1, 2 * W + g + 1)], whole)

    def block(ev, ix):
        _, a = ix
        assert ev.first[a] < 4 * W <= ev.last[a] and ev.first[a] // W == 3 and ev.slots[a] == [7, 8]

    c["crosses-the-block-of-four-windows"] = _case(4 * W + 2 * g, [(2 * g + 1, 2 * g + 4), (4 * W - g - 2, 4 * W + g)], block,
                                                   des=[1])

    def exactly_w(ev, ix):
        assert ev.N == W and ev.n_windows == 1 and ev.last[ix[-1]] == W - 1 and "fold" not in set(ev.site)
        assert {ev.site[i] for i in ix} == {"stretch", "close"}

    c["view-of-W"] = _case(W, [(3, 5), (W - 2 * g - 1, W - 1)], exactly_w)

    def two_w(ev, ix):
        (a,) = ix
        assert ev.N == 2 * W and ev.first[a] < W <= ev.last[a] and ev.slots[a] == [1, 2]

    c["view-of-2W"] = _case(2 * W, [(W - 2 * g, W + 2 * g)], two_w)

    def w_plus_1(ev, ix):
        (a,) = ix
        assert ev.N == W + 1 and ev.last[a] == W and ev.first[a] < W and ev.pieces[a] == [2, 1]

    c["view-of-W+1"] = _case(W + 1, [(W - g - 2, W)], w_plus_1)

    def short(ev, ix):
        assert ev.N < g and set(ev.site) == {"stretch"} and ev.last[ix[-1]] == ev.N - 1

    c["view-under-one-stretch"] = _case(g - 3, [(1, 3), (g - 6, g - 4)], short)

    def one(ev, ix):
        assert ev.N == 1 and list(ev.site) == ["stretch"]

    c["view-of-one-entry"] = _case(1, [(0, 0)], one)

    def partial(ev, ix):
        (a,) = ix
        assert ev.N % W != 0 and ev.last[a] == ev.N - 1 and ev.site[a] == "fold" and ev.pieces[a][-1] >= 2

    c["open-to-a-partial-window's-last"] = _case(W + g + 5, [(W - 2, W + g + 4)], partial)

    def owners(ev, ix):
        assert ev.N == OWNERS * W + LEAD and ev.owners == list(range(OWNERS))
        for j, a in enumerate(ix):
            assert ev.slots[a] == [2 * j + 1, 2 * j + 2] and ev.last[a] - ev.first[a] + 1 == W

    c["48-owning-windows"] = _case(OWNERS * W + LEAD, [(LEAD + j * W, LEAD + (j + 1) * W - 1) for j in range(OWNERS)], owners,
                                   des=[0, 15, 16, OWNERS - 1])
    # (every second case runs with its designated rows absent; a lone entry's absent row has a V gradient of exactly
    # 0 and a w gradient under lambda1, so the one-entry view takes an even place)
    order = [n for n in c if n not in ("view-of-one-entry", "open-to-a-partial-window's-last")]
    order[9:9] = ["open-to-a-partial-window's-last", "view-of-one-entry"]
    return {n: c[n] for n in order}


def ada_cases(L):
    """The named AdaGrad cases for pieces of L entries."""
    c = {}

    def lengths(ev, ix):
        a, b, d = ix
        assert [int(ev.last[i] - ev.first[i] + 1) for i in ix] == [L, L + 1, 2 * L]
        assert (ev.site[a], ev.n_pieces[a]) == ("piece", 1) and ev.n_pieces[b] == 2 and ev.n_pieces[d] == 2
        assert ev.site[b] == ev.site[d] == "fold"

    c["runs-of-L-L+1-2L"] = _case(4 * L + 30, [(3, L + 2), (L + 9, 2 * L + 9), (2 * L + 15, 4 * L + 14)], lengths)

    def share(ev, ix):
        a, b = ix
        assert ev.slots[a][-1] + 1 == ev.slots[b][0] and ev.slots[a][-1] % 2 == 0 and ev.n_pieces[b] >= 2

    c["two-slots-of-one-window"] = _case(3 * L, [(5, L + 14), (L + 15, 2 * L + 15)], share)

    def at_end(ev, ix):
        (a,) = ix
        assert ev.last[a] == ev.N - 1 and ev.n_pieces[a] == 3 and (ev.last[a] - ev.first[a] + 1) % L != 0

    c["multi-piece-run-ends-the-view"] = _case(2 * L + 40, [(20, 2 * L + 39)], at_end)

    def owners(ev, ix):
        assert len(ev.hot) == OWNERS and all(ev.n_pieces[a] == 2 for a in ix) and ev.N // L >= OWNERS

    c["48-runs-of-L+1"] = _case(OWNERS * (L + 1), [(j * (L + 1), (j + 1) * (L + 1) - 1) for j in range(OWNERS)], owners,
                                des=[0, 15, 16, OWNERS - 1])

    def one(ev, ix):
        assert ev.N == 1 and list(ev.site) == ["piece"]

    c["view-of-one-entry"] = _case(1, [(0, 0)], one)
    # (the table's order decides which cases run with their designated rows absent: every second one, and those
    # must hold both apply sites)
    order = ["two-slots-of-one-window", "runs-of-L-L+1-2L", "multi-piece-run-ends-the-view", "48-runs-of-L+1", "view-of-one-entry"]
    return {n: c[n] for n in order}


def case_events(opt, case, geom):
    """The events of the case's own batch under geom = (W, stretch) or (L,), and the run index of each span."""
    lengths = runs.layout(case.N, case.spans, 1)
    starts = np.concatenate([[0], np.cumsum(lengths)])[:-1]
    at = {int(s): i for i, s in enumerate(starts)}
    ix = [at[a] for a, _ in case.spans]
    keys = np.repeat(np.arange(len(lengths)), lengths)
    ev = ftrl_events(keys, *geom) if opt == "ftrl" else ada_events(keys, *geom)
    return ev, ix, lengths


def assert_holds(opt, case, geom):
    ev, ix, _ = case_events(opt, case, geom)
    case.holds(ev, ix)
    return ev, ix


def designated(opt, case, geom):
    """The runs a case is about (indices into its view's runs)."""
    _, ix, _ = case_events(opt, case, geom)
    return [ix[j] for j in case.des]


def piece_positions(opt, f, l, geom):
    """The sorted positions [(lo, hi)] of the pieces a run [f, l] is summed from: FTRL's stretch pieces (a window
    edge is a stretch edge), AdaGrad's pieces of L from the run's first entry."""
    if opt == "ftrl":
        g = geom[1]
        cuts = [f] + list(range((f // g + 1) * g, l + 1, g))
    else:
        cuts = list(range(f, l + 1, geom[0]))
    return [(a, min(b - 1, l)) for a, b in zip(cuts, cuts[1:] + [l + 1])]


def window_partials(f, l, W):
    """The positions of the window partials of an FTRL "fold" run."""
    return [(max(f, w * W), min(l, w * W + W - 1)) for w in range(f // W, l // W + 1)]


# ------------------------------------------------------------------------------------- the three-step protocol
def _batch(seed, lengths, des, opt, geom, F, k, lead):
    starts = np.concatenate([[0], np.cumsum(lengths)])
    big = []
    for i in des:
        f, l = int(starts[i]), int(starts[i + 1]) - 1
        for a, b in piece_positions(opt, f + lead, l + lead, geom):  # where the pieces fall in THIS batch's view
            big.append((a + b) // 2)
    n = len(lengths)
    if lead:
        lengths, ids = np.concatenate([[lead], lengths]), np.arange(0, n + 1)
    else:
        ids = np.arange(1, n + 1)
    n_rows = max(int(np.max(lengths)), -(-int(np.sum(lengths)) // ROW_LEN))
    csr, ids, w, V = runs.make_runs(seed, lengths, F, k, ids=ids, n_rows=n_rows, big=sorted(set(big)), big_x=BIG_X, big_y=BIG_Y)
    pad = max(M_MIN - csr.n_rows, 0)  # empty rows behind the batch: they count in m and touch nothing
    ptr = np.concatenate([csr.row_ptr, np.full(pad, csr.row_ptr[-1], dtype=np.int64)])
    label = np.concatenate([csr.label, f32(np.random.default_rng(seed).normal(0.0, 1.0, pad))])
    return R.CSR(row_ptr=ptr, col=csr.col, val=csr.val, label=label), ids, w, V


SEEDS = 24  # draws tried, in order, for one that meets the separation (as update_cases.SEEDS)


@functools.lru_cache(maxsize=None)
def build(opt, name, k, geom, absent=False):
    """build_once for the first of SEEDS draws in which omitting any one piece of a designated run moves its row
    by more than FACTOR budgets (the last draw where none does: the CPU test then fails)."""
    for seed in range(SEEDS):
        c = build_once(opt, name, k, geom, absent, 100 * seed)
        c.margin, c.draw = separation(c, floor=FACTOR), seed
        if c.margin > FACTOR:
            break
    return c


def build_once(opt, name, k, geom, absent=False, seed=0):
    """The case ``name`` at k factors: three batches (run i of the case's view is feature i + 1 in all of them;
    feature 0 is the second batch's lead), the tables, which ids are loaded (``absent``: not the designated
    ones) and the events of the first and the shifted batch."""
    case = (ftrl_cases(*geom) if opt == "ftrl" else ada_cases(*geom))[name]
    ev, ix = assert_holds(opt, case, geom)
    _, _, lengths = case_events(opt, case, geom)
    des = [ix[j] for j in case.des]
    F = len(lengths) + 2
    seed0 = 9000 + 31 * k + 7 * sum(map(ord, name)) % 1000 + seed
    first, ids, w, V = _batch(seed0, lengths, des, opt, geom, F, k, 0)
    shifted = _batch(seed0 + 1, lengths, des, opt, geom, F, k, LEAD)[0]
    des_ids = np.asarray(des, dtype=np.int64) + 1
    keep = np.setdiff1d(ids, des_ids).astype(np.int32) if absent else ids
    _, keys2 = runs.sorted_view(shifted)
    ev2 = ftrl_events(keys2, *geom) if opt == "ftrl" else ada_events(keys2, *geom)
    _, keys1 = runs.sorted_view(first)
    np.testing.assert_array_equal(keys1, np.repeat(np.arange(1, len(lengths) + 1), lengths))
    return SimpleNamespace(opt=opt, name=name, k=k, geom=geom, case=case, F=F, w=w, V=V, keep=keep, absent=absent,
                           batches=[first, shifted, first], des=des, des_ids=des_ids, events=ev, events_shifted=ev2,
                           lengths=lengths)


def new_ref(opt, c, **kw):
    model = R.Model.empty(c.F, c.k)
    model.load(c.keep, c.w[c.keep], c.V[c.keep])
    return A.AdaRef(model, A.G0) if opt == "adagrad" else Fr.FtrlRef(model, **kw)


def consts(opt):
    return A if opt == "adagrad" else Fr


def reference(c):
    """The case's three steps on the fp64 reference: (ref, [StepResult], the reference before the third step)."""
    mod = consts(c.opt)
    ref, outs, before = new_ref(c.opt, c), [], None
    for t, b in enumerate(c.batches, start=1):
        if t == len(c.batches):
            before = copy.deepcopy(ref)
        outs.append(ref.step(b, t, mod.STEP, mod.REG))
    return ref, outs, before


def without(csr, key, lo, hi):
    """The batch restricted to the rows that hold an entry of feature ``key`` (the others emptied: the row of
    ``key`` hangs on no other row, and the batch size stays), less the entries at sorted positions lo .. hi."""
    order, _ = runs.sorted_view(csr)
    rows = np.repeat(np.arange(csr.n_rows), np.diff(csr.row_ptr))
    keep = np.isin(rows, rows[csr.col == key])
    keep[order[lo:hi + 1]] = False
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=csr.n_rows))]).astype(np.int64)
    return R.CSR(row_ptr=ptr, col=csr.col[keep], val=csr.val[keep], label=csr.label)


def separation(c, floor=None):
    """min over the designated runs and over every piece (and, for FTRL fold runs, every window partial) of the
    largest move of the run's w or of a column of its V, in budgets, when the third step omits that piece.  With
    ``floor`` the search ends at the first piece that moves its row by no more than that (the draw has failed)."""
    mod = consts(c.opt)
    ref, _, before = reference(c)
    bw, bV = ref.budget()
    csr, worst = c.batches[-1], np.inf
    starts = np.concatenate([[0], np.cumsum(c.lengths)])
    for i in c.des:
        f, l, key = int(starts[i]), int(starts[i + 1]) - 1, i + 1
        parts = piece_positions(c.opt, f, l, c.geom)
        if c.opt == "ftrl" and c.events.site[i] == "fold":
            parts = parts + window_partials(f, l, c.geom[0])
        for lo, hi in sorted(set(parts)):
            other = copy.deepcopy(before)
            other.step(without(csr, key, lo, hi), len(c.batches), mod.STEP, mod.REG)
            move = max(abs(other.model.w[key] - ref.model.w[key]) / bw[key],
                       np.max(np.abs(other.model.V[key] - ref.model.V[key]) / bV[key]))
            worst = min(worst, float(move))
            if floor is not None and worst <= floor:
                return worst
    return worst


def conditioning(c, seed=1):
    """The largest move of the final table, in budgets, when every stored value is disturbed by one fp32 rounding
    (a factor 1 +- 2^-24) before every step: what the comparison cannot tell from the device's own storage, and so
    must stay well under 1 for the budget to be a fair bound of a correct kernel (M_MIN above)."""
    mod = consts(c.opt)
    ref, _, _ = reference(c)
    other = new_ref(c.opt, c)
    rng = np.random.default_rng(seed)
    for t, b in enumerate(c.batches, start=1):
        m = other.model
        m.w *= 1.0 + 2.0 ** -24 * rng.choice([-1.0, 1.0], m.w.shape)
        m.V *= 1.0 + 2.0 ** -24 * rng.choice([-1.0, 1.0], m.V.shape)
        other.step(b, t, mod.STEP, mod.REG)
    bw, bV = ref.budget()
    return float(max(np.max(np.abs(other.model.w - ref.model.w) / bw), np.max(np.abs(other.model.V - ref.model.V) / bV)))


# ------------------------------------------------------------------------------------- repeated ids
def repeat_reference(opt, c):
    """A repeat_cases case on the optimizer's reference at its own STEP and REG: (ref after both batches,
    [StepResult], the reference before the second batch)."""
    mod = consts(opt)
    model = R.Model.empty(c.F, c.k)
    model.load(c.keep, c.w[c.keep], c.V[c.keep])
    ref = A.AdaRef(model, A.G0) if opt == "adagrad" else Fr.FtrlRef(model)
    o1 = ref.step(c.batches[0], 1, mod.STEP, mod.REG)
    before = copy.deepcopy(ref)
    return ref, [o1, ref.step(c.batches[1], 2, mod.STEP, mod.REG)], before
