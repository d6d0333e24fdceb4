"""GPU: k_forward where a team walks several samples, in every mode and team shape.

k_forward (fm_spark_amd/csrc/fm_forward.hip) strides its grid over the samples, and the fused mode
carries state from one sample of a team to the next (SingletonStash::pend, neighbour_pend(), the
paired header stores flushed during the next sample from two call sites).  At the tuned grid a team
takes a second sample only beyond tens of thousands of rows (millions of pairs for the partial pass's
one-lane teams), so these tests cap the grid through the forward probe (tests/forward_probe.py) at 1
block and at 3 (a team count that is no power of two; the partial pass at 3 for one case per GS), and run batches of a few hundred
rows whose lengths are laid out round by round: every team's successive samples go long -> empty,
empty -> empty, long -> odd-short, odd-short -> long, and end on a long one, with a last round that is
partly filled.  That layout is checked on the CPU from the expected geometry before anything is
launched (test_layouts_meet_their_transitions runs the same check without a GPU), and the launch log
then confirms the geometry: sample s of a launch goes to team s mod (blocks * 256 / TEAM).

Every case runs the same call on fresh contexts at the default grid and under the cap, and asserts
(a) the capped launches ran with blocks == cap and every team took at least 3 samples, (b) the log
shows the (mode, GS, TEAM, U) the case names, (c) the capped results are bit for bit the default's --
none of them depends on which team computes a sample -- with the counts exact and loss_sum within
rows * 2^-52 relative (its non-negative terms are added in another order), and (d) the default run
matches the fp64 oracle at test_gpu_parity's tolerances (the three-rank paths with test_gpu_fuzz's
4-ulp floor).  With no cap set the log stays empty.

The fused cases add the stash's edges: samples of NS RPP - 1, NS RPP, NS RPP + 1 and 2 NS RPP + 3
entries (NS = kFuseNS, read from the probe), each all singletons, all multi and interleaved (so the
re-walk's `seen` counter skips multi entries and the stashed singletons), each followed on its team by
an empty and by an odd-short sample, three steps under an L1 of 1e-2 that shows a double shrink or a
lost header.
"""

import math
from contextlib import nullcontext

import numpy as np
import pytest

from oracle import fm_ref as R
from problems import make_rows
from test_gpu_parity import ATOL, RTOL, _gauss_draw, assert_tables, to_host

gpu_test = pytest.mark.gpu

BLOCK = 256  # threads per forward block (checked against the probe's value by every GPU case)
L_RANKS = 3  # ranks of the sharded contexts


# ------------------------------------------------------------------------------------------ layouts
def odd_shorts(RPP):
    """Two odd lengths below RPP (one lane group of a neighbour pair gets an entry, the other none);
    1 where a pass holds one or two entries."""
    odd = list(range(1, RPP, 2)) or [1]
    return odd[len(odd) // 2], odd[-1]


def general_rounds(RPP, U, empty=True):
    """One length per round (every team gets a sample of that length in that round): the edge set 0, 1,
    odd below RPP, RPP - 1, RPP, RPP + 1, U RPP - 1, U RPP, U RPP + 1, 2 U RPP + 1, ordered for the
    transitions.  empty = False (the partial pass: a pair has at least one entry): 1 in place of 0."""
    E = 0 if empty else 1
    L1, L2 = U * RPP + 1, 2 * U * RPP + 1
    oa, ob = odd_shorts(RPP)
    return [L2, E, E, L1, oa, L2, 1, ob, max(RPP - 1, E), RPP, RPP + 1, U * RPP - 1, U * RPP, L1, E, oa, L1]


def lay_out(rounds, nteams):
    """The rounds' lengths sample by sample, then a last round of long samples that is partly filled."""
    rem = max(1, nteams // 2 - 1)  # (two or three such layouts in a row leave a partly filled round too)
    return np.concatenate([np.repeat(np.asarray(rounds, dtype=np.int64), nteams),
                           np.full(rem, max(rounds), dtype=np.int64)])


def check_walk(seq, nteams, RPP, U, empty=True, what=""):
    """Every team of a launch over samples of lengths `seq` takes at least 3 samples, the last of them
    long, with the transitions long -> odd-short, odd-short -> long and (empty) long -> empty, empty ->
    empty among its successive samples; the last round is partly filled."""
    seq = np.asarray(seq)
    assert len(seq) >= 3 * nteams and len(seq) % nteams != 0, (what, len(seq), nteams)
    long_ = seq >= U * RPP + 1
    none = seq == 0
    odd = (seq % 2 == 1) & (seq < max(RPP, 2))
    for t in range(nteams):
        lg, em, od = long_[t::nteams], none[t::nteams], odd[t::nteams]
        assert len(lg) >= 3 and lg[-1], (what, t)
        assert (lg[:-1] & od[1:]).any() and (od[:-1] & lg[1:]).any(), (what, t)
        if empty:
            assert (lg[:-1] & em[1:]).any() and (em[:-1] & em[1:]).any(), (what, t)


def nteams_of(cap, TEAM):
    return cap * BLOCK // TEAM


# ------------------------------------------------------------------------------------ the probe
@pytest.fixture
def door(gpu):
    """The forward probe with the tuned grid and an empty log, before and after; a missing probe
    fails here (run build())."""
    import forward_probe as fp

    fp.load()
    fp.set_grid_cap(0)
    fp.clear_log()
    try:
        assert fp.consts().block == BLOCK
        yield fp
    finally:
        fp.set_grid_cap(0)


def capped(fp, cap, run):
    """run() under the cap (0: the tuned grid, where the log must stay empty) -> (result, log)."""
    fp.clear_log()
    with fp.grid_cap(cap) if cap else nullcontext():
        out = run()
        log = fp.read_log()
    if not cap:
        assert log == [], "launches were logged with no cap set"
    return out, log


def assert_log(fp, log, want, cap, n_launches, rows):
    """(a) and (b) for launches that all walk `rows` samples: n_launches records of the instantiation
    `want` = (mode, GS, TEAM, U), each of `cap` blocks, every team with at least 3 samples."""
    assert len(log) == n_launches, log
    for r in log:
        assert (r.mode, r.gs, r.team, r.u) == want, (r, want)
        assert (r.chunk, r.chunks) == (0, 1) and r.blocks == cap and r.rows == rows, r
        assert r.rows >= 3 * r.blocks * (BLOCK // r.team) and r.rows % (r.blocks * (BLOCK // r.team)) != 0, r


def assert_loss_close(a, b, rows):
    """loss_sum at two grids: the same non-negative fp64 terms added in another order."""
    assert abs(a - b) <= rows * 2.0 ** -52 * max(abs(a), abs(b)), (a, b)


# ----------------------------------------------------------------------------- the single-table cases
# k -> (GS, TEAM, U) of the step's forward, predict and loss-grad: every shape launch_forward serves,
# each at a quad boundary of k and just past one (k = 9 and 17: lanes with qok == false take part)
SHAPES = {1: (1, 32, 3), 4: (1, 32, 3), 5: (2, 32, 3), 8: (2, 32, 3), 9: (4, 32, 2), 12: (4, 32, 2), 16: (4, 32, 2),
          17: (8, 32, 2), 32: (8, 32, 2), 33: (16, 32, 2), 64: (16, 32, 2), 65: (32, 32, 4), 128: (32, 32, 4),
          129: (64, 64, 4), 256: (64, 64, 4)}
PLAIN_CASES = [(k, cap) for cap in (1, 3) for k in SHAPES]  # under 1 block, and under 3 (24 or 12 teams)
# the fused forward: k -> (GS, TEAM) at U = kFuseU (k = 9 and 12: kp = 12; 16: kp = 16)
FUSED_SHAPES = {1: (1, 32), 4: (1, 32), 5: (2, 32), 8: (2, 32), 9: (4, 32), 12: (4, 32), 16: (4, 32)}
FUSED_CASES = [(k, cap) for cap in (1, 3) for k in FUSED_SHAPES]
F_PLAIN = 1500


def plain_problem(k, cap, seed, F=F_PLAIN, extra=0):
    GS, TEAM, U = SHAPES[k]
    RPP, nt = TEAM // GS, nteams_of(cap, TEAM)
    lengths = lay_out(general_rounds(RPP, U), nt)
    check_walk(lengths, nt, RPP, U, what=f"k={k} cap={cap}")
    return make_rows(seed, lengths, F + extra, k)


def bits_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@gpu_test
@pytest.mark.parametrize("k,cap", PLAIN_CASES)
def test_train_teams_walk_several_samples(door, k, cap):
    """kTrain: two unfused steps from the host CSR."""
    from fm_spark_amd.engine import FMContext

    csr, ids, w, V = plain_problem(k, cap, 1000 + k)
    F = F_PLAIN

    def run():
        ctx = FMContext(F, k)
        ctx.load_tables(ids, w, V)
        outs = [ctx.step(to_host(csr), t, 0.3, 1e-4) for t in (1, 2)]
        tabs = ctx.export_tables()
        ctx.close()
        return outs, tabs

    (o0, t0), _ = capped(door, 0, run)
    (o1, t1), log = capped(door, cap, run)
    assert_log(door, log, (door.TRAIN, *SHAPES[k]), cap, 2, csr.n_rows)
    assert bits_equal(t0, t1)
    for a, b in zip(o0, o1):
        assert (a.n_rows, a.n_loss_rows, a.n_unique) == (b.n_rows, b.n_loss_rows, b.n_unique)
        assert_loss_close(a.loss_sum, b.loss_sum, csr.n_rows)
    model = R.Model.empty(F, k)
    model.load(ids, w, V)
    for t, o in zip((1, 2), o0):
        ro = R.sgd_step_fast(model, csr, t, 0.3, 1e-4)
        assert (o.n_rows, o.n_loss_rows, o.n_unique) == (ro.n_rows, ro.n_loss_rows, ro.n_unique)
        assert o.loss_sum == pytest.approx(ro.loss_sum, rel=RTOL)
    assert_tables(model, t0)


@gpu_test
@pytest.mark.parametrize("k,cap", PLAIN_CASES)
def test_predict_teams_walk_several_samples(door, k, cap):
    """kPredict: ids >= num_features, ids absent from the model, and rows left with no learned
    feature (they score w0 unclamped) among the samples."""
    from fm_spark_amd.engine import FMContext

    F = F_PLAIN
    csr, ids, w, V = plain_problem(k, cap, 2000 + k, extra=150)  # ids up to F + 149
    keep = ids[(ids % 3 != 0) & (ids < F)]  # every third id absent from the model
    # every seventh row keeps absent ids only (multiples of 3, distinct within the row)
    col = csr.col.copy()
    n_unlearned = 0
    for s in range(0, csr.n_rows, 7):
        a, b = csr.row_ptr[s], csr.row_ptr[s + 1]
        col[a:b] = 3 * ((s + np.arange(b - a)) % (F // 3))
        n_unlearned += int(b > a)
    csr = R.CSR(csr.row_ptr, col, csr.val, csr.label)
    assert n_unlearned > 3 and (csr.col >= F).any()

    def run():
        ctx = FMContext(F, k, w0=0.25)
        ctx.load_tables(keep, w[keep], V[keep])
        p = ctx.predict(to_host(csr), -0.5, 1.5)
        ctx.close()
        return p

    p0, _ = capped(door, 0, run)
    p1, log = capped(door, cap, run)
    assert_log(door, log, (door.PREDICT, *SHAPES[k]), cap, 1, csr.n_rows)
    assert np.array_equal(p0, p1)
    model = R.Model.empty(F, k)
    model.load(keep, w[keep], V[keep])
    model.w0 = 0.25
    ref = R.predict(model, csr, -0.5, 1.5, num_features=F)
    assert (ref[::7][np.diff(csr.row_ptr)[::7] > 0] == 0.25).all()
    np.testing.assert_allclose(p0, ref, rtol=RTOL, atol=ATOL)


@gpu_test
@pytest.mark.parametrize("fill", [False, True])
@pytest.mark.parametrize("k,cap", PLAIN_CASES)
def test_loss_grad_teams_walk_several_samples(door, k, cap, fill):
    """kLossGrad and its second walk, without the fill (fm_loss_grad) and with it (fm_calc_loss_grad:
    entries whose id the model lacks draw their own row, keyed by the entry index)."""
    from fm_spark_amd.engine import FMContext

    F, sd, seed = F_PLAIN, 0.05, 11
    csr, ids, w, V = plain_problem(k, cap, 3000 + k, extra=150 if fill else 0)
    keep = ids[(ids % 4 != 1) & (ids < F)] if fill else ids

    def run():
        ctx = FMContext(F, k)
        ctx.load_tables(keep, w[keep], V[keep])
        out = ctx.loss_grad(to_host(csr), initial_sd=sd, seed=seed) if fill else ctx.loss_grad(to_host(csr))
        ctx.close()
        return out

    g0, _ = capped(door, 0, run)
    g1, log = capped(door, cap, run)
    assert_log(door, log, (door.LOSS_GRAD, *SHAPES[k]), cap, 1, csr.n_rows)
    assert bits_equal(g0, g1)
    col = csr.col.astype(np.int64).copy()
    e_abs = np.nonzero(~np.isin(csr.col, keep))[0]
    assert (len(e_abs) > 0 and (csr.col[e_abs] >= F).any()) if fill else len(e_abs) == 0
    Fo = F + 150 + len(e_abs)
    col[e_abs] = F + 150 + np.arange(len(e_abs))  # every such entry a feature of its own holding its draw
    model = R.Model.empty(Fo, k)
    model.load(keep, w[keep], V[keep])
    if fill:
        wd = _gauss_draw(seed, e_abs, -1, sd).astype(np.float64)
        Vd = np.stack([_gauss_draw(seed, e_abs, f, sd) for f in range(k)], axis=1).astype(np.float64)
        model.load(col[e_abs], wd, Vd)
    rp, rl, rdw, rdv = R.loss_grad(model, R.CSR(csr.row_ptr, col.astype(np.int32), csr.val, csr.label))
    gp, gl, gdw, gdv = g0
    np.testing.assert_allclose(gp, rp, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(gl, rl, rtol=1e-5, atol=1e-9)
    np.testing.assert_array_equal(gdw, rdw)
    np.testing.assert_allclose(gdv, rdv, rtol=1e-5, atol=1e-9)


# ---------------------------------------------------------------------------------- the fused forward
F_FUSED, POOL_FUSED = 200_000, 512
SINGLE, MULTI, INTER, MIX = "single", "multi", "interleaved", "mix"


def fused_layout(RPP, U, NS, nteams):
    """The general rounds, then every stash edge: a sample of NS RPP - 1, NS RPP, NS RPP + 1 or
    2 NS RPP + 3 entries -- NS - 1, NS, NS + 1 singletons in a lane group, and the re-read path -- all
    singletons, all multi or interleaved, followed on its team by an empty and by an odd-short sample.
    -> (lengths per sample, variant per sample)."""
    oa, _ = odd_shorts(RPP)
    rounds = [(n, MIX) for n in general_rounds(RPP, U)]
    rounds.pop()  # (the edges below end on the long last round)
    for n in (NS * RPP - 1, NS * RPP, NS * RPP + 1, 2 * NS * RPP + 3):
        for var in (SINGLE, MULTI, INTER):
            rounds += [(n, var), (0, MIX), (n, var), (oa, MIX)]
    rounds.append((U * RPP + 1, MIX))
    lengths = lay_out([n for n, _ in rounds], nteams)
    variant = np.concatenate([np.repeat(np.asarray([v for _, v in rounds], dtype=object), nteams),
                              np.full(len(lengths) - len(rounds) * nteams, SINGLE, dtype=object)])
    return lengths, variant


def fused_problem(k, cap, NS, U):
    GS, TEAM = FUSED_SHAPES[k]
    RPP, nt = TEAM // GS, nteams_of(cap, TEAM)
    lengths, variant = fused_layout(RPP, U, NS, nt)
    check_walk(lengths, nt, RPP, U, what=f"fused k={k} cap={cap}")
    # every edge sample is followed, on its team, by an empty and by an odd-short sample
    oa, _ = odd_shorts(RPP)
    for n in (NS * RPP - 1, NS * RPP, NS * RPP + 1, 2 * NS * RPP + 3):
        for var in (SINGLE, MULTI, INTER):
            at = np.nonzero((lengths == n) & (variant == var))[0]
            at = at[at + nt < len(lengths)]
            nxt = lengths[at + nt]
            for t in range(nt):
                mine = nxt[at % nt == t]
                assert (mine == 0).any() and (mine == oa).any(), (k, cap, n, var, t)
    # per entry: 1 = an id unique in the batch, 0 = a pool id
    rng = np.random.default_rng(77 + k)
    row = np.repeat(np.arange(len(lengths)), lengths)
    pos = np.arange(len(row)) - np.repeat(np.concatenate([[0], np.cumsum(lengths)])[:-1], lengths)
    var_e = variant[row]
    kinds = (rng.random(len(row)) < 0.5).astype(np.int64)
    kinds[var_e == SINGLE] = 1
    kinds[var_e == MULTI] = 0
    inter = var_e == INTER  # two singletons, then a multi entry, down each lane group's passes
    kinds[inter] = ((pos[inter] // RPP + pos[inter] % RPP) % 3 != 0).astype(np.int64)
    csr, ids, w, V = make_rows(4000 + k, lengths, F_FUSED, k, kinds=kinds, pool=POOL_FUSED)
    cnt = np.bincount(csr.col, minlength=F_FUSED)[csr.col]
    assert (cnt[kinds == 1] == 1).all() and (cnt[kinds == 0] >= 2).all()  # singletons and multi rows as laid out
    # the singletons of a lane group in the edge samples: NS - 1, NS, NS + 1 and beyond all occur
    per_group = set()
    for s in np.nonzero((variant != MIX) & (lengths > 0))[0][:: max(1, nt)]:
        a = csr.row_ptr[s]
        kk = kinds[a:a + lengths[s]]
        per_group |= {int(kk[rs::RPP].sum()) for rs in range(RPP)}
    assert {NS - 1, NS, NS + 1, 2 * NS + 1} <= per_group, per_group
    return csr, ids, w, V


def fused_steps(csr, k, ids, w, V, fuse):
    from fm_spark_amd.engine import FMContext

    ctx = FMContext(F_FUSED, k, fuse=fuse)
    ctx.load_tables(ids, w, V)
    assert ctx.fuse_active == fuse
    db = ctx.batch(to_host(csr))
    outs = []
    for t in (1, 2, 3):  # step 2 reads the headers step 1 wrote
        db.prepare()
        outs.append(ctx.step_batch(db, t, 0.3, 1e-2))
    tabs = ctx.export_tables()
    ctx.close()
    return outs, tabs


@gpu_test
@pytest.mark.parametrize("k,cap", FUSED_CASES)
def test_fused_teams_hand_over_between_samples(door, k, cap):
    """kTrainFused: three fused steps, the stash handed from sample to sample at every edge."""
    c = door.consts()
    csr, ids, w, V = fused_problem(k, cap, c.fuse_ns, c.fuse_u)
    (o0, t0), _ = capped(door, 0, lambda: fused_steps(csr, k, ids, w, V, True))
    (o1, t1), log = capped(door, cap, lambda: fused_steps(csr, k, ids, w, V, True))
    assert_log(door, log, (door.TRAIN_FUSED, *FUSED_SHAPES[k], c.fuse_u), cap, 3, csr.n_rows)
    assert bits_equal(t0, t1)
    for a, b in zip(o0, o1):
        assert (a.n_rows, a.n_loss_rows, a.n_unique) == (b.n_rows, b.n_loss_rows, b.n_unique)
        assert_loss_close(a.loss_sum, b.loss_sum, csr.n_rows)
    model = R.Model.empty(F_FUSED, k)
    model.load(ids, w, V)
    for t, o in zip((1, 2, 3), o0):
        ro = R.sgd_step_fast(model, csr, t, 0.3, 1e-2)
        assert (o.n_rows, o.n_loss_rows, o.n_unique) == (ro.n_rows, ro.n_loss_rows, ro.n_unique)
        assert o.loss_sum == pytest.approx(ro.loss_sum, rel=RTOL)
    assert_tables(model, t0)


# ------------------------------------------------------------------- the sharded owner's partial pass
PARTIAL_U = 4
# (GS, TEAM) -> the ks that reach it (the first with the fp32 wire in one exchange, the second with
# the fp64 wire in 4 chunks): every team the partial pass can choose
PARTIAL_SHAPES = {(1, 1): (1, 4), (1, 2): (4, 3), (1, 16): (3, 1), (2, 2): (5, 8), (2, 4): (8, 6), (2, 16): (7, 5),
                  (4, 4): (9, 16), (4, 8): (12, 9), (4, 16): (16, 13), (8, 8): (17, 32), (8, 16): (32, 17),
                  (16, 16): (33, 64), (32, 32): (65, 128), (64, 64): (129, 256)}
PARTIAL_CASES = ([(gs, tm, ks[0], "fp32", 1, 1) for (gs, tm), ks in PARTIAL_SHAPES.items()] +
                 [(gs, tm, ks[1], "fp64", 4, 1) for (gs, tm), ks in PARTIAL_SHAPES.items()] +
                 [(1, 2, 2, "fp32", 4, 1), (4, 8, 10, "fp64", 1, 1), (1, 1, 3, "fp32", 4, 3), (1, 16, 2, "fp64", 1, 3),
                  (2, 2, 8, "fp64", 1, 3), (2, 4, 7, "fp32", 4, 3), (4, 4, 11, "fp64", 4, 3), (4, 16, 16, "fp32", 4, 3),
                  (8, 8, 20, "fp32", 1, 3), (8, 16, 24, "fp64", 4, 3), (16, 16, 40, "fp32", 4, 3),
                  (32, 32, 100, "fp32", 4, 3), (64, 64, 200, "fp64", 1, 3)])
F_PARTIAL = 3000


def partial_band(GS, TEAM):
    """Entries per pair (lo, hi] that steer the owners' passes to TEAM (about 2, 6 or 12 entries per
    pair and owner); the log, not this, confirms the team that ran."""
    if GS >= 16:
        return 0.0, math.inf
    if TEAM == GS:
        return 0.0, 3.8
    if TEAM == 2 * GS and GS < 8:
        return 4.4, 7.6
    return 8.5, math.inf


def partial_block(GS, TEAM, nteams, short):
    """The lengths, pair by pair, of one block of an owner's pairs: the general rounds without empty
    samples (a pair has an entry), padded with rounds of 1 or of long samples into the band."""
    RPP = TEAM // GS
    lo, hi = partial_band(GS, TEAM)
    oa, _ = odd_shorts(RPP)
    L1, L2 = PARTIAL_U * RPP + 1, 2 * PARTIAL_U * RPP + 1
    rounds = [L2, oa, L1, 1, L1] if short else general_rounds(RPP, PARTIAL_U, empty=False)
    while True:
        seq = lay_out(rounds, nteams)
        if seq.mean() > hi:
            rounds.insert(len(rounds) - 1, 1)
        elif seq.mean() <= lo:
            rounds.insert(len(rounds) - 1, L2)
        else:
            return seq


def owner_launches(lengths, C):
    """Per owner, the pair lengths each of its C launches walks, in order: the owner's pairs are the
    (source, row) pairs with an entry for it, source after source (source l holds rows [B l / L,
    B (l + 1) / L)), and chunk c takes [P c / C, P (c + 1) / C) of each source's P pairs."""
    B = len(lengths)
    out = []
    for o in range(L_RANKS):
        per_src = []
        for l in range(L_RANKS):
            rows = lengths[B * l // L_RANKS: B * (l + 1) // L_RANKS, o]
            per_src.append(rows[rows > 0])
        out.append([np.concatenate([p[len(p) * c // C: len(p) * (c + 1) // C] for p in per_src]) for c in range(C)])
    return out


def partial_problem(GS, TEAM, k, C, cap, starved=False):
    nt = nteams_of(cap, TEAM)
    RPP = TEAM // GS
    block = partial_block(GS, TEAM, nt, short=C > 1)
    # one block per (source, chunk): every launch of an owner walks whole blocks, source after source
    one = np.tile(block, C)
    lengths = np.stack([np.tile(one, L_RANKS)] * L_RANKS, axis=1)  # every owner the same length in every row
    if starved:
        # owner 2 gets no entry (no pair: it launches nothing); source 1's rows are empty (no pair in
        # any chunk); source 0 sends owner 0 two pairs only (none in chunks 0 and 2 of 4)
        B1 = len(one)
        lengths[:, 2] = 0
        lengths[B1:2 * B1, :] = 0
        lengths[2:B1, 0] = 0
    launches = owner_launches(lengths, C)
    for o, per_chunk in enumerate(launches):
        for c, seq in enumerate(per_chunk):
            if len(seq):
                check_walk(seq, nt, RPP, PARTIAL_U, empty=False, what=f"owner {o} chunk {c}")
    csr, ids, w, V = make_rows(5000 + 7 * k + C, lengths, F_PARTIAL, k, pool=F_PARTIAL)
    return csr, ids, w, V, launches


def vector_predict(model, csr, lo, hi):
    """R.predict for a batch whose ids the model all holds, with numpy reductions in fp64 (R.predict
    walks entry by entry; the first rows are checked against it)."""
    n = csr.n_rows
    row = np.repeat(np.arange(n), np.diff(csr.row_ptr))
    x = csr.val
    Vx = model.V[csr.col] * x[:, None]
    s = np.zeros((n, model.k))
    np.add.at(s, row, Vx)
    vv = np.zeros(n)
    np.add.at(vv, row, (Vx * Vx).sum(axis=1))
    ws = np.zeros(n)
    np.add.at(ws, row, model.w[csr.col] * x)
    yhat = 0.5 * ((s * s).sum(axis=1) - vv) + ws + model.w0
    out = np.where(np.diff(csr.row_ptr) > 0, np.clip(yhat, lo, hi), model.w0)
    m = min(n, 200)
    head = R.CSR(csr.row_ptr[: m + 1], csr.col[: csr.row_ptr[m]], csr.val[: csr.row_ptr[m]], csr.label[:m])
    np.testing.assert_allclose(out[:m], R.predict(model, head, lo, hi), rtol=1e-12, atol=1e-14)
    return out


def run_partial_case(door, GS, TEAM, k, wire, C, cap, starved=False):
    from fm_spark_amd.engine import FMContext
    from test_gpu_fuzz import score_terms

    F = F_PARTIAL
    csr, ids, w, V, launches = partial_problem(GS, TEAM, k, C, cap, starved)
    step, reg = 0.3, 1e-4

    def run():
        ctx = FMContext(F, k, parallel="sharded", n_gpus=L_RANKS, devices=[0] * L_RANKS, transport="copy",
                        xchg_chunks=C, wire=wire)
        ctx.load_tables(ids, w, V)
        db = ctx.batch(to_host(csr))
        outs = []
        for t in (1, 2):
            db.prepare()
            outs.append(ctx.step_batch(db, t, step, reg))
        tabs = ctx.export_tables()
        pred = ctx.predict(to_host(csr), -2.0, 3.0)
        ctx.close()
        return outs, tabs, pred

    (o0, t0, p0), _ = capped(door, 0, run)
    (o1, t1, p1), log = capped(door, cap, run)
    # (a), (b): per owner with pairs, C launches per step and one per predict, each of cap blocks over
    # the owner's pairs, the chunk's share of them at least 3 per team
    mode = door.PARTIAL64 if wire == "fp64" else door.PARTIAL
    want = []
    for per_chunk in launches:
        P = sum(len(s) for s in per_chunk)
        if P:
            want += 2 * [(c, C, P) for c in range(C)] + [(0, 1, P)]
    assert sorted((r.chunk, r.chunks, r.rows) for r in log) == sorted(want), log
    pairs_of = {(c, C, sum(len(s) for s in pc)): len(pc[c]) for pc in launches for c in range(C)}
    for r in log:
        assert (r.mode, r.gs, r.team, r.u) == (mode, GS, TEAM, PARTIAL_U) and r.blocks == cap, r
        walked = r.rows if r.chunks == 1 else pairs_of[(r.chunk, r.chunks, r.rows)]
        assert walked >= 3 * r.blocks * (BLOCK // r.team), r
    # (c)
    assert bits_equal(t0, t1) and np.array_equal(p0, p1)
    for a, b in zip(o0, o1):
        assert (a.n_rows, a.n_loss_rows, a.n_unique) == (b.n_rows, b.n_loss_rows, b.n_unique)
        assert_loss_close(a.loss_sum, b.loss_sum, csr.n_rows)
    # (d)
    model = R.Model.empty(F, k)
    model.load(ids, w, V)
    for t, o in zip((1, 2), o0):
        ro = R.sgd_step_fast(model, csr, t, step, reg)
        assert (o.n_rows, o.n_loss_rows, o.n_unique) == (ro.n_rows, ro.n_loss_rows, ro.n_unique)
        assert o.loss_sum == pytest.approx(ro.loss_sum, rel=RTOL, abs=1e-9)
    pids = np.nonzero(model.present)[0]
    ulp4 = 4 * 2.0 ** -24 * max(float(np.max(np.abs(model.V[pids]))), float(np.max(np.abs(model.w[pids]))))
    gids, gw, gV = t0
    np.testing.assert_array_equal(gids, pids)
    np.testing.assert_allclose(gw, model.w[pids], rtol=RTOL, atol=max(ATOL, ulp4))
    np.testing.assert_allclose(gV, model.V[pids], rtol=RTOL, atol=max(ATOL, ulp4))
    trained = R.Model.empty(F, k)  # the transform's arithmetic on the tables this path trained (test_gpu_fuzz)
    trained.load(gids, gw, gV)
    ref = vector_predict(trained, csr, -2.0, 3.0)
    bound = RTOL * np.abs(ref) + np.maximum(1e-7, 8 * 2.0 ** -24 * score_terms(trained, csr))
    assert np.all(np.abs(p0 - ref) <= bound), float(np.max(np.abs(p0 - ref) - bound))


@gpu_test
@pytest.mark.parametrize("GS,TEAM,k,wire,C,cap", PARTIAL_CASES)
def test_partial_teams_walk_several_pairs(door, GS, TEAM, k, wire, C, cap):
    """kPartial / kPartial64 through a three-rank sharded context on one GPU: two steps and a predict,
    the owners' passes in one exchange or in 4 chunks (the chunk prologue's walk over the sources)."""
    run_partial_case(door, GS, TEAM, k, wire, C, cap)


@gpu_test
@pytest.mark.parametrize("wire", ["fp32", "fp64"])
def test_partial_owner_without_pairs_and_source_without_a_pair_in_a_chunk(door, wire):
    """One owner receives no pair at all, one source sends nobody a pair, and one source sends an owner
    two pairs, so chunks 0 and 2 of 4 hold none of them: the prologue's `while (sl >= ch_base[r + 1])`
    must step over sources whose share of the chunk is empty."""
    run_partial_case(door, 4, 16, 16, wire, 4, 1, starved=True)


# --------------------------------------------------------------------------------- without a GPU
def test_door_without_a_launch():
    """The door itself: the forward's constants are readable, a cap can be set and taken back, and
    nothing is logged where nothing was launched (a negative cap is refused, the setting unchanged)."""
    import forward_probe as fp

    c = fp.consts()
    assert c.block == BLOCK and c.grid >= 1 and c.fuse_ns >= 1 and c.fuse_u >= 1 and c.log_cap >= 64
    with fp.grid_cap(3):
        assert fp.read_log() == []
        with pytest.raises(RuntimeError, match="status -1"):
            fp.set_grid_cap(-1)
    assert fp.read_log() == []


def test_layouts_meet_their_transitions():
    """Every case's batch is laid out and checked on the CPU exactly as its GPU test does before it
    launches anything (NS = 5 and U = 5 stand in for the probe's values here; the GPU cases read them)."""
    for k, cap in PLAIN_CASES:
        plain_problem(k, cap, 1)
    for k, cap in FUSED_CASES:
        fused_problem(k, cap, 5, 5)
    for GS, TEAM, k, wire, C, cap in PARTIAL_CASES:
        partial_problem(GS, TEAM, k, C, cap)
    partial_problem(4, 16, 16, 4, 1, starved=True)


def test_every_forward_instantiation_is_a_case():
    """The coverage list: each (GS, TEAM, U) of the step's forward, the fused forward and the partial
    pass is some case's expected tuple."""
    assert set(SHAPES.values()) == {(1, 32, 3), (2, 32, 3), (4, 32, 2), (8, 32, 2), (16, 32, 2), (32, 32, 4), (64, 64, 4)}
    assert {k: SHAPES[k][0] for k in (9, 17)} == {9: 4, 17: 8}  # lanes with qok == false take part
    assert set(FUSED_SHAPES.values()) == {(1, 32), (2, 32), (4, 32)} and {9, 12, 16} <= set(FUSED_SHAPES)
    teams = {(1, 1), (1, 2), (1, 16), (2, 2), (2, 4), (2, 16), (4, 4), (4, 8), (4, 16), (8, 8), (8, 16), (16, 16),
             (32, 32), (64, 64)}
    for wire in ("fp32", "fp64"):
        assert {(c[0], c[1]) for c in PARTIAL_CASES if c[3] == wire} == teams
    for C in (1, 4):
        assert {(c[0], c[1]) for c in PARTIAL_CASES if c[4] == C} == teams
