"""GPU: training on rows that hold one feature id more than once, in every step path.

The library takes such rows -- each occurrence is an entry of its own in the score, the gradients and
fm_loss_grad's output, and the id counts once in n_unique (include/fm_hip.h) -- but every other
generator of the suite rules them out by construction.  tests/repeat_cases.py builds them: a run of 2
from one sample whose id no other row holds (pair-only), b(+3) .. b(-3) in one row (cancel), one id at
five places of a row of 261 entries (spread), one id G .. 2 Wv + 1 times in one row, from a wave's first
entry and astride a wave boundary (one-sample-run-*), a run of 6 over three samples with a hot id that
a third of the rows hold twice (mixed), every row concatenated with itself (self-pair).  Every case
asserts first, on the oracle alone, that its view holds the event it is named for and that reading a
row's repeats as one entry (x summed) or keeping only the first moves every designated row by at least
8 tolerances (tests/test_repeat_cases_cpu.py does the same without a GPU).

Every case is update_cases' two steps (reg_param > 0, every other designated id absent, a first batch
that touches none of the second's rows).  Checked: the whole table against oracle.fm_ref.sgd_step_fast at
RTOL 1e-5 / ATOL 1e-8 (on three ranks the floor max(ATOL, 4 * 2^-24 * max|table|) of test_gpu_fuzz),
(n_rows, n_loss_rows, n_unique) exactly, loss_sum to RTOL, a second run bit for bit.  Each test prints
its largest error in units of the tolerance in force.

Paths: fm_step from the host, unprepared and prepared unfused (bit for bit equal); fused (k <= 16; the
layout is the compacted view, true singletons sprinkled into the full one -- pair-only's run [a, a]
must not leave with them); the replicated emit at world 1 and three replicated ranks; sharded at world 1
(fp64 wire) and on three ranks with both wires, and a batch in which one owner's pair of a sample is
nothing but repeats of one id while another owner receives nothing from that sample; pair batches
(fm_batch_from_pairs) whose rows share one id, all ids or none, stepped under the squared, logistic
and BPR objectives; fm_loss_grad, its seeded fill, fm_init_from_batch, predict and evaluate.

(case, k) left out, because a kept one reaches the same branch: the three-rank paths run k = 8 and 24
(64 for one-sample-run-*) only -- the packed S record (kp <= 16) and the separate S rows above; their
kernels are world 1's, which runs every case at every k -- and of the one-sample-run-*
cases only G + 1, Wv + 1 and 2 Wv + 1 (inside a wave, two ranges, the long combine); the fp64 wire on
three ranks runs k = 8 only.
"""

from types import SimpleNamespace

import numpy as np
import pytest

import objective_ref as O
import pair_ref as P
import repeat_cases as rc
import shard_cases
from oracle import fm_ref as R
from problems import f32, make_rows
from test_gpu_fuse import _assert_same
from test_gpu_fuzz import run_path
from test_gpu_parity import ATOL, RTOL, _gauss_draw, to_host
from test_gpu_update_edges import _assert_bitwise, _assert_oracle, _emit, _sharded, _single

pytestmark = pytest.mark.gpu

CASES = [(n, k) for n in rc.NAMES for k in rc.ks_of(n)]
ONE_KEPT = {"one-sample-run-G+1", "one-sample-run-Wv+1", "one-sample-run-2Wv+1"}
THREE = [(n, k) for n, k in CASES if k in (8, 24, 64) and (n not in rc.ONE or n in ONE_KEPT)]


def _case(name, k, fused=False):
    import update_probe

    c = rc.case(name, k, update_probe.geometry(k), fused)
    rc.assert_case(c)
    return c


def _ratio(model, tables, atol=ATOL):
    """The largest error of the tables in units of the tolerance RTOL |want| + atol."""
    gids, gw, gV = tables
    want_w, want_V = model.w[gids], model.V[gids]
    return max(float(np.max(np.abs(gw - want_w) / (RTOL * np.abs(want_w) + atol))),
               float(np.max(np.abs(gV - want_V) / (RTOL * np.abs(want_V) + atol))))


def _report(path, c, ratio):
    print(f"repeated-ids {path} {c.name} k={c.k}: largest error {ratio:.3g} of the tolerance")


def _designated_rows(c, tables, atol=ATOL):
    """The designated (repeated) ids' rows on their own: what the wrong readings would move."""
    gids, gw, gV = tables
    at = np.searchsorted(gids, c.des)
    np.testing.assert_array_equal(gids[at], c.des)
    np.testing.assert_allclose(gw[at], c.model.w[c.des], rtol=RTOL, atol=atol)
    np.testing.assert_allclose(gV[at], c.model.V[c.des], rtol=RTOL, atol=atol)


# ------------------------------------------------------------------------------------- single table
@pytest.mark.parametrize("name,k", CASES)
def test_host_unprepared_and_prepared(gpu, name, k):
    c = _case(name, k)
    inline, n_rows = _single(c, fuse=False, prepare=False)
    _assert_oracle(c, inline, n_rows)
    _designated_rows(c, inline[1])
    _report("single", c, _ratio(c.model, inline[1]))
    prepared, _ = _single(c, fuse=False, prepare=True)
    _assert_bitwise(inline, prepared)
    cfg = dict(F=c.F, k=c.k, step=c.steps[0], reg=c.reg)
    outs, tabs, _ = run_path("host", cfg, c.batches, c.keep, c.w[c.keep], c.V[c.keep])
    _assert_bitwise(inline, ([(o.loss_sum, o.n_unique, o.n_loss_rows) for o in outs], tabs))  # fm_step from the host
    _assert_bitwise(inline, _single(c, fuse=False, prepare=False)[0])  # and a second run repeats the first


@pytest.mark.parametrize("name,k", [(n, k) for n, k in CASES if rc.fusable(k)])
def test_fused(gpu, name, k):
    """A row is a singleton by the length of its run, not by how many samples touch it: a run [s, s] goes
    to the segmented update (the first-only reading is what the forward's stash would apply)."""
    c = _case(name, k, fused=True)
    fused, n_rows = _single(c, fuse=True, prepare=True)
    _assert_oracle(c, fused, n_rows)
    _designated_rows(c, fused[1])
    assert fused[0][1][1] == c.outs[1].n_unique == len(np.unique(c.batches[1].col))
    _report("fused", c, _ratio(c.model, fused[1]))
    _assert_same(fused, _single(c, fuse=False, prepare=True)[0])
    _assert_bitwise(fused, _single(c, fuse=True, prepare=True)[0])


@pytest.mark.parametrize("k", rc.K_CASES)
def test_spread_positions_against_the_forwards_teams(gpu, k):
    """The five places of spread's repeated id lie in five passes and in different lane groups of the team
    that walks the row, by the (GS, TEAM) the forward itself logs (tests/forward_probe.py; the cap is
    the tuned grid's own size, so nothing but the log changes)."""
    import forward_probe as fp

    c = _case("spread", k)
    with fp.grid_cap(fp.consts().grid):
        _single(c, fuse=False, prepare=True)
        if rc.fusable(k):
            _single(_case("spread", k, fused=True), fuse=True, prepare=True)
        log = fp.read_log()
    assert {r.mode for r in log} >= ({fp.TRAIN, fp.TRAIN_FUSED} if rc.fusable(k) else {fp.TRAIN}), log
    for r in log:
        assert rc.spread_ok(r.team // r.gs), r


# ------------------------------------------------------------------------------------- replicated
@pytest.mark.parametrize("name,k", CASES)
def test_replicated_emit(gpu, name, k):
    c = _case(name, k)
    res, grads = _emit(c)
    _assert_oracle(c, res, [b.n_rows for b in c.batches])
    _report("replicated-emit", c, _ratio(c.model, res[1]))
    again, grads2 = _emit(c)
    _assert_bitwise(res, again)
    for a, b in zip(grads, grads2):
        assert np.array_equal(a, b)


def _floor(model):
    pids = np.nonzero(model.present)[0]
    return max(ATOL, 4 * 2.0 ** -24 * max(float(np.max(np.abs(model.V[pids]))), float(np.max(np.abs(model.w[pids])))))


def _three(c, parallel, wire="fp32"):
    if wire == "fp32":
        outs, tabs, _ = run_path(parallel + "3", dict(F=c.F, k=c.k, step=c.steps[0], reg=c.reg), c.batches, c.keep,
                                 c.w[c.keep], c.V[c.keep])
        return [(o.loss_sum, o.n_unique, o.n_loss_rows, o.n_rows) for o in outs], tabs
    from fm_spark_amd.engine import FMContext

    ctx = FMContext(c.F, c.k, parallel=parallel, n_gpus=3, devices=[0] * 3, transport="copy", wire=wire)
    ctx.load_tables(c.keep, c.w[c.keep], c.V[c.keep])
    outs = [ctx.step(to_host(b), t, s, c.reg) for t, (b, s) in enumerate(zip(c.batches, c.steps), start=1)]
    tabs = ctx.export_tables()
    ctx.close()
    return [(o.loss_sum, o.n_unique, o.n_loss_rows, o.n_rows) for o in outs], tabs


def _assert_three(c, res, path):
    stats, tabs = res
    atol = _floor(c.model)
    for (loss, nu, nl, m), ro in zip(stats, c.outs):
        assert (m, nl, nu) == (ro.n_rows, ro.n_loss_rows, ro.n_unique)
        assert loss == pytest.approx(ro.loss_sum, rel=RTOL)
    pids = np.nonzero(c.model.present)[0]
    np.testing.assert_array_equal(tabs[0], pids)
    np.testing.assert_allclose(tabs[1], c.model.w[pids], rtol=RTOL, atol=atol)
    np.testing.assert_allclose(tabs[2], c.model.V[pids], rtol=RTOL, atol=atol)
    _report(path, c, _ratio(c.model, tabs, atol))


@pytest.mark.parametrize("name,k", THREE)
def test_replicated_three_ranks(gpu, name, k):
    c = _case(name, k)
    res = _three(c, "replicated")
    _assert_three(c, res, "replicated3")
    _assert_bitwise(res, _three(c, "replicated"))


# ------------------------------------------------------------------------------------- sharded
@pytest.mark.parametrize("name,k", CASES)
def test_sharded_world1(gpu, name, k):
    c = _case(name, k)
    res, n_rows = _sharded(c)
    _assert_oracle(c, res, n_rows)
    _designated_rows(c, res[1])
    _report("sharded1-fp64", c, _ratio(c.model, res[1]))
    _assert_bitwise(res, _sharded(c)[0])


@pytest.mark.parametrize("name,k,wire",
                         [(n, k, "fp32") for n, k in THREE] + [(n, k, "fp64") for n, k in THREE if k == 8])
def test_sharded_three_ranks(gpu, name, k, wire):
    c = _case(name, k)
    res = _three(c, "sharded", wire)
    _assert_three(c, res, f"sharded3-{wire}")
    _assert_bitwise(res, _three(c, "sharded", wire))


def _only_repeats(k, R_=3):
    """Rows 0 and 1 are [a, a, a, b] and [c, c] with a, c owned by rank 0 and b by rank 1 (ids modulo
    R_): rank 0's pair of either sample holds nothing but repeats of one id, rank 2 receives nothing from
    sample 0 and ranks 1 and 2 nothing from sample 1.  Twenty ordinary rows follow."""
    F = 96
    rest, ids, w, V = make_rows(31, np.random.default_rng(31).integers(1, 9, 20), F, k, labels="real")
    a, b, c_ = 9, 10, 12
    assert a % R_ == 0 and c_ % R_ == 0 and b % R_ == 1
    col = np.concatenate([[a, a, a, b, c_, c_], rest.col]).astype(np.int32)
    val = np.concatenate([f32([0.75, -1.5, 0.5, 1.0, 2.0, -0.5]), rest.val])
    ptr = np.concatenate([[0, 4], rest.row_ptr + 6]).astype(np.int64)
    csr = R.CSR(ptr, col, val, np.concatenate([[10.0, -10.0], rest.label]))
    has = shard_cases.masks(csr, R_, F)
    assert has[0].tolist() == [True, True, False] and has[1].tolist() == [True, False, False]
    return csr, F, ids, w, V


@pytest.mark.parametrize("wire", ["fp32", "fp64"])
@pytest.mark.parametrize("k", [8, 24])
def test_sharded_pair_of_nothing_but_repeats(gpu, k, wire):
    csr, F, ids, w, V = _only_repeats(k)
    keep = ids[ids != 12]  # c arrives absent
    model = R.Model.empty(F, k)
    model.load(keep, w[keep], V[keep])
    outs = [R.sgd_step_fast(model, csr, t, 0.05, 1e-3) for t in (1, 2)]
    wrong = R.Model.empty(F, k)
    wrong.load(keep, w[keep], V[keep])
    for t in (1, 2):
        R.sgd_step_fast(wrong, rc.first_only(csr), t, 0.05, 1e-3)
    for i in (9, 12):  # a pair opened at its first entry and closed there would be this reading
        assert abs(wrong.w[i] - model.w[i]) > 8 * (RTOL * abs(model.w[i]) + _floor(model))
    c = SimpleNamespace(name="only-repeats", k=k, F=F, keep=keep, w=w, V=V, batches=[csr, csr], steps=[0.05, 0.05],
                           reg=1e-3, model=model, outs=outs)
    res = _three(c, "sharded", wire)
    _assert_three(c, res, f"sharded3-{wire}")
    _assert_bitwise(res, _three(c, "sharded", wire))


# ------------------------------------------------------------------------------------- pair batches
PF, PK = 120, 16
# The step size of the pair tests: no row's update in a step exceeds UPDATE_MAX on the reference (asserted).
# The device forms an update from fp32 inputs, so it is off by about 2^-23 of its size; where the L1 leaves
# the new value next to zero that must still lie under ATOL (update_cases.step_size_for states the same).
PSTEP, UPDATE_MAX = 0.05, 0.05
assert UPDATE_MAX * 2.0 ** -23 < ATOL


def _pair_rows():
    """Eight context rows over ids [0, 60); eight candidate rows of which row j < 4 holds exactly one id of
    context row j and the others none of any context row (ids [60, 120)).  |x| >= 1/2."""
    rng = np.random.default_rng(77)

    def rows(lists):
        ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
        n = int(ptr[-1])
        x = f32(rng.uniform(0.5, 1.5, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0))
        return ptr, np.concatenate(lists).astype(np.int32), x

    u = [np.sort(rng.choice(60, int(n), replace=False)) for n in (3, 1, 5, 2, 4, 6, 2, 3)]
    c = [60 + np.sort(rng.choice(60, int(n), replace=False)) for n in (2, 4, 1, 3, 5, 2, 3, 1)]
    for j in range(4):
        c[j] = np.concatenate([c[j], [u[j][len(u[j]) // 2]]])  # the shared id comes last: the row is not sorted
    return rows(u), rows(c)


def _pair_batches():
    """[(contexts, candidates, pair_ctx, pair_cand)]: twenty pairs that share one id or none, ten that are
    a row with itself."""
    u, c = _pair_rows()
    one = np.arange(4)
    pc = np.concatenate([one, one, np.arange(8), [4, 5, 6, 7]])
    pd = np.concatenate([one, one, np.arange(8)[::-1], [4, 6, 5, 7]])
    share = [len(np.intersect1d(u[1][u[0][a]:u[0][a + 1]], c[1][c[0][b]:c[0][b + 1]])) for a, b in zip(pc, pd)]
    assert sorted(set(share)) == [0, 1] and share.count(1) == 8
    r = np.asarray([0, 1, 2, 3, 4, 5, 6, 7, 2, 5])
    return u, c, [("uc", pc, pd), ("uu", r, r)]


def _pair_labels(loss, n, seed):
    rng = np.random.default_rng(seed)
    return f32(rng.normal(0, 2.0, n)) if loss == "squared" else (rng.random(n) < 0.5).astype(np.float64)


def _pair_steps(loss, group, device_pairs, fuse=None, prepare=False):
    from fm_spark_amd.engine import FMContext

    u, c, sels = _pair_batches()
    rng = np.random.default_rng(78)
    ids, w, V = np.arange(PF, dtype=np.int32), f32(rng.normal(0, 0.1, PF)), f32(rng.normal(0, 0.1, (PF, PK)))
    ctx = FMContext(PF, PK, loss=loss, fuse=fuse)
    ctx.load_tables(ids, w, V)
    zero = lambda rows: to_host(R.CSR(rows[0], rows[1], rows[2], np.zeros(len(rows[0]) - 1)))  # noqa: E731
    bu, bc = ctx.batch(zero(u)), ctx.batch(zero(c))
    out, refs = [], []
    for t, (kind, pc, pd) in enumerate(sels, start=1):
        y = _pair_labels(loss, len(pc), 80 + t)
        ref = P.concat_pairs(u, u if kind == "uu" else c, pc, pd, y)
        if device_pairs:
            b = ctx.batch_from_pairs(bu, bu if kind == "uu" else bc, pc, pd, y)  # "uu": contexts is candidates
        else:
            b = ctx.batch(to_host(ref))
        if group:
            b.set_group(group)
        if prepare:
            b.prepare()
        o = ctx.step_batch(b, t, PSTEP, 1e-3)
        out.append((o.loss_sum, o.n_rows, o.n_loss_rows, o.n_unique))
        refs.append(ref)
        b.close()
    tabs = ctx.export_tables()
    ctx.close()
    return out, tabs, refs, (ids, w, V)


def _pair_reference(loss, group, refs, table):
    """The reference's steps over the pair batches (objective_ref with the device's contract; under
    "squared" that is sgd_step_fast's arithmetic) -> (model, [StepResult]).  Asserted on the way, on the
    reference alone: no update exceeds UPDATE_MAX, every batch holds repeats, and for EVERY id that a row
    holds twice both wrong readings (rc.merged, rc.first_only) move its w or a column of its V by 8
    tolerances or more."""
    ids, w, V = table
    models = [R.Model.empty(PF, PK) for _ in range(3)]
    for m in models:
        m.load(ids, w, V)
    outs, shared = [], set()
    for t, ref in enumerate(refs, start=1):
        pair, n = np.unique(np.repeat(np.arange(ref.n_rows), np.diff(ref.row_ptr)) * PF + ref.col, return_counts=True)
        assert (n > 1).any()
        shared |= set((pair[n > 1] % PF).tolist())
        before = models[0].copy()
        for m, read in zip(models, (lambda x: x, rc.merged, rc.first_only)):
            o = O.step(m, read(ref), t, PSTEP, 1e-3, loss, group, round_scores=True, fast=True)
            if m is models[0]:
                outs.append(o)
        assert max(np.abs(models[0].V - before.V).max(), np.abs(models[0].w - before.w).max()) <= UPDATE_MAX
    model, shared = models[0], np.asarray(sorted(shared))
    assert len(shared) >= 20
    for wrong in models[1:]:
        dv = np.abs(wrong.V[shared] - model.V[shared]) / (RTOL * np.abs(model.V[shared]) + ATOL)
        dw = np.abs(wrong.w[shared] - model.w[shared]) / (RTOL * np.abs(model.w[shared]) + ATOL)
        assert np.maximum(dv.max(axis=1), dw).min() >= rc.FACTOR
    return model, outs


@pytest.mark.parametrize("fuse,prepare", [(False, False), (False, True), (True, True)])
def test_pair_batches_squared_step_is_the_host_batch_step(gpu, fuse, prepare):
    a = _pair_steps("squared", 0, True, fuse, prepare)
    b = _pair_steps("squared", 0, False, fuse, prepare)
    assert a[0] == b[0]
    for x, y in zip(a[1], b[1]):
        assert x.tobytes() == y.tobytes()
    model, outs = _pair_reference("squared", 0, a[2], a[3])
    oracle = R.Model.empty(PF, PK)
    oracle.load(*a[3])
    for t, (ref, got, ro) in enumerate(zip(a[2], a[0], outs), start=1):
        R.sgd_step_fast(oracle, ref, t, PSTEP, 1e-3)
        assert got[1:] == (ro.n_rows, ro.n_loss_rows, ro.n_unique) and got[0] == pytest.approx(ro.loss_sum, rel=RTOL)
    np.testing.assert_allclose(a[1][1], oracle.w[a[1][0]], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(a[1][2], oracle.V[a[1][0]], rtol=RTOL, atol=ATOL)
    print(f"repeated-ids pairs-squared fuse={fuse}: largest error {_ratio(oracle, a[1]):.3g} of the tolerance")


@pytest.mark.parametrize("loss,group", [("logistic", 0), ("bpr", 2), ("bpr", 5)])
def test_pair_batches_under_the_other_objectives(gpu, loss, group):
    """Against tests/objective_ref.py at test_gpu_objective's tolerance (RTOL, ATOL; the loss abs=ATOL)."""
    out, tabs, refs, table = _pair_steps(loss, group, True)
    model, outs = _pair_reference(loss, group, refs, table)
    for got, ro in zip(out, outs):
        assert got[0] == pytest.approx(ro.loss_sum, rel=RTOL, abs=ATOL)
        assert got[1:] == (ro.n_rows, ro.n_loss_rows, ro.n_unique)
    np.testing.assert_array_equal(tabs[0], np.nonzero(model.present)[0])
    assert np.all(np.isfinite(tabs[1])) and np.all(np.isfinite(tabs[2]))
    np.testing.assert_allclose(tabs[1], model.w[tabs[0]], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(tabs[2], model.V[tabs[0]], rtol=RTOL, atol=ATOL)
    print(f"repeated-ids {loss} group={group}: largest error {_ratio(model, tabs):.3g} of the tolerance")
    again = _pair_steps(loss, group, True)
    assert again[0] == out and all(x.tobytes() == y.tobytes() for x, y in zip(again[1], tabs))


# ------------------------------------------------------------------------------------- around the step
def _full(c):
    model = R.Model.empty(c.F, c.k)
    model.load(np.arange(c.F), c.w, c.V)
    return model


@pytest.mark.parametrize("name", ["spread", "cancel"])
def test_loss_grad_answers_per_entry(gpu, name):
    """fm_loss_grad: one line per entry, each repeat its own (its own x, its own v x^2 taken from S x)."""
    from fm_spark_amd.engine import FMContext

    c = _case(name, 8)
    csr, model = c.batches[1], _full(c)
    ctx = FMContext(c.F, c.k)
    ctx.load_tables(np.arange(c.F, dtype=np.int32), c.w, c.V)
    gp, gl, gdw, gdv = ctx.loss_grad(to_host(csr))
    rp, rl, rdw, rdv = R.loss_grad(model, csr)
    assert len(gp) == csr.nnz and gdv.shape == (csr.nnz, c.k)
    np.testing.assert_allclose(gp, rp, rtol=1e-6, atol=1e-9)  # test_gpu_parity.test_loss_grad_matches_oracle's tolerances
    np.testing.assert_allclose(gl, rl, rtol=1e-5, atol=1e-9)
    np.testing.assert_array_equal(gdw, rdw)
    np.testing.assert_allclose(gdv, rdv, rtol=1e-5, atol=1e-9)
    e = np.nonzero(np.isin(csr.col, c.des))[0]
    assert len(np.unique(rdv[e], axis=0)) == len(e) and len(np.unique(gdv[e], axis=0)) == len(e)  # no two repeats alike
    ctx.close()


@pytest.mark.parametrize("name", ["spread", "cancel"])
def test_loss_grad_fill_draws_by_entry(gpu, name):
    """With initial_sd > 0 an absent id's entries each draw their own row, keyed by the entry's index."""
    from fm_spark_amd.engine import FMContext

    c = _case(name, 8)
    csr, sd, seed = c.batches[1], 0.05, 11
    keep = np.setdiff1d(np.arange(c.F), c.des).astype(np.int32)  # every repeated id absent
    ctx = FMContext(c.F, c.k)
    ctx.load_tables(keep, c.w[keep], c.V[keep])
    got = ctx.loss_grad(to_host(csr), initial_sd=sd, seed=seed)
    e_abs = np.nonzero(np.isin(csr.col, c.des))[0]
    col = csr.col.astype(np.int64).copy()
    col[e_abs] = c.F + np.arange(len(e_abs))  # every such entry a feature of its own holding its draw
    model = R.Model.empty(c.F + len(e_abs), c.k)
    model.load(keep, c.w[keep], c.V[keep])
    wd = _gauss_draw(seed, e_abs, -1, sd).astype(np.float64)
    Vd = np.stack([_gauss_draw(seed, e_abs, f, sd) for f in range(c.k)], axis=1).astype(np.float64)
    assert len(np.unique(Vd, axis=0)) == len(e_abs)
    model.load(col[e_abs], wd, Vd)
    ref_csr = R.CSR(csr.row_ptr, col.astype(np.int32), csr.val, csr.label)
    ref = R.loss_grad(model, ref_csr)
    for g, r in zip(got, ref):  # test_gpu_parity.test_calc_loss_grad_fills_absent_ids' tolerance
        np.testing.assert_allclose(g, r, rtol=1e-5, atol=1e-9)
    np.testing.assert_array_equal(got[2], ref[2])
    ctx.close()


def test_init_from_batch_counts_an_id_once(gpu):
    from fm_spark_amd.engine import FMContext

    c = _case("self-pair", 8)
    csr = c.batches[1]
    distinct = np.unique(csr.col)
    assert 2 * len(distinct) <= csr.nnz
    rw, rV = R.init_draw(distinct, c.k, 77, 0.02)
    tabs = []
    for kw in (dict(), dict(parallel="sharded", n_gpus=3, devices=[0] * 3, transport="copy")):
        ctx = FMContext(c.F, c.k, seed=77, init_sd=0.02, **kw)
        n = ctx.init_from_batch(ctx.batch(to_host(csr)))
        gids, gw, gV = ctx.export_tables()
        ctx.close()
        assert n == len(distinct)
        np.testing.assert_array_equal(gids, distinct)
        np.testing.assert_allclose(gw, rw, rtol=1e-6)  # test_init_random_matches_oracle_draw's tolerance
        np.testing.assert_allclose(gV, rV, rtol=1e-6)
        tabs.append((gw, gV))
    assert np.array_equal(tabs[0][0], tabs[1][0]) and np.array_equal(tabs[0][1], tabs[1][1])


@pytest.mark.parametrize("name", ["spread", "mixed", "self-pair"])
def test_predict_and_evaluate_on_the_trained_table(gpu, name):
    import eval_ref
    from fm_spark_amd.engine import FMContext

    c = _case(name, 8)
    csr = c.batches[1]
    pids = np.nonzero(c.model.present)[0]
    trained = R.Model.empty(c.F, c.k)
    trained.load(pids, f32(c.model.w[pids]), f32(c.model.V[pids]))
    ctx = FMContext(c.F, c.k)
    ctx.load_tables(pids.astype(np.int32), trained.w[pids], trained.V[pids])
    b = ctx.batch(to_host(csr))
    ref = R.predict(trained, csr, -20.0, 20.0, num_features=c.F)
    wrong = R.predict(trained, rc.merged(csr), -20.0, 20.0, num_features=c.F)
    bound = RTOL * np.abs(ref) + 1e-7  # test_gpu_fuzz's tolerance for a single table's transform
    assert (np.abs(wrong - ref) > 8 * bound).any()  # the merged reading scores otherwise
    got = ctx.predict_batch(b, -20.0, 20.0)
    assert np.array_equal(got, ctx.predict(to_host(csr), -20.0, 20.0))
    assert (np.abs(got - ref) <= bound).all(), float(np.max(np.abs(got - ref) / bound))
    rec, pred = ctx.evaluate_batch(b, -20.0, 20.0, want_pred=True)
    assert np.array_equal(pred, got)
    n_unlearned = int((~eval_ref.learned_rows(trained, csr, c.F)).sum())  # the rows without entries
    eval_ref.check(rec, csr.label, pred, n_unlearned=n_unlearned)
    b.close()
    ctx.close()
