"""GPU: the fp64 partial-sum wire of the sharded step (fm_config.wire = FM_WIRE_FP64).

With the fp32 wire every owner rounds its share of a sample's forward sums (sum v x, sum v^2 x^2,
sum w x) to fp32 before the requester adds the shares; with the fp64 wire the shares cross
unrounded, so the sums are fp64 over all of the sample's entries and rounded once, as on one
table (the reference sums in Double, FactorizationMachinesSGD.scala:145-154).  The ranks share
this box's GPU through the COPY transport, as in test_gpu_group.py.

1. known answers that only an unrounded wire gives: owner 0 holds 1 and eps = 2^-30, owner 1
   holds -1; the sample's sum is eps, and 1 + eps rounds to 1 in fp32;
2. the fuzz problems on three ranks within the single table's own bounds (no fp32-ulp floor);
3. the shapes at which the wide kernels take another path;
4. the contract of the switch (determinism, the default untouched, refusals, the struct layout).
"""

import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import fm_ref as R_
from problems import make_problem
from test_gpu_fuzz import draw, to_host

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-8  # the single table's bounds (test_gpu_parity.py)
EPS = 2.0 ** -30


def _ctx(F, k, R, mode="sharded", transport="copy", wire="fp64", **kw):
    from fm_spark_amd.engine import FMContext

    devs = [0] * R if transport == "copy" else list(range(R))
    return FMContext(F, k, parallel=mode, n_gpus=R, devices=devs, transport=transport, wire=wire, **kw)


def _check_tables(ctx, model):
    gi, gw, gV = ctx.export_tables()
    np.testing.assert_array_equal(gi, np.nonzero(model.present)[0])
    np.testing.assert_allclose(gw, model.w[gi], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(gV, model.V[gi], rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------- 1. known answers
# (R, F, ids of every row, k): ids[0] and ids[2] sit on owner 0, ids[1] on owner 1
KAT_SHAPES = {"R2": (2, 3, (0, 1, 2), 1), "R3": (3, 4, (0, 1, 3), 1), "R2k5": (2, 3, (0, 1, 2), 5)}


def _kat(shape, side):
    """Four identical rows holding the three ids with x = 1, labels 0; the values 1, -1, eps on w
    (side "w", V = 0) or on V's last column (side "V", w = 0, the other columns 0)."""
    R, F, ids, k = KAT_SHAPES[shape]
    ids = np.asarray(ids, np.int32)
    csr = R_.CSR(np.arange(5, dtype=np.int64) * 3, np.tile(ids, 4), np.ones(12), np.zeros(4))
    vals = np.array([1.0, -1.0, EPS])
    w = vals if side == "w" else np.zeros(3)
    V = np.zeros((3, k))
    if side == "V":
        V[:, k - 1] = vals
    return R, F, k, ids, csr, w, V


def _kat_step(ctx, csr, via):
    if via == "host":
        return ctx.step(to_host(csr), 1, 0.5, 0.0)
    b = ctx.batch(to_host(csr))
    b.prepare()
    out = ctx.step_batch(b, 1, 0.5, 0.0)
    b.close()
    return out


@pytest.mark.parametrize("via", ["host", "batch"])
@pytest.mark.parametrize("chunks", [1, 4])
@pytest.mark.parametrize("shape", sorted(KAT_SHAPES))
def test_known_answer_w_side(gpu, shape, chunks, via):
    """w = [1, -1, eps], V = 0: every row scores eps exactly, one step (t = 1, stepSize 0.5,
    regParam 0) reports loss_sum = 4 * 2^-60 and leaves w[eps row] = eps - 0.5 * eps = 2^-31.  With the
    shares rounded to fp32 owner 0's 1 + eps is 1: score 0, loss 0, the eps row not moved."""
    R, F, k, ids, csr, w, V = _kat(shape, "w")
    ctx = _ctx(F, k, R, xchg_chunks=chunks)
    ctx.load_tables(ids, w, V)
    pred = ctx.predict(to_host(csr), -math.inf, math.inf)
    out = _kat_step(ctx, csr, via)
    gi, gw, gV = ctx.export_tables()
    ctx.close()
    print(f"\nw side {shape} chunks {chunks} {via}: predict {pred.tolist()}, loss_sum {out.loss_sum!r}, "
          f"w[eps row] {gw[2]!r}")
    assert np.array_equal(pred, np.full(4, EPS))
    assert out.loss_sum == 4 * 2.0 ** -60
    assert (out.n_rows, out.n_loss_rows, out.n_unique) == (4, 4, 3)
    np.testing.assert_array_equal(gi, ids)
    assert gw[2] == 2.0 ** -31
    assert not gV.any()


@pytest.mark.parametrize("via", ["host", "batch"])
@pytest.mark.parametrize("chunks", [1, 4])
@pytest.mark.parametrize("shape", sorted(KAT_SHAPES))
def test_known_answer_v_side(gpu, shape, chunks, via):
    """w = 0, V's last column = [1, -1, eps]: S = eps, yhat = 0.5 (eps^2 - 2) = -1 = r, and the eps
    row's gradient sum is A - v b = 4 eps r - eps 4 r = 0, so the row keeps eps exactly.  With the shares
    rounded to fp32 S is 0 and the row moves to eps - 0.5 eps = 2^-31."""
    R, F, k, ids, csr, w, V = _kat(shape, "V")
    ctx = _ctx(F, k, R, xchg_chunks=chunks)
    ctx.load_tables(ids, w, V)
    out = _kat_step(ctx, csr, via)
    gi, gw, gV = ctx.export_tables()
    ctx.close()
    print(f"\nV side {shape} chunks {chunks} {via}: loss_sum {out.loss_sum!r}, V[eps row] {gV[2].tolist()}")
    np.testing.assert_array_equal(gi, ids)
    assert gV[2, k - 1] == EPS
    assert not gV[:, : k - 1].any()  # the zero columns (and the kp padding behind them) stay zero
    assert out.loss_sum == 4.0


# ---------------------------------------------------------------- 2. the single table's floors
_worst = {"fp64": 0.0, "fp32": 0.0}


def _rel_err(got, ref):
    big = np.abs(ref) >= 1e-6
    return float(np.max(np.abs(got - ref)[big] / np.abs(ref[big]))) if big.any() else 0.0


def _bound_use(got, ref):
    return float(np.max(np.abs(got - ref) / (ATOL + RTOL * np.abs(ref)), initial=0.0))


def _run3(cfg, batches, ids, w, V, wire):
    ctx = _ctx(cfg["F"], cfg["k"], 3, wire=wire)
    ctx.load_tables(ids, w, V)
    dbs = [ctx.batch(to_host(c)) for c in batches]
    outs = []
    for t, b in enumerate(dbs, start=1):
        b.prepare()
        outs.append(ctx.step_batch(b, t, cfg["step"], cfg["reg"]))
    tabs = ctx.export_tables()
    pred = ctx.predict(to_host(batches[0]), -2.0, 3.0)
    ctx.close()
    return outs, tabs, pred


@pytest.mark.parametrize("case", range(40))
def test_fuzz_three_ranks_within_single_table_bounds(gpu, case):
    """The fuzz problems of test_gpu_fuzz.py on three sharded ranks with the fp64 wire: three steps,
    then transform of the first batch, inside the bounds the single-table paths are held to there --
    tables rtol 1e-5 / atol 1e-8 without the 4-ulp floor, predict atol 1e-7 without the score-terms
    term.  What is left between the two is fp64 summation order.  Prints (run with -s) the largest
    relative table error over values >= 1e-6 for this wire and for the fp32 wire on the same case,
    and the running maxima."""
    cfg, batches, ids, w, V = draw(2027 + case)
    model = R_.Model.empty(cfg["F"], cfg["k"])
    model.load(ids, w, V)
    ref = [R_.sgd_step_fast(model, c, t, cfg["step"], cfg["reg"]) for t, c in enumerate(batches, start=1)]
    pids = np.nonzero(model.present)[0]
    outs, (gids, gw, gV), pred = _run3(cfg, batches, ids, w, V, "fp64")
    _, (_, fw, fV), _ = _run3(cfg, batches, ids, w, V, "fp32")
    e64 = max(_rel_err(gw, model.w[pids]), _rel_err(gV, model.V[pids]))
    e32 = max(_rel_err(fw, model.w[pids]), _rel_err(fV, model.V[pids]))
    a64 = max(float(np.max(np.abs(gw - model.w[pids]), initial=0.0)), float(np.max(np.abs(gV - model.V[pids]), initial=0.0)))
    a32 = max(float(np.max(np.abs(fw - model.w[pids]), initial=0.0)), float(np.max(np.abs(fV - model.V[pids]), initial=0.0)))
    # the largest error in units of the single table's bound atol + rtol |ref| (<= 1 passes below)
    u64 = max(_bound_use(gw, model.w[pids]), _bound_use(gV, model.V[pids]))
    u32 = max(_bound_use(fw, model.w[pids]), _bound_use(fV, model.V[pids]))
    _worst["fp64"], _worst["fp32"] = max(_worst["fp64"], e64), max(_worst["fp32"], e32)
    print(f"\ncase {case}: max rel table err (|ref| >= 1e-6) fp64 wire {e64:.3g}, fp32 wire {e32:.3g}; max abs err "
          f"fp64 {a64:.3g}, fp32 {a32:.3g}; of the bound fp64 {u64:.3g}, fp32 {u32:.3g}; so far max rel fp64 "
          f"{_worst['fp64']:.3g}, fp32 {_worst['fp32']:.3g}")
    for o, r in zip(outs, ref):
        assert o.executed == r.executed, cfg
        if r.executed:
            assert (o.n_rows, o.n_loss_rows, o.n_unique) == (r.n_rows, r.n_loss_rows, r.n_unique), cfg
            assert o.loss_sum == pytest.approx(r.loss_sum, rel=RTOL, abs=1e-9), cfg
    np.testing.assert_array_equal(gids, pids, err_msg=str(cfg))
    np.testing.assert_allclose(gw, model.w[pids], rtol=RTOL, atol=ATOL, err_msg=str(cfg))
    np.testing.assert_allclose(gV, model.V[pids], rtol=RTOL, atol=ATOL, err_msg=str(cfg))
    trained = R_.Model.empty(cfg["F"], cfg["k"])
    trained.load(gids, gw, gV)
    ref_pred = R_.predict(trained, batches[0], -2.0, 3.0, num_features=cfg["F"])
    np.testing.assert_allclose(pred, ref_pred, rtol=RTOL, atol=1e-7, err_msg=f"predict {cfg}")


# ---------------------------------------------------------------- 3. shapes
# k = 17: kp = 20, five quads on a team of eight; k = 40: 320-B partial rows, ten quads on a team of
# sixteen; R = 12: the combine's owner-by-owner variant (R <= 8 keeps the pair slots in registers)
@pytest.mark.parametrize("R,k,F,hot,transport", [
    (1, 8, 503, 11, "copy"), (2, 1, 503, 11, "copy"), (3, 13, 401, 7, "copy"), (4, 16, 513, 512, "copy"),
    (4, 17, 513, 512, "copy"), (8, 40, 1031, 1030, "copy"), (12, 8, 1031, 1030, "copy"), (1, 16, 300, 2, "rccl"),
])
def test_sharded_step_and_predict_match_oracle(gpu, R, k, F, hot, transport):
    _, ids, w, V = make_problem(3, 1, F, k, 1)
    ctx = _ctx(F, k, R, transport=transport)
    ctx.load_tables(ids, w, V)
    model = R_.Model.empty(F, k)
    model.load(ids, w, V)
    probs = [make_problem(40 + t, 150 + 13 * t, F, k, 9, hot=hot)[0] for t in range(1, 5)]
    for t in (1, 2):  # host CSRs
        o = ctx.step(to_host(probs[t - 1]), t, 0.3, 1e-4)
        ref = R_.sgd_step_fast(model, probs[t - 1], t, 0.3, 1e-4)
        assert o.loss_sum == pytest.approx(ref.loss_sum, rel=RTOL)
        assert (o.n_rows, o.n_loss_rows, o.n_unique) == (ref.n_rows, ref.n_loss_rows, ref.n_unique)
    bs = [ctx.batch(to_host(p)) for p in probs[2:]]
    bs[0].prepare()
    for t in (3, 4):  # device batches, the next one prepared behind the step
        o = ctx.step_batch(bs[t - 3], t, 0.3, 1e-4, sync=True)
        if t == 3:
            bs[1].prepare()
        ref = R_.sgd_step_fast(model, probs[t - 1], t, 0.3, 1e-4)
        assert o.loss_sum == pytest.approx(ref.loss_sum, rel=RTOL)
        assert o.n_unique == ref.n_unique
    _check_tables(ctx, model)
    got = ctx.predict(to_host(probs[0]), 0.0, 1.0)
    np.testing.assert_allclose(got, R_.predict(model, probs[0], 0.0, 1.0, num_features=F), rtol=RTOL, atol=1e-7)
    ctx.close()


@pytest.mark.parametrize("chunks", [1, 3, 16])
def test_exchange_chunks(gpu, chunks):
    """The chunked partial pass with the wide store: a 7-row batch over R = 4 leaves chunks without pairs."""
    F, k, R = 257, 8, 4
    _, ids, w, V = make_problem(21, 1, F, k, 1)
    ctx = _ctx(F, k, R, xchg_chunks=chunks)
    ctx.load_tables(ids, w, V)
    model = R_.Model.empty(F, k)
    model.load(ids, w, V)
    for t, rows in ((1, 90), (2, 7), (3, 140)):
        p = make_problem(60 + t, rows, F, k, 6, hot=3)[0]
        o = ctx.step(to_host(p), t, 0.3, 1e-4)
        ref = R_.sgd_step_fast(model, p, t, 0.3, 1e-4)
        assert o.loss_sum == pytest.approx(ref.loss_sum, rel=RTOL)
        assert o.n_unique == ref.n_unique
    _check_tables(ctx, model)
    ctx.close()


def test_empty_part_and_empty_rows(gpu):
    """Two rows over three ranks (one rank gets none), an empty global batch, and rows without entries."""
    F, k, R = 97, 4, 3
    _, ids, w, V = make_problem(8, 1, F, k, 1)
    ctx = _ctx(F, k, R)
    ctx.load_tables(ids, w, V)
    model = R_.Model.empty(F, k)
    model.load(ids, w, V)
    empty = R_.CSR(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0), np.zeros(0))
    o = ctx.step(to_host(empty), 1, 0.3, 1e-4)
    assert not o.executed and ctx.epoch == 0
    two = make_problem(9, 2, F, k, 5, empty_frac=0.0)[0]
    o = ctx.step(to_host(two), 1, 0.3, 1e-4)
    ref = R_.sgd_step_fast(model, two, 1, 0.3, 1e-4)
    assert o.loss_sum == pytest.approx(ref.loss_sum, rel=RTOL)
    p = make_problem(10, 60, F, k, 5, hot=3, empty_frac=0.3)[0]
    o = ctx.step(to_host(p), 2, 0.3, 1e-4)
    ref = R_.sgd_step_fast(model, p, 2, 0.3, 1e-4)
    assert o.loss_sum == pytest.approx(ref.loss_sum, rel=RTOL) and o.n_rows == p.n_rows
    assert o.n_loss_rows == ref.n_loss_rows
    _check_tables(ctx, model)
    ctx.close()


@pytest.mark.parametrize("R", [1, 3, 4])
def test_predict_drops_outside_and_absent_ids(gpu, R):
    """transform with the wide combine: ids >= F and ids absent from the model drop out, a row left
    without a learned feature scores w0 unclamped."""
    F, k, w0 = 211, 8, 0.25
    _, _, w, V = make_problem(5, 1, F, k, 1)
    present = np.sort(np.random.default_rng(1).choice(F, size=150, replace=False)).astype(np.int32)
    ctx = _ctx(F, k, R, w0=w0)
    ctx.load_tables(present, w[present], V[present])
    model = R_.Model.empty(F, k, w0=w0)
    model.load(present, w[present], V[present])
    p = make_problem(6, 300, F + 40, k, 6, empty_frac=0.15)[0]
    lone = np.nonzero(~np.isin(np.arange(F), present))[0][:3]
    rp = np.concatenate([p.row_ptr, [p.row_ptr[-1] + len(lone)]]).astype(np.int64)
    csr = R_.CSR(rp, np.concatenate([p.col, lone]).astype(np.int32), np.concatenate([p.val, np.ones(len(lone))]),
                 np.concatenate([p.label, [0.0]]))
    for lo, hi in ((0.0, 1.0), (-math.inf, math.inf)):
        got = ctx.predict(to_host(csr), lo, hi)
        np.testing.assert_allclose(got, R_.predict(model, csr, lo, hi, num_features=F), rtol=RTOL, atol=1e-7)
    assert got[-1] == w0
    ctx.close()


def _split_pairs(buf, counts, kp):
    """A pair buffer in the wire layout ([P][kp] vectors, then [P][2] scalars) cut per peer."""
    import torch

    counts = [int(c) for c in counts]
    P = sum(counts)
    return list(zip(torch.split(buf[: P * kp], [c * kp for c in counts]),
                    torch.split(buf[P * kp:], [c * 2 for c in counts])))


def _cat_pairs(parts):
    import torch

    return torch.cat([v for v, _ in parts] + [s for _, s in parts])


def _phase_step(engines, batches, t, step_size, reg):
    """One iteration through the fm_shard_* phases, the all-to-alls done by slicing on the host side."""
    import torch

    R, kp = len(engines), engines[0].kp
    routed = [e.route(b) for e, b in zip(engines, batches)]
    ent_cnt = [c[:R] for _, _, c in routed]
    pair_cnt = [c[R:] for _, _, c in routed]
    torch.cuda.synchronize()
    keep = []
    for o in range(R):
        slots = torch.cat([torch.split(routed[r][0], ent_cnt[r].tolist())[o] for r in range(R)])
        ents = torch.cat([torch.split(routed[r][1], (2 * ent_cnt[r]).tolist())[o] for r in range(R)])
        src_p = np.array([pair_cnt[r][o] for r in range(R)])
        engines[o].owner_prepare(batches[o], slots, ents, np.array([ent_cnt[r][o] for r in range(R)]), src_p)
        keep.append((slots, ents, src_p))
    torch.cuda.synchronize()
    partials = []
    for o in range(R):
        out = engines[o].owner_forward(batches[o], int(keep[o][2].sum()))
        assert out.dtype == torch.float64  # the partial direction's words
        partials.append(_split_pairs(out, keep[o][2], kp))
    s_rows = []
    for r in range(R):
        s = engines[r].combine(batches[r], _cat_pairs([partials[o][r] for o in range(R)]), int(pair_cnt[r].sum()))
        assert s.dtype == torch.float32  # the S rows stay fp32
        s_rows.append(_split_pairs(s, pair_cnt[r], kp))
    gm = sum(int(b.n_rows) for b in batches)
    for o in range(R):
        engines[o].owner_update(batches[o], _cat_pairs([s_rows[r][o] for r in range(R)]), t, step_size, reg, gm)
    torch.cuda.synchronize()
    return sum(e.last_stats()[0] for e in engines), sum(e.last_stats()[2] for e in engines)


def test_manual_phases_match_single_table(gpu):
    """Three HipShardEngine(wire="fp64") contexts in one process (FM_PARALLEL_NONE, shard_index /
    shard_count, the context's own fm_config.wire), exchanged by slicing: against the single-table
    context on the concatenated batches, and both against the fp64 oracle."""
    from fm_spark_amd.distributed import HipShardEngine
    from fm_spark_amd.engine import FMContext

    R, k, F, hot = 3, 8, 503, 11
    _, ids, w, V = make_problem(3, 1, F, k, 1)
    engines = [HipShardEngine(F, k, r, R, wire="fp64") for r in range(R)]
    one = FMContext(F, k, fuse=False)
    for e in engines + [one]:
        e.load_tables(ids, w, V)
    model = R_.Model.empty(F, k)
    model.load(ids, w, V)
    for t in range(1, 4):
        parts = [make_problem(100 * t + r, 120 + 17 * r, F, k, 9, hot=hot)[0] for r in range(R)]
        offs = np.cumsum([0] + [p.nnz for p in parts])
        cat = R_.CSR(np.concatenate([np.zeros(1, np.int64)] + [p.row_ptr[1:] + o for p, o in zip(parts, offs)]),
                     np.concatenate([p.col for p in parts]), np.concatenate([p.val for p in parts]),
                     np.concatenate([p.label for p in parts]))
        bs = [e.batch(to_host(p)) for e, p in zip(engines, parts)]
        loss, nu = _phase_step(engines, bs, t, 0.3, 1e-4)
        so = one.step(to_host(cat), t, 0.3, 1e-4)
        ref = R_.sgd_step_fast(model, cat, t, 0.3, 1e-4)
        assert loss == pytest.approx(ref.loss_sum, rel=RTOL), f"step {t}"
        assert loss == pytest.approx(so.loss_sum, rel=1e-9), f"step {t}"
        assert nu == so.n_unique == ref.n_unique
    gi, gw, gV = (np.concatenate(x) for x in zip(*[e.export_tables() for e in engines]))
    order = np.argsort(gi)
    si, sw, sV = one.export_tables()
    np.testing.assert_array_equal(gi[order], si)
    np.testing.assert_allclose(gw[order], sw, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(gV[order], sV, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(gw[order], model.w[si], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(gV[order], model.V[si], rtol=RTOL, atol=ATOL)
    one.close()


class _SelfComm:
    """The collectives of a one-rank job (what ShardedTrainer calls on torch.distributed): like the
    real all-to-all, it does not convert between element types."""

    @staticmethod
    def all_reduce(t, group=None):
        pass

    @staticmethod
    def all_to_all_single(out, inp, output_split_sizes=None, input_split_sizes=None, group=None):
        assert out.dtype == inp.dtype and out.numel() == inp.numel()
        out.copy_(inp)


def test_sharded_trainer_sizes_its_partials_by_the_wire(gpu):
    """ShardedTrainer(wire="fp64"): the engine's partials and the trainer's receive buffer are float64,
    the S buffers float32; three steps (the third's batch prefetched) against the oracle."""
    import torch

    from fm_spark_amd.distributed import ShardedTrainer

    F, k = 300, 5
    _, ids, w, V = make_problem(4, 1, F, k, 1)
    tr = ShardedTrainer(F, k, rank=0, world=1, comm=_SelfComm, wire="fp64")
    assert tr.engine.wire_dtype == torch.float64 and tr.ctx.wire == "fp64"
    tr.load_tables(ids, w, V)
    model = R_.Model.empty(F, k)
    model.load(ids, w, V)
    probs = [make_problem(50 + t, 200, F, k, 8, hot=2)[0] for t in range(1, 4)]
    bs = [tr.batch(to_host(p)) for p in probs]
    for t in range(1, 4):
        o = tr.step(bs[t - 1], t, 0.2, 1e-5, prefetch=bs[t] if t == 2 else None)
        ref = R_.sgd_step_fast(model, probs[t - 1], t, 0.2, 1e-5)
        assert o.loss_sum == pytest.approx(ref.loss_sum, rel=RTOL)
        assert o.n_unique == ref.n_unique
    gi, gw, gV = tr.export_tables()
    np.testing.assert_array_equal(gi, np.nonzero(model.present)[0])
    np.testing.assert_allclose(gw, model.w[gi], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(gV, model.V[gi], rtol=RTOL, atol=ATOL)


def test_estimator_keeps_the_wire(gpu):
    """setParallel(..., wire="fp64"): the fitted model's context carries the wire, so transform uses
    it too; the model and its predictions are the single-table fit's."""
    from fm_spark_amd.data import synthetic_batch
    from fm_spark_amd.linalg import SparseVector
    from fm_spark_amd.ml import DataFrame, FactorizationMachinesSGD

    b = synthetic_batch(600, 2000, batch_index=11)
    vecs = [SparseVector(2000, b.col[b.row_ptr[i]:b.row_ptr[i + 1]], b.val[b.row_ptr[i]:b.row_ptr[i + 1]])
            for i in range(b.n_rows)]
    df = DataFrame({"label": [float(y) for y in b.label], "features": vecs}, [300, 300])

    def est():
        return (FactorizationMachinesSGD().setDimFactorization(5).setMaxIter(3).setStepSize(0.5).setRegParam(1e-5)
                .setNumFeatures(2000).setSeed(9))

    single = est().fit(df)
    multi = est().setParallel("sharded", n_gpus=3, devices=[0, 0, 0], transport="copy", wire="fp64").fit(df)
    assert multi._ctx.wire == "fp64" and single._ctx.wire == "fp32"
    i1, w1, V1 = single._ctx.export_tables()
    i2, w2, V2 = multi._ctx.export_tables()
    np.testing.assert_array_equal(i2, i1)
    np.testing.assert_allclose(w2, w1, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(V2, V1, rtol=RTOL, atol=ATOL)
    p1 = [r["prediction"] for r in single.transform(df).collect()]
    p2 = [r["prediction"] for r in multi.transform(df).collect()]
    np.testing.assert_allclose(p2, p1, rtol=RTOL, atol=1e-7)
    with pytest.raises(ValueError):
        est().setParallel("sharded", n_gpus=3, wire="fp16")


# ---------------------------------------------------------------- 4. contract
def _three_steps(F, k, ids, w, V, probs, **kw):
    from fm_spark_amd.engine import FMContext

    ctx = FMContext(F, k, **kw)
    ctx.load_tables(ids, w, V)
    for t, p in enumerate(probs, start=1):
        ctx.step(to_host(p), t, 0.3, 1e-4)
    out = (ctx.export_tables(), ctx.loss_history())
    ctx.close()
    return out


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1])


def test_fp64_wire_is_deterministic(gpu):
    F, k = 401, 8
    _, ids, w, V = make_problem(17, 1, F, k, 1)
    probs = [make_problem(70 + t, 200, F, k, 8, hot=5)[0] for t in range(3)]
    kw = dict(parallel="sharded", n_gpus=3, devices=[0] * 3, transport="copy", wire="fp64")
    a, b = _three_steps(F, k, ids, w, V, probs, **kw), _three_steps(F, k, ids, w, V, probs, **kw)
    assert len(a[1]) == 3 and _same(a, b)


def test_default_wire_is_fp32(gpu):
    """fm_config.wire left at 0 and FM_WIRE_FP32 given explicitly: the same tables and losses bit for bit."""
    from fm_spark_amd import _native as N

    assert N.FM_WIRE_FP32 == 0 and N.FM_WIRE_FP64 == 1
    F, k = 401, 8
    _, ids, w, V = make_problem(17, 1, F, k, 1)
    probs = [make_problem(70 + t, 200, F, k, 8, hot=5)[0] for t in range(3)]
    kw = dict(parallel="sharded", n_gpus=3, devices=[0] * 3, transport="copy")
    assert _same(_three_steps(F, k, ids, w, V, probs, **kw), _three_steps(F, k, ids, w, V, probs, wire="fp32", **kw))


def test_single_table_ignores_wire(gpu):
    """A context that exchanges nothing accepts the field and steps bit for bit as without it."""
    F, k = 401, 8
    _, ids, w, V = make_problem(17, 1, F, k, 1)
    probs = [make_problem(70 + t, 200, F, k, 8, hot=5)[0] for t in range(3)]
    assert _same(_three_steps(F, k, ids, w, V, probs), _three_steps(F, k, ids, w, V, probs, wire="fp64"))


def test_create_refuses_bad_wire(gpu):
    from fm_spark_amd import _native as N
    from fm_spark_amd.engine import FMContext

    lib = N.load()
    cfg = N.fm_config(num_features=100, k=4, shard_count=1, wire=2)
    h = C.c_void_p()
    assert lib.fm_create(C.byref(cfg), C.byref(h)) == -1  # FM_ERR_ARG
    assert b"wire" in lib.fm_last_error() and not h
    with pytest.raises(N.FMError, match=r"\(-1\).*wire.*replicated"):
        FMContext(100, 4, parallel="replicated", n_gpus=2, devices=[0, 0], transport="copy", wire="fp64")
    with pytest.raises(ValueError):
        FMContext(100, 4, wire="fp16")


def test_config_wire_offset_matches_c(gpu, tmp_path):
    """fm_config.wire sits where the C compiler puts it (the struct's size is test_capi.py's check)."""
    from fm_spark_amd import _native as N

    header = Path(__file__).resolve().parents[1] / "include"
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fm_hip.h"\n'
                   'int main(void){printf("%zu %zu %d %d\\n", sizeof(fm_config), offsetof(fm_config, wire), '
                   'FM_WIRE_FP32, FM_WIRE_FP64);return 0;}\n')
    exe = tmp_path / "off"
    subprocess.run(["gcc", f"-I{header}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(N.fm_config), N.fm_config.wire.offset, N.FM_WIRE_FP32, N.FM_WIRE_FP64]
    assert N.fm_config.wire.offset == N.fm_config.xchg_chunks.offset + 4
