"""GPU: the sharded step's own kernels (csrc/fm_shard.hip), phase by phase, each against the NumPy
reference of the same phase (tests/shard_ref_engine.py) -- where test_gpu_shard.py and test_gpu_group.py
see them only through whole steps on random problems of a few hundred rows and R <= 12.

One context acts as one rank of R (a route reads no table and a combine no peer, so R = 64 costs what
R = 3 costs).  The cases and the conditions that show which tile, wave, trip, sweep or source boundary each
crosses are tests/shard_cases.py's, sized from the library's own geometry (tests/shard_probe.py) and checked
without a GPU by tests/test_shard_phases_cpu.py; every test here asserts its case's conditions again before
it runs.

A. route: counts, send_slot and both words of send_ent, integers, `==`.
B. owner_prepare + owner_forward on received buffers taken from the reference's route (so a failure does not
   depend on A): every partial word within the bound of its arithmetic (partial_bound).
C. combine on hand-made partials that name their (owner, pair): the S rows `==`, {r, yhat} within
   scalar_bound.  Every k_shard_combine<GS, OW, W> the library can launch.
D. whole steps of simulated ranks against the oracle where only a whole step reaches the path: the combine's
   second grid-stride sweep (its loss partials accumulate across sweeps), k_pack_srec's second sweep, the
   masks' high half through a step, at R = 64.

fm_batch_create refuses an id >= num_features, and the manual phases take no other batch, so a route with
such ids is reachable through a group context's predict alone (R <= 16: tests/test_gpu_group.py); the
reference's rule for them is pinned on the CPU.

The largest observed error / bound ratio of B and C is printed by each test (run with -s); it sets no bound.
"""

import numpy as np
import pytest

import shard_cases as sc
from oracle import fm_ref as R_
from problems import make_rows
from shard_ref_engine import NpBatch, NumpyShardEngine
from shard_sim import simulated_step

pytestmark = pytest.mark.gpu

L = np.longdouble
RTOL, ATOL = 1e-5, 1e-8  # the project's whole-step tolerance: no bound here may be looser


def _geom(k=sc.K_ROUTE):
    import shard_probe

    return shard_probe.geometry(k)


def _host(c):
    from fm_spark_amd._native import CSRHost

    return CSRHost(c.row_ptr, c.col, c.val, c.label)


def _engine(F, k, rank, R, **kw):
    from fm_spark_amd.distributed import HipShardEngine

    return HipShardEngine(F, k, rank, R, **kw)


def _assert_edges(case):
    assert case.edges, case.name
    for what, ok in case.edges:
        assert ok, f"{case.name}: {what}"


# ------------------------------------------------------------------------------------------ A. route
def _route(eng, b):
    import torch

    slot, ent, counts = eng.route(b)
    torch.cuda.synchronize()
    return slot.cpu().numpy(), ent.cpu().numpy().view(np.uint32).reshape(-1, 2), counts


def _check_route(case, twice=False):
    R = case.R
    ref = NumpyShardEngine(case.F, sc.K_ROUTE, 0, R)
    rs, re, rc = ref.route(NpBatch(case.csr))
    rs, re = rs.numpy(), re.numpy().view(np.uint32).reshape(-1, 2)
    eng = _engine(case.F, sc.K_ROUTE, 0, R)
    try:
        b = eng.batch(_host(case.csr))
        slot, ent, counts = _route(eng, b)
        np.testing.assert_array_equal(counts, rc)
        n = int(rc[:R].sum())
        assert n == case.csr.nnz == len(rs)
        np.testing.assert_array_equal(slot[:n], rs)
        np.testing.assert_array_equal(ent[:n, 0], re[:, 0], err_msg="pair index of an entry")
        np.testing.assert_array_equal(ent[:n, 1], re[:, 1], err_msg="x bits of an entry")
        if twice:
            slot2, ent2, counts2 = _route(eng, b)
            np.testing.assert_array_equal(counts2, counts)
            np.testing.assert_array_equal(slot2[:n], slot[:n])
            np.testing.assert_array_equal(ent2[:n], ent[:n])
    finally:
        eng.ctx.close()


@pytest.mark.parametrize("name", sc.ROUTE_NAMES)
def test_route_matches_reference(gpu, name):
    case = sc.route_cases(_geom())[name]()
    _assert_edges(case)
    _check_route(case, twice=name in ("rows_2T+1_Rmax", "owners_Rmax", "coprime5_R3"))


@pytest.mark.parametrize("R", [3, 64])
def test_route_large_matches_reference(gpu, R):
    """A second k_sample_mask sweep, a second k_rows_scan trip and k_route_keys' unrolled entries: each
    condition asserted from the geometry (shard_cases.large_route_case)."""
    case = sc.large_route_case(_geom(), R)
    _assert_edges(case)
    _check_route(case, twice=R == 64)


# ------------------------------------------------------------------------------------------ B. owner
def partial_bound(ref, aref, n, wide):
    """The bound on a partial word of a pair of n entries, against the exact value ref whose terms' absolute
    values sum to aref: (n + 2) 2^-52 aref for the reordered fp64 sum, and 2^-24 |ref| for the fp32 wire's one
    rounding.  k_forward's partial pass forms no product in fp32: v x and w x are exact in fp64 (24-bit
    factors), v^2 x^2 = (the lane's four squares, exact, summed: 3 roundings) * x * x (2 roundings), so a term
    carries at most 5 units of 2^-53 before it is added; any order of the at most n GS terms then adds the depth
    of the sum, at most n - 1 adds of a lane's serial walk and the tree over its team.  At kp <= 8 (the k this
    family uses: GS <= 2) that is 5 + (n - 1) + 1 <= 2 n + 4 units for every n >= 1, which is the bound."""
    b = (n[:, None].astype(L) + 2) * L(2.0) ** -52 * aref
    if not wide:
        b = b + L(2.0) ** -24 * np.abs(ref)
    return b


def _to_dev(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.cuda()


def _owner_run(eng, b, slots, ents, se, sp):
    import torch

    rs, re = _to_dev(slots.astype(np.int32)), _to_dev(ents.view(np.int32).reshape(-1))
    torch.cuda.synchronize()  # owner_prepare runs on the side stream
    eng.owner_prepare(b, rs, re, se, sp)
    P = int(sp.sum())
    out = eng.owner_forward(b, P)
    torch.cuda.synchronize()
    flat = out.cpu().numpy()
    kp = eng.kp
    return flat[: P * kp].reshape(P, kp), flat[P * kp:].reshape(P, 2), (rs, re)


def _check_owner(case, wire):
    wide = wire == "fp64"
    slots, ents, se, sp = sc.received(case)
    ref = NumpyShardEngine(case.F, case.k, case.owner, case.R)
    ref.load_tables(case.ids, case.w, case.V)
    vec, scl, avec, asc, n = ref.owner_forward_exact(slots, ents, se, sp)
    eng = _engine(case.F, case.k, case.owner, case.R, wire=wire)
    try:
        eng.load_tables(case.ids, case.w, case.V)
        b = eng.batch(_host(sc._empty_csr()))
        gv, gs, keep = _owner_run(eng, b, slots, ents, se, sp)
        assert gv.dtype == (np.float64 if wide else np.float32) and gv.shape == vec.shape and gs.shape == scl.shape
        worst = 0.0
        for got, want, mag in ((gv, vec, avec), (gs, scl, asc)):
            bound = partial_bound(want, mag, n, wide)
            assert (bound <= ATOL + RTOL * np.abs(want)).all()
            err = np.abs(got.astype(L) - want)
            bad = err > bound
            assert not bad.any(), (f"{case.name} {wire}: {int(bad.sum())} words beyond their bound, first at "
                                   f"{tuple(np.argwhere(bad)[0])}: got {got[bad][0]!r}, want {want[bad][0]!r}")
            if err.size:
                worst = max(worst, float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0))))
        assert (gv[:, case.k:] == 0).all()  # the padding columns
        print(f"owner {case.name} {wire}: largest error / bound = {worst:.3f}")
        return eng, b
    except BaseException:
        eng.ctx.close()
        raise


@pytest.mark.parametrize("wire", ["fp32", "fp64"])
@pytest.mark.parametrize("name", sc.OWNER_NAMES)
def test_owner_partials_match_reference(gpu, name, wire):
    case = sc.owner_cases(_geom())[name]()
    _assert_edges(case)
    eng, _ = _check_owner(case, wire)
    eng.ctx.close()


@pytest.mark.parametrize("wire", ["fp32", "fp64"])
def test_owner_large_matches_reference(gpu, wire):
    """More received entries than one k_pair_table sweep takes: its unrolled entries (u >= 1) open pairs too."""
    case = sc.large_owner_case(_geom())
    _assert_edges(case)
    eng, _ = _check_owner(case, wire)
    eng.ctx.close()


def test_owner_prepare_refuses_bad_counts(gpu):
    """FM_ERR_ARG and nothing enqueued: more pairs than entries at a source, entries without a pair, counts
    that do not add up to n -- and the context serves a good call right after."""
    from fm_spark_amd._native import FMError

    case = sc.owner_cases(_geom())["random_R3_k8"]()
    slots, ents, se, sp = sc.received(case)
    eng, b = _check_owner(case, "fp32")
    try:
        rs, re = _to_dev(slots.astype(np.int32)), _to_dev(ents.view(np.int32).reshape(-1))
        more_pairs, no_pair, short = sp.copy(), sp.copy(), se.copy()
        more_pairs[1] = se[1] + 1
        no_pair[2] = 0
        short[0] -= 1
        assert se[2] > 0
        for bad_se, bad_sp in ((se, more_pairs), (se, no_pair), (short, sp)):
            with pytest.raises(FMError, match=r"\(-1\)"):
                eng.owner_prepare(b, rs, re, bad_se, bad_sp)
        gv, gs, _ = _owner_run(eng, b, slots, ents, se, sp)
        ref = NumpyShardEngine(case.F, case.k, case.owner, case.R)
        ref.load_tables(case.ids, case.w, case.V)
        vec, scl, avec, asc, n = ref.owner_forward_exact(slots, ents, se, sp)
        assert (np.abs(gv.astype(L) - vec) <= partial_bound(vec, avec, n, False)).all()
        assert (np.abs(gs.astype(L) - scl) <= partial_bound(scl, asc, n, False)).all()
    finally:
        eng.ctx.close()


# ------------------------------------------------------------------------------------------ C. combine
def scalar_bound(ref, kp, R, w0, value):
    """{r, yhat}: (kp + R + 6) 2^-53 (sum a^2 + sum |vv_o| + sum |wx_o| + |w0|) for the fp64 arithmetic (kp
    squares and their sum, R adds per scalar, the last four operations and r's subtraction), and 2^-24 |value|
    for the one rounding to the fp32 word."""
    return (kp + R + 6) * L(2.0) ** -53 * (ref.sum_a2 + ref.abs_vv + ref.abs_wx + abs(w0)) + L(2.0) ** -24 * np.abs(value)


@pytest.mark.parametrize("wire", ["fp32", "fp64"])
@pytest.mark.parametrize("R", sc.COMBINE_R)
@pytest.mark.parametrize("k", sc.COMBINE_K)
def test_combine_matches_reference(gpu, k, R, wire):
    """S rows: fp64 adds in owner order and one rounding, so `==`, and every pair of a sample gets the same
    row.  {r, yhat} within scalar_bound, with w0 != 0 and fp64 labels next to yhat, which an r formed from
    fp32 operands misses by orders of magnitude."""
    import torch

    wide, w0 = wire == "fp64", 0.3
    g = _geom(k)
    kp = (k + 3) // 4 * 4
    csr, F = sc.combine_batch(R)
    ref = NumpyShardEngine(F, k, 0, R, w0=w0)
    nb = NpBatch(csr)
    _, _, counts = ref.route(nb)
    vec, scl = sc.tagged_partials(counts[R:], kp, wide)
    y = sc.near_labels(ref.combine_exact(nb, vec, scl).yhat, k + R)
    want = ref.combine_exact(nb, vec, scl, label=y)
    csr = R_.CSR(csr.row_ptr, csr.col, csr.val, y)
    assert (y.astype(np.float32) != y).all()
    if k == max(sc.COMBINE_K):
        assert kp // 4 > g.combine_team  # a lane takes a second quad
    eng = _engine(F, k, 0, R, wire=wire, w0=w0)
    try:
        b = eng.batch(_host(csr))
        _, _, got_counts = _route(eng, b)
        np.testing.assert_array_equal(got_counts, counts)
        Ps = int(counts[R:].sum())
        pin = _to_dev(np.concatenate([vec.reshape(-1), scl.reshape(-1)]))
        torch.cuda.synchronize()
        out = eng.combine(b, pin, Ps)
        torch.cuda.synchronize()
        flat = out.cpu().numpy()
        S, rs = flat[: Ps * kp].reshape(Ps, kp), flat[Ps * kp:].reshape(Ps, 2)
        ps = want.pair_sample
        assert (S == want.S[ps]).all(), f"S rows differ at pairs {np.nonzero((S != want.S[ps]).any(axis=1))[0][:8]}"
        worst = 0.0
        for col, exact in ((0, want.r), (1, want.yhat)):
            bound = scalar_bound(want, kp, R, w0, exact)[ps]
            err = np.abs(rs[:, col].astype(L) - exact[ps])
            assert (err <= bound).all(), (col, float(err.max()), np.nonzero(err > bound)[0][:8])
            worst = max(worst, float((err / bound).max()))
        print(f"combine k={k} R={R} {wire}: team {g.combine_team}, largest error / bound = {worst:.3f}")
    finally:
        eng.ctx.close()


# ------------------------------------------------------------------------------------------ D. whole steps
def _concat(parts):
    row_ptr, off = [np.zeros(1, np.int64)], 0
    for p in parts:
        row_ptr.append(p.row_ptr[1:] + off)
        off += p.nnz
    return R_.CSR(np.concatenate(row_ptr), np.concatenate([p.col for p in parts]), np.concatenate([p.val for p in parts]),
                  np.concatenate([p.label for p in parts]))


def _steps_match_oracle(R, k, F, parts_of, steps=2, wire="fp32"):
    """steps iterations of R simulated ranks against sgd_step_fast on the concatenation: loss_sum to rel 1e-5,
    counts `==`, tables to rtol 1e-5 / atol 1e-8 (as tests/test_gpu_shard.py).  -> pair counts of the last step."""
    _, ids, w, V = make_rows(3, [0], F, k)
    engines = [_engine(F, k, r, R, wire=wire) for r in range(R)]
    try:
        for e in engines:
            e.load_tables(ids, w, V)
        model = R_.Model.empty(F, k)
        model.load(ids, w, V)
        for t in range(1, steps + 1):
            parts = parts_of(t)
            bs = [e.batch(_host(p)) for e, p in zip(engines, parts)]
            pair_cnt = simulated_step(engines, bs, t, 0.3, 1e-4)
            cat = _concat(parts)
            ref = R_.sgd_step_fast(model, cat, t, 0.3, 1e-4)
            stats = [e.last_stats() for e in engines]
            assert sum(s[0] for s in stats) == pytest.approx(ref.loss_sum, rel=1e-5), f"step {t}"
            assert sum(s[1] for s in stats) == ref.n_loss_rows
            assert sum(s[2] for s in stats) == ref.n_unique == len(np.unique(cat.col))
        gi, gw, gV = zip(*[e.export_tables() for e in engines])
        gi = np.concatenate(gi)
        order = np.argsort(gi)
        np.testing.assert_array_equal(gi[order], np.nonzero(model.present)[0])
        np.testing.assert_allclose(np.concatenate(gw)[order], model.w[gi[order]], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(np.concatenate(gV)[order], model.V[gi[order]], rtol=RTOL, atol=ATOL)
        return np.asarray(pair_cnt)
    finally:
        for e in engines:
            e.ctx.close()


def test_step_combine_second_sweep(gpu):
    """R = 2, k = 33: more rows on a rank than one sweep of the combine takes at its widest team, so every
    block's loss partial accumulates over two sweeps."""
    R, k, F = 2, 33, 2 * 2048 + 1
    g = _geom(k)
    rows = int(g.combine_sweep) + 17
    assert g.combine_team == 16 and rows > g.combine_sweep

    def parts_of(t):
        rng = np.random.default_rng(t)
        has = np.stack([rng.integers(0, 3, rows), rng.integers(0, 2, rows)], axis=1)  # 0..3 entries a row
        return [sc.by_owner(10 * t + r, has, R, slots=2048)[0] for r in range(R)]

    _steps_match_oracle(R, k, F, parts_of)


def test_step_pack_second_sweep(gpu):
    """R = 2, k = 16: more pairs at owner 0 than one sweep of k_pack_srec takes (asserted from the counts).
    The rows per rank follow from the geometry: half a pack sweep and a few, every row with an entry of owner 0."""
    R, k, F = 2, 16, 2 * 2048 + 1
    g = _geom(k)
    assert g.pack_sweep > 0
    rows = int(g.pack_sweep) // R + 17

    def parts_of(t):
        rng = np.random.default_rng(t)
        has = np.stack([rng.integers(1, 3, rows), rng.integers(0, 2, rows)], axis=1)  # 1..3 entries a row
        return [sc.by_owner(20 * t + r, has, R, slots=2048)[0] for r in range(R)]

    pair_cnt = _steps_match_oracle(R, k, F, parts_of)
    assert pair_cnt[:, 0].sum() > g.pack_sweep  # the pairs owner 0 received


def test_step_r64(gpu):
    """R = 64, k = 8, 257 rows per rank, F = 4099: the owner masks' high half, the owner-by-owner combine and
    64 sources at every owner, through two whole steps."""
    R, k, F = 64, 8, 4099
    assert R == _geom(k).max_r

    def parts_of(t):
        return [sc.by_owner(1000 * t + r, sc.random_has(7 * t + r, 257, R), R, slots=64, F=F)[0] for r in range(R)]

    _steps_match_oracle(R, k, F, parts_of)
