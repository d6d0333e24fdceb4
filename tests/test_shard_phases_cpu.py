"""CPU: the reference of the sharded phases (tests/shard_ref_engine.py) and the cases of
tests/test_gpu_shard_phases.py (tests/shard_cases.py), with no GPU and no kernel.

The reference against itself and against a direct fp64 FM forward: route with ids outside the model equals
route without those entries; route -> owner_forward -> combine chained over all R ranks (the all-to-alls
by slicing) gives every sample's S and yhat.  Then every case builder: the edge a case is named for, as a
condition on the case and the geometry (listed by the builder, asserted here and again by the GPU test
before it runs):

    case                  crosses                                         condition
    rows_<n>_R<r>         the pair tile / the wave of the pair numbering  n in {1, W-1, W, W+1, T-1, T, T+1, 2T+1}
    lengths_R<r>          a route team's trips                            rows of 0, 1, t-1, t, t+1, 2t+1 entries
    owners_Rmax           the owner mask's halves                         rows of all owners, of 63, 32, 31 alone, of none
    coprime<p>_R<r>       ballots that differ from wave to wave           gcd(p, 64) = 1 and neighbouring waves differ
    topslot_R<r>          the slot bits of the route key                  F = R 2^s + 1 and id F - 1 is routed
    F<f>_R<r>             owners without a feature                        F < R, nothing for owners >= F
    large_R<r>            k_sample_mask's second sweep, k_rows_scan's     B > mask_sweep, tiles > scan_trip,
                          second trip, k_route_keys' unrolled entries     nnz > route_sweep
    empty_*/all_but_one   a source without entries (k_pair_table's walk)  src_entries[r] = 0 where named
    one_each_R<r>         pairs opened by i == so[r] alone                every source: one pair, local index 0
    pairs_1_and_300       a pair of one entry beside a long one           pair lengths {1, 300}
    large_R3 (owner)      k_pair_table's unrolled entries                 n > table_sweep

(T = pair_tile, W = 64, t = route_team.)  The geometry comes from the built library through
tests/shard_probe.py (a host call); where the probe has not been built, GEOM_AS_OF_WRITING stands in, and a
second, made-up geometry is always run, so the builders are shown to follow the geometry.
"""

import itertools

import numpy as np
import pytest
import torch

import shard_cases as sc
from shard_probe import Geometry
from shard_ref_engine import NpBatch, NumpyShardEngine, rows_to_soa, soa_to_rows

# fm_shard.hip as it was when this was written; only a stand-in for an unbuilt probe (the GPU tests never
# read it)
GEOM_AS_OF_WRITING = dict(pair_tile=256, route_team=16, mask_sweep=65536, scan_trip=256, route_sweep=1048576,
                          route_unroll=4, table_sweep=1048576, table_unroll=4, slot_regs=8, max_r=64)


def team_then(k):
    nq, G = (k + 3) // 4, 1
    while G < nq and G < 16:
        G <<= 1
    return G


def geom(k=4):
    try:
        import shard_probe

        return shard_probe.geometry(k)
    except (RuntimeError, OSError, ImportError):
        kp = (k + 3) // 4 * 4
        rec = (16 if kp + 2 <= 16 else 32) if kp <= 16 else 0
        return Geometry(**GEOM_AS_OF_WRITING, combine_team=team_then(k), combine_sweep=2048 * 256 // team_then(k),
                        pack_sweep=1048576 * 4 // rec if rec else 0)


def other_geom():
    """A geometry no build has: tiles of 128 samples, teams of 8 lanes, small sweeps."""
    return Geometry(128, 8, 2048, 16, 4096, 2, 8192, 2, 4, 64, 2, 4096, 1024)


def assert_edges(case):
    assert case.edges, case.name
    for what, ok in case.edges:
        assert ok, f"{case.name}: {what}"


# ------------------------------------------------------------------------------------- the reference
def direct_forward(csr, ids, w, V, F, k, w0):
    """Every sample's S and yhat by a direct fp64 FM forward (ids outside the model or absent from it dropped)."""
    Vt, wt = np.zeros((F, k)), np.zeros(F)
    Vt[ids], wt[ids] = V, w
    S, yhat = np.zeros((csr.n_rows, k)), np.full(csr.n_rows, w0)
    for s in range(csr.n_rows):
        e = slice(csr.row_ptr[s], csr.row_ptr[s + 1])
        col, x = csr.col[e].astype(np.int64), csr.val[e]
        col, x = col[col < F], x[col < F]
        vx = Vt[col] * x[:, None]
        S[s] = vx.sum(axis=0)
        yhat[s] += 0.5 * (np.sum(S[s] ** 2) - np.sum(vx * vx)) + np.sum(wt[col] * x)
    return S, yhat


@pytest.mark.parametrize("R", [1, 2, 3, 4, 64])
def test_route_drops_ids_outside_the_model(R):
    F = R * 64 + 1
    csr, _ = sc.by_owner(R, sc.random_has(R + 1, 150, R), R)
    csr2, out = sc.outside_ids(R + 2, csr, F)
    assert out.any() and (np.diff(csr2.row_ptr) > 0).sum() > (sc.masks(csr2, R, F).any(axis=1)).sum()  # rows wholly outside
    eng = NumpyShardEngine(F, 4, 0, R)
    a, b = NpBatch(csr2), NpBatch(sc.drop_entries(csr2, out))
    ra, rb = eng.route(a), eng.route(b)
    for x, y in zip(ra, rb):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    np.testing.assert_array_equal(a.pairidx, b.pairidx)
    np.testing.assert_array_equal(a.pairs_out, b.pairs_out)
    assert int(ra[2][:R].sum()) == int((~out).sum()) < csr2.nnz
    # and a batch without such ids routes as it did before the rule existed: owners by id % R, CSR order kept
    s, e, counts = eng.route(NpBatch(csr))
    order = np.argsort(csr.col % R, kind="stable")
    np.testing.assert_array_equal(s.numpy(), csr.col[order] // R)
    np.testing.assert_array_equal(counts[:R], np.bincount(csr.col % R, minlength=R))


@pytest.mark.parametrize("R,wide", [(3, False), (3, True), (64, False), (64, True)])
def test_chained_phases_give_the_direct_forward(R, wide):
    F, k, w0 = R * 16 + 1, 5, 0.3
    ids, w, V = sc._table(R, F, k)
    engines = [NumpyShardEngine(F, k, r, R, w0=w0) for r in range(R)]
    for e in engines:
        e.load_tables(ids, w, V)
    kp = engines[0].kp
    parts = [sc.outside_ids(50 + r, sc.combine_batch(R, seed=r)[0], F, frac=0.1)[0] for r in range(R)]
    parts = [p for p in parts[: min(R, 5)]] + [sc._empty_csr()] * max(0, R - 5)  # five ranks hold rows
    bs = [NpBatch(p) for p in parts]
    routed = [e.route(b) for e, b in zip(engines, bs)]
    ent_cnt = [c[:R] for _, _, c in routed]
    pair_cnt = [c[R:] for _, _, c in routed]
    vec_of, sc_of = {}, {}
    for o in range(R):
        slots = np.concatenate([np.split(routed[r][0].numpy(), np.cumsum(ent_cnt[r])[:-1])[o] for r in range(R)])
        ents = np.concatenate([np.split(routed[r][1].numpy().reshape(-1, 2), np.cumsum(ent_cnt[r])[:-1])[o] for r in range(R)])
        se, sp = [ent_cnt[r][o] for r in range(R)], [pair_cnt[r][o] for r in range(R)]
        vec, scl, avec, asc, n = engines[o].owner_forward_exact(slots, ents, se, sp)
        assert (avec >= np.abs(vec)).all() and (asc >= np.abs(scl)).all() and n.sum() == len(slots)
        word = np.float64 if wide else np.float32
        for r, (v, s2) in enumerate(zip(np.split(vec.astype(word), np.cumsum(sp)[:-1]), np.split(scl.astype(word), np.cumsum(sp)[:-1]))):
            vec_of[o, r], sc_of[o, r] = v, s2
    for r in range(min(R, 5)):
        vec = np.concatenate([vec_of[o, r] for o in range(R)])
        scl = np.concatenate([sc_of[o, r] for o in range(R)])
        ref = engines[r].combine_exact(bs[r], vec, scl)
        S, yhat = direct_forward(parts[r], ids, w, V, F, k, w0)
        tol = dict(rtol=1e-12, atol=1e-13) if wide else dict(rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(ref.S[:, :k], S, rtol=1e-5, atol=1e-6)  # S is fp32 either way
        np.testing.assert_allclose(ref.yhat.astype(np.float64), yhat, **tol)
        np.testing.assert_allclose(ref.r.astype(np.float64), yhat - parts[r].label, **tol)
        assert (ref.S[:, k:] == 0).all() and (ref.sum_a2 >= 0).all()
        np.testing.assert_array_equal(ref.has_pair, sc.masks(parts[r], R, F).any(axis=1))
        # the wire form of the same combine (what test_distributed_gloo.py drives) agrees
        if not wide:
            flat = engines[r].combine(bs[r], torch.from_numpy(rows_to_soa(np.concatenate([vec, scl], axis=1), kp)),
                                      int(pair_cnt[r].sum()))
            rows = soa_to_rows(flat.numpy(), kp)
            np.testing.assert_array_equal(rows[:, :kp].astype(np.float32), ref.S[ref.pair_sample])
            np.testing.assert_allclose(rows[:, kp + 1], ref.yhat[ref.pair_sample].astype(np.float64), rtol=1e-6)


def test_tagged_partials_name_their_row():
    for wide in (False, True):
        vec, s2 = sc.tagged_partials(np.array([5, 0, 7, 300]), 8, wide)
        rows = np.concatenate([vec, s2], axis=1)
        assert len(np.unique(rows, axis=0)) == len(rows) == 312
        assert (rows > 0).any() and (rows < 0).any() and np.abs(rows).max() / np.abs(rows).min() > 2 ** 20
        assert ((rows.astype(np.float32) == rows).all()) == (not wide)
    y = sc.near_labels(np.linspace(-3, 3, 11).astype(np.longdouble), 1)
    assert (y.astype(np.float32) != y).all()


# ------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize("g", [geom(), other_geom()], ids=["library", "made_up"])
def test_route_cases_cross_their_edges(g):
    cases = sc.route_cases(g)
    assert set(cases) == set(sc.ROUTE_NAMES) and len(sc.ROUTE_NAMES) == len(set(sc.ROUTE_NAMES))
    T = g.pair_tile
    assert {(c().csr.n_rows, c().R) for n, c in cases.items() if n.startswith("rows_")} == (
        {(B, R) for B in (1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1) for R in (3, g.max_r)} | {(T + 1, R) for R in sc.ROUTE_R})
    for name, build in cases.items():
        c = build()
        assert c.name == name and c.csr.col.max(initial=0) < c.F and 1 <= c.R <= g.max_r
        assert_edges(c)


def test_large_route_case_crosses_its_sweeps():
    g = geom()
    c = sc.large_route_case(g, 3)
    assert_edges(c)
    h = other_geom()
    assert_edges(sc.large_route_case(h, 64))


@pytest.mark.parametrize("g", [geom(), other_geom()], ids=["library", "made_up"])
def test_owner_cases_cross_their_edges(g):
    assert set(sc.owner_cases(g)) == set(sc.OWNER_NAMES)
    for name, build in sc.owner_cases(g).items():
        c = build()
        assert c.name == name and len(c.sources) == c.R
        assert_edges(c)
        slots, ents, se, sp = sc.received(c)
        assert (sp <= se).all() and ((se == 0) | (sp >= 1)).all() and se.sum() == len(slots)
        assert len(slots) == 0 or slots.max() < (c.F - c.owner + c.R - 1) // c.R


def test_large_owner_case_crosses_the_table_sweep():
    assert_edges(sc.large_owner_case(other_geom()))
    c = sc.large_owner_case(geom())
    assert_edges(c)
    assert sum(s.nnz for s in c.sources) > geom().table_sweep


def test_combine_cases_cover_every_instantiation():
    """k_shard_combine<GS, OW, W>: every team width the library picks, both ways of reaching the owners'
    rows, both wires -- and a kp whose quads outnumber the widest team."""
    teams = {geom(k).combine_team for k in range(1, 257)}
    got = {(geom(k).combine_team, R <= geom(k).slot_regs, wide) for k, R, wide in
           itertools.product(sc.COMBINE_K, sc.COMBINE_R, (False, True))}
    assert got == set(itertools.product(teams, (True, False), (False, True)))
    assert any((k + 3) // 4 > max(teams) for k in sc.COMBINE_K)
    assert max(sc.COMBINE_R) == geom().max_r
    for R in sc.COMBINE_R:
        csr, F = sc.combine_batch(R)
        m = sc.masks(csr, R, F)
        assert csr.n_rows == sc.COMBINE_B > geom().pair_tile
        assert (~m.any(axis=1)).any() and m.all(axis=1).any() and (m[:, R - 1] & (m.sum(axis=1) == 1)).any()
