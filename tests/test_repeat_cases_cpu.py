"""CPU: the cases of tests/test_gpu_repeated_ids.py (tests/repeat_cases.py) on the oracle alone.

A row may hold one feature id more than once; each occurrence is an entry of its own.  Every case is
built here as the GPU test builds it and must show, with no GPU: its second batch's sorted view is
the layout and holds the event the case is named for (runs.classify), a repeated id counts once in
n_unique, reading a row's repeats as one entry (x summed) or keeping only the first would each move
every designated row by at least 8 tolerances, and the oracle's two forms (sgd_step's per-entry dicts,
sgd_step_fast's np.add.at) agree.  The builders that existed before keep their bytes.

The geometry comes from the built library (tests/update_probe.py, a host call); where the probe has
not been built the stand-in of tests/test_runs_cpu.py serves, and a made-up geometry is always run.
"""

import hashlib

import numpy as np
import pytest

import repeat_cases as rc
import runs
from oracle import fm_ref as R
from problems import make_problem, make_rows
from test_runs_cpu import geom, other_geom

CASES = [(n, k) for n in rc.NAMES for k in rc.ks_of(n)]


@pytest.mark.parametrize("name,k", CASES)
def test_case_events_discriminators_and_oracles(name, k):
    g = geom(k)
    for fused in (False, True):
        if fused and not rc.fusable(k):
            continue
        c = rc.case(name, k, g, fused)
        rc.assert_case(c)
        print(f"{name} k={k} fused={fused}: nnz {c.batches[1].nnz} rows {c.batches[1].n_rows} F {c.F} "
              f"margins (merged, first-only) {c.margins[0]:.3g} {c.margins[1]:.3g} x {rc.FACTOR:g} tolerances")
    # the two oracles, from the state before the second step
    c = rc.case(name, k, g, False)
    a, b = c.before.copy(), c.before.copy()
    oa = R.sgd_step(a, c.batches[1], 2, c.steps[1], c.reg)
    ob = R.sgd_step_fast(b, c.batches[1], 2, c.steps[1], c.reg)
    assert (oa.n_rows, oa.n_loss_rows, oa.n_unique) == (ob.n_rows, ob.n_loss_rows, ob.n_unique)
    assert np.array_equal(a.present, b.present) and np.array_equal(b.w, c.model.w) and np.array_equal(b.V, c.model.V)
    assert oa.loss_sum == pytest.approx(ob.loss_sum, rel=1e-12)  # the rows' losses: added in turn, and by np.sum in pairs
    if name in rc.SMALL:  # the tables bit for bit: both forms add an id's entries in entry order
        assert np.array_equal(a.w, b.w) and np.array_equal(a.V, b.V)
    else:
        np.testing.assert_allclose(a.w, b.w, rtol=1e-12, atol=0)
        np.testing.assert_allclose(a.V, b.V, rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", [n for n in rc.NAMES if n != "self-pair"])
def test_layouts_follow_the_geometry(name):
    """Every case holds its events under a geometry no build has."""
    for k in (1, 16):
        for fused in (False, True):
            rc.assert_case(rc.case(name, k, other_geom(k), fused))


def test_spread_positions_fall_into_different_passes_and_lane_groups():
    for rpp in (1, 2, 4, 8, 16, 32, 64):
        assert rc.spread_ok(rpp), rpp


def test_wrong_readings_on_a_hand_made_batch():
    csr = R.CSR(np.asarray([0, 2, 5, 5, 6], np.int64), np.asarray([7, 7, 3, 9, 3, 7], np.int32),
                np.asarray([0.5, 1.0, 3.0, 0.7, -3.0, 2.0]), np.asarray([1.0, -10.0, 0.0, 2.0]))
    m, f = rc.merged(csr), rc.first_only(csr)
    assert m.row_ptr.tolist() == f.row_ptr.tolist() == [0, 1, 3, 3, 4]
    assert m.col.tolist() == f.col.tolist() == [7, 3, 9, 7]
    assert m.val.tolist() == [1.5, 0.0, 0.7, 2.0] and f.val.tolist() == [0.5, 3.0, 0.7, 2.0]
    # the coincidence the cases avoid by designating the repeated ids: 9 beside b(+3), b(-3) does not move under merging
    model = R.Model.empty(10, 2)
    rng = np.random.default_rng(0)
    model.load(np.arange(10), rng.normal(0, 0.1, 10), rng.normal(0, 0.1, (10, 2)))
    a, b = model.copy(), model.copy()
    R.sgd_step(a, csr, 1, 0.5, 0.0)
    R.sgd_step(b, m, 1, 0.5, 0.0)
    assert np.allclose(a.V[9], b.V[9], rtol=0, atol=1e-15) and not np.allclose(a.V[3], b.V[3], rtol=1e-3)
    assert R.sgd_step(model.copy(), csr, 1, 0.5, 0.0).n_unique == 3


def test_builder_places_samples_and_values():
    lengths = np.asarray([2, 3, 1, 2, 4])
    csr, ids, w, V = rc.make_repeat_runs(3, lengths, 9, 2, n_rows=6, n_reserved=1, designated=[1],
                                         samples={1: [2, 5, 5], 3: [0, 5]}, x_at={(1, 1): 3.0, (1, 2): -3.0},
                                         place={5: (1, (0, 2))})
    order, keys = runs.sorted_view(csr)
    np.testing.assert_array_equal(keys, np.repeat(np.arange(5), lengths))
    assert rc.run_samples(csr, 1).tolist() == [2, 5, 5] and rc.run_samples(csr, 3).tolist() == [0, 5]
    a = csr.row_ptr[5]
    assert csr.col[a:].tolist() == [1, 3, 1] and csr.val[a] == 3.0 and csr.val[a + 2] == -3.0
    assert abs(csr.label[5]) == 10.0 and abs(csr.label[2]) == 10.0 and (np.abs(csr.val[csr.col == 1]) >= 0.5).all()
    assert (csr.val == csr.val.astype(np.float32)).all() and w.shape == (9,) and V.shape == (9, 2)


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


# sha256 (first 16 hex digits) of the three builders' outputs for the arguments below, taken before this file existed
EARLIER = {"make_runs": "0496c9a535055195", "make_rows": "7ca5cee9b94b4f52", "make_problem": "8546634bdfd2aaf6"}


def test_earlier_builders_keep_their_bytes():
    """make_runs, make_rows and make_problem for fixed arguments, as they were before repeat_cases.py."""
    csr, ids, w, V = runs.make_runs(11, [3, 1, 4, 1, 5, 9, 2, 6], 20, 3, big=[0, 7, 30])
    assert _digest(csr.row_ptr, csr.col, csr.val, csr.label, ids, w, V) == EARLIER["make_runs"]
    csr, ids, w, V = make_rows(12, [0, 3, 7, 1, 12], 40, 4)
    assert _digest(csr.row_ptr, csr.col, csr.val, csr.label, ids, w, V) == EARLIER["make_rows"]
    csr, ids, w, V = make_problem(13, 30, 50, 3, 6, hot=4)
    assert _digest(csr.row_ptr, csr.col, csr.val, csr.label, ids, w, V) == EARLIER["make_problem"]
    for a, b in zip(csr.row_ptr[:-1], csr.row_ptr[1:]):
        assert len(set(csr.col[a:b].tolist())) == b - a  # these builders still make no repeat

