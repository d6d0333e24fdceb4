"""CPU: the stream-order scenarios' inputs (tests/stream_cases.py) have the shape the GPU harness relies
on, and the fp64 oracle separates program order from the order a lost wait would produce by more than
SEPARATION tolerances of tests/test_gpu_parity.py -- so a lost wait cannot hide inside the bits."""

import numpy as np
import pytest

import stream_cases as sc


@pytest.mark.parametrize("k", sc.KS)
def test_every_contents_has_the_fixed_shape(k):
    keys = sorted({key for prog, lost in sc.SCENARIOS.values() for key in prog + lost} | {f"V{s}" for s in range(sc.N_SEL)})
    for key in keys:
        c = sc.contents(k, key)
        assert c.n_rows == sc.ROWS and c.nnz == sc.ROWS * sc.LEN, key
        assert (np.diff(c.row_ptr) == sc.LEN).all(), key
        assert c.col.min() >= 0 and c.col.max() < sc.F, key
        ids = c.col.reshape(sc.ROWS, sc.LEN)
        assert (np.diff(np.sort(ids, axis=1), axis=1) > 0).all(), f"{key}: ids distinct within a row"
        assert set(np.unique(c.label)) <= {0.0, 1.0}, key  # the binary evaluation's labels


def test_selections_and_splits_tile_the_dataset():
    csr = sc.dataset(sc.KS[0])[0]
    assert csr.n_rows == sc.N_SEL * sc.ROWS and (np.diff(csr.row_ptr) == sc.LEN).all()
    sr = sc.split_rows()
    assert sr[0] == 0 and sr[-1] == csr.n_rows and (np.diff(sr) == sc.ROWS).all()
    for i in range(sc.N_SEL):
        s = sc.selection(i)
        assert len(s) == sc.ROWS == len(np.unique(s)) and s.min() >= 0 and s.max() < csr.n_rows
        for j in range(i):
            assert not np.array_equal(np.sort(s), np.sort(sc.selection(j)))


def test_pair_inputs():
    u, c = sc.pair_sources()
    assert u.n_rows == sc.N_CTX and c.n_rows == sc.N_CAND
    assert (np.diff(u.row_ptr) == sc.CTX_LEN).all() and (np.diff(c.row_ptr) == sc.CAND_LEN).all()
    assert u.col.max() < sc.F // 2 <= c.col.min() and c.col.max() < sc.F
    for j in range(2):
        pc, pd, y = sc.pair_list(j)
        assert len(pc) == len(pd) == len(y) == sc.ROWS
        assert pc.min() >= 0 and pc.max() < sc.N_CTX and pd.min() >= 0 and pd.max() < sc.N_CAND
        qc, qd, lists = sc.positives(j)
        assert len(qc) == len(qd) == sc.N_POS and len(lists) == sc.N_CTX
        assert all(len(l) < sc.N_CAND for l in lists)  # every context keeps an eligible candidate
    assert not np.array_equal(sc.pair_list(0)[0], sc.pair_list(1)[0])


@pytest.mark.parametrize("k", sc.KS)
@pytest.mark.parametrize("family", sorted(sc.SCENARIOS))
def test_oracle_separates_program_order_from_a_lost_wait(family, k):
    sep = sc.separation(k, family)
    print(f"{family} k={k}: separation {sep:.1f} tolerances")
    assert sep > sc.SEPARATION


@pytest.mark.parametrize("k", sc.KS)
@pytest.mark.parametrize("pair", [("S0", "S1"), ("S1", "S0"), ("V0", "V1"), ("P0", "P1")])
def test_oracle_separates_the_predictions(pair, k):
    sep = sc.prediction_separation(k, *pair)
    print(f"{pair} k={k}: separation {sep:.1f} tolerances")
    assert sep > sc.SEPARATION


def test_the_measured_figures():
    """The figures behind the choice of seeds (SEED_DATA 300, SEED_SEL 301, step 0.2, reg 1e-4): a step that
    reads the wrong selection moves the second loss sum by more than 1e-4 relative and some V word by more
    than 1e-4 absolute -- ten and more times the parity tolerance."""
    k = sc.KS[0]
    la, ma = sc.oracle_run(k, ["S0", "S1"])
    lb, mb = sc.oracle_run(k, ["S0", "S0"])
    assert abs(la[1] - lb[1]) / abs(la[1]) > 1e-4
    assert np.max(np.abs(ma.V - mb.V)) > 1e-4
