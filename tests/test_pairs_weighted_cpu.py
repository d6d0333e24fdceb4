"""CPU: the weighted draw's contract (tests/pairs_weighted_ref.py) against its brute-force statement and
against the uniform contract -- what tests/test_gpu_pairs_weighted.py compares the device with."""

import numpy as np
import pytest

import pair_ref as P
import pairs_weighted_ref as W


def random_lists(rng, U, C, weight):
    """U strictly ascending lists that each leave eligible weight >= 1."""
    lists = []
    while len(lists) < U:
        e = np.sort(rng.choice(C, rng.integers(0, C), replace=False))
        if weight.sum() - weight[e].sum() >= 1:
            lists.append(e)
    return np.concatenate([[0], np.cumsum([len(e) for e in lists])]).astype(np.int64), np.concatenate(lists).astype(np.int32)


@pytest.mark.parametrize("C", [1, 2, 7, 33, 64])
def test_reference_is_element_r_of_the_expanded_eligible_list(C):
    rng = np.random.default_rng(C)
    weight = rng.integers(0, 6, C)
    weight[rng.integers(0, C)] = max(1, weight.max())
    U, n_draw = 12, 300
    ptr, rows = random_lists(rng, U, C, weight)
    pos_ctx = np.arange(U)
    got = W.weighted_negatives(3, pos_ctx, n_draw, ptr, rows, weight)
    for u in pos_ctx:
        brute = W.eligible_expanded(rows[ptr[u]:ptr[u + 1]], weight)
        r = P.draw_ranks(3, U, n_draw, np.full(U, len(brute)))[u]
        np.testing.assert_array_equal(got[u], brute[r])
    none = W.weighted_negatives(3, pos_ctx, n_draw, None, None, weight)
    np.testing.assert_array_equal(none, W.eligible_expanded([], weight)[P.draw_ranks(3, U, n_draw, np.full(U, weight.sum()))])


@pytest.mark.parametrize("C", [1, 40, 97])
def test_unit_weights_are_the_uniform_contract(C):
    rng = np.random.default_rng(100 + C)
    ones = np.ones(C, np.int64)
    ptr, rows = random_lists(rng, 9, C, ones)
    pos_ctx = rng.integers(0, 9, 50)
    np.testing.assert_array_equal(W.weighted_negatives(8, pos_ctx, 16, ptr, rows, ones),
                                  P.sample_negatives(8, pos_ctx, 16, ptr, rows, C))
    np.testing.assert_array_equal(W.weighted_negatives(8, pos_ctx, 16, None, None, ones),
                                  P.sample_negatives(8, pos_ctx, 16, None, None, C))
