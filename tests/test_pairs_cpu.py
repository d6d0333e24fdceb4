"""CPU: the contract of fm_batch_sample_pairs' draw (tests/pair_ref.py is its NumPy form) and the planted
recommender problem on the fp64 oracle -- what the GPU tests of the pair batches compare against."""

import numpy as np

import pair_ref as P
from oracle import fm_ref as R
from rank_ref import concat_rows


def test_rank_to_row_is_the_rth_eligible_row():
    """r -> r + #{t : excl[t] - t <= r} is the r-th element of setdiff1d(arange(C), excl), for every r, over
    random lists at every C < 40 with 0 .. C - 1 excluded rows."""
    rng = np.random.default_rng(11)
    for C in range(1, 40):
        for n_excl in range(C):
            excl = np.sort(rng.choice(C, n_excl, replace=False))
            r = np.arange(C - n_excl)
            c = r + np.searchsorted(excl - np.arange(n_excl), r, side="right")
            np.testing.assert_array_equal(c, np.setdiff1d(np.arange(C), excl))


def test_concat_pairs_is_the_materialised_row():
    rng = np.random.default_rng(12)
    from rank_ref import make_rows

    u = make_rows(rng, [0, 3, 1, 5], 40)
    c = make_rows(rng, [2, 0, 4], 40)
    rp, col, val = concat_rows(u, c)  # row a * 3 + b
    pc, pd = np.array([3, 0, 0, 2, 3, 1]), np.array([2, 1, 0, 2, 2, 0])
    got = P.concat_pairs(u, c, pc, pd, np.arange(6.0))
    for i, (a, b) in enumerate(zip(pc, pd)):
        s = a * 3 + b
        np.testing.assert_array_equal(got.col[got.row_ptr[i]:got.row_ptr[i + 1]], col[rp[s]:rp[s + 1]])
        np.testing.assert_array_equal(got.val[got.row_ptr[i]:got.row_ptr[i + 1]], val[rp[s]:rp[s + 1]])
    assert got.row_ptr[2] - got.row_ptr[1] == 0  # both rows empty: a row without entries


def test_draws_are_uniform_over_the_eligible_rows():
    """200 000 draws at E = 7: every bin within 5 sqrt(n p (1 - p)) of n / 7."""
    n, E, C = 200_000, 7, 10
    ptr, rows = np.array([0, 3]), np.array([1, 4, 9], np.int32)
    c = P.sample_negatives(99, np.zeros(n // 8, np.int64), 8, ptr, rows, C).reshape(-1)
    assert len(c) == n and not np.isin(c, rows).any()
    counts = np.bincount(c, minlength=C)[np.setdiff1d(np.arange(C), rows)]
    p = 1.0 / E
    assert np.all(np.abs(counts - n * p) <= 5.0 * np.sqrt(n * p * (1 - p))), counts


def test_no_draw_lands_in_its_contexts_list():
    rng = np.random.default_rng(13)
    U, C = 50, 97
    sizes = rng.integers(0, C, U)  # 0 .. C - 1 excluded rows
    lists = [np.sort(rng.choice(C, s, replace=False)) for s in sizes]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = np.concatenate(lists).astype(np.int32)
    pos_ctx = rng.integers(0, U, 400)
    c = P.sample_negatives(5, pos_ctx, 16, ptr, rows, C)
    assert c.min() >= 0 and c.max() < C
    for i, u in enumerate(pos_ctx):
        assert not np.isin(c[i], lists[u]).any()
    # a function of (seed, i, j), the list and C alone: a prefix of the positives draws the same rows
    np.testing.assert_array_equal(P.sample_negatives(5, pos_ctx[:37], 16, ptr, rows, C), c[:37])
    np.testing.assert_array_equal(P.sample_negatives(5, pos_ctx, 9, ptr, rows, C), c[:, :9])
    assert not np.array_equal(P.sample_negatives(6, pos_ctx, 16, ptr, rows, C), c)
    # nothing excluded: the rank is the row
    np.testing.assert_array_equal(P.sample_negatives(5, pos_ctx, 16, None, None, C),
                                  P.draw_ranks(5, len(pos_ctx), 16, np.full(len(pos_ctx), C)))


def test_planted_problem_shape():
    p = P.planted()
    assert len(p.pos_ctx) == 1536 and p.excl_ptr[-1] == 1536
    for u in range(p.U):
        assert len(p.train[u]) == 24 and len(p.held[u]) == 8
        assert np.all(np.concatenate([p.train[u], p.held[u]]) % 8 == u % 8)
        assert not np.isin(p.held[u], p.train[u]).any()
    b = P.iteration_batch(p, 1)
    assert b.n_rows == 384 * 5 and b.nnz == 2 * b.n_rows and b.label.sum() == 384


def test_planted_fit_on_the_oracle_learns_the_held_out_rows():
    """The planted configuration on the fp64 oracle over pair_ref's batches: precision@8 of the held-out
    rows >= 0.95 (untrained: about 0.04)."""
    p = P.planted()
    before = P.held_out_metric("precisionAtK", 8, P.initial_model(p), p)
    model, _ = P.oracle_fit(P.ITERS)
    after = P.held_out_metric("precisionAtK", 8, model, p)
    hit = P.held_out_metric("hitRateAtK", 10, model, p)
    print(f"planted fit on the oracle: precision@8 {before:.3f} -> {after:.3f}, hitRate@10 {hit:.3f}")
    assert before < 0.2
    assert after >= 0.95
