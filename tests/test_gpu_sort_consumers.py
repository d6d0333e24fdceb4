"""The consumers of the radix sort (fm_sort.hip), through the public API, at the sizes and digit plans
the rest of the suite does not reach: fm_vector_sum_by_key (the 4-byte implicit-index sort; its sums
are bitwise the oracle's only if the sort is stable) and the step with one batch of 65537 entries at
F = 1024 (one 10-bit pass) and F = 2^20 (2 x 10 bits).  The sort itself is compared with a stable host
sort in tests/test_gpu_sort.py.  These tests use the sorted payload as an index: they belong to a
correct build of the sort only, never to a deliberately broken one (a sort that leaves outputs
unwritten makes fm_vector_sum_by_key read its vectors at an uninitialised index).
"""

import functools

import numpy as np
import pytest

from oracle import fm_ref as R
from problems import make_problem  # noqa: E402
from sort_probe import PLAN

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------- consumers: fm_vector_sum_by_key
@pytest.fixture(scope="module")
def vs_ctx(gpu):
    from fm_spark_amd.engine import FMContext

    ctx = FMContext(4, 3)
    yield ctx
    ctx.close()


# (width 1 at n = 65537 would be two runs of about 32 768 entries, and k_segment_sum sums a run in one
# thread: the longest run here stays below 20 000)
VS_CASES = [(n, b) for n in (1, 255, 256, 257, 4097, 65537) for b in (1, 10, 20, 31) if not (b == 1 and n == 65537)]


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("n,bits", VS_CASES)
def test_vector_sum_by_key_sizes_and_widths(vs_ctx, n, bits, k):
    """fm_vector_sum_by_key (sort by key with the implicit index, run starts, one thread per run): the
    sums bitwise the oracle's sequential sums -- the sort's order is the summation order -- across
    kBlock = 256 of the single-block run index and the 1 / 2 / 4-pass plans of bits_for(max key)."""
    rng = np.random.default_rng([n, bits, k])
    keys = rng.integers(0, 1 << bits, n, dtype=np.int64)
    keys[rng.integers(0, n)] = (1 << bits) - 1  # bits_for(max key) = bits
    keys = keys.astype(np.int32)
    assert np.bincount(np.unique(keys, return_inverse=True)[1]).max() < 20000
    vecs = rng.normal(size=(n, k)) * 10.0 ** rng.uniform(-3, 3, size=(n, 1))  # six decades: order shows
    gk, gs = vs_ctx.vector_sum_by_key(keys, vecs)
    rk, rs = R.vector_sum_by_key(keys, vecs)
    np.testing.assert_array_equal(gk, rk)
    assert np.array_equal(gs, rs)


# ----------------------------------------------------- consumers: the step at the 10-bit digit plans
RTOL, ATOL = 1e-5, 1e-8  # test_gpu_parity.py
STEP_ENTRIES = 65537
STEPS = 2


@functools.lru_cache(maxsize=2)
def step_problem(F):
    """One batch of exactly 65537 entries (17 tiles, two chunks): make_problem's rows of 1 to 40 entries,
    cut at that total; and the oracle's two steps on it."""
    k = 4
    csr, ids, w, V = make_problem(9100 + F % 97, 4200, F, k, 20.5)
    last = int(np.searchsorted(csr.row_ptr, STEP_ENTRIES, side="left"))  # first row_ptr >= the total
    assert 0 < last < len(csr.row_ptr), "too few rows drawn"
    row_ptr = csr.row_ptr[: last + 1].copy()
    row_ptr[-1] = STEP_ENTRIES  # the last row keeps its first entries: still 1 to 40 of them
    lens = np.diff(row_ptr)
    assert lens.max() <= 40 and lens[-1] >= 1 and lens[lens > 0].min() >= 1
    csr = R.CSR(row_ptr, csr.col[:STEP_ENTRIES].copy(), csr.val[:STEP_ENTRIES].copy(), csr.label[:last].copy())
    model = R.Model.empty(F, k)
    model.load(ids, w, V)
    outs = [R.sgd_step_fast(model, csr, t, 0.3, 1e-5) for t in range(1, STEPS + 1)]
    return csr, ids, w, V, model, outs


@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("F", [1024, 1 << 20])
def test_step_at_the_10_bit_digit_plans(gpu, F, fuse):
    """F = 1024: one 10-bit pass, the input sorted straight into the batch's view; F = 2^20: 2 x 10
    bits.  Inline-sorted and prepared steps against the oracle (counts exact), and against each other
    as test_gpu_parity.test_prepared_batches_match_inline_sort compares them: bit for bit without the
    fused step."""
    from fm_spark_amd._native import CSRHost
    from fm_spark_amd.engine import FMContext

    assert PLAN[(F - 1).bit_length()] == ((10, 1) if F == 1024 else (10, 2))
    csr, ids, w, V, model, ref = step_problem(F)
    pids = np.nonzero(model.present)[0]
    runs = []
    for prep in (False, True):
        ctx = FMContext(F, 4, fuse=fuse)
        ctx.load_tables(ids, w, V)
        db = ctx.batch(CSRHost(csr.row_ptr, csr.col, csr.val, csr.label))
        for t, ro in enumerate(ref, start=1):
            if prep:
                db.prepare()
            go = ctx.step_batch(db, t, 0.3, 1e-5)
            assert go.executed and (go.n_unique, go.n_loss_rows, go.n_rows) == (ro.n_unique, ro.n_loss_rows, ro.n_rows)
            assert go.loss_sum == pytest.approx(ro.loss_sum, rel=RTOL)
        gids, gw, gV = ctx.export_tables()
        losses = ctx.loss_history()
        ctx.close()
        np.testing.assert_array_equal(gids, pids)
        np.testing.assert_allclose(gw, model.w[pids], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(gV, model.V[pids], rtol=RTOL, atol=ATOL)
        runs.append((gids, gw, gV, losses))
    a, b = runs
    if not fuse:
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        return
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_allclose(a[1], b[1], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(a[2], b[2], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(a[3], b[3], rtol=1e-9)
