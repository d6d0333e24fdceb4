"""GPU: mini-batches of (context row, candidate row, label) triples assembled on the device from two
resident batches (fm_batch_from_pairs), and implicit-feedback batches whose negatives are drawn there
(fm_batch_sample_pairs).

A pair batch must be the batch fm_batch_create makes of the host CSR of the concatenated rows
(tests/pair_ref.py concat_pairs) -- so its steps, predictions and entry count are compared with that
batch's bit for bit -- and the drawn rows must be pair_ref.sample_negatives' exactly.

The scan that turns the drawn rows' lengths into row_ptr (fm_pairs.hip) works in chunks of kPairChunk = 256
rows; one block scans the chunk totals, kPairScanNT * kPairScanPer = 256 * 4 = 1024 of them per round, so a
second round starts past 262 144 rows.  test_scan_edges places its row counts against both."""

import gc

import numpy as np
import pytest

import pair_ref as P
from fm_spark_amd import _native as N
from problems import f32
from rank_ref import make_rows

pytestmark = pytest.mark.gpu

F, K = 200, 16       # context ids in [0, 100), candidate ids in [100, 200)
LENS = [0, 1, 15, 16, 17, 33]  # the 16-lane team's trip edges


def host(csr):
    return N.CSRHost(csr.row_ptr, csr.col, csr.val, csr.label)


def rows_host(rows):
    rp, col, val = rows
    return N.CSRHost(rp, col, val, np.zeros(len(rp) - 1))


def cand_rows(rng, lens):
    rp, col, val = make_rows(rng, lens, 100)
    return rp, (col + 100).astype(np.int32), val


def table(seed=1):
    rng = np.random.default_rng(seed)
    return np.arange(F, dtype=np.int32), f32(0.3 * rng.standard_normal(F)), f32(0.3 * rng.standard_normal((F, K)))


def new_ctx(fuse=None, **kw):
    from fm_spark_amd.engine import FMContext

    ctx = FMContext(F, K, fuse=fuse, **kw)
    ctx.load_tables(*table())
    return ctx


@pytest.fixture(scope="module")
def edge_rows():
    """Six rows a side with the lengths LENS, and selections of their pairs: out of order and repeated, every
    combination of lengths (both rows empty among them), a refill that grows the batch, an empty one."""
    rng = np.random.default_rng(21)
    u, c = make_rows(rng, LENS, 100), cand_rows(rng, LENS[::-1])
    every = np.array([(a, b) for a in range(6) for b in range(6)])
    sels = [every[rng.integers(0, 36, 20)], np.concatenate([every[rng.permutation(36)], every[rng.integers(0, 36, 30)]]),
            every[:0], every[rng.integers(0, 36, 5)]]
    sels = [(s[:, 0], s[:, 1], rng.integers(0, 2, len(s)).astype(np.float64)) for s in sels]
    return u, c, sels


def _run(fuse, prepare, u, c, sels, device_pairs):
    """test_gpu_resident_fit's _run: steps over the selections, as pair batches (one batch refilled in turn)
    or as host batches of the concatenated rows; losses + table."""
    ctx = new_ctx(fuse)
    bu, bc = ctx.batch(rows_host(u)), ctx.batch(rows_host(c))
    into, out = None, []
    for t, (pc, pd, y) in enumerate(sels, start=1):
        if device_pairs:
            db = into = ctx.batch_from_pairs(bu, bc, pc, pd, y, into=into)
        else:
            db = ctx.batch(host(P.concat_pairs(u, c, pc, pd, y)))
        assert (db.n_rows, db.nnz) == (len(pc), int(np.sum(np.diff(u[0])[pc] + np.diff(c[0])[pd])))
        if prepare:
            db.prepare()
        o = ctx.step_batch(db, t, 0.3, 1e-3)
        out.append((o.loss_sum, o.n_rows, o.n_loss_rows, o.n_unique, o.executed))
    tab = ctx.export_tables()
    ctx.close()
    return out, tab


@pytest.mark.parametrize("fuse,prepare", [(False, False), (False, True), (True, True)])
def test_from_pairs_bitwise_equal_host_batch(gpu, edge_rows, fuse, prepare):
    u, c, sels = edge_rows
    a = _run(fuse, prepare, u, c, sels, True)
    b = _run(fuse, prepare, u, c, sels, False)
    assert a[0] == b[0]
    assert a[0][2][4] is False and a[0][1][4] is True  # n = 0: FM_NOTHING_TO_DO
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x, y)


def test_from_pairs_predict_with_a_shared_id(gpu, edge_rows):
    """predict_batch of a pair batch == predict of the concatenated host CSR, bit for bit; one pair's rows
    share an id, which counts twice.  contexts and candidates may be one batch."""
    u, c, _ = edge_rows
    rp, col, val = c
    shared = int(u[1][u[0][3]])  # the first id of context row 3
    c2 = (np.append(rp, rp[-1] + 2), np.append(col, [shared, 150]).astype(np.int32), np.append(val, [0.5, -1.25]))
    ctx = new_ctx()
    bu, bc = ctx.batch(rows_host(u)), ctx.batch(rows_host(c2))
    pc, pd = np.array([3, 5, 0, 3, 2, 3]), np.array([6, 0, 5, 2, 6, 6])
    b = ctx.batch_from_pairs(bu, bc, pc, pd, np.zeros(6))
    ref = P.concat_pairs(u, c2, pc, pd, np.zeros(6))
    assert np.sum(ref.col[ref.row_ptr[0]:ref.row_ptr[1]] == shared) == 2
    assert ctx.predict_batch(b, -5.0, 5.0).tobytes() == ctx.predict(host(ref), -5.0, 5.0).tobytes()
    same = ctx.batch_from_pairs(bu, bu, pc[:3], pc[3:], np.zeros(3))
    ref = P.concat_pairs(u, u, pc[:3], pc[3:], np.zeros(3))
    assert ctx.predict_batch(same, -5.0, 5.0).tobytes() == ctx.predict(host(ref), -5.0, 5.0).tobytes()
    ctx.close()


@pytest.fixture(scope="module")
def sampled_case():
    """8 contexts, 70 000 candidate rows of 0 .. 3 entries; exclude lists of 0, 1 and 65 537 rows, all rows but
    row 0 / row C - 1 / a middle row, and two short ones."""
    rng = np.random.default_rng(22)
    C = 70_000
    u, c = make_rows(rng, [3, 0, 17, 1, 2, 16, 5, 4], 100), cand_rows(rng, np.arange(C) % 4)
    but = lambda r: np.delete(np.arange(C), r)
    lists = [np.zeros(0, np.int64), np.array([5]), np.sort(rng.choice(C, 65_537, replace=False)), but(0), but(C - 1),
             but(12_345), np.sort(rng.choice(C, 200, replace=False)), np.sort(rng.choice(C, 10, replace=False))]
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    rows = np.concatenate(lists).astype(np.int32)
    pos_ctx = np.concatenate([np.arange(8), rng.integers(0, 8, 32)])
    pos_cand = rng.integers(0, C, 40)
    return C, u, c, lists, ptr, rows, pos_ctx, pos_cand


def test_sampled_batch_draws_and_bits(gpu, sampled_case):
    C, u, c, lists, ptr, rows, pos_ctx, pos_cand = sampled_case
    n_neg, seed = 7, 0x9E3779B97F4A7C15
    ctx, ref_ctx = new_ctx(), new_ctx()
    bu, bc = ctx.batch(rows_host(u)), ctx.batch(rows_host(c))
    ru, rc = ref_ctx.batch(rows_host(u)), ref_ctx.batch(rows_host(c))
    b, got = ctx.batch_sample_pairs(bu, bc, pos_ctx, pos_cand, n_neg, exclude=lists, pos_label=1.0, neg_label=-0.5,
                                    seed=seed, want_sampled=True)
    want = P.sample_negatives(seed, pos_ctx, n_neg, ptr, rows, C)
    np.testing.assert_array_equal(got, want)
    for i, ctx_row in enumerate(pos_ctx):
        assert not np.isin(got[i], lists[ctx_row]).any()
        only = {3: 0, 4: C - 1, 5: 12_345}.get(int(ctx_row))  # all but one row excluded: always that row
        if only is not None:
            assert np.all(got[i] == only)
    # the batch is fm_batch_from_pairs' of the same pairs and labels: predictions, entry count, a step
    pc, pd, y = P.sampled_pairs(pos_ctx, pos_cand, want, 1.0, -0.5)
    rb = ref_ctx.batch_from_pairs(ru, rc, pc, pd, y)
    assert (b.n_rows, b.nnz) == (rb.n_rows, rb.nnz) == (40 * 8, P.concat_pairs(u, c, pc, pd, y).nnz)
    p0 = ctx.predict_batch(b, -5.0, 5.0)
    assert p0.tobytes() == ref_ctx.predict_batch(rb, -5.0, 5.0).tobytes()
    # equal calls give equal bytes; another seed draws other rows
    b2, again = ctx.batch_sample_pairs(bu, bc, pos_ctx, pos_cand, n_neg, exclude=lists, pos_label=1.0, neg_label=-0.5,
                                       seed=seed, want_sampled=True)
    assert again.tobytes() == got.tobytes() and ctx.predict_batch(b2, -5.0, 5.0).tobytes() == p0.tobytes()
    _, other = ctx.batch_sample_pairs(bu, bc, pos_ctx, pos_cand, n_neg, exclude=lists, seed=seed + 1, into=b2,
                                      want_sampled=True)
    assert not np.array_equal(other, got)
    np.testing.assert_array_equal(other, P.sample_negatives(seed + 1, pos_ctx, n_neg, ptr, rows, C))
    for cx, bb in ((ctx, b), (ref_ctx, rb)):
        bb.prepare()
    so, sr = ctx.step_batch(b, 1, 0.3, 1e-3), ref_ctx.step_batch(rb, 1, 0.3, 1e-3)
    assert (so.loss_sum, so.n_loss_rows, so.n_unique) == (sr.loss_sum, sr.n_loss_rows, sr.n_unique)
    for x, y_ in zip(ctx.export_tables(), ref_ctx.export_tables()):
        assert np.array_equal(x, y_)
    # n_neg = 0 is fm_batch_from_pairs with a constant label; excl_ptr = NULL excludes nothing
    z = ctx.batch_sample_pairs(bu, bc, pos_ctx, pos_cand, 0, exclude=lists, pos_label=0.25)
    rz = ref_ctx.batch_from_pairs(ru, rc, pos_ctx, pos_cand, np.full(40, 0.25))
    assert (z.n_rows, z.nnz) == (rz.n_rows, rz.nnz)
    assert ctx.predict_batch(z, -5.0, 5.0).tobytes() == ref_ctx.predict_batch(rz, -5.0, 5.0).tobytes()
    ez, er = ctx.evaluate_batch(z, -5.0, 5.0), ref_ctx.evaluate_batch(rz, -5.0, 5.0)
    assert ez == er  # the labels
    nb, free = ctx.batch_sample_pairs(bu, bc, pos_ctx, pos_cand, 3, seed=4, want_sampled=True)
    want = P.sample_negatives(4, pos_ctx, 3, None, None, C)
    np.testing.assert_array_equal(free, want)
    rn = ref_ctx.batch_from_pairs(ru, rc, *P.sampled_pairs(pos_ctx, pos_cand, want))
    assert ctx.predict_batch(nb, -5.0, 5.0).tobytes() == ref_ctx.predict_batch(rn, -5.0, 5.0).tobytes()
    ctx.close()
    ref_ctx.close()


@pytest.fixture(scope="module")
def small_case():
    rng = np.random.default_rng(23)
    U, C = 5, 23
    u, c = make_rows(rng, [1, 2, 0, 1, 3], 100), cand_rows(rng, 1 + np.arange(C) % 3)
    lists = [np.sort(rng.choice(C, n, replace=False)) for n in (0, 3, 22, 7, 1)]
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return U, C, u, c, lists, ptr, np.concatenate(lists).astype(np.int32)


@pytest.mark.parametrize("n_pos,n_neg", [(51, 4), (128, 1), (257, 0), (171, 2), (52_429, 4)])
def test_scan_edges(gpu, small_case, n_pos, n_neg):
    """n_pos (1 + n_neg) rows = kPairChunk - 1, kPairChunk, kPairChunk + 1, 2 kPairChunk + 1 (kPairChunk = 256)
    and 262 145, one past kPairScanNT * kPairScanPer * kPairChunk = 1024 chunks: the chunk-total scan's second
    round.  row_ptr through fm_batch_nnz and through predict_batch against the host batch."""
    U, C, u, c, lists, ptr, rows = small_case
    assert n_pos * (1 + n_neg) in (255, 256, 257, 513, 262_145)
    rng = np.random.default_rng(n_pos)
    pos_ctx, pos_cand = rng.integers(0, U, n_pos), rng.integers(0, C, n_pos)
    ctx = new_ctx()
    bu, bc = ctx.batch(rows_host(u)), ctx.batch(rows_host(c))
    b, got = ctx.batch_sample_pairs(bu, bc, pos_ctx, pos_cand, n_neg, exclude=lists, seed=77, want_sampled=True)
    want = P.sample_negatives(77, pos_ctx, n_neg, ptr, rows, C)
    np.testing.assert_array_equal(got, want)
    ref = P.concat_pairs(u, c, *P.sampled_pairs(pos_ctx, pos_cand, want))
    assert (b.n_rows, b.nnz) == (ref.n_rows, ref.nnz)
    assert ctx.predict_batch(b, -5.0, 5.0).tobytes() == ctx.predict(host(ref), -5.0, 5.0).tobytes()
    ctx.close()


def test_pipelined_refills_equal_synchronous_ones(gpu, small_case):
    """8 iterations over two output batches in turn: enqueue-only steps (the next batch drawn, gathered and
    sorted while a step runs) leave the table of the same loop with every step waited for."""
    U, C, u, c, lists, ptr, rows = small_case
    rng = np.random.default_rng(24)
    pos = [(rng.integers(0, U, 300 + 40 * t), rng.integers(0, C, 300 + 40 * t)) for t in range(8)]
    tabs = []
    for sync in (False, True):
        ctx = new_ctx()
        bu, bc = ctx.batch(rows_host(u)), ctx.batch(rows_host(c))
        bufs = [None, None]
        for t, (pc, pd) in enumerate(pos, start=1):
            bufs[t % 2] = ctx.batch_sample_pairs(bu, bc, pc, pd, 4, exclude=lists, seed=t, into=bufs[t % 2])
            bufs[t % 2].prepare()
            ctx.step_batch(bufs[t % 2], t, 0.3, 1e-3, sync=sync)
        ctx.sync()
        assert ctx.epoch == 8
        tabs.append(ctx.export_tables())
        ctx.close()
    for x, y in zip(*tabs):
        assert np.array_equal(x, y)


def test_steady_device_memory(gpu, small_case):
    U, C, u, c, lists, ptr, rows = small_case
    lib = N.load()
    gc.collect()
    start = (lib.fm_device_bytes_live(), lib.fm_device_allocs_live())
    ctx = new_ctx()
    bu, bc = ctx.batch(rows_host(u)), ctx.batch(rows_host(c))
    rng = np.random.default_rng(25)
    pc, pd = rng.integers(0, U, 500), rng.integers(0, C, 500)
    live = []
    into = None
    for _ in range(2):
        into = ctx.batch_sample_pairs(bu, bc, pc, pd, 4, exclude=lists, seed=3, into=into)
        ctx.sync()
        live.append((lib.fm_device_bytes_live(), lib.fm_device_allocs_live()))
    assert live[0] == live[1]
    into2 = None
    for _ in range(2):
        into2 = ctx.batch_from_pairs(bu, bc, pc, pd, np.ones(500), into=into2)
        ctx.sync()
        live.append((lib.fm_device_bytes_live(), lib.fm_device_allocs_live()))
    assert live[2] == live[3]
    for b in (into, into2, bu, bc):
        b.close()
    ctx.close()
    assert (lib.fm_device_bytes_live(), lib.fm_device_allocs_live()) == start


def test_refusals_leave_the_batch_as_it_was(gpu, small_case):
    from fm_spark_amd.engine import FMContext

    U, C, u, c, lists, ptr, rows = small_case
    ctx = new_ctx()
    bu, bc = ctx.batch(rows_host(u)), ctx.batch(rows_host(c))
    pc, pd = np.array([0, 4, 1, 3]), np.array([22, 0, 7, 7])
    into = ctx.batch_sample_pairs(bu, bc, pc, pd, 2, exclude=lists, seed=1)
    before = ctx.predict_batch(into, -5.0, 5.0).tobytes()
    raw = lambda ex, n_neg=2, pos=(pc, pd), out=into: ctx._sample_pairs(bu, bc, pos[0], pos[1], n_neg, ex, 1.0, 0.0, 1, out,
                                                                       False)
    everything = (np.array([0, 0, 0, C, C, C], np.int64), np.arange(C, dtype=np.int32))  # context 2 sees every row
    cases = [
        ("pair_ctx index out of", lambda: ctx.batch_from_pairs(bu, bc, [0, U], [0, 0], [1.0, 0.0], into=into)),
        ("pair_cand index out of", lambda: ctx.batch_from_pairs(bu, bc, [0, 1], [0, -1], [1.0, 0.0], into=into)),
        ("pos_ctx index out of", lambda: raw((ptr, rows), pos=(np.array([U]), np.array([0])))),
        ("pos_cand index out of", lambda: raw((ptr, rows), pos=(np.array([0]), np.array([C])))),
        ("other than contexts and candidates", lambda: ctx.batch_from_pairs(bu, bc, pc, pd, np.ones(4), into=bu)),
        ("other than contexts and candidates", lambda: raw((ptr, rows), out=bc)),
        (r"n_neg must be in \[0, 1024\]", lambda: raw((ptr, rows), n_neg=1025)),
        (r"n_neg must be in \[0, 1024\]", lambda: raw((ptr, rows), n_neg=-1)),
        ("exclude list: context 1, position 1: row 3 after row 5: a list must be strictly ascending",
         lambda: raw((np.array([0, 0, 2, 2, 2, 2], np.int64), np.array([5, 3], np.int32)))),
        (r"exclude list: context 0, position 0: row 23 is out of range \[0, 23\)",
         lambda: raw((np.array([0, 1, 1, 1, 1, 1], np.int64), np.array([C], np.int32)))),
        ("context 2 .* no eligible candidate row", lambda: raw(everything, pos=(np.array([0, 2]), np.array([1, 1])))),
    ]
    for message, call in cases:
        with pytest.raises(N.FMError, match=message):
            call()
        assert ctx.predict_batch(into, -5.0, 5.0).tobytes() == before, message
    # a context with every row excluded that no positive names is no obstacle
    ok = raw(everything, pos=(np.array([0, 1]), np.array([1, 1])), out=None)
    assert ok.n_rows == 6
    # a foreign batch, as a source and as the result
    other = new_ctx()
    with pytest.raises(N.FMError, match="another context"):
        other.batch_from_pairs(bu, bc, pc, pd, np.ones(4))
    with pytest.raises(N.FMError, match="another context"):
        other.batch_sample_pairs(bu, bc, pc, pd, 2)
    ou, oc = other.batch(rows_host(u)), other.batch(rows_host(c))
    with pytest.raises(N.FMError, match="out must be a batch of this context"):
        other.batch_from_pairs(ou, oc, pc, pd, np.ones(4), into=into)
    assert ctx.predict_batch(into, -5.0, 5.0).tobytes() == before
    other.close()
    ctx.close()
    # a multi-GPU context's batches are cut over its ranks: both modes, both calls
    for mode in ("sharded", "replicated"):
        group = FMContext(F, K, parallel=mode, n_gpus=2, devices=[0, 0], transport="copy")
        gu, gc_ = group.batch(rows_host(u)), group.batch(rows_host(c))
        with pytest.raises(N.FMError, match="cut over its ranks"):
            group.batch_from_pairs(gu, gc_, pc, pd, np.ones(4))
        with pytest.raises(N.FMError, match="cut over its ranks"):
            group.batch_sample_pairs(gu, gc_, pc, pd, 2)
        group.close()
