"""GPU: top-N candidate ranking (fm_rank_candidates / fm_rank_batch; fm_rank.hip) against the fp64
NumPy reference of tests/rank_ref.py.

The constants of fm_rank.hip whose edges the shapes below sit on:
  kRankChunk = 1024       candidates a block scores and sorts at a time -> C in 1023, 1024, 1025, 2049;
  kRankMaxSplits = 64     blocks per context at most, so from 64 * 1024 = 65536 candidates on a block
                          streams several chunks into its running list -> C in 65535, 65536, 65537, 131073;
  kRankTargetBlocks = 512 blocks of one call, about: U contexts take at most ceil(512 / U) splits -> U = 65
                          (8 splits) with C at 7, 8, 8 + and 17 + chunks: 7168, 8192, 8193, 17409;
  kRankListBudget = 4 MiB the split lists of one pass over the contexts -> the same calls at n_top = 1024:
                          8 * 1024 * 12 B per context, 42 contexts per pass, two passes.

Tolerance (the bound for reordered fp64 sums): every returned score lies within
(nnz_u + nnz_c + kp + 16) 2^-52 M of the reference, M = |w0| + sum |w x| + (sum_f (sum_e |v_ef x_e|)^2
+ sum_e |v_e|^2 x_e^2) / 2 over both rows; one fp32 rounding on the path would exceed it by about 2^26.
Where two bounds meet (two pairs compared) the smaller one is taken."""

import math

import numpy as np
import pytest

import rank_ref as R
from fm_spark_amd import _native as N
from fm_spark_amd.engine import FMContext

pytestmark = pytest.mark.gpu
INF = math.inf
F = 4096


def csr(rows):
    rp, col, val = rows
    return N.CSRHost(rp, col, val, np.zeros(len(rp) - 1))


def loaded(w, V, present, w0=0.0, **kw):
    ctx = FMContext(len(w), V.shape[1], w0=w0, **kw)
    ids = np.flatnonzero(present)
    ctx.load_tables(ids, w[ids], V[ids])
    return ctx


def cut(ref, Cn):
    """The reference of the first Cn candidates."""
    return R.PairRef(ref.key[:, :Cn], ref.learned[:, :Cn], ref.bound[:, :Cn], ref.w0)


def check(idx, score, ref, lo=-INF, hi=INF):
    """The issue's conditions on one call's result."""
    U, Cn = ref.key.shape
    n = idx.shape[1]
    assert idx.shape == score.shape == (U, n) and idx.dtype == np.int32
    assert idx.min() >= 0 and idx.max() < Cn
    rows = np.arange(U)[:, None]
    key, bnd = ref.key[rows, idx], ref.bound[rows, idx]
    # scores: within the bound of the reference, exactly w0 where nothing is learned
    want = ref.score(lo, hi)[rows, idx]
    err = np.abs(score - want)
    assert np.all(err <= bnd), float(np.max(err - bnd))
    assert np.all(score[~ref.learned[rows, idx]] == ref.w0)
    # the returned keys are non-increasing (a clamp keeps that)
    shown = np.where(ref.learned[rows, idx], score, min(max(ref.w0, lo), hi))  # w0 pairs rank at w0, return it unclamped
    assert np.all(np.diff(shown, axis=1) <= 0)
    tri = np.triu(np.ones((n, n), bool), 1)
    for u in range(U):
        assert len(np.unique(idx[u])) == n
        # nothing left out beats the list's last key by more than the bound
        out = np.ones(Cn, bool)
        out[idx[u]] = False
        over = ref.key[u, out] - key[u, -1]
        assert np.all(over <= np.minimum(ref.bound[u, out], bnd[u, -1])), (u, float(over.max()))
        # where two reference keys differ by more than the bound, the order is the reference's
        rise = key[u][None, :] - key[u][:, None]  # [j, l] = key_l - key_j, a violation where j < l
        assert not np.any(tri & (rise > np.minimum(bnd[u][None, :], bnd[u][:, None]))), u


def ctx_lens(U, rng):
    return np.concatenate([[200, 0, 1][:U], rng.choice([0, 1, 3, 20, 200], max(U - 3, 0))]).astype(np.int64)


def cand_lens(Cn):
    return np.array([13, 0, 1])[np.arange(Cn) % 3]


def centred_w0(w, V, present, ctxs, cands):
    """A globalBias that puts the middle context's scores on both sides of zero."""
    key0 = R.pair_ref(w, V, present, 0.0, ctxs, cands).key
    return 0.25 - float(np.median(key0[len(key0) // 2]))


def tops(Cn):
    return sorted({t for t in (1, 2, 64, 100, min(Cn, 1024)) if t <= Cn})


# ------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("U", [1, 3, 65])
@pytest.mark.parametrize("k", [1, 4, 5, 16, 17, 32, 80])
def test_chunk_edges_for_every_k_and_u(gpu, k, U):
    rng = np.random.default_rng(1000 * k + U)
    w, V, present = R.make_table(rng, F, k)
    ctxs, cands = R.make_rows(rng, ctx_lens(U, rng), F), R.make_rows(rng, cand_lens(2049), F)
    w0 = centred_w0(w, V, present, ctxs, cands)
    ref = R.pair_ref(w, V, present, w0, ctxs, cands)
    assert ((ref.key > 0).any(axis=1) & (ref.key < 0).any(axis=1)).any()  # both signs within one context's sort
    ctx = loaded(w, V, present, w0=w0)
    cu = csr(ctxs)
    for Cn in (1023, 1024, 1025, 2049):
        cc = csr(R.take_rows(cands, np.arange(Cn)))
        for n_top in tops(Cn):
            idx, score = ctx.rank(cu, cc, n_top, -INF, INF)
            check(idx, score, cut(ref, Cn))
    ctx.close()


def test_every_candidate_count_to_130(gpu):
    rng = np.random.default_rng(7)
    k, U = 5, 3
    w, V, present = R.make_table(rng, F, k)
    ctxs, cands = R.make_rows(rng, ctx_lens(U, rng), F), R.make_rows(rng, cand_lens(130), F)
    w0 = centred_w0(w, V, present, ctxs, cands)
    ref = R.pair_ref(w, V, present, w0, ctxs, cands)
    assert ((ref.key > 0).any(axis=1) & (ref.key < 0).any(axis=1)).any()  # both signs within one context's sort
    ctx = loaded(w, V, present, w0=w0)
    cu = csr(ctxs)
    for Cn in range(1, 131):
        cc = csr(R.take_rows(cands, np.arange(Cn)))
        for n_top in tops(Cn):
            idx, score = ctx.rank(cu, cc, n_top, -INF, INF)
            check(idx, score, cut(ref, Cn))
    ctx.close()


def test_split_cap_edges(gpu):
    """kRankMaxSplits * kRankChunk candidates and beyond: a block folds several chunks into its list."""
    rng = np.random.default_rng(11)
    k, U = 4, 3
    w, V, present = R.make_table(rng, F, k)
    ctxs, cands = R.make_rows(rng, ctx_lens(U, rng), F), R.make_rows(rng, cand_lens(131073), F)
    ref = R.pair_ref(w, V, present, 0.0, ctxs, cands)
    ctx = loaded(w, V, present)
    cu = csr(ctxs)
    for Cn in (65535, 65536, 65537, 131073):
        cc = csr(R.take_rows(cands, np.arange(Cn)))
        for n_top in (100, 1024):
            idx, score = ctx.rank(cu, cc, n_top, -INF, INF)
            check(idx, score, cut(ref, Cn))
    ctx.close()


def test_split_count_edges_and_context_tiles(gpu):
    """U = 65: 8 splits from 8 chunks on (blocks stream one to three chunks); at n_top = 1024 the
    lists take 8 * 1024 * 12 B per context, so the contexts go in two passes of 42 and 23."""
    rng = np.random.default_rng(12)
    k, U = 4, 65
    w, V, present = R.make_table(rng, F, k)
    ctxs, cands = R.make_rows(rng, ctx_lens(U, rng), F), R.make_rows(rng, cand_lens(17409), F)
    ref = R.pair_ref(w, V, present, 0.0, ctxs, cands)
    ctx = loaded(w, V, present)
    for Cn in (7168, 8192, 17409, 8193):
        n_top = 1024 if Cn == 8193 else 100
        cc = csr(R.take_rows(cands, np.arange(Cn)))
        idx, score = ctx.rank(csr(ctxs), cc, n_top, -INF, INF)
        check(idx, score, cut(ref, Cn))
    cands = R.take_rows(cands, np.arange(8193))
    # a context of the second pass ranked alone: the same bytes
    one, one_s = ctx.rank(csr(R.take_rows(ctxs, [50])), csr(cands), 1024, -INF, INF)
    assert one.tobytes() == idx[50].tobytes() and one_s.tobytes() == score[50].tobytes()
    ctx.close()


# ------------------------------------------------------------------- ties and determinism (bitwise)
@pytest.mark.parametrize("Cn,n_top", [(300, 100), (2500, 1024), (70000, 1024)])
def test_identical_candidates_come_in_row_order(gpu, Cn, n_top):
    rng = np.random.default_rng(21)
    w, V, present = R.make_table(rng, F, 5)
    ctxs = R.make_rows(rng, [200, 0, 1], F)
    one = R.make_rows(rng, [13], F)
    cands = R.take_rows(one, np.zeros(Cn, np.int64))
    ctx = loaded(w, V, present)
    idx, score = ctx.rank(csr(ctxs), csr(cands), n_top, -INF, INF)
    assert np.array_equal(idx, np.tile(np.arange(n_top, dtype=np.int32), (3, 1)))
    assert np.all(score == score[:, :1])
    ctx.close()


def test_duplicated_candidates_interleaved_with_others(gpu):
    rng = np.random.default_rng(22)
    w, V, present = R.make_table(rng, F, 17)
    ctxs = R.make_rows(rng, [200, 1, 40, 0], F)
    distinct = R.make_rows(rng, np.full(40, 13), F)
    content = rng.integers(0, 40, 2300)  # candidate row -> which distinct row it copies
    cands = R.take_rows(distinct, content)
    ctx = loaded(w, V, present)
    idx, score = ctx.rank(csr(ctxs), csr(cands), 1024, -INF, INF)
    check(idx, score, R.pair_ref(w, V, present, 0.0, ctxs, cands))
    for u in range(4):
        g = content[idx[u]]
        for d in np.unique(g):
            at = np.flatnonzero(g == d)
            assert np.all(np.diff(idx[u, at]) > 0)       # copies of one row: ascending candidate row
            assert np.all(score[u, at] == score[u, at[0]])  # and the same bits, wherever they sit
            assert np.all(np.diff(at) == 1)              # equal keys: adjacent in the list
    ctx.close()


def test_determinism_and_independence(gpu):
    rng = np.random.default_rng(23)
    k, U, Cn = 17, 5, 2600
    w, V, present = R.make_table(rng, F, k, present_frac=1.0)
    ctxs = R.make_rows(rng, [200, 1, 30, 7, 100], F)
    cands = R.make_rows(rng, np.full(Cn, 13), F)
    ctx = loaded(w, V, present)
    cu, cc = csr(ctxs), csr(cands)
    full_i, full_s = ctx.rank(cu, cc, 1024, -INF, INF)
    check(full_i, full_s, R.pair_ref(w, V, present, 0.0, ctxs, cands))
    assert np.all(np.diff(full_s, axis=1) < 0)  # a problem without exact ties
    again_i, again_s = ctx.rank(cu, cc, 1024, -INF, INF)
    assert again_i.tobytes() == full_i.tobytes() and again_s.tobytes() == full_s.tobytes()
    for u in range(U):  # each context alone
        i1, s1 = ctx.rank(csr(R.take_rows(ctxs, [u])), cc, 1024, -INF, INF)
        assert i1.tobytes() == full_i[u].tobytes() and s1.tobytes() == full_s[u].tobytes()
    for n in (1, 2, 64, 100):  # n_top = n is a prefix
        i_n, s_n = ctx.rank(cu, cc, n, -INF, INF)
        assert np.array_equal(i_n, full_i[:, :n]) and s_n.tobytes() == np.ascontiguousarray(full_s[:, :n]).tobytes()
    perm = rng.permutation(Cn)  # new candidate row j = old row perm[j]
    p_i, p_s = ctx.rank(cu, csr(R.take_rows(cands, perm)), 1024, -INF, INF)
    assert np.array_equal(perm[p_i], full_i) and p_s.tobytes() == full_s.tobytes()
    bu, bc = ctx.batch(cu), ctx.batch(cc)  # rank_batch equals rank
    b_i, b_s = ctx.rank_batch(bu, bc, 1024, -INF, INF)
    assert b_i.tobytes() == full_i.tobytes() and b_s.tobytes() == full_s.tobytes()
    bu.close(), bc.close()
    ctx.close()


# -------------------------------------------------------------------------------- semantics
def test_w0_pairs_dropped_ids_and_clamped_ties(gpu):
    rng = np.random.default_rng(31)
    Fm, k, w0 = 500, 5, 5.0
    w, V, present = R.make_table(rng, Fm, k, present_frac=0.6)
    absent = np.flatnonzero(~present)
    ctxs = list(R.make_rows(rng, [0, 3, 60, 2], Fm + 200))  # ids >= F among them
    ctxs[1][ctxs[0][1]:ctxs[0][2]] = absent[:3]            # context 1: absent ids only
    ctxs[1][ctxs[0][3]:ctxs[0][4]] = [Fm + 5, Fm + 100]    # context 3: ids beyond the table only
    cands = list(R.make_rows(rng, cand_lens(400), Fm + 200, scale=3.0))
    cands = tuple(cands)
    ctxs = tuple(ctxs)
    ref = R.pair_ref(w, V, present, w0, ctxs, cands)
    assert (~ref.learned).sum() >= 3 * 133 and ref.learned[0].any()
    assert ((ref.key < w0) & ref.learned).any() and ((ref.key > w0) & ref.learned).any()
    ctx = loaded(w, V, present, w0=w0)
    cu, cc = csr(ctxs), csr(cands)
    free_i, free_s = ctx.rank(cu, cc, 400, -INF, INF)
    check(free_i, free_s, ref)
    # a clamp range that excludes w0: the pair without a learned entry returns w0 and ranks at w0
    idx, score = ctx.rank(cu, cc, 400, 0.0, 1.0)
    check(idx, score, ref, 0.0, 1.0)
    assert np.array_equal(idx, free_i)  # many scores tie at 0 and 1: the order stays the unclamped key's
    nolearn = ~ref.learned[np.arange(4)[:, None], idx]
    assert nolearn.any() and np.all(score[nolearn] == w0) and np.all(score[~nolearn] <= 1.0)
    assert (np.sum(score == 1.0, axis=1) > 1).any() and (np.sum(score == 0.0, axis=1) > 1).any()
    assert not nolearn[2].any() and nolearn[[0, 1, 3]].any(axis=1).all()
    for u in (0, 1, 3):  # at w0: learned keys above come before, learned keys below after
        pos = np.flatnonzero(nolearn[u])
        assert np.all(np.diff(pos) == 1)
        lk = ref.key[u, idx[u]]
        assert np.all(lk[: pos[0]] >= w0 - ref.bound[u, idx[u, : pos[0]]])
        assert np.all(lk[pos[-1] + 1:] <= w0 + ref.bound[u, idx[u, pos[-1] + 1:]])
    ctx.close()


def test_an_id_in_both_rows_counts_twice(gpu):
    rng = np.random.default_rng(32)
    Fm, k = 64, 4
    w, V, present = R.make_table(rng, Fm, k, present_frac=1.0)
    ctxs = (np.array([0, 3]), np.array([5, 9, 20], np.int32), R.f32([1.5, -0.5, 2.0]))
    cands = (np.array([0, 2, 4, 5]), np.array([9, 30, 5, 20, 31], np.int32), R.f32([0.75, 1.0, -2.0, 3.0, 0.5]))
    ref = R.pair_ref(w, V, present, 0.5, ctxs, cands)
    ctx = loaded(w, V, present, w0=0.5)
    idx, score = ctx.rank(csr(ctxs), csr(cands), 3, -INF, INF)
    check(idx, score, ref)
    # the formula by hand for candidate 0 (shares id 9): entries (5, 1.5) (9, -.5) (20, 2) (9, .75) (30, 1)
    ids, x = np.array([5, 9, 20, 9, 30]), np.array([1.5, -0.5, 2.0, 0.75, 1.0])
    S = (V[ids] * x[:, None]).sum(0)
    y = 0.5 + (w[ids] * x).sum() + 0.5 * ((S * S).sum() - ((V[ids] ** 2).sum(1) * x * x).sum())
    j = int(np.flatnonzero(idx[0] == 0)[0])
    assert abs(score[0, j] - y) <= ref.bound[0, 0]
    # and fm_predict of the concatenated rows
    pred = ctx.predict(csr(R.concat_rows(ctxs, cands)), -INF, INF)
    assert np.all(np.abs(score[0] - pred[idx[0]]) <= ref.bound[0, idx[0]])
    ctx.close()


def test_lazy_l1_is_caught_up_on_read(gpu):
    rng = np.random.default_rng(33)
    Fm, k = 256, 8
    w, V, present = R.make_table(rng, Fm, k, present_frac=1.0)
    ctx = loaded(w, V, present)
    # three steps with L1; the first batch's rows (ids < 100) are not touched by the later ones
    for t, (lo_id, hi_id) in enumerate([(0, 100), (100, 200), (100, 200)], start=1):
        rp, col, val = R.make_rows(rng, np.full(64, 6), hi_id - lo_id)
        b = ctx.batch(N.CSRHost(rp, col + lo_id, val, rng.integers(0, 2, 64).astype(np.float64)))
        ctx.step_batch(b, t, 0.05, 0.02)
        b.close()
    ctxs, cands = R.make_rows(rng, [0, 1, 150, 40], Fm), R.make_rows(rng, cand_lens(300), Fm)
    idx, score = ctx.rank(csr(ctxs), csr(cands), 100, -INF, INF)  # no export in between
    pred = ctx.predict(csr(R.concat_rows(ctxs, cands)), -INF, INF).reshape(4, 300)
    ids, w1, V1 = ctx.export_tables()
    assert len(ids) == Fm and not np.array_equal(w1, w)
    ref = R.pair_ref(w1, V1, present, 0.0, ctxs, cands)
    check(idx, score, ref)
    rows = np.arange(4)[:, None]
    assert np.all(np.abs(score - pred[rows, idx]) <= ref.bound[rows, idx])
    assert ctx.epoch == 3
    ctx.close()


# ------------------------------------------------------------------- refusals and lifetime
def _small(seed=41, k=4, Cn=50):
    rng = np.random.default_rng(seed)
    w, V, present = R.make_table(rng, 200, k)
    return w, V, present, R.make_rows(rng, [5, 0, 20], 200), R.make_rows(rng, cand_lens(Cn), 200)


def test_sharded_tables_refuse_and_replicated_answers(gpu):
    w, V, present, ctxs, cands = _small()
    cu, cc = csr(ctxs), csr(cands)
    single = loaded(w, V, present)
    want_i, want_s = single.rank(cu, cc, 10, 0.0, 1.0)
    shard = FMContext(200, 4, shard_count=2)
    with pytest.raises(N.FMError, match="shard"):
        shard.rank(cu, cc, 10, 0.0, 1.0)
    shard.close()
    group = FMContext(200, 4, parallel="sharded", n_gpus=2, devices=[0, 0])
    with pytest.raises(N.FMError, match="shard"):
        group.rank(cu, cc, 10, 0.0, 1.0)
    group.close()
    repl = loaded(w, V, present, parallel="replicated", n_gpus=2, devices=[0, 0])
    got_i, got_s = repl.rank(cu, cc, 10, 0.0, 1.0)
    assert got_i.tobytes() == want_i.tobytes() and got_s.tobytes() == want_s.tobytes()
    repl.close()
    single.close()


def test_bad_arguments_and_steady_device_memory(gpu):
    lib = N.load()
    w, V, present, ctxs, cands = _small(Cn=1100)
    ctx = loaded(w, V, present)
    cu, cc = csr(ctxs), csr(cands)
    few = csr(R.take_rows(cands, np.arange(50)))
    ctx.rank(cu, cc, 1024, 0.0, 1.0)  # warmed
    live = lib.fm_device_bytes_live(), lib.fm_device_allocs_live()
    first = ctx.rank(cu, cc, 1024, 0.0, 1.0)
    assert (lib.fm_device_bytes_live(), lib.fm_device_allocs_live()) == live
    for rows, n_top in ((cc, 0), (few, 51), (cc, 1025), (cc, -1)):
        with pytest.raises(N.FMError, match="n_top"):
            ctx.rank(cu, rows, n_top, 0.0, 1.0)
        assert (lib.fm_device_bytes_live(), lib.fm_device_allocs_live()) == live
    empty = csr((np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0)))
    with pytest.raises(N.FMError, match="candidate"):
        ctx.rank(cu, empty, 1, 0.0, 1.0)
    idx, score = ctx.rank(empty, cc, 5, 0.0, 1.0)  # U = 0: nothing to do
    assert idx.shape == score.shape == (0, 5)
    assert lib.fm_rank_candidates(ctx.handle, None, None, 1, 0.0, 1.0, None, None) == -1
    assert lib.fm_rank_candidates(ctx.handle, cu.c, cc.c, 1, 0.0, 1.0, None, None) == -1
    assert lib.fm_rank_batch(ctx.handle, None, None, 1, 0.0, 1.0, None, None) == -1
    again = ctx.rank(cu, cc, 1024, 0.0, 1.0)  # neither the failures nor the calls changed anything
    assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
    assert ctx.epoch == 0 and len(ctx.loss_history()) == 0
    ctx.close()


def test_rank_batch_views_refusals_and_profile(gpu):
    w, V, present, ctxs, cands = _small(Cn=90)
    ctx = loaded(w, V, present)
    cu, cc = csr(ctxs), csr(cands)
    want = ctx.rank(cu, cc, 7, 0.0, 1.0)
    # candidates as split 1 of a split dataset: the view ranks, the dataset itself is refused
    both = R.take_rows(cands, np.concatenate([np.arange(20), np.arange(90)]))
    data = ctx.batch_splits(csr(both), [0, 20, 110])
    view = ctx.split_view(data, 1)
    bu = ctx.batch(cu)
    ctx.profile_enable(True)
    got = ctx.rank_batch(bu, view, 7, 0.0, 1.0)
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert {"rank_summary", "rank_score", "rank_merge"} <= set(prof)
    with pytest.raises(N.FMError, match="split"):
        ctx.rank_batch(bu, data, 7, 0.0, 1.0)
    # a batch refilled on the device (fm_batch_from_rows): the call waits for the gather
    src = ctx.batch(cc)
    sel = ctx.batch_from_rows(src, np.arange(90))
    got = ctx.rank_batch(bu, sel, 7, 0.0, 1.0)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    other = loaded(w, V, present)
    with pytest.raises(N.FMError, match="another context"):
        other.rank_batch(bu, sel, 7, 0.0, 1.0)
    other.close()
    for b in (view, sel, src, data, bu):
        b.close()
    ctx.close()


# -------------------------------------------------------------------------------- recommend
def test_recommend_against_transform_of_the_concatenated_rows(gpu):
    from fm_spark_amd.linalg import Vectors
    from fm_spark_amd.ml import DataFrame, FactorizationMachinesSGD

    rng = np.random.default_rng(51)
    nf, n_users, n_items = 60, 8, 40  # features: a user one-hot [0, 8), an item one-hot [8, 48), a few tags
    def vec(u, i):
        pairs = ([(u, 1.0)] if u is not None else []) + ([(8 + i, 1.0), (48 + i % 12, 0.5)] if i is not None else [])
        return Vectors.sparse(nf, pairs)
    seen = [(int(rng.integers(n_users)), int(rng.integers(n_items))) for _ in range(400)]
    train = DataFrame.from_rows([(float((u + i) % 3 == 0), vec(u, i)) for u, i in seen], ["label", "features"],
                                num_partitions=2)
    fm = (FactorizationMachinesSGD().setDimFactorization(4).setMaxIter(8).setStepSize(0.3).setRegParam(0.001)
          .setNumFeatures(nf).setSeed(3))
    model = fm.fit(train)
    users = DataFrame.from_rows([(u, vec(u, None)) for u in range(n_users)], ["user", "features"])
    items = DataFrame.from_rows([(i, vec(None, i)) for i in range(n_items)], ["item", "features"])
    out = model.recommend(users, items, 6)
    assert out.count() == n_users and out["user"] == list(range(n_users))
    pairs = DataFrame.from_rows([(u, i, vec(u, i)) for u in range(n_users) for i in range(n_items)],
                                ["user", "item", "features"])
    pred = np.asarray(model.transform(pairs)["prediction"]).reshape(n_users, n_items)
    free = np.asarray(model.copy({"minLabel": -INF, "maxLabel": INF}).transform(pairs)["prediction"]).reshape(
        n_users, n_items)
    tol = 64 * 2.0 ** -52 * (1.0 + np.abs(free).max())  # the same fp64 sums in another order, |terms| <= a few
    for u, recs in enumerate(out["recommendations"]):
        assert len(recs) == 6
        cand = [c for c, _ in recs]
        assert len(set(cand)) == 6
        for c, p in recs:
            assert abs(p - pred[u, c]) <= tol and model.getMinLabel() <= p <= model.getMaxLabel()
        key = free[u, cand]
        assert np.all(np.diff(key) <= tol)                               # in the unclamped score's order
        assert np.all(np.delete(free[u], cand) <= key[-1] + tol)         # and nothing better left out
    with pytest.raises(ValueError):
        model.recommend(users, items, 41)
