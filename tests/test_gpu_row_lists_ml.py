"""GPU: the training loop over resident exclude lists.  A hand loop of 6 iterations over two batches in turn
(sample, prepare, step) with the lists handed over as host lists at every call against the same loop with a
RowLists built on the device from the interactions -- same seeds, so the tables and the loss history must be
equal byte for byte; and fitInteractions, which builds its default lists that way, against fitInteractions
given the same lists explicitly."""

import numpy as np
import pytest

import pair_ref as P
from fm_spark_amd import _native as N
from test_gpu_pairs_ml import estimator, frames

pytestmark = pytest.mark.gpu


def hand_loop(resident):
    from fm_spark_amd.engine import FMContext

    p = P.planted()
    n, m = 384, 96  # a few hundred interactions: six contexts' rows of every residue class
    pos_ctx, pos_cand = p.pos_ctx[:n], p.pos_cand[:n]
    ctx = FMContext(p.F, P.K, seed=3, init_sd=P.SD)
    bu, bc = (ctx.batch(N.CSRHost(rp, col, val, np.zeros(len(rp) - 1))) for rp, col, val in (p.contexts, p.candidates))
    ctx.init_from_batch(bu)
    ctx.init_from_batch(bc)
    if resident:
        ex = ctx.row_lists_from_pairs(pos_ctx, pos_cand, p.U, p.C)
    else:
        ex = [np.unique(pos_cand[pos_ctx == u]) for u in range(p.U)]
    perm = np.random.default_rng(5).permutation(n)
    bufs = [None, None]
    for t in range(1, 7):
        take = perm[((t - 1) * m + np.arange(m)) % n]
        bufs[t % 2] = ctx.batch_sample_pairs(bu, bc, pos_ctx[take], pos_cand[take], P.NEG, exclude=ex, seed=1000 + t,
                                             into=bufs[t % 2])
        bufs[t % 2].prepare()
        ctx.step_batch(bufs[t % 2], t, 20.0, 1e-4, sync=False)
    ctx.sync()
    out = (ctx.export_tables(), ctx.loss_history())
    if resident:
        lists = ex.export()
        ex.close()
    else:
        lists = None
    ctx.close()
    return out, lists


def test_hand_loop_with_resident_lists_equals_host_lists(gpu):
    (tab_h, loss_h), _ = hand_loop(False)
    (tab_r, loss_r), lists = hand_loop(True)
    assert len(loss_h) == 6 and loss_h.tobytes() == loss_r.tobytes()
    for x, y in zip(tab_h, tab_r):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    p = P.planted()
    assert lists[0][-1] == 384 and np.array_equal(lists[1], np.concatenate(p.train[:16]))  # 16 contexts of 24 rows


def test_fit_interactions_default_lists_equal_explicit_ones(gpu):
    p, contexts, candidates, interactions = frames()
    a = estimator(6).fitInteractions(contexts, candidates, interactions)
    b = estimator(6).fitInteractions(contexts, candidates, interactions, exclude=p.train)
    assert a._ctx.epoch == b._ctx.epoch == 6
    assert a._ctx.loss_history().tobytes() == b._ctx.loss_history().tobytes()
    for x, y in zip(a._ctx.export_tables(), b._ctx.export_tables()):
        assert x.tobytes() == y.tobytes()
