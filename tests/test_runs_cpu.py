"""CPU: the run-structured batch builder (tests/runs.py) and the layouts of tests/test_gpu_update_edges.py
(tests/update_cases.py), with no GPU.

make_runs against a stable host sort; layout, sprinkle and compact against each other; classify's model
of the update kernels' control flow on hand-made views; then every case of the GPU file: its second
batch's sorted view is the layout, the layout holds the structural events the case is named for (the
same assertion the GPU test makes before it runs), and the designated boundary entries meet the
sensitivity condition on the oracle alone.

The geometry comes from the built library through tests/update_probe.py (a host call: no GPU); where
the probe has not been built, GEOM_AS_OF_WRITING stands in, and a second, made-up geometry is always
run, so the layouts are shown to follow the geometry and not today's constants.
"""

import numpy as np
import pytest

import runs
import update_cases as uc
from update_probe import Geometry

# k -> entries per lane group as fm_update.hip had them when this was written; only a stand-in for an
# unbuilt probe (the GPU tests never read it)
GEOM_AS_OF_WRITING = {1: 4, 5: 8, 8: 8, 9: 16, 12: 16, 16: 16, 24: 32, 32: 32, 3: 4}


def geom(k):
    try:
        import update_probe

        return update_probe.geometry(k)
    except (RuntimeError, OSError, ImportError):
        G = GEOM_AS_OF_WRITING.get(k, 64)
        return Geometry(256, G, 1024, G in (8, 16) and (k + 3) // 4 * 4 == G, 16, 10, 1024, 12288)


def other_geom(k):
    """A geometry no build has: half-size waves, blocks of two waves, other groups, 8 lanes per range."""
    G = {1: 8, 8: 4, 16: 32}.get(k, 16)
    return Geometry(128, G, 256, False, 8, 6, 512, 64)


# ------------------------------------------------------------------------------------- the builders
@pytest.mark.parametrize("seed,n_rows", [(1, None), (2, 41), (3, 700)])
def test_make_runs_sorted_view_is_the_runs(seed, n_rows):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 40, 60)
    lens[7] = 41
    ids = np.sort(rng.choice(500, 60, replace=False))
    big = np.asarray([0, 5, int(lens.sum()) - 1])
    csr, all_ids, w, V = runs.make_runs(seed, lens, 500, 3, n_rows=n_rows, ids=ids, big=big)
    order = np.argsort(csr.col, kind="stable")
    np.testing.assert_array_equal(csr.col[order], np.repeat(ids, lens))
    # entry at sorted position p lies in row p mod n_rows: distinct rows within a run, rows filled evenly
    m = csr.n_rows
    rows = np.repeat(np.arange(m), np.diff(csr.row_ptr))
    np.testing.assert_array_equal(np.sort(rows[order].reshape(-1)), np.sort(np.arange(len(order)) % m))
    at = 0
    for n in lens:
        assert len(set(rows[order[at:at + n]].tolist())) == n
        at += n
    assert np.diff(csr.row_ptr).max() - np.diff(csr.row_ptr).min() <= 1
    for a, b in zip(csr.row_ptr[:-1], csr.row_ptr[1:]):
        assert (np.diff(csr.col[a:b]) > 0).all()  # ids distinct within a row
    np.testing.assert_array_equal(runs.rows_of_view(lens, m), rows[order])
    assert (np.abs(csr.val[order[big]]) == 6.0).all() and (np.abs(csr.label[rows[order[big]]]) == 10.0).all()
    assert (csr.val == csr.val.astype(np.float32)).all() and (csr.val == 0).any() and (csr.val == 1).any()
    assert w.shape == (500,) and V.shape == (500, 3) and (all_ids == np.arange(500)).all()


def test_layout_sprinkle_compact():
    spans = [(5, 9), (10, 11), (20, 20), (31, 40)]
    for fill in (1, 2, 7):
        sp = [s for s in spans if fill == 1 or s[0] != s[1]]
        lens = runs.layout(50, sp, fill)
        assert lens.sum() == 50 and (fill == 1 or lens.min() >= 2)
        starts = np.concatenate([[0], np.cumsum(lens)])
        for a, b in sp:
            i = int(np.searchsorted(starts, a))
            assert starts[i] == a and lens[i] == b - a + 1
    with pytest.raises(AssertionError):
        runs.layout(10, [(1, 4)], 2)  # a gap of 1 cannot hold a run of 2
    c = runs.layout(40, [(3, 9)], 2)
    assert 3 in c  # the odd gap's run of 3
    full, idx = runs.sprinkle(c)
    keys = np.repeat(np.arange(len(full)), full)
    kept, pos = runs.compact(keys)
    np.testing.assert_array_equal(np.diff(np.nonzero(np.diff(kept, prepend=-1))[0], append=len(kept)), c)
    np.testing.assert_array_equal(full[idx], c)
    assert (full == 1).sum() >= 3 and len(pos) == c.sum()


def test_classify_models_the_kernels_on_hand_made_views():
    g = Geometry(16, 4, 32, False, 16, 10, 8, 4)  # 4 groups of 4 per wave, 2 waves per block
    keys = np.repeat(np.arange(6), [4, 2, 9, 1, 17, 3])  # 36 entries
    ev = runs.classify_update(keys, g)
    assert ev.n_runs == 6 and "run_fills_group" in ev.flags and "last_wave_partial" in ev.flags
    # run 2 = [6, 14]: a tail from group 1 through whole group 2, closing in group 3 before its end
    assert (1, True) in ev.tail_chains
    # run 4 = [16, 32]: opens wave 1 at its first entry, fills it, ends on the first entry of wave 2
    assert ev.run_is_wave == [] and [r.c for r in ev.owners_two] == [1] and ev.owners_two[0].head == 1
    assert "owner_starts_on_p0_later" in ev.flags and "head_closed_in_first_group" in ev.flags
    long = np.repeat(np.arange(3), [5, 16 * 66 + 1, 9])
    ev = runs.classify_update(long, g)
    (rec,) = ev.owners_long
    assert (rec.c, rec.follow, rec.rounds) == (0, 66, [64, 2]) and set(ev.nonowners_inside) == set(range(1, 66))
    sp = runs.classify_split(np.repeat(np.arange(7), [1, 2, 5, 1, 1, 7, 2]), g)  # 19 entries, chunks of 8
    assert sp.nchunks == 3 and sp.nm.tolist() == [7, 6, 3] and sp.ns.tolist() == [1, 2, 0]
    # entry 16 closes the run of 7 as its chunk's first entry: only the key before the chunk says it is multi
    assert sp.after.tolist() == [False, False, False] and sp.before.tolist() == [False, False, True]
    sp = runs.classify_split(np.repeat(np.arange(4), [7, 2, 6, 1]), g)  # a run of 2 astride entries 7 | 8
    assert sp.after[0] and sp.before[1] and sp.rounds == 1


# ------------------------------------------------------------------------------------- every case
CASES = [(n, k) for n in uc.LAYOUTS for k in uc.ks_of(n)]


@pytest.mark.parametrize("name", list(uc.LAYOUTS) + list(uc.SPLIT))
def test_layouts_follow_the_geometry(name):
    """Every layout holds its events under a geometry no build has (the check runs inside the builder)."""
    for k in (1, 8, 16, 64):
        g = other_geom(k)
        lay = (uc.SPLIT.get(name) or uc.LAYOUTS[name])(g)
        if name in uc.SPLIT:
            lay.check(runs.classify_split(np.repeat(np.arange(len(l := runs.layout(lay.N, lay.spans, 2))), l), g))
            continue
        for fill in (1, 2):
            if fill == 2 and name in uc.UNFUSED_ONLY:
                continue
            lens = runs.layout(lay.N, lay.spans, getattr(lay, "fill", fill))
            lay.check(runs.classify_update(np.repeat(np.arange(len(lens)), lens), g))


@pytest.mark.parametrize("name,k", [(n, k) for n, k in CASES if n in uc.STRUCT or k <= 12])
def test_case_events_and_sensitivity(name, k):
    """The case as the GPU test builds it, from the library's geometry: view, events (checked in the
    builder), sensitivity; and its fused form where there is one."""
    g = geom(k)
    for fused in (False, True):
        if fused and not uc.fusable(name, k):
            continue
        c = uc.case(name, k, g, fused)
        uc.assert_case(c)
        if fused:
            kept, _ = runs.compact(c.keys)
            assert len(kept) < len(c.keys)  # singletons were sprinkled in, and the split removes them
            lay = uc.LAYOUTS[name](g)
            assert len(kept) == lay.N


@pytest.mark.parametrize("name,k", [(n, k) for n, k in CASES if n in uc.LONG and k > 12])
def test_long_case_sensitivity_wide(name, k):
    c = uc.case(name, k, geom(k))
    uc.assert_case(c)


@pytest.mark.parametrize("name", list(uc.SPLIT))
@pytest.mark.parametrize("k", uc.K_SPLIT)
def test_split_case_events_and_sensitivity(name, k):
    c = uc.case(name, k, geom(k))
    uc.assert_case(c)
    assert c.fused and c.events.split.N == len(c.keys)
