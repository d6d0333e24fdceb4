"""CPU: the cases of tests/test_gpu_optimizer_edges.py (tests/optimizer_cases.py) on the fp64 references alone.

Every named case holds its event under the events model at the geometry of the kernels as written (W = 256,
stretches 16 and 64, L = 128) and at one no build has; the model agrees with an entry-by-entry restatement on
random views; on the references, a step that omits any single piece (or window partial) of a designated run
moves that run's row by more than 8 budgets -- what lets the GPU comparison see a dropped or doubly-added piece;
and the references read a repeated id as repeat_cases' oracle does, far from its two misreadings.
"""

import copy

import numpy as np
import pytest

import adagrad_ref as A
import optimizer_cases as oc
import repeat_cases as rc
from oracle import fm_ref as R
from test_runs_cpu import geom

FTRL_GEOMS = [(256, 16), (256, 64), (96, 12), (96, 24)]  # today's two, and two no build has
ADA_GEOMS = [(128,), (48,)]
FTRL_NAMES = list(oc.ftrl_cases(256, 16))
ADA_NAMES = list(oc.ada_cases(128))
K_FULL = {16: (256, 16), 20: (256, 64), 68: (256, 64), 132: (256, 64)}  # the GPU test's k, with their stretch lengths


@pytest.mark.parametrize("g", FTRL_GEOMS)
def test_ftrl_cases_hold_their_events(g):
    for name, case in oc.ftrl_cases(*g).items():
        oc.assert_holds("ftrl", case, g)
        assert oc.designated("ftrl", case, g), name
    assert len(FTRL_NAMES) == 12


@pytest.mark.parametrize("g", ADA_GEOMS)
def test_adagrad_cases_hold_their_events(g):
    for name, case in oc.ada_cases(*g).items():
        oc.assert_holds("adagrad", case, g)
        assert oc.designated("adagrad", case, g), name


def test_absent_rows_reach_every_apply_site():
    """Every second case of either table loads its table without its designated ids: between them those runs
    are applied by all three FTRL sites and both AdaGrad sites."""
    for g in FTRL_GEOMS[:2]:
        sites = set()
        for name in FTRL_NAMES[1::2]:
            case = oc.ftrl_cases(*g)[name]
            ev, _ = oc.assert_holds("ftrl", case, g)
            sites |= {ev.site[i] for i in oc.designated("ftrl", case, g)}
        assert sites == {"stretch", "close", "fold"}, sites
    sites = set()
    for name in ADA_NAMES[1::2]:
        case = oc.ada_cases(128)[name]
        ev, _ = oc.assert_holds("adagrad", case, (128,))
        sites |= {ev.site[i] for i in oc.designated("adagrad", case, (128,))}
    assert sites == {"piece", "fold"}, sites


def test_events_agree_with_the_entry_by_entry_walk():
    rng = np.random.default_rng(2024)
    for trial in range(200):
        W, g = [(256, 16), (256, 64), (96, 12), (64, 16)][trial % 4]
        L = (128, 48, 7)[trial % 3]
        n_runs = int(rng.integers(1, 40))
        scale = (3, g, W, 3 * W)[int(rng.integers(0, 4))]
        lengths = rng.integers(1, scale + 1, n_runs)
        keys = np.repeat(np.sort(rng.choice(10 * n_runs, n_runs, replace=False)), lengths)
        ev = oc.ftrl_events(keys, W, g)
        got = [(int(f), int(l), s, p, sl) for f, l, s, p, sl in zip(ev.first, ev.last, ev.site, ev.pieces, ev.slots)]
        assert got == oc.ftrl_events_brute(keys, W, g)
        assert ev.n_pieces.tolist() == [sum(p) for p in ev.pieces] and ev.N == len(keys)
        ea = oc.ada_events(keys, L)
        got = [(int(f), int(l), s, int(n), [int(x) for x in sl])
               for f, l, s, n, sl in zip(ea.first, ea.last, ea.site, ea.n_pieces, ea.slots)]
        assert got == oc.ada_events_brute(keys, L)
        slots = [x for sl in ea.slots for x in sl]
        assert len(slots) == len(set(slots)) and all(x < 2 * (len(keys) // L + 1) for x in slots)  # no two pieces share one
        slots = [x for sl in ev.slots for x in sl]
        assert len(slots) == len(set(slots)) and all(x < 2 * ev.n_windows for x in slots)


@pytest.mark.parametrize("k", sorted(K_FULL))
@pytest.mark.parametrize("name", FTRL_NAMES)
def test_ftrl_omitted_piece_moves_its_row(name, k):
    c = oc.build("ftrl", name, k, K_FULL[k], absent=FTRL_NAMES.index(name) % 2 == 1)
    worst = c.margin
    print(f"ftrl {name} k={k}: an omitted piece moves its row by at least {worst:.1f} budgets (draw {c.draw}); one fp32 rounding of the "
          f"stored values per step moves the final table by {oc.conditioning(c):.2f}")
    assert worst > oc.FACTOR


@pytest.mark.parametrize("k", sorted(K_FULL))
@pytest.mark.parametrize("name", ADA_NAMES)
def test_adagrad_omitted_piece_moves_its_row(name, k):
    c = oc.build("adagrad", name, k, (128,), absent=ADA_NAMES.index(name) % 2 == 1)
    worst = c.margin
    print(f"adagrad {name} k={k}: an omitted piece moves its row by at least {worst:.1f} budgets (draw {c.draw}); one fp32 rounding of the "
          f"stored values per step moves the final table by {oc.conditioning(c):.2f}")
    assert worst > oc.FACTOR


# ------------------------------------------------------------------------------------- repeated ids
REPEAT = [(n, k) for n in rc.NAMES for k in rc.ks_of(n)]


def _loaded(c):
    model = R.Model.empty(c.F, c.k)
    model.load(c.keep, c.w[c.keep], c.V[c.keep])
    return model


@pytest.mark.parametrize("name,k", REPEAT)
def test_references_read_a_repeat_as_the_oracle_does(name, k):
    """AdaRef without its accumulator and with no L1 is the oracle's SGD step on every repeat_cases batch: each
    occurrence of a repeated id is an entry of its own."""
    c = rc.case(name, k, geom(k), False)
    ref, oracle = A.AdaRef(_loaded(c), A.G0, "sgd"), _loaded(c)
    for t, (b, s) in enumerate(zip(c.batches, c.steps), start=1):
        ro, oo = ref.step(b, t, s, 0.0), R.sgd_step_fast(oracle, b, t, s, 0.0)
        assert (ro.n_rows, ro.n_loss_rows, ro.n_unique) == (oo.n_rows, oo.n_loss_rows, oo.n_unique)
        assert ro.loss_sum == pytest.approx(oo.loss_sum, rel=A.RTOL, abs=A.ATOL)
    assert np.array_equal(ref.model.present, oracle.present)
    np.testing.assert_allclose(ref.model.w, oracle.w, rtol=A.RTOL, atol=A.ATOL)
    np.testing.assert_allclose(ref.model.V, oracle.V, rtol=A.RTOL, atol=A.ATOL)


@pytest.mark.parametrize("opt", ["adagrad", "ftrl"])
@pytest.mark.parametrize("name,k", REPEAT)
def test_misreadings_of_a_repeat_move_the_designated_rows(name, k, opt):
    c = rc.case(name, k, geom(k), False)
    mod = oc.consts(opt)
    ref, _, before = oc.repeat_reference(opt, c)
    bw, bV = ref.budget()
    des = np.asarray(c.des, dtype=np.int64)
    worst = []
    for read in (rc.merged, rc.first_only):
        other = copy.deepcopy(before)
        other.step(read(c.batches[1]), 2, mod.STEP, mod.REG)
        move = np.maximum(np.abs(other.model.w[des] - ref.model.w[des]) / bw[des],
                          (np.abs(other.model.V[des] - ref.model.V[des]) / bV[des]).max(axis=1))
        worst.append(float(move.min()))
    print(f"{opt} {name} k={k}: (merged, first-only) move the designated rows by at least {worst[0]:.1f} {worst[1]:.1f} budgets")
    assert min(worst) > rc.FACTOR
