"""GPU: the AdaGrad and FTRL update stages (fm_adagrad.hip, fm_ftrl.hip) at their cut edges, in all four lane-group
configurations, against tests/adagrad_ref.py / tests/ftrl_ref.py and their budgets.

with_ada_cfg / with_ftrl_cfg pick Q = 4 / NF = 1 up to kp = 16, Q = 16 / NF = 1 up to 64, NF = 2 up to 128 and NF = 4
above: K_ALL holds both sides of each boundary.  The named cases of tests/optimizer_cases.py (runs placed by
absolute sorted position in units of the seams W, stretch and L; every case asserts through the events model that
it holds the event it is named for before anything runs) are stepped three times -- the case's batch, its layout
behind a lead of 7, the case's batch again -- so the rows applied by the stretch walk, the LDS close phase,
k_ftrl_fold, k_ada_piece and k_ada_fold are updated with live state, and every second case loads its table without
its designated ids (the absent-row branch of every apply site; tests/test_optimizer_cases_cpu.py asserts the
coverage and that an omitted piece would move its row by more than 8 budgets).  Checked: the whole table within
the reference's budget, the step's counts exactly, the loss at RTOL / ATOL, FTRL's exact zeros, and equal bytes
from a prepared step, an inline-sorted one and a second context.  Every test prints its largest error over budget.
"""

import functools

import numpy as np
import pytest

import adagrad_ref as A
import ftrl_ref as Fr
import optimizer_cases as oc
import repeat_cases as rc
import runs
import test_gpu_adagrad as TA
import test_gpu_ftrl as TF
from fm_spark_amd import _native as N
from oracle import fm_ref as R
from problems import f32

pytestmark = pytest.mark.gpu

K_ALL = (4, 16, 20, 64, 68, 128, 132)  # kp 4, 16 (Q = 4) | 20, 64 (NF = 1) | 68, 128 (NF = 2) | 132 (NF = 4)
K_FULL = (16, 20, 68, 132)  # the full case table: one k of every configuration
K_REST = tuple(k for k in K_ALL if k not in K_FULL)
MOD = {"adagrad": TA, "ftrl": TF}
FTRL_NAMES = list(oc.ftrl_cases(256, 64))
ADA_NAMES = list(oc.ada_cases(128))
FAN_OUT = {"ftrl": "48-owning-windows", "adagrad": "48-runs-of-L+1"}


def geometry(opt, k):
    """(W, stretch) or (L,) of the built library for a table of k factors."""
    lib = N.load()
    if opt == "adagrad":
        return (int(lib.fm_seam_adagrad_piece()),)
    return int(lib.fm_seam_ftrl_window()) & 0xFFFF, int(lib.fm_seam_ftrl_stretch((k + 3) // 4 * 4))


def _bytes(tab):
    return [np.ascontiguousarray(a).tobytes() for a in tab]


def _stepped(opt, F, k, keep, w, V, batches, prepare=False):
    ctx = MOD[opt].new_ctx(F, k, keep, w[keep], V[keep])
    outs = MOD[opt].run_steps(ctx, batches, prepare=prepare)
    tab = ctx.export_tables()
    ctx.close()
    return outs, tab


def _assert_stats(outs, ros, rtol, atol):
    for go, ro in zip(outs, ros):
        assert (go.n_rows, go.n_loss_rows, go.n_unique) == (ro.n_rows, ro.n_loss_rows, ro.n_unique)
        assert go.loss_sum == pytest.approx(ro.loss_sum, rel=rtol, abs=atol)


def _assert_zeros(ref, tab, what):
    touched, zeroed = ref.zeroed(Fr.REG)
    print(f"{what}: {int(zeroed.sum())} of {int(touched.sum())} touched coordinates lie safely inside the threshold"
          + (" (none: the exact-zero check is empty here)" if not zeroed.any() else ""))
    assert np.all(np.column_stack([tab[1], tab[2]])[zeroed[tab[0]]] == 0.0)


@functools.lru_cache(maxsize=None)
def _reference(opt, name, k, geom, absent):
    c = oc.build(opt, name, k, geom, absent=absent)
    ref, ros, _ = oc.reference(c)
    return c, ref, ros


def _run_case(opt, names, name, k):
    geom = geometry(opt, k)
    c, ref, ros = _reference(opt, name, k, geom, names.index(name) % 2 == 1)
    ev, ix = oc.assert_holds(opt, c.case, geom)  # the case holds its event under the library's own geometry
    sites = sorted({c.events.site[i] for i in c.des} | {c.events_shifted.site[i + 1] for i in c.des})
    if name == FAN_OUT[opt] and (k + 3) // 4 * 4 > 16:
        n_owners = len(ev.owners) if opt == "ftrl" else len(ev.hot)
        assert n_owners > 2 * 16  # 16 lane groups of 16 lanes per block: owners in the fold grid's third block
    assert c.margin > oc.FACTOR, (name, k, geom, c.margin)  # the separation, at the library's own geometry
    what = f"{opt} {name} k={k} absent={c.absent} sites={'/'.join(sites)} draw={c.draw}"
    outs, tab = _stepped(opt, c.F, k, c.keep, c.w, c.V, c.batches)
    _assert_stats(outs, ros, oc.consts(opt).RTOL, oc.consts(opt).ATOL)
    assert outs[0].n_unique == len(c.lengths) and outs[1].n_unique == len(c.lengths) + 1
    MOD[opt].assert_within_budget(ref, tab, what)
    if opt == "ftrl":
        _assert_zeros(ref, tab, what)
    # bits: a prepared batch, and a second context
    _, prepared = _stepped(opt, c.F, k, c.keep, c.w, c.V, c.batches, prepare=True)
    _, again = _stepped(opt, c.F, k, c.keep, c.w, c.V, c.batches)
    assert _bytes(tab) == _bytes(prepared) == _bytes(again)


@pytest.mark.parametrize("k", K_FULL)
@pytest.mark.parametrize("name", FTRL_NAMES)
def test_ftrl_case(gpu, name, k):
    _run_case("ftrl", FTRL_NAMES, name, k)


@pytest.mark.parametrize("k", K_FULL)
@pytest.mark.parametrize("name", ADA_NAMES)
def test_adagrad_case(gpu, name, k):
    _run_case("adagrad", ADA_NAMES, name, k)


# ------------------------------------------------------------------------------------- the other widths
def _geometry_lists(opt, k, lengths, seed):
    F = len(lengths) + 2
    csr, ids, w, V = runs.make_runs(seed, lengths, F, k)
    model = R.Model.empty(F, k)
    model.load(ids, w, V)
    mod = oc.consts(opt)
    ref = A.AdaRef(model, A.G0) if opt == "adagrad" else Fr.FtrlRef(model)
    ros = [ref.step(csr, t, mod.STEP, mod.REG) for t in (1, 2)]  # the second step meets live state
    outs, tab = _stepped(opt, F, k, ids, w, V, [csr, csr])
    _assert_stats(outs, ros, mod.RTOL, mod.ATOL)
    assert outs[0].n_unique == len(lengths)
    return ref, tab


@pytest.mark.parametrize("k", K_REST)
@pytest.mark.parametrize("lead", [0, 7])
def test_ftrl_run_geometry_at_the_other_widths(gpu, k, lead):
    W, g = geometry("ftrl", k)
    ref, tab = _geometry_lists("ftrl", k, TF.geometry_lengths(W, g, lead), 11 + k)
    TF.assert_within_budget(ref, tab, f"ftrl geometry k={k} W={W} g={g} lead={lead}")
    _assert_zeros(ref, tab, f"ftrl geometry k={k} lead={lead}")


@pytest.mark.parametrize("k", K_REST)
def test_adagrad_run_geometry_at_the_other_widths(gpu, k):
    (L,) = geometry("adagrad", k)
    ref, tab = _geometry_lists("adagrad", k, TA.geometry_lengths(L), 11 + k)
    TA.assert_within_budget(ref, tab, f"adagrad geometry k={k} L={L}")


# ------------------------------------------------------------------------------------- bits at another offset
@pytest.mark.parametrize("k", [68, 132])
@pytest.mark.parametrize("n_of", ["L+1", "2L", "3L+1"])
def test_adagrad_multi_piece_run_gives_the_same_bits_behind_77_entries(gpu, k, n_of):
    """tests/test_gpu_adagrad.py's offset test at NF = 2 and 4, for runs of several pieces: rows 0 .. n - 1 hold id
    X and one partner id above it (so X's V gradient is not identically zero); the other 77 rows hold one entry
    each of ids above every partner, or below X: the run begins the view, or lies 77 entries in."""
    (L,) = geometry("adagrad", k)
    n = {"L+1": L + 1, "2L": 2 * L, "3L+1": 3 * L + 1}[n_of]
    fill, X, F = 77, 100, 260
    partner = 110 + np.arange(n) % 30
    assert oc.ada_events(np.repeat([X], n), L).site[0] == "fold"
    rng = np.random.default_rng(k)
    x, y = f32(rng.normal(0, 1, 2 * n + fill)), f32(rng.normal(0, 1, n + fill))
    w, V = f32(rng.normal(0, 0.1, F)), f32(rng.normal(0, 0.1, (F, k)))
    ptr = np.concatenate([2 * np.arange(n), 2 * n + np.arange(fill + 1)]).astype(np.int64)
    rows = []
    for base in (200, 0):  # the filler ids' rows hold the same values wherever they lie
        col = np.concatenate([np.column_stack([np.full(n, X), partner]).reshape(-1), base + np.arange(fill) % 50]).astype(np.int32)
        Vb, wb = V.copy(), w.copy()
        Vb[base:base + 50], wb[base:base + 50] = V[200:250], w[200:250]
        csr = R.CSR(ptr, col, x, y)
        _, keys = runs.sorted_view(csr)
        assert int(np.nonzero(keys == X)[0][0]) == (0 if base else fill)
        ctx = TA.new_ctx(F, k, np.arange(F, dtype=np.int32), wb, Vb)
        TA.run_steps(ctx, [csr])
        rows.append(ctx.export_rows(np.array([X], np.int32)))
        ctx.close()
    assert all(np.array_equal(a, b) for a, b in zip(*rows))


# ------------------------------------------------------------------------------------- a run of explicit zeros
@pytest.mark.parametrize("k", [16, 68])
@pytest.mark.parametrize("opt", ["adagrad", "ftrl"])
def test_a_run_of_explicit_zeros(gpu, opt, k):
    """Feature Z's every entry has x = 0: its V gradient is exactly 0, so the reference keeps V[Z] (AdaGrad: but
    for the L1 shrink) and FTRL's n stays 0 -- the second step is again a first touch."""
    W, _ = geometry("ftrl", k)
    lengths, Z = [7, 2 * W + 5, 3, 40, W // 2], 1
    F = len(lengths) + 2
    csr, ids, w, V = runs.make_runs(77 + k, lengths, F, k)
    csr.val[csr.col == Z] = 0.0
    mod = oc.consts(opt)
    model = R.Model.empty(F, k)
    model.load(ids, w, V)
    ref = A.AdaRef(model, A.G0) if opt == "adagrad" else Fr.FtrlRef(model)
    ros = [ref.step(csr, t, mod.STEP, mod.REG) for t in (1, 2)]
    bw, bV = ref.budget()
    if opt == "ftrl":
        assert np.all(ref.nV[Z] == 0.0) and ref.nw[Z] > 0.0
        assert np.all(np.abs(ref.model.V[Z] - V[Z]) <= bV[Z])
    else:
        assert np.all(ref.GV[Z] == f32(A.G0)) and ref.Gw[Z] > f32(A.G0)
    outs, tab = _stepped(opt, F, k, ids, w, V, [csr, csr])
    _assert_stats(outs, ros, mod.RTOL, mod.ATOL)
    MOD[opt].assert_within_budget(ref, tab, f"{opt} zero run k={k}")
    eZ = np.abs(tab[2][Z] - ref.model.V[Z]) / bV[Z]
    print(f"{opt} zero run k={k}: V[Z] largest error over budget {eZ.max():.3f}")


# ------------------------------------------------------------------------------------- repeated ids
REPEAT = [(n, k) for n in rc.NAMES for k in rc.ks_of(n)]


@pytest.mark.parametrize("opt", ["adagrad", "ftrl"])
@pytest.mark.parametrize("name,k", REPEAT)
def test_rows_that_repeat_an_id(gpu, name, k, opt):
    """The repeat_cases batches (each occurrence an entry of its own; the id counts once in n_unique), unprepared
    and prepared.  Both stages are single-GPU and never fused: those are all the paths."""
    import update_probe

    c = rc.case(name, k, update_probe.geometry(k))
    rc.assert_case(c)
    ref, ros, _ = oc.repeat_reference(opt, c)
    mod = oc.consts(opt)
    outs, tab = _stepped(opt, c.F, k, c.keep, c.w, c.V, c.batches)
    _assert_stats(outs, ros, mod.RTOL, mod.ATOL)
    assert outs[1].n_unique == len(np.unique(c.batches[1].col))
    MOD[opt].assert_within_budget(ref, tab, f"{opt} repeated ids {name} k={k}")
    _, prepared = _stepped(opt, c.F, k, c.keep, c.w, c.V, c.batches, prepare=True)
    assert _bytes(tab) == _bytes(prepared)


# ------------------------------------------------------------------------------------- FTRL's hyper-parameter edges
@pytest.mark.parametrize("reg,l2", [(0.0, Fr.L2), (Fr.REG, 0.0), (0.0, 0.0)])
def test_ftrl_hyper_parameter_edges(gpu, reg, l2):
    """reg_param = 0 (nothing is zeroed unless z is exactly 0) and opt_l2 = 0: where sgn(0) and |z| <= lambda1
    meet.  The designated rows arrive absent (v = 0 at the first touch), and every entry of the first of them has
    x = 0: its V coordinates start from z = 0 and take a gradient of exactly 0, so z' = 0 = lambda1 at reg_param = 0
    -- the reference zeroes them, and the device must give 0.0."""
    from fm_spark_amd.engine import FMContext

    k = 20
    geom = geometry("ftrl", k)
    c = oc.build("ftrl", "ends-on-stretch-and-window-last", k, geom, absent=True)
    oc.assert_holds("ftrl", c.case, geom)
    Z = int(c.des_ids[0])
    batches = [R.CSR(b.row_ptr, b.col, np.where(b.col == Z, 0.0, b.val), b.label) for b in c.batches]
    ref = oc.new_ref("ftrl", c, l2=l2)
    ctx = FMContext(c.F, k, optimizer="ftrl", opt_init=Fr.BETA, opt_l2=l2)
    ctx.load_tables(c.keep, c.w[c.keep], c.V[c.keep])
    for t, csr in enumerate(batches, start=1):
        ro = ref.step(csr, t, Fr.STEP, reg)
        go = ctx.step(N.CSRHost(csr.row_ptr, csr.col, csr.val, csr.label), t, Fr.STEP, reg)
        assert (go.n_rows, go.n_loss_rows, go.n_unique) == (ro.n_rows, ro.n_loss_rows, ro.n_unique)
        assert go.loss_sum == pytest.approx(ro.loss_sum, rel=Fr.RTOL, abs=Fr.ATOL)
    tab = ctx.export_tables()
    ctx.close()
    TF.assert_within_budget(ref, tab, f"ftrl reg={reg} l2={l2}")
    assert np.all(ref.lV[Z] == 0.0) and np.all(ref.nV[Z] == 0.0) and ref.lw[Z] > reg  # z' exactly 0 on all of V[Z]
    last = np.column_stack([ref.lw, ref.lV])
    touched, zeroed = np.isfinite(last), last <= reg * (1.0 - 1e-3)
    got = np.column_stack([tab[1], tab[2]])
    print(f"ftrl reg={reg} l2={l2}: {int(zeroed.sum())} of {int(touched.sum())} touched coordinates are zeroed by the reference")
    assert zeroed[Z, 1:].all() and np.all(got[zeroed[tab[0]]] == 0.0)
