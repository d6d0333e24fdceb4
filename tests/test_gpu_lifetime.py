"""GPU: device-memory lifetime of long-lived contexts, on the library's own live-allocation counter
(fm_device_bytes_live / fm_device_allocs_live: every hipMalloc / hipFree of the library, process-wide;
tests/test_lifetime_source.py keeps it complete).  The library lives inside one Spark driver for a whole
fit -- hundreds of iterations, model Datasets queried by id between them, CrossValidator creating and
destroying models -- so: a call repeated with the same sizes allocates nothing, a call that fails
frees what it took, no step allocates after fm_reserve, and destroying every batch and context
returns both counters to where they started.  Every comparison is exact equality of both counters
(the device's free memory is shared with other work and says nothing).

Context kinds: the single table with the fused step on and off, one manual shard (1 of 3: the table
entry points and batch creation -- its step is driven through the fm_shard_* phases by a caller that
owns the wire buffers), and the three-rank sharded and replicated contexts (COPY transport on one GPU).

With the counter alone and DevBuf not yet owning its memory, 24 of these tests failed (allocations per
call): fm_export_rows +4 on every context kind (+12 on sharded3, 4 per rank: 23100 bytes per call of
300 rows at k = 8), fm_loss_grad / fm_calc_loss_grad +5 (single and replicated3, also on the absent-id
error path: 92052 bytes per call), and through fm_export_rows every create/destroy cycle.  The other
argument errors are found before anything is allocated and the per-rank lists of the multi-GPU
contexts held; they are pinned here so that they stay that way."""

import functools

import numpy as np
import pytest

from problems import make_problem

pytestmark = pytest.mark.gpu

F, ROWS, NNZ = 2000, 200, 6
KINDS = ["fused", "unfused", "shard1of3", "sharded3", "replicated3"]
STEP, REG = 0.3, 1e-4


def counters():
    from fm_spark_amd import _native as N

    lib = N.load()
    return int(lib.fm_device_bytes_live()), int(lib.fm_device_allocs_live())


def host(csr):
    from fm_spark_amd._native import CSRHost

    return CSRHost(csr.row_ptr, csr.col, csr.val, csr.label)


@functools.lru_cache(maxsize=None)
def problem(k, seed=0):
    """(batch, ids, w, V): 200 rows x ~6 entries over F = 2000 ids, the whole table to load."""
    return make_problem(900 + seed, ROWS, F, k, NNZ)


def make_ctx(kind, k=8, num_features=F, **kw):
    from fm_spark_amd.engine import FMContext

    if kind in ("sharded3", "replicated3"):
        return FMContext(num_features, k, parallel=kind[:-1], n_gpus=3, devices=[0] * 3, transport="copy", **kw)
    if kind == "shard1of3":
        return FMContext(num_features, k, shard_index=1, shard_count=3, **kw)
    return FMContext(num_features, k, fuse=(kind == "fused"), **kw)


def owned(kind, ids):
    return ids[ids % 3 == 1] if kind == "shard1of3" else ids


def cycle_split_rows(n):
    return np.array([0, n // 3, n // 3, n - 7, n], dtype=np.int64)  # an empty split among them


class Env:
    """One context of a kind with the whole table loaded, a device batch, a split dataset of the same
    rows with two reusable handles (a selection and a view: what fit refills every iteration), and the
    calls it answers."""

    def __init__(self, kind, k):
        self.kind, self.k = kind, k
        csr, ids, w, V = problem(k)
        self.csr, self.ids, self.w, self.V = csr, ids, w, V
        self.ctx = ctx = make_ctx(kind, k)
        ctx.load_tables(ids, w, V)
        self.hb = host(csr)
        self.db = ctx.batch(self.hb)
        self.data = ctx.batch_splits(self.hb, cycle_split_rows(csr.n_rows))
        self.rows = np.arange(0, csr.n_rows, 2, dtype=np.int64)  # a fixed 100-row list
        self.sel = ctx.batch_from_rows(self.db, self.rows)
        self.view = ctx.split_view(self.data, 0)
        self.n_views = 0
        self.own = owned(kind, ids)
        self.t = 0
        rng = np.random.default_rng(5)
        self.keys = rng.integers(0, 300, 1000).astype(np.int32)
        self.vecs = rng.normal(size=(1000, k))

    def close(self):
        for b in (self.sel, self.view, self.data, self.db):  # views before the dataset they borrow from
            b.close()
        self.ctx.close()

    def split_view_into(self):
        self.n_views += 1
        self.ctx.split_view(self.data, (0, 2)[self.n_views % 2], into=self.view)  # the two large splits in turn

    def view_selection_cycle(self):
        """A selection becomes a view and a selection again: the call ends in the state it started in."""
        self.ctx.split_view(self.data, 2, into=self.sel)
        self.ctx.batch_from_rows(self.db, self.rows, into=self.sel)

    def profiled_steps(self):
        self.ctx.profile_enable(True)
        for _ in range(2):
            self.t += 1
            self.db.prepare()
            self.ctx.step_batch(self.db, self.t, STEP, REG)
        prof = self.ctx.profile_read()
        assert prof and all(n > 0 for _, n in prof.values())

    def calls(self):
        ctx, own = self.ctx, self.own
        sub = own[:: 7]
        c = {
            "export_rows": lambda: ctx.export_rows(own[:300]),
            "export_tables": lambda: ctx.export_tables(),
            "num_present": lambda: ctx.num_present(),
            "load_tables": lambda: ctx.load_tables(sub, self.w[sub], self.V[sub]),
            "init_random": lambda: ctx.init_random(sub),
            "init_random_range": lambda: ctx.init_random_range(100, 900),
            "init_from_batch": lambda: ctx.init_from_batch(self.db),
            "vector_sum_by_key": lambda: ctx.vector_sum_by_key(self.keys, self.vecs),
            "loss_history": lambda: ctx.loss_history(),
            "from_rows_into": lambda: ctx.batch_from_rows(self.db, self.rows, into=self.sel),
            "split_view_into": self.split_view_into,
            "view_selection_cycle": self.view_selection_cycle,
        }
        if self.kind != "shard1of3":
            c["predict"] = lambda: ctx.predict(self.hb, -1.0, 2.0)
            c["predict_batch"] = lambda: ctx.predict_batch(self.db, -1.0, 2.0)
            c["profile_read"] = self.profiled_steps
        if self.kind in ("fused", "unfused", "replicated3"):
            c["loss_grad"] = lambda: ctx.loss_grad(self.hb)
            c["loss_grad_initial_sd"] = lambda: ctx.loss_grad(self.hb, initial_sd=0.01, seed=3)
        return c


CALLS = ["export_rows", "export_tables", "num_present", "load_tables", "init_random", "init_random_range",
         "init_from_batch", "predict", "predict_batch", "loss_grad", "loss_grad_initial_sd", "vector_sum_by_key",
         "loss_history", "profile_read", "from_rows_into", "split_view_into", "view_selection_cycle"]


@pytest.fixture(scope="module")
def envs():
    made = {}

    def get(kind, k=8):
        if (kind, k) not in made:
            made[(kind, k)] = Env(kind, k)
        return made[(kind, k)]

    yield get
    for e in made.values():
        e.close()


def answers(kind, call):
    if kind == "shard1of3":
        return call not in ("predict", "predict_batch", "profile_read", "loss_grad", "loss_grad_initial_sd")
    if kind == "sharded3":
        return call not in ("loss_grad", "loss_grad_initial_sd")  # the per-entry outputs need the whole table
    return True


@pytest.mark.parametrize("kind,call", [(kind, call) for kind in KINDS for call in CALLS if answers(kind, call)])
def test_steady_state_call_allocates_nothing(gpu, envs, kind, call):
    """Two warm-up calls (workspaces and the reused host batch may grow), then 8 more with the same
    sizes: both counters unchanged, exactly."""
    f = envs(kind).calls()[call]
    f()
    f()
    before = counters()
    for _ in range(8):
        f()
    after = counters()
    assert after == before, f"{kind} {call}: {after[1] - before[1]:+d} allocations, {after[0] - before[0]:+d} bytes in 8 calls"


def _bad_csr(what):
    csr = problem(8)[0]
    col, rp = csr.col.copy(), csr.row_ptr.copy()
    if what == "col":
        col[len(col) // 2] = F
    else:
        full = np.nonzero(np.diff(rp) > 0)[0]
        i = int(full[len(full) // 2])
        rp[i + 1] = rp[i] - 1  # row_ptr steps back in the middle; the ends still run from 0 to nnz
    from oracle import fm_ref as R

    return host(R.CSR(rp, col, csr.val, csr.label))


def _error_calls(kind, ctx, ids, w, V):
    k = ctx.k
    big = np.array([3, F], dtype=np.int32)
    c = {
        "export_rows_id_ge_F": lambda: ctx.export_rows(np.array([1, 4, F + 2], dtype=np.int32)),
        "load_tables_id_out_of_range": lambda: ctx.load_tables(big, np.zeros(2), np.zeros((2, k))),
        "batch_col_ge_F": lambda: ctx.batch(_bad_csr("col")),
        "batch_row_ptr_not_monotone": lambda: ctx.batch(_bad_csr("row_ptr")),
    }
    if kind == "shard1of3":
        c["export_rows_id_not_owned"] = lambda: ctx.export_rows(np.array([1, 4, 5], dtype=np.int32))
    if kind in ("fused", "unfused", "replicated3"):
        c["loss_grad_absent_ids"] = lambda: ctx.loss_grad(host(problem(8)[0]))
    return c


ERRORS = ["loss_grad_absent_ids", "export_rows_id_ge_F", "export_rows_id_not_owned", "load_tables_id_out_of_range",
          "batch_col_ge_F", "batch_row_ptr_not_monotone"]


def has_error(kind, err):
    if err == "export_rows_id_not_owned":
        return kind == "shard1of3"  # one process holds every rank of a multi-GPU context: it owns every id
    if err == "loss_grad_absent_ids":
        return kind in ("fused", "unfused", "replicated3")
    return True


@pytest.mark.parametrize("kind,err", [(kind, err) for kind in KINDS for err in ERRORS if has_error(kind, err)])
def test_failing_call_frees_what_it_took(gpu, kind, err):
    """Argument errors the C-ABI reports as FM_ERR_ARG, some of them found only after the call has
    allocated (the absent-id flag of fm_loss_grad comes back from the device): the failing call leaves
    both counters where they were."""
    from fm_spark_amd._native import FMError

    _, ids, w, V = problem(8)
    ctx = make_ctx(kind)
    half = ids[ids % 2 == 0]  # the odd ids stay absent: fm_loss_grad refuses the batch
    ctx.load_tables(half, w[half], V[half])
    f = _error_calls(kind, ctx, ids, w, V)[err]
    for _ in range(2):  # the reused host batch and staging may grow once
        with pytest.raises(FMError):
            f()
    before = counters()
    for _ in range(8):
        with pytest.raises(FMError):
            f()
    after = counters()
    ctx.close()
    assert after == before, f"{kind} {err}: {after[1] - before[1]:+d} allocations, {after[0] - before[0]:+d} bytes in 8 calls"


@pytest.mark.parametrize("source", ["prepared", "host"])
@pytest.mark.parametrize("kind,k", [("fused", 8), ("fused", 16), ("unfused", 8), ("unfused", 16), ("sharded3", 8),
                                    ("replicated3", 8)])
def test_no_step_allocates_after_reserve(gpu, kind, k, source):
    """include/fm_hip.h on fm_reserve: "Pre-size the per-step workspace so no step allocates".  After
    reserve(max_rows, max_nnz) and 3 warm steps over 3 batches, 40 more steps cycling them leave both
    counters unchanged -- from prepared device batches and from host CSRs.  fm_reserve sizes the step's
    workspace, not fm_step's two upload slots (include/fm_hip.h): each grows to the largest host batch
    it has held, so the host-CSR variant warms with 6 steps -- every batch through both slots -- not 3."""
    probs = [problem(k, seed=s)[0] for s in (1, 2, 3)]
    _, ids, w, V = problem(k)
    ctx = make_ctx(kind, k)
    ctx.load_tables(ids, w, V)
    ctx.reserve(max(p.n_rows for p in probs), max(p.nnz for p in probs))
    hbs = [host(p) for p in probs]
    dbs = [ctx.batch(h) for h in hbs] if source == "prepared" else []

    def step(t):
        if source == "prepared":
            b = dbs[(t - 1) % 3]
            b.prepare()
            ctx.step_batch(b, t, STEP, REG, sync=False)
        else:
            ctx.step(hbs[(t - 1) % 3], t, STEP, REG, sync=False)

    warm = 3 if source == "prepared" else 6  # fm_step: each of its two upload slots has held each batch
    for t in range(1, warm + 1):
        step(t)
    ctx.sync()
    before = counters()
    for t in range(warm + 1, warm + 41):
        step(t)
    ctx.sync()
    after = counters()
    assert ctx.epoch == warm + 40
    for b in dbs:
        b.close()
    ctx.close()
    assert after == before, f"{kind} k={k} {source}: {after[1] - before[1]:+d} allocations, {after[0] - before[0]:+d} bytes in 40 steps"


def _cycle(kind, ctx_first):
    """One model's life: a context, one batch of every kind, two steps, a transform, rows by id; then
    everything is closed -- the batches first, or (ctx_first) the context first."""
    csr, ids, w, V = problem(8)
    hb = host(csr)
    ctx = make_ctx(kind)
    ctx.load_tables(ids, w, V)
    n = csr.n_rows
    split_rows = cycle_split_rows(n)
    order = np.random.default_rng(1).permutation(n)
    plain = ctx.batch(hb)
    data = ctx.batch_splits(hb, split_rows)
    laid = ctx.batch_layout_splits(hb, split_rows, order)
    view = ctx.split_view(data, 0)
    view = ctx.split_view(laid, 3, into=view)  # re-pointed once
    sel = ctx.batch_from_rows(plain, np.arange(0, n, 2))
    sel = ctx.batch_from_rows(plain, np.arange(n - 1, -1, -1), into=sel)  # refilled once, larger
    batches = [plain, data, laid, view, sel]
    if kind != "shard1of3":
        for t, b in enumerate((view, sel), start=1):
            b.prepare()
            ctx.step_batch(b, t, STEP, REG)
        assert ctx.epoch == 2
        assert np.all(np.isfinite(ctx.predict_batch(plain, -1.0, 2.0)))
    own = owned(kind, ids)
    assert ctx.export_rows(own[:50])[2].all()
    if ctx_first:
        ctx.close()
        for b in batches:
            b.close()
    else:
        for b in reversed(batches):  # views before the datasets they borrow from
            b.close()
        ctx.close()


@pytest.mark.parametrize("ctx_first", [False, True], ids=["batches_first", "context_first"])
@pytest.mark.parametrize("kind", KINDS)
def test_create_destroy_returns_to_baseline(gpu, kind, ctx_first):
    """10 lives of a model (CrossValidator): both counters end where they began.  context_first:
    fm_destroy before fm_batch_destroy, which include/fm_hip.h allows (a batch's destructor touches
    only its own events and buffers)."""
    _cycle(kind, ctx_first)  # the process's first use of the device, kept out of the reading
    before = counters()
    for _ in range(10):
        _cycle(kind, ctx_first)
    after = counters()
    assert after == before, f"{kind}: {after[1] - before[1]:+d} allocations, {after[0] - before[0]:+d} bytes after 10 cycles"


def test_counter_sees_the_table(gpu):
    """F = 2^20 rows of k = 8 (a 16-float record each) are 64 MiB: creating the context raises the live
    bytes by at least that, destroying it brings both counters back."""
    before = counters()
    ctx = make_ctx("unfused", 8, num_features=1 << 20)
    during = counters()
    ctx.close()
    after = counters()
    assert during[0] - before[0] >= 64 << 20 and during[1] > before[1]
    assert during[0] - before[0] < 2 * (64 << 20)
    assert after == before
