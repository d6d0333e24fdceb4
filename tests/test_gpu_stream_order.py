"""GPU: cross-stream ordering, tested by holding one stream back at a time.

Every asynchronous path of the library rests on events between a context's three streams: main (steps,
evaluation), side (fm_batch_prepare, the inline sort, the sharded route and owner prepare) and copy
(fm_step's uploads and the fm_batch_from_rows / from_pairs / sample_pairs refills).  The rest of the suite
checks what each kernel computes; at its shapes every kernel has finished long before the host enqueues
the next call, so a deleted wait changes nothing it observes.  Here a bounded delay (tests/stream_probe.py:
one wave spinning on the device clock, no flag, no gate) is enqueued on one lane immediately before the
call whose wait is under test, the calls are enqueued while it is pending, so the other lanes run ahead as
far as the events allow, and every bit of the result is compared with program order.  A missing wait then
gives a wrong bit on every run.

Harness.  A scenario is a function of a World that makes library calls through World.call, arms a delay
with World.hold(lane) and states its premise with World.premise().  It runs in two rounds on one context:
round 1 is a warm-up with fm_sync after every call, which sizes every buffer (the inputs all have
stream_cases.ROWS rows of stream_cases.LEN entries, so no call of round 2 grows one); the tables are
reloaded; round 2 is measured.  The program-order result comes from a fresh context that runs both rounds
with fm_sync after every call and ignores hold / premise; the held-back result from a fresh context whose
round 2 arms the delays and never syncs between calls.  The premise -- the newest token is still pending
at the point the scenario names -- is asserted, never skipped, so a delay too short to cover the enqueue
cannot pass silently.  The loss history, the exported tables, the evaluation records and every value a
call returned must be bitwise equal; one scenario per family is also held to the fp64 oracle at
tests/test_gpu_parity.py's tolerance, so the baseline is not only the library itself.  What a lost wait
would read is valid, in-range, stale data of the same shape (tests/stream_cases.py;
tests/test_stream_cases_cpu.py proves the oracle separates the two orders by more than ten tolerances).

Lanes.  A process opens four hardware queues, and two streams that share one hold each other back: which
queue a new stream gets depends on every stream the process made before (the rest of the suite leaves
torch's stream pool and many dead contexts behind), and in a whole-suite run the context's own main and
side streams did share one.  So one context lives at a time, its copy stream is created first (it has no
setter), and main and side are torch streams supplied through fm_set_stream / fm_set_side_stream, drawn
from torch's pool until the three lanes are pairwise independent (choose_lanes: a 2 ms delay on one, a
kernel and an event on the other must complete while it is pending).  test_lanes_are_independent proves
the result at the full delay for every ordered pair; test_unordered_work_is_reordered proves the method
sees a missing edge.

The edges, by their event in csrc/fm_capi.hip (lane held back in brackets):
  ev_fork      main -> side  two inline-sorted steps of different batches share the sort workspace [main]
  ev_join      side -> main  the inline step's update waits for its sort [side]
  ready        side -> main  prepare(b), step(b): the unfused update and the fused split [side]
  ev_upd_done  main -> side  inline step of A, then prepare(B) [main]
  last_use     main -> side  step of a view, re-point, prepare: rewrites the sorted view [main]
  built        copy -> main  refill b, then step / predict / evaluate / evaluate_binary / init_from_batch /
                             rank (b as contexts, as candidates) [copy]
  built        copy -> side  refill b, then prepare(b) [copy]
  last_use     main -> copy  step and asynchronous evaluate of b, then refill by from_rows, from_pairs,
                             sample_pairs (host lists, fm_lists) [main]
  ready        side -> copy  prepare(b) never stepped, then refill b [side].  Nothing reads that
                             preparation's view afterwards, so this scenario runs the path and its
                             premise; its bits cannot show the wait.
  copied / consumed          five fm_step(sync=False) over the two upload slots [main, then copy]
  the fit's loop             two batches refilled, prepared and stepped in turn, six iterations, each lane
                             held back in turn and re-armed every iteration
Sharded phases (csrc/fm_shard.hip, a world-1 HipShardEngine whose send buffers are its receive buffers):
ready_fwd, ready_upd [side], S.last_use [main], wait_built [copy], sh->last_use [main].

Delay.  DELAY_US = 50 ms per hold (the door clamps at 200 ms), the first value tried: every premise
held on the MI355X.  Measured there from the hold to the premise (printed by every premise, run with -s):
0.01 - 0.56 ms of host time wherever the calls do not wait by design (median 0.05 ms; the longest are the
first refills of a fresh batch, which allocate).  The fit loop's iterations 2 and 3 measure 50 ms: a refill
reuses its batch's pinned staging and so waits, by design, for that batch's refill of two iterations
before, which sits behind an earlier delay of the same lane; their own token is behind one more delay, so
the premise holds there by construction, not by speed.
"""

import dataclasses
import math
import time

import numpy as np
import pytest

import stream_cases as sc
from oracle import fm_ref as R

pytestmark = pytest.mark.gpu

DELAY_US = 50_000
MAIN, SIDE, COPY = "main", "side", "copy"
INF = math.inf


def _host(c):
    from fm_spark_amd._native import CSRHost

    return CSRHost(c.row_ptr, c.col, c.val, c.label)


PROBE_US = 2_000
_served = []  # torch streams that served as lanes before: tried first


def independent(sp, x, y):
    """Stream y runs a kernel and an event to completion while a short delay on stream x is pending."""
    tok = sp.delay(x, PROBE_US)
    other = sp.delay(y, 0)
    other.release()  # waits for y's kernel and event
    still = tok.pending()
    tok.release()
    return still


def choose_lanes(ctx):
    """Main and side streams for ctx, from torch's pool, pairwise independent of each other and of the
    context's copy stream (which exists already), installed through the setters -> the torch streams."""
    import stream_probe as sp
    import torch

    copy = sp.ctx_streams(ctx)[COPY]
    assert copy, "the copy stream is created by the first refill"
    chosen, seen = [], set()

    def candidates():
        yield from list(_served)
        for _ in range(64):
            yield torch.cuda.Stream()

    for st in candidates():
        h = st.cuda_stream
        if h in seen or h == copy:
            continue
        seen.add(h)
        if all(independent(sp, o, h) for o in [copy, *(c.cuda_stream for c in chosen)]):
            chosen.append(st)
            if len(chosen) == 2:
                break
    assert len(chosen) == 2, "no two streams of torch's pool are independent of the copy stream and of each other"
    for st in chosen:
        if st not in _served:
            _served.append(st)
    ctx.set_stream(chosen[0].cuda_stream)
    ctx.set_side_stream(chosen[1].cuda_stream)
    return chosen


class World:
    """One context, the resident inputs of stream_cases, and the bookkeeping of a two-round run."""

    def __init__(self, k, fuse, held, tables=True):
        import stream_probe as sp
        from fm_spark_amd.engine import FMContext

        self.sp = sp
        self.k, self.held = k, held
        self.ctx = FMContext(sc.F, k, fuse=fuse)
        csr, ids, w, V = sc.dataset(k)
        self.tables = (ids, w, V) if tables else None
        self.load()
        self.data = self.ctx.batch(_host(csr))
        self.splits = self.ctx.batch_splits(_host(csr), sc.split_rows())
        u, c = sc.pair_sources()
        self.U, self.C = self.ctx.batch(_host(u)), self.ctx.batch(_host(c))
        self.bands = self.ctx.batch(_host(band_rows()))
        self.fixed = self.ctx.batch(_host(sc.contents(k, "S5")))  # a batch no scenario refills
        self.hosts = [_host(sc.contents(k, f"S{i}")) for i in range(5)]  # fm_step's host batches
        self._lists = {}
        self.batches, self.contents = {}, {}
        # the copy stream exists from here on (the first call that copies creates it)
        self.scratch = self.ctx.batch_from_rows(self.data, sc.selection(0))
        self.ctx.sync()
        self.lanes = choose_lanes(self.ctx)
        self.round, self.t = 1, 0
        self.tokens, self.out, self.trace, self.retired = [], [], [[], []], []

    def load(self):
        if self.tables is not None:
            self.ctx.load_tables(*self.tables)

    # ------------------------------------------------------------------ the run
    @property
    def measuring(self):
        return self.held and self.round == 2

    def call(self, fn, *a, **kw):
        r = fn(*a, **kw)
        if not self.measuring:
            self.ctx.sync()
        return r

    def stream(self, lane):
        return self.sp.ctx_streams(self.ctx)[lane]

    def hold(self, lane):
        if self.measuring:
            assert len(self.tokens) < 8
            self.tokens.append(self.sp.delay(self.stream(lane), DELAY_US))
            self.armed = time.perf_counter()

    def premise(self, what="the calls under test"):
        if self.measuring:
            print(f"premise ({what}): {1e3 * (time.perf_counter() - self.armed):.3f} ms after the hold")
            assert self.tokens[-1].pending(), f"the delay ended before {what} were enqueued: raise DELAY_US"

    def other_stream(self):
        """A torch stream that is none of the lanes."""
        import torch

        while True:
            st = torch.cuda.Stream()
            if st.cuda_stream not in [self.stream(lane) for lane in (MAIN, SIDE, COPY)]:
                return st

    def keep(self, value):
        for v in value if isinstance(value, tuple) else (value,):
            self.out.append(np.array(v))

    # ------------------------------------------------------------------ the calls
    def b(self, name):
        return self.batches[name]

    def refill(self, name, key):
        """from_rows (S<i>), split_view (V<s>) or from_pairs (P<j>) into batch `name` (made at first use)."""
        into = self.batches.get(name)
        kind, n = key[0], int(key[1:])
        if kind == "S":
            b = self.call(self.ctx.batch_from_rows, self.data, sc.selection(n), into=into)
        elif kind == "V":
            b = self.call(self.ctx.split_view, self.splits, n, into=into)
        elif kind == "E":
            b = self.call(self.ctx.batch_from_rows, self.bands, np.arange(n * sc.ROWS, (n + 1) * sc.ROWS), into=into)
        else:
            b = self.call(self.ctx.batch_from_pairs, self.U, self.C, *sc.pair_list(n), into=into)
        assert b.n_rows == sc.ROWS and b.nnz == sc.ROWS * sc.LEN
        self.batches[name], self.contents[name] = b, key
        return b

    def sample(self, name, j, resident):
        """sample_pairs into batch `name`: positives j, exclude lists on the host or resident (fm_lists)."""
        pc, pd, lists = sc.positives(j)
        if resident and j not in self._lists:
            self._lists[j] = self.ctx.row_lists(lists, sc.N_CAND)
            self.ctx.sync()
        b = self.call(self.ctx.batch_sample_pairs, self.U, self.C, pc, pd, sc.N_NEG, exclude=self._lists[j] if resident else lists,
                      seed=11 + j, into=self.batches.get(name))
        assert b.n_rows == sc.ROWS and b.nnz == sc.ROWS * sc.LEN
        self.batches[name], self.contents[name] = b, None
        return b

    def fresh(self, name):
        """The next refill of `name` makes a new batch (the old one is kept until close: freeing device
        memory drains the device, which would hide the held-back lane)."""
        if name in self.batches:
            self.retired.append(self.batches.pop(name))

    def host_batch(self, name, key):
        """A batch uploaded from the host (fm_batch_create: no refill, no `built`), made in round 1."""
        if name not in self.batches:
            self.batches[name], self.contents[name] = self.ctx.batch(_host(sc.contents(self.k, key))), key
        return self.batches[name]

    def prepare(self, name):
        self.call(self.b(name).prepare)

    def step(self, name):
        self.t += 1
        self.trace[self.round - 1].append((self.contents[name], self.t))
        self.call(self.ctx.step_batch, self.b(name), self.t, sc.STEP, sc.REG, sync=False)

    def host_step(self, i):
        self.t += 1
        self.trace[self.round - 1].append((f"S{i}", self.t))
        self.call(self.ctx.step, self.hosts[i], self.t, sc.STEP, sc.REG, sync=False)

    # ------------------------------------------------------------------ the result
    def finish(self):
        self.ctx.sync()
        for t in self.tokens:
            assert not t.pending()
            t.release()
        ids, w, V = self.ctx.export_tables()
        res = {"loss": self.ctx.loss_history(), "ids": ids, "w": w, "V": V,
               "eval": np.array([dataclasses.astuple(e) for e in self.ctx.eval_history()], dtype=np.float64),
               "binary": np.array([dataclasses.astuple(e) for e in self.ctx.eval_binary_history()], dtype=np.float64)}
        for i, v in enumerate(self.out):
            res[f"out{i}"] = v
        return res

    def close(self):
        for b in [*self.batches.values(), *self.retired, self.scratch, self.fixed, self.bands, self.U, self.C, self.splits, self.data]:
            b.close()
        for l in self._lists.values():
            l.close()
        self.ctx.close()


_band_rows = []


def band_rows():
    """3 * ROWS rows of LEN entries whose ids lie in band r // ROWS of three ([0, 100), [100, 200), [200, 300)):
    what init_from_batch makes present tells which band it read."""
    if not _band_rows:
        from problems import make_rows

        parts = [make_rows(310 + i, np.full(sc.ROWS, sc.LEN), sc.F // 3, 1)[0] for i in range(3)]
        _band_rows.append(R.CSR(np.arange(3 * sc.ROWS + 1, dtype=np.int64) * sc.LEN,
                                np.concatenate([p.col + i * (sc.F // 3) for i, p in enumerate(parts)]).astype(np.int32),
                                np.concatenate([p.val for p in parts]), np.concatenate([p.label for p in parts])))
    return _band_rows[0]


def run(scenario, k, fuse, held, tables=True):
    """Both rounds of a scenario on a fresh context -> (result, trace of the steps per round)."""
    w = World(k, fuse, held, tables)
    try:
        scenario(w)
        w.ctx.sync()
        w.load()
        w.round = 2
        scenario(w)
        if held:
            assert w.tokens, "the scenario armed no delay"
        return w.finish(), w.trace
    finally:
        w.close()


_program = {}


def program_order(name, scenario, k, fuse, tables=True):
    """The program-order result, computed once per (scenario family, k, fuse) and left unchanged."""
    key = (name, k, fuse)
    if key not in _program:
        res, trace = run(scenario, k, fuse, held=False, tables=tables)
        for v in res.values():
            v.setflags(write=False)
        _program[key] = (res, trace)
    return _program[key]


def assert_bitwise(got, want):
    assert got.keys() == want.keys()
    for name in want:
        a, b = got[name], want[name]
        assert a.shape == b.shape and a.dtype == b.dtype, name
        if a.tobytes() != b.tobytes():
            bad = np.nonzero(np.atleast_1d(a != b).reshape(-1))[0]
            pytest.fail(f"{name}: {len(bad)} of {a.size} words differ from program order, first at {bad[:8]}")


def assert_oracle(k, res, trace):
    """The loss history and the final tables against sgd_step_fast in program order (both rounds, the
    tables reloaded between them), at tests/test_gpu_parity.py's tolerance."""
    losses = []
    for rnd in trace:
        model = None
        for key, t in rnd:
            l, model = sc.oracle_run(k, [key], t0=t, model=model)
            losses.append(l[0])
    assert len(losses) == len(res["loss"]) > 0
    np.testing.assert_allclose(res["loss"], losses, rtol=sc.RTOL, atol=sc.ATOL)
    np.testing.assert_array_equal(res["ids"], np.nonzero(model.present)[0])
    np.testing.assert_allclose(res["w"], model.w[res["ids"]], rtol=sc.RTOL, atol=sc.ATOL)
    np.testing.assert_allclose(res["V"], model.V[res["ids"]], rtol=sc.RTOL, atol=sc.ATOL)


def check(name, scenario, k, fuse, oracle=False, tables=True, program_name=None):
    want, _ = program_order(program_name or name, scenario, k, fuse, tables)
    got, trace = run(scenario, k, fuse, held=True, tables=tables)
    assert_bitwise(got, want)
    if oracle:
        assert_oracle(k, got, trace)


# (k, fuse): the unfused step at k = 8, the fused step (prepared batches) at k = 16
UNFUSED, FUSED = (8, False), (16, True)
BOTH = [pytest.param(*UNFUSED, id="k8"), pytest.param(*FUSED, id="k16-fused")]


# ---------------------------------------------------------------------------------- harness self-checks
def test_lanes_are_independent(gpu):
    """For each ordered pair of lanes (X, Y), X is held back; a trivial kernel and an event on Y complete
    while X's token is still pending."""
    w = World(8, False, held=True)
    try:
        lanes = {lane: w.stream(lane) for lane in (MAIN, SIDE, COPY)}
        assert all(lanes.values()) and len(set(lanes.values())) == 3
        assert lanes[MAIN] == w.lanes[0].cuda_stream and lanes[SIDE] == w.lanes[1].cuda_stream
        for x, sx in lanes.items():
            for y, sy in lanes.items():
                if x == y:
                    continue
                tok = w.sp.delay(sx, DELAY_US)
                other = w.sp.delay(sy, 0)
                other.release()  # waits for Y's kernel and event
                still = tok.pending()
                tok.release()
                assert still, f"work on {y} waited for the delay on {x}: the lanes share a queue"
    finally:
        w.close()


def test_unordered_work_is_reordered(gpu):
    """A torch fill on a held-back stream, read from another stream with no wait, is not seen: the method
    can see a missing edge."""
    import torch

    w = World(8, False, held=True)
    try:
        x = torch.zeros(4096, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        side = torch.cuda.ExternalStream(w.stream(SIDE))
        main = torch.cuda.ExternalStream(w.stream(MAIN))
        tok = w.sp.delay(w.stream(SIDE), DELAY_US)
        with torch.cuda.stream(side):
            x.fill_(1.0)
        with torch.cuda.stream(main):
            y = x.clone()
        main.synchronize()
        assert tok.pending()
        assert float(y.sum().item()) == 0.0  # (on the default stream, after main was drained)
        tok.release()
        side.synchronize()
        assert float(x.sum().item()) == 4096.0
    finally:
        w.close()


# ------------------------------------------------------------------------------- single-table scenarios
def s_ev_fork(w):
    w.host_batch("A", "S0")
    w.host_batch("B", "S1")
    w.hold(MAIN)
    w.step("A")
    w.step("B")
    w.premise()


def s_ev_join(w):
    w.host_batch("A", "S0")
    w.hold(SIDE)
    w.step("A")
    w.premise()
    w.step("A")


def s_ready(w):
    w.host_batch("A", "S0")
    w.host_batch("B", "S1")
    w.prepare("A")
    w.step("A")
    w.hold(SIDE)
    w.prepare("B")
    w.step("B")
    w.premise()


def s_ev_upd_done(w):
    w.host_batch("A", "S0")
    w.host_batch("B", "S1")
    w.hold(MAIN)
    w.step("A")
    w.prepare("B")
    w.premise()
    w.step("B")


def s_last_use_prepare(w):
    w.refill("v", "V0")
    w.prepare("v")
    w.hold(MAIN)
    w.step("v")
    w.refill("v", "V1")
    w.prepare("v")
    w.premise()
    w.step("v")


def test_ev_fork_second_sort_waits_for_first_update(gpu):
    check("ev_fork", s_ev_fork, *UNFUSED, oracle=True)


def test_ev_join_update_waits_for_inline_sort(gpu):
    check("ev_join", s_ev_join, *UNFUSED)


@pytest.mark.parametrize("k, fuse", BOTH)
def test_ready_step_waits_for_prepare(gpu, k, fuse):
    check("ready", s_ready, k, fuse, oracle=True)


@pytest.mark.parametrize("k, fuse", BOTH)
def test_ev_upd_done_prepare_waits_for_inline_update(gpu, k, fuse):
    check("ev_upd_done", s_ev_upd_done, k, fuse)


@pytest.mark.parametrize("k, fuse", BOTH)
def test_last_use_prepare_waits_for_step_of_the_view(gpu, k, fuse):
    check("last_use_prepare", s_last_use_prepare, k, fuse, oracle=True)


def r_step(w):
    w.step("b")


def r_predict(w):
    w.keep(w.call(w.ctx.predict_batch, w.b("b"), -INF, INF))


def r_evaluate(w):
    w.call(w.ctx.evaluate_batch, w.b("b"), -INF, INF, sync=False)


def r_evaluate_binary(w):
    w.call(w.ctx.evaluate_binary_batch, w.b("b"), sync=False)


def r_rank_contexts(w):
    w.keep(w.call(w.ctx.rank_batch, w.b("b"), w.fixed, 5, -INF, INF))


def r_rank_candidates(w):
    w.keep(w.call(w.ctx.rank_batch, w.fixed, w.b("b"), 5, -INF, INF))


READERS = {"step": r_step, "predict": r_predict, "evaluate": r_evaluate, "evaluate_binary": r_evaluate_binary,
           "rank_contexts": r_rank_contexts, "rank_candidates": r_rank_candidates}


def s_built_reader(reader):
    def scenario(w):
        w.refill("b", "S0")
        w.hold(COPY)
        w.refill("b", "S1")
        w.premise("the refill")
        reader(w)
        w.step("b")

    return scenario


@pytest.mark.parametrize("reader", sorted(READERS))
def test_built_reader_waits_for_refill(gpu, reader):
    check(f"built_{reader}", s_built_reader(READERS[reader]), *UNFUSED, oracle=reader == "step")


def s_built_init(w):
    """Round 1 makes band 2's ids present; round 2 refills band 0, then -- held back -- band 1, and
    init_from_batch must make band 1's ids present, not band 0's."""
    if w.round == 1:
        w.refill("b", "E2")
        w.refill("b", "E2")
    else:
        w.refill("b", "E0")
        w.hold(COPY)
        w.refill("b", "E1")
        w.premise("the refill")
    w.keep(w.call(w.ctx.init_from_batch, w.b("b")))


def test_built_init_from_batch_waits_for_refill(gpu):
    bands = band_rows().col.reshape(3, -1)
    assert all(bands[i].min() >= 100 * i and bands[i].max() < 100 * (i + 1) for i in range(3))
    check("built_init", s_built_init, *UNFUSED, tables=False)
    want, _ = program_order("built_init", s_built_init, *UNFUSED, tables=False)
    assert set(want["ids"]) == set(np.unique(bands[1])) | set(np.unique(bands[2]))


def s_built_prepare(w):
    w.refill("b", "S0")
    w.hold(COPY)
    w.refill("b", "S1")
    w.prepare("b")
    w.premise()
    w.step("b")


@pytest.mark.parametrize("k, fuse", BOTH)
def test_built_prepare_waits_for_refill(gpu, k, fuse):
    check("built_prepare", s_built_prepare, k, fuse, oracle=True)


def s_last_use_refill(kind):
    def scenario(w):
        first = {"rows": "S0", "pairs": "P0", "sample": "P0", "sample_lists": "P0"}[kind]
        w.refill("b", first)
        w.hold(MAIN)
        w.step("b")
        w.call(w.ctx.evaluate_batch, w.b("b"), -INF, INF, sync=False)
        if kind == "rows":
            w.refill("b", "S1")
        elif kind == "pairs":
            w.refill("b", "P1")
        else:
            w.sample("b", 0, resident=kind == "sample_lists")
        w.premise()
        w.call(w.ctx.evaluate_batch, w.b("b"), -INF, INF, sync=False)
        if kind in ("rows", "pairs"):
            w.step("b")

    return scenario


@pytest.mark.parametrize("kind", ["rows", "pairs", "sample", "sample_lists"])
def test_last_use_refill_waits_for_step_and_evaluate(gpu, kind):
    check(f"last_use_{kind}", s_last_use_refill(kind), *UNFUSED, oracle=kind in ("rows", "pairs"))


def s_ready_refill(w):
    w.refill("b", "S0")
    w.hold(SIDE)
    w.prepare("b")
    w.refill("b", "S1")
    w.premise()
    w.prepare("b")
    w.step("b")


@pytest.mark.parametrize("k, fuse", BOTH)
def test_ready_refill_after_a_preparation_never_stepped(gpu, k, fuse):
    check("ready_refill", s_ready_refill, k, fuse)


def s_host_slots(lane):
    def scenario(w):
        w.hold(lane)
        for i in range(5):
            w.host_step(i)
            if i == 1:
                w.premise("the first two fm_step calls")

    return scenario


@pytest.mark.parametrize("lane", [MAIN, COPY])
def test_fm_step_slots_copied_and_consumed(gpu, lane):
    check(f"host_slots_{lane}", s_host_slots(lane), *UNFUSED, oracle=lane == MAIN, program_name="host_slots")


def s_fit_loop(lane):
    """run_minibatch_sgd_resident's schedule over two batches: step j, prepare j + 1, refill j + 2 into the
    batch step j read."""

    def scenario(w):
        n = 6
        w.refill("b0", "S0")
        w.prepare("b0")
        w.refill("b1", "S1")
        for j in range(n):
            w.hold(lane)
            w.step(f"b{j % 2}")
            if j + 1 < n:
                w.prepare(f"b{(j + 1) % 2}")
            if j + 2 < n:
                w.refill(f"b{j % 2}", f"S{j + 2}")
            w.premise(f"iteration {j}")

    return scenario


@pytest.mark.parametrize("k, fuse", BOTH)
@pytest.mark.parametrize("lane", [MAIN, SIDE, COPY])
def test_fit_loop_with_each_lane_held_back(gpu, lane, k, fuse):
    check(f"fit_loop_{lane}", s_fit_loop(lane), k, fuse, oracle=lane == MAIN, program_name="fit_loop")


# --------------------------------------------------------------------------------------- stream setters
def s_set_stream(w):
    """The main stream switched mid-sequence: the first torch stream -> another -> NULL -> back, steps
    queued on the stream being left, which is held back."""
    w.host_batch("A", "S0")
    w.host_batch("B", "S1")
    if not hasattr(w, "torch_stream"):
        w.torch_stream = w.other_stream()
    for target in (w.torch_stream.cuda_stream, None, w.torch_stream.cuda_stream):
        w.hold(MAIN)
        w.step("A")
        w.step("B")
        w.premise()
        w.ctx.set_stream(target)
    w.step("A")


def s_set_side_stream(w):
    """The same for the side stream (NULL: the context's own), with a prepare queued on the stream being
    left."""
    w.host_batch("A", "S0")
    w.host_batch("B", "S1")
    if not hasattr(w, "torch_stream"):
        w.torch_stream = w.other_stream()
    for target in (w.torch_stream.cuda_stream, None, w.torch_stream.cuda_stream, None):
        w.hold(SIDE)
        w.prepare("A")
        w.premise()
        w.ctx.set_side_stream(target)
        w.step("A")
        w.step("B")


def test_set_stream_mid_sequence(gpu):
    check("set_stream", s_set_stream, *UNFUSED, oracle=True)


@pytest.mark.parametrize("k, fuse", BOTH)
def test_set_side_stream_mid_sequence(gpu, k, fuse):
    check("set_side_stream", s_set_side_stream, k, fuse)


# ------------------------------------------------------------------------- the header's "no host wait"
def s_no_host_wait_main(w):
    """With main held back, each of these returns while the delay is pending."""
    w.host_batch("A", "S0")
    w.host_batch("B", "S1")
    if w.round == 1:
        w.sample("q", 0, resident=False)
        w.refill("v", "V0")
    w.hold(MAIN)
    w.step("A")
    w.premise("step_batch(sync=False)")
    # (before anything queues on the copy stream behind main: the call waits for the copy stream)
    w.sample("q", 1, resident=False)
    w.premise("sample_pairs refilling a batch that is not in flight")
    w.host_step(2)
    w.host_step(3)
    w.premise("the first two fm_step(sync=False)")
    w.prepare("B")
    w.premise("prepare")
    w.refill("v", "V1" if w.round == 2 else "V2")
    w.premise("a split-view re-point")
    w.call(w.ctx.evaluate_batch, w.b("A"), -INF, INF, sync=False)
    w.premise("evaluate_batch(sync=False)")
    w.fresh("f")
    w.refill("f", "S3")
    w.premise("the first from_rows refill of a batch")
    w.fresh("g")
    w.refill("g", "P0")
    w.premise("the first from_pairs refill of a batch")
    w.step("B")
    w.step("f")
    w.step("g")


def s_no_host_wait_side(w):
    """With the side stream held back, the first refill of a fresh batch returns once it is enqueued: its
    staging event is new, nothing has used it, and the host must not wait for unrelated side-stream work."""
    w.host_batch("A", "S0")
    w.hold(SIDE)
    w.prepare("A")
    w.fresh("f")
    w.refill("f", "S3")
    w.premise("the first from_rows refill of a batch")
    w.fresh("g")
    w.refill("g", "P0")
    w.premise("the first from_pairs refill of a batch")
    w.fresh("q")
    w.sample("q", 0, resident=False)
    w.premise("the first sample_pairs refill of a batch")
    w.refill("q", "P1")
    w.premise("from_pairs into a batch sample_pairs made")
    w.step("A")
    w.step("f")
    w.step("g")
    w.step("q")


def test_no_host_wait_with_main_held_back(gpu):
    check("no_host_wait_main", s_no_host_wait_main, *UNFUSED)


def test_no_host_wait_with_side_held_back(gpu):
    check("no_host_wait_side", s_no_host_wait_side, *UNFUSED)


# --------------------------------------------------------------------------------------- sharded phases
SH_K = 8


def shard_inputs():
    """tests/shard_cases.py's rows at world 1 (every entry of owner 0, F = 300) and its table.  Rows of 6 and
    8 entries alternate, the other way round in every second block of ROWS rows: each block still holds
    ROWS * LEN entries in ROWS rows (no buffer grows, stale data stays in range), but two blocks' pair
    tables differ, so a forward that ran ahead of its owner_prepare would sum the wrong entries."""
    import shard_cases as shc

    if not _shard_inputs:
        i = np.arange(3 * sc.ROWS)
        has = np.where((i + i // sc.ROWS) % 2 == 0, sc.LEN - 1, sc.LEN + 1).reshape(-1, 1)
        csr, F = shc.by_owner(41, has, 1, slots=sc.F - 1)
        assert F == sc.F
        for blk in range(3):
            assert csr.row_ptr[(blk + 1) * sc.ROWS] - csr.row_ptr[blk * sc.ROWS] == sc.ROWS * sc.LEN
        assert not np.array_equal(np.diff(csr.row_ptr)[: sc.ROWS], np.diff(csr.row_ptr)[sc.ROWS: 2 * sc.ROWS])
        _shard_inputs.append((csr, shc._table(7, F, SH_K, absent_fifth=False)))
    return _shard_inputs[0]


_shard_inputs = []


def shard_rows(key):
    return np.arange(int(key[1:]) * sc.ROWS, (int(key[1:]) + 1) * sc.ROWS)


class ShardWorld(World):
    """A world-1 HipShardEngine driven phase by phase: its send buffers are its receive buffers.  Main and
    side are torch streams (choose_lanes), copy the context's own; no device synchronisation between the
    phases of a measured round.  The phases' buffers are torch tensors kept alive until close."""

    def __init__(self, held):
        import stream_probe as sp
        from fm_spark_amd.distributed import HipShardEngine

        self.sp, self.k, self.held = sp, SH_K, held
        csr, self.tables = shard_inputs()
        self.eng = HipShardEngine(sc.F, SH_K, 0, 1)
        self.ctx = self.eng.ctx
        self.load()
        self.data = self.eng.batch(_host(csr))
        self.batches, self.contents, self.bufs, self.tensors = {}, {}, {}, []
        self.scratch = self.ctx.batch_from_rows(self.data, shard_rows("R0"))
        self.ctx.sync()
        self.lanes = choose_lanes(self.ctx)
        self.eng.main_stream, self.eng.side_stream = self.lanes
        self.round, self.t = 1, 0
        self.tokens, self.out, self.trace, self.retired = [], [], [[], []], []
        self.log = []  # (phase, batch, contents) in call order, for the NumPy engine

    def refill(self, name, key):
        b = self.call(self.ctx.batch_from_rows, self.data, shard_rows(key), into=self.batches.get(name))
        self.batches[name], self.contents[name] = b, key
        self.log.append(("refill", name, key))

    def route(self, name):
        slot, ent, counts = self.call(self.eng.route, self.b(name))
        assert counts.tolist() == [sc.ROWS * sc.LEN, sc.ROWS]
        self.bufs[name] = (slot, ent, counts)
        self.tensors += [slot, ent]  # alive until close: queued work reads them
        self.log.append(("route", name, name))

    def owner_prepare(self, name, src=None):
        """src: the batch whose routed entries this owner received (default: its own)."""
        slot, ent, counts = self.bufs[src or name]
        self.call(self.eng.owner_prepare, self.b(name), slot, ent, counts[:1], counts[1:])
        self.log.append(("prepare", name, src or name))

    def forward_combine(self, name):
        part = self.call(self.eng.owner_forward, self.b(name), sc.ROWS)
        s = self.call(self.eng.combine, self.b(name), part, sc.ROWS)
        self.bufs[name + "/s"] = s
        self.tensors += [part, s]
        self.log.append(("forward_combine", name, name))

    def update(self, name):
        self.t += 1
        self.call(self.eng.owner_update, self.b(name), self.bufs[name + "/s"], self.t, sc.STEP, sc.REG, sc.ROWS)
        self.log.append(("update", name, self.t))

    def iteration(self, name):
        self.route(name)
        self.owner_prepare(name)
        self.forward_combine(name)
        self.update(name)

    def finish(self):
        self.ctx.sync()
        for t in self.tokens:
            assert not t.pending()
            t.release()
        ids, w, V = self.ctx.export_tables()
        return {"loss": self.ctx.loss_history(), "ids": ids, "w": w, "V": V}

    def close(self):
        for b in [*self.batches.values(), self.scratch, self.data]:
            b.close()
        self.ctx.close()


def shard_reference(log_by_round):
    """The same phases, in program order, on tests/shard_ref_engine.py's NumPy engine -> (losses, ids, w, V)."""
    from shard_ref_engine import NpBatch, NumpyShardEngine

    csr, tables = shard_inputs()
    losses = []
    for log in log_by_round:
        ref = NumpyShardEngine(sc.F, SH_K, 0, 1)
        ref.load_tables(*tables)
        batches, bufs = {}, {}
        for phase, name, arg in log:
            if phase == "refill":
                batches[name] = NpBatch(sc.take(csr, shard_rows(arg)))
            elif phase == "route":
                bufs[name] = ref.route(batches[name])
            elif phase == "prepare":
                slot, ent, counts = bufs[arg]
                ref.owner_prepare(batches[name], slot, ent, counts[:1], counts[1:])
            elif phase == "forward_combine":
                part = ref.owner_forward(batches[name], sc.ROWS)
                bufs[name + "/s"] = ref.combine(batches[name], part, sc.ROWS)
            else:
                ref.owner_update(batches[name], bufs[name + "/s"], arg, sc.STEP, sc.REG, sc.ROWS)
                losses.append(ref.last_stats()[0])
    return (np.asarray(losses), *ref.export_tables())


def run_sharded(scenario, held):
    w = ShardWorld(held)
    try:
        scenario(w)
        w.ctx.sync()
        w.load()
        first, w.log = w.log, []
        w.round = 2
        scenario(w)
        if held:
            assert w.tokens, "the scenario armed no delay"
        return w.finish(), (first, w.log)
    finally:
        w.close()


def check_sharded(scenario):
    want, _ = run_sharded(scenario, held=False)
    got, logs = run_sharded(scenario, held=True)
    assert_bitwise(got, want)
    losses, ids, w, V = shard_reference(logs)
    np.testing.assert_allclose(got["loss"], losses, rtol=sc.RTOL, atol=sc.ATOL)
    np.testing.assert_array_equal(got["ids"], ids)
    np.testing.assert_allclose(got["w"], w, rtol=sc.RTOL, atol=sc.ATOL)
    np.testing.assert_allclose(got["V"], V, rtol=sc.RTOL, atol=sc.ATOL)


def sh_ready(w):
    """owner_forward after owner_prepare (ready_fwd) and owner_update after the slot sort (ready_upd): side
    held back between route and prepare, after an iteration over other rows left its pair table and
    sorted view in the batch's state."""
    w.refill("b", "R0")
    w.iteration("b")
    w.refill("b", "R1")
    w.route("b")
    w.hold(SIDE)
    w.owner_prepare("b")
    w.forward_combine("b")
    w.update("b")
    w.premise()


def sh_state_last_use(w):
    """The next owner_prepare of the same batch, over other received entries, after an owner_update that is
    held back on main: it rewrites the sorted view the update reads (S.last_use)."""
    w.refill("b", "R0")
    w.refill("c", "R1")
    w.route("b")
    w.route("c")
    w.owner_prepare("b")
    w.forward_combine("b")
    w.hold(MAIN)
    w.update("b")
    w.owner_prepare("b", src="c")
    w.premise()
    w.forward_combine("b")
    w.update("b")


def sh_built(w):
    """route after a refill: copy held back (wait_built)."""
    w.refill("b", "R0")
    w.iteration("b")
    w.hold(COPY)
    w.refill("b", "R1")
    w.premise("the refill")
    w.iteration("b")


def sh_batch_last_use(w):
    """A refill after a sharded iteration: main held back (sh->last_use, recorded by owner_update)."""
    w.refill("b", "R0")
    w.route("b")
    w.owner_prepare("b")
    w.hold(MAIN)
    w.forward_combine("b")
    w.update("b")
    w.refill("b", "R1")
    w.premise()
    w.iteration("b")


@pytest.mark.parametrize("scenario", [sh_ready, sh_state_last_use, sh_built, sh_batch_last_use], ids=lambda f: f.__name__)
def test_sharded_phases(gpu, scenario):
    check_sharded(scenario)
