"""Pythonic handle over one fm_ctx (one device's FM tables) — thin, no arithmetic.

Every method calls straight through the C-ABI of include/fm_hip.h; errors raise FMError.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N


@dataclass
class StepOut:
    loss_sum: float
    n_rows: int
    n_loss_rows: int
    n_unique: int
    executed: bool = True


@dataclass(frozen=True)
class EvalSums:
    """One evaluation record (fm_eval_out): the sums of e = label - prediction over the rows of a
    batch, formed on the device in fp64, and the metrics RegressionEvaluator derives from them."""

    n_rows: int
    n_unlearned: int
    epoch: int
    sum_err: float
    sum_abs_err: float
    sum_sq_err: float
    executed: bool = True

    @staticmethod
    def from_struct(o: "N.fm_eval_out", executed: bool = True) -> "EvalSums":
        return EvalSums(int(o.n_rows), int(o.n_unlearned), int(o.epoch), float(o.sum_err), float(o.sum_abs_err),
                        float(o.sum_sq_err), executed)

    @property
    def mae(self) -> float:
        return self.sum_abs_err / self.n_rows

    @property
    def mse(self) -> float:
        return self.sum_sq_err / self.n_rows

    @property
    def rmse(self) -> float:
        return float(np.sqrt(self.mse))

    @property
    def bias(self) -> float:
        """mean (label - prediction)"""
        return self.sum_err / self.n_rows

    def r2(self, ss_tot: float) -> float:
        """1 - SS_err / SS_tot; SS_tot = sum (y - mean y)^2 comes from the caller's labels (two-pass,
        on the host: include/fm_hip.h, fm_eval_out)."""
        return 1.0 - self.sum_sq_err / ss_tot


def _ratio(num, den) -> float:
    return float(num) / float(den) if den else float("nan")


@dataclass(frozen=True)
class BinarySums:
    """One binary evaluation record (fm_binary_out): the class counts, the confusion counts at the
    threshold score > 0, twice the Mann-Whitney U of the positives over the negatives and the log loss
    sum, formed on the device, and the metrics BinaryClassificationEvaluator derives from them.  A metric
    whose denominator is 0 is NaN."""

    n_rows: int
    n_pos: int
    epoch: int
    tp: int
    fp: int
    two_u: int
    sum_log_loss: float
    executed: bool = True

    @staticmethod
    def from_struct(o: "N.fm_binary_out", executed: bool = True) -> "BinarySums":
        return BinarySums(int(o.n_rows), int(o.n_pos), int(o.epoch), int(o.tp), int(o.fp), int(o.two_u),
                          float(o.sum_log_loss), executed)

    @property
    def n_neg(self) -> int:
        return self.n_rows - self.n_pos

    @property
    def logLoss(self) -> float:
        """mean softplus(score) - label * score"""
        return _ratio(self.sum_log_loss, self.n_rows)

    @property
    def auc(self) -> float:
        """area under the ROC curve, ties counted as half: two_u / (2 n_pos n_neg), from exact integers"""
        return _ratio(self.two_u, 2 * self.n_pos * self.n_neg)

    @property
    def accuracy(self) -> float:
        return _ratio(self.tp + (self.n_neg - self.fp), self.n_rows)

    @property
    def precision(self) -> float:
        return _ratio(self.tp, self.tp + self.fp)

    @property
    def recall(self) -> float:
        return _ratio(self.tp, self.n_pos)

    @property
    def f1(self) -> float:
        return _ratio(2 * self.tp, self.tp + self.fp + self.n_pos)


class DeviceBatch:
    """A CSR mini-batch resident in HBM (fm_batch_create)."""

    def __init__(self, ctx: "FMContext", csr: N.CSRHost | None):
        self._lib = N.load()
        self.ctx = ctx
        h = C.c_void_p()
        self.handle = h
        self.n_rows = self.nnz = 0
        if csr is not None:
            N.check(self._lib.fm_batch_create(ctx.handle, C.byref(csr.c), C.byref(h)), "fm_batch_create")
            self.n_rows = csr.n_rows
            self.nnz = csr.nnz

    def select_rows(self, data: "DeviceBatch", rows):
        """Refill this batch with rows[i] of the resident dataset `data`, on the device
        (fm_batch_from_rows); returns self."""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        h = self.handle if self.handle else C.c_void_p()
        N.check(self._lib.fm_batch_from_rows(self.ctx.handle, data.handle, N.ptr(rows, C.c_int64), len(rows),
                                             C.byref(h)), "fm_batch_from_rows")
        self.handle = h
        self.n_rows = len(rows)
        self.nnz = int(self._lib.fm_batch_nnz(h))
        self._data = data  # the dataset stays alive while this batch's gather may be queued
        return self

    def view_split(self, data: "DeviceBatch", split: int):
        """Re-point this batch at split `split` of the split-ordered dataset `data`
        (fm_batch_split_view: no copy, no device work); returns self."""
        h = self.handle if self.handle else C.c_void_p()
        N.check(self._lib.fm_batch_split_view(self.ctx.handle, data.handle, int(split), C.byref(h)),
                "fm_batch_split_view")
        self.handle = h
        self.n_rows = int(self._lib.fm_batch_rows(h))
        self.nnz = int(self._lib.fm_batch_nnz(h))
        self._data = data  # the dataset outlives the view (its rows are borrowed)
        return self

    def set_group(self, group: int):
        """Mark every ``group`` consecutive rows as a positive followed by its negatives, which a "bpr"
        context's step reads (fm_batch_set_group): 0 = ungrouped, else 2 .. 1025 and a divisor of n_rows.
        Returns self."""
        N.check(self._lib.fm_batch_set_group(self.ctx.handle, self.handle, int(group)), "fm_batch_set_group")
        return self

    @property
    def group(self) -> int:
        """Rows per group (fm_batch_group): set by set_group and by batch_sample_pairs (1 + n_neg), reset
        to 0 by every other refill."""
        return int(self._lib.fm_batch_group(self.handle)) if self.handle else 0

    def prepare(self):
        """Sort this batch by feature on the side stream ahead of its step (fm_batch_prepare)."""
        N.check(self._lib.fm_batch_prepare(self.ctx.handle, self.handle), "fm_batch_prepare")

    def close(self):
        if self.handle:
            self._lib.fm_batch_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RowLists:
    """Per-context candidate-row lists resident in HBM (fm_lists_create / fm_lists_from_pairs): built once,
    then passed wherever a call of the same context takes ``only`` / ``exclude`` / ``targets`` lists over
    resident batches, which then checks, stages and uploads nothing of them."""

    def __init__(self, ctx: "FMContext", handle):
        self._lib = N.load()
        self.ctx = ctx
        self.handle = handle
        self.n_contexts = int(self._lib.fm_lists_contexts(handle))
        self.n_candidates = int(self._lib.fm_lists_candidates(handle))
        self.total = int(self._lib.fm_lists_total(handle))
        self.longest = int(self._lib.fm_lists_longest(handle))

    def export(self):
        """(ptr int64 [n_contexts + 1], rows int32 [total]) read back from the device (fm_lists_export)."""
        ptr = np.zeros(self.n_contexts + 1, dtype=np.int64)
        rows = np.zeros(max(self.total, 1), dtype=np.int32)
        N.check(self._lib.fm_lists_export(self.ctx.handle, self.handle, N.ptr(ptr, C.c_int64), N.ptr(rows, C.c_int32),
                                          len(rows)), "fm_lists_export")
        return ptr, rows[: self.total]

    def close(self):
        if self.handle:
            self._lib.fm_lists_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def comm_unique_id() -> bytes:
    """RCCL unique id (128 bytes) that process 0 of a multi-process job hands to the others
    (fm_comm_unique_id)."""
    lib = N.load()
    buf = (C.c_uint8 * 128)()
    N.check(lib.fm_comm_unique_id(buf), "fm_comm_unique_id")
    return bytes(buf)


def normalize_row_lists(lists, n_ctx: int):
    """The per-context row lists of rank(only= / exclude=) as the C-ABI takes them: (ptr int64
    [n_ctx + 1], rows int32), every list sorted and without duplicates.  ``lists``: a sequence of
    n_ctx integer sequences, or a CSR pair (ptr, rows) -- a tuple of two 1-D NumPy arrays whose
    first holds n_ctx + 1 offsets (so two contexts' lists go in a list, not a tuple).  A wrong number of
    lists, entries that are not integers, or rows outside int32 raise ValueError; whether a row is a
    candidate row is the library's check."""
    if (isinstance(lists, tuple) and len(lists) == 2 and all(isinstance(a, np.ndarray) and a.ndim == 1 for a in lists)
            and len(lists[0]) == n_ctx + 1):
        ptr, flat = lists
        if ptr.dtype.kind not in "iu" or (flat.size and flat.dtype.kind not in "iu"):
            raise ValueError("row lists must hold integers")
        ptr = ptr.astype(np.int64)
        if ptr[0] != 0 or np.any(np.diff(ptr) < 0) or ptr[-1] != flat.size:
            raise ValueError("(ptr, rows): ptr must start at 0, not decrease and end at len(rows)")
        parts = [flat[ptr[u]:ptr[u + 1]] for u in range(n_ctx)]
    else:
        parts = [np.asarray(r) for r in lists]
        if len(parts) != n_ctx:
            raise ValueError(f"expected one row list per context ({n_ctx}), got {len(parts)}")
    out = []
    for u, r in enumerate(parts):
        if r.ndim != 1 or (r.size and r.dtype.kind not in "iu"):
            raise ValueError(f"row list of context {u} must be a flat sequence of integers")
        r = np.unique(r.astype(np.int64))
        if r.size and (r[0] < -2**31 or r[-1] >= 2**31):
            raise ValueError(f"row list of context {u} holds a row outside int32")
        out.append(r.astype(np.int32))
    ptr = np.zeros(n_ctx + 1, dtype=np.int64)
    np.cumsum([len(r) for r in out], out=ptr[1:])
    rows = np.concatenate(out) if out else np.zeros(0, np.int32)
    return ptr, np.ascontiguousarray(rows, dtype=np.int32)


class FMContext:
    """One fm_ctx.  ``parallel`` = "sharded" / "replicated": the context drives ``n_gpus`` local
    ranks on ``devices`` (default device, device + 1, ...) of a job of ``n_procs`` processes and runs
    the multi-GPU step itself (include/fm_hip.h); ``transport`` "auto" | "rccl" | "copy".
    ``fuse`` None (the library's default: on) | True | False: the fused step for prepared batches
    (fm_config.fuse_single); ``xchg_chunks``: 0 = default (fm_config.xchg_chunks); ``wire`` "fp32" |
    "fp64": the format of the sharded step's partial sums on the wire (fm_config.wire).  ``loss``
    "squared" | "logistic" | "bpr": the step's objective (fm_config.loss); the last two are single-GPU,
    never fuse, and "bpr" steps grouped batches only (DeviceBatch.set_group, batch_sample_pairs)."""

    _PAR = {None: N.FM_PARALLEL_NONE, "none": N.FM_PARALLEL_NONE, "sharded": N.FM_PARALLEL_SHARDED,
            "replicated": N.FM_PARALLEL_REPLICATED}
    _TR = {"auto": N.FM_TRANSPORT_AUTO, "rccl": N.FM_TRANSPORT_RCCL, "copy": N.FM_TRANSPORT_COPY}
    _WIRE = {"fp32": N.FM_WIRE_FP32, "fp64": N.FM_WIRE_FP64}
    _LOSS = {"squared": N.FM_LOSS_SQUARED, "logistic": N.FM_LOSS_LOGISTIC, "bpr": N.FM_LOSS_BPR}

    def __init__(self, num_features: int, k: int, *, device: int = 0, seed: int = 0, init_sd: float = 0.01,
                 w0: float = 0.0, shard_index: int = 0, shard_count: int = 1, parallel: str | None = None,
                 n_gpus: int = 1, devices=None, transport: str = "auto", n_procs: int = 1, proc_rank: int = 0,
                 comm_id: bytes | None = None, fuse: bool | None = None, xchg_chunks: int = 0, wire: str = "fp32",
                 loss: str = "squared"):
        if loss not in self._LOSS:
            raise ValueError('loss must be "squared", "logistic" or "bpr"')
        self._lib = N.load()
        if wire not in self._WIRE:
            raise ValueError('wire must be "fp32" or "fp64"')
        cfg = N.fm_config(num_features=int(num_features), k=int(k), device=int(device), seed=int(seed) & (2**64 - 1),
                          init_sd=float(init_sd), w0=float(w0), shard_index=int(shard_index),
                          shard_count=int(shard_count))
        cfg.parallel = self._PAR[parallel]
        cfg.n_gpus = int(n_gpus)
        devs = list(devices) if devices is not None else [int(device) + i for i in range(int(n_gpus))]
        if cfg.parallel != N.FM_PARALLEL_NONE and len(devs) != n_gpus:
            raise ValueError("devices must list n_gpus devices")
        for i, d in enumerate(devs[: N.FM_MAX_LOCAL]):
            cfg.devices[i] = int(d)
        if cfg.parallel != N.FM_PARALLEL_NONE:
            cfg.device = int(devs[0])
        cfg.transport = self._TR[transport]
        cfg.fuse_single = N.FM_FUSE_DEFAULT if fuse is None else (N.FM_FUSE_ON if fuse else N.FM_FUSE_OFF)
        cfg.xchg_chunks = int(xchg_chunks)
        cfg.wire = self._WIRE[wire]
        cfg.loss = self._LOSS[loss]
        cfg.n_procs = int(n_procs)
        cfg.proc_rank = int(proc_rank)
        if comm_id is not None:
            if len(comm_id) != 128:
                raise ValueError("comm_id must be 128 bytes")
            for i, b in enumerate(comm_id):
                cfg.comm_id[i] = b
        self.parallel = parallel if parallel not in (None, "none") else None
        self.n_gpus = int(n_gpus)
        h = C.c_void_p()
        N.check(self._lib.fm_create(C.byref(cfg), C.byref(h)), "fm_create")
        self.handle = h
        self.num_features = int(num_features)
        self.k = int(k)
        self.w0 = float(w0)
        self.shard_index = int(shard_index)
        self.shard_count = int(shard_count)
        self.wire = wire
        self.loss = loss

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "handle", None):
            self._lib.fm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr: int | None):
        """Launch on this hipStream_t (an int handle, e.g. torch.cuda.current_stream().cuda_stream);
        0 / None = the device's default (null) stream."""
        N.check(self._lib.fm_set_stream(self.handle, C.c_void_p(stream_ptr or None)), "fm_set_stream")

    def set_side_stream(self, stream_ptr: int | None):
        """Run the batch-only work (fm_batch_prepare, the inline sort, the sharded route and owner
        prepare) on this hipStream_t (fm_set_side_stream); 0 / None = the context's own side stream."""
        N.check(self._lib.fm_set_side_stream(self.handle, C.c_void_p(stream_ptr or None)), "fm_set_side_stream")

    def sync(self):
        N.check(self._lib.fm_sync(self.handle), "fm_sync")

    def reserve(self, max_rows: int, max_nnz: int):
        N.check(self._lib.fm_reserve(self.handle, int(max_rows), int(max_nnz)), "fm_reserve")

    # --------------------------------------------------------------------- tables
    def load_tables(self, ids, w, V):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        w = np.ascontiguousarray(w, dtype=np.float64)
        V = np.ascontiguousarray(V, dtype=np.float64).reshape(len(ids), self.k)
        N.check(self._lib.fm_load_tables(self.handle, N.ptr(ids, C.c_int32), len(ids), N.ptr(w, C.c_double),
                                         N.ptr(V, C.c_double)), "fm_load_tables")

    def init_random(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        N.check(self._lib.fm_init_random(self.handle, N.ptr(ids, C.c_int32), len(ids)), "fm_init_random")

    def init_random_range(self, begin: int, end: int):
        N.check(self._lib.fm_init_random_range(self.handle, int(begin), int(end)), "fm_init_random_range")

    def init_from_batch(self, b: "DeviceBatch") -> int:
        """createInitialModel over a device-resident dataset (SGD.scala:224-241): the seeded draw for
        every absent id of b's entries, on the device; returns the number of present rows."""
        n = C.c_int64()
        N.check(self._lib.fm_init_from_batch(self.handle, b.handle, C.byref(n)), "fm_init_from_batch")
        return n.value

    def export_tables(self):
        n = C.c_int64()
        N.check(self._lib.fm_export_tables(self.handle, None, None, None, 0, C.byref(n)), "fm_export_tables")
        cnt = n.value
        ids = np.zeros(max(cnt, 1), dtype=np.int32)
        w = np.zeros(max(cnt, 1))
        V = np.zeros((max(cnt, 1), self.k))
        if cnt:
            N.check(self._lib.fm_export_tables(self.handle, N.ptr(ids, C.c_int32), N.ptr(w, C.c_double),
                                               N.ptr(V, C.c_double), cnt, C.byref(n)), "fm_export_tables")
        return ids[:cnt], w[:cnt], V[:cnt]

    def export_rows(self, ids):
        """(w, V, present) of the given ids as they stand now (pending L1 applied), without a
        whole-table export (fm_export_rows)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        n = len(ids)
        w = np.zeros(max(n, 1))
        V = np.zeros((max(n, 1), self.k))
        pres = np.zeros(max(n, 1), dtype=np.int8)
        N.check(self._lib.fm_export_rows(self.handle, N.ptr(ids, C.c_int32), n, N.ptr(w, C.c_double),
                                         N.ptr(V, C.c_double), N.ptr(pres, C.c_int8)), "fm_export_rows")
        return w[:n], V[:n], pres[:n].astype(bool)

    def num_present(self) -> int:
        return N.check(self._lib.fm_num_present(self.handle), "fm_num_present")

    @property
    def epoch(self) -> int:
        return int(self._lib.fm_epoch(self.handle))

    # ------------------------------------------------------------------- stepping
    def batch(self, csr: N.CSRHost) -> DeviceBatch:
        return DeviceBatch(self, csr)

    def batch_splits(self, csr: N.CSRHost, split_rows) -> DeviceBatch:
        """A dataset laid out split after split (fm_batch_create_splits): split s = rows
        [split_rows[s], split_rows[s + 1]) of csr; each split is then stepped in place through
        split_view."""
        sr = np.ascontiguousarray(split_rows, dtype=np.int64)
        b = DeviceBatch(self, None)
        h = C.c_void_p()
        N.check(self._lib.fm_batch_create_splits(self.handle, C.byref(csr.c), len(sr) - 1, N.ptr(sr, C.c_int64),
                                                 C.byref(h)), "fm_batch_create_splits")
        b.handle = h
        b.n_rows, b.nnz = csr.n_rows, csr.nnz
        b.split_rows = sr
        return b

    def batch_layout_splits(self, csr: N.CSRHost, split_rows, order) -> DeviceBatch:
        """The dataset batch_splits makes of rows `order` of csr, laid out on the device from csr in its
        own row order (fm_batch_layout_splits): laid-out row i = row order[i] of csr, split s = laid-out
        rows [split_rows[s], split_rows[s + 1]); no permuted host copy is built."""
        sr = np.ascontiguousarray(split_rows, dtype=np.int64)
        od = np.ascontiguousarray(order, dtype=np.int64)
        if len(sr) < 2 or len(od) != sr[-1]:
            raise ValueError("order must hold split_rows[-1] row indices")
        b = DeviceBatch(self, None)
        h = C.c_void_p()
        N.check(self._lib.fm_batch_layout_splits(self.handle, C.byref(csr.c), len(sr) - 1, N.ptr(sr, C.c_int64),
                                                 N.ptr(od, C.c_int64), C.byref(h)), "fm_batch_layout_splits")
        b.handle = h
        b.n_rows = int(self._lib.fm_batch_rows(h))
        b.nnz = int(self._lib.fm_batch_nnz(h))
        b.split_rows = sr
        return b

    def split_view(self, data: DeviceBatch, split: int, into: DeviceBatch | None = None) -> DeviceBatch:
        """Split `split` of a dataset made by batch_splits as a mini-batch, in place (fm_batch_split_view);
        `into` (a view of this context) is re-pointed instead of creating one."""
        b = into if into is not None else DeviceBatch(self, None)
        return b.view_split(data, split)

    def batch_from_rows(self, data: DeviceBatch, rows, into: DeviceBatch | None = None) -> DeviceBatch:
        """The mini-batch of rows `rows` of the resident dataset `data`, gathered on the device
        (fm_batch_from_rows); `into` (a batch of this context) is refilled in place instead of
        creating one."""
        b = into if into is not None else DeviceBatch(self, None)
        return b.select_rows(data, rows)

    def row_lists(self, lists, n_candidates: int) -> RowLists:
        """``lists`` (what normalize_row_lists accepts: one integer sequence per context, or a CSR pair; or
        an already normalised (ptr, rows)) over n_candidates candidate rows, made resident (fm_lists_create)."""
        if isinstance(lists, RowLists):
            raise ValueError("lists is a RowLists already")
        if (isinstance(lists, tuple) and len(lists) == 2 and all(isinstance(a, np.ndarray) and a.ndim == 1 for a in lists)
                and lists[0].dtype.kind in "iu" and len(lists[0]) >= 1):
            n_ctx = len(lists[0]) - 1
        else:
            n_ctx = len(lists)
        return self._row_lists(normalize_row_lists(lists, n_ctx), n_candidates)

    def _row_lists(self, normalised, n_candidates: int) -> RowLists:
        """row_lists with the lists already normalised: (ptr, rows) as normalize_row_lists returns them."""
        ptr, rows = normalised
        h = C.c_void_p()
        N.check(self._lib.fm_lists_create(self.handle, len(ptr) - 1, int(n_candidates), N.ptr(ptr, C.c_int64),
                                          N.ptr(rows, C.c_int32), C.byref(h)), "fm_lists_create")
        return RowLists(self, h)

    def row_lists_from_pairs(self, pair_ctx, pair_cand, n_contexts: int, n_candidates: int) -> RowLists:
        """The lists the pairs spell out, built on the device (fm_lists_from_pairs): context u's list is the
        distinct pair_cand[i] with pair_ctx[i] == u, ascending; pairs in any order, repeats allowed."""
        pc = np.ascontiguousarray(pair_ctx, dtype=np.int32)
        pd = np.ascontiguousarray(pair_cand, dtype=np.int32)
        if not (pc.ndim == pd.ndim == 1 and len(pc) == len(pd)):
            raise ValueError("pair_ctx and pair_cand must be flat and of one length")
        h = C.c_void_p()
        N.check(self._lib.fm_lists_from_pairs(self.handle, int(n_contexts), int(n_candidates), N.ptr(pc, C.c_int32),
                                              N.ptr(pd, C.c_int32), len(pc), C.byref(h)), "fm_lists_from_pairs")
        return RowLists(self, h)

    def batch_from_pairs(self, contexts: DeviceBatch, candidates: DeviceBatch, pair_ctx, pair_cand, labels,
                         into: DeviceBatch | None = None) -> DeviceBatch:
        """The mini-batch whose row i is row pair_ctx[i] of `contexts` followed by row pair_cand[i] of
        `candidates` (both resident batches of this context), labelled labels[i], built on the device
        (fm_batch_from_pairs); `into` is refilled in place instead of creating a batch."""
        pc = np.ascontiguousarray(pair_ctx, dtype=np.int32)
        pd = np.ascontiguousarray(pair_cand, dtype=np.int32)
        y = np.ascontiguousarray(labels, dtype=np.float64)
        if not (pc.ndim == pd.ndim == y.ndim == 1 and len(pc) == len(pd) == len(y)):
            raise ValueError("pair_ctx, pair_cand and labels must be flat and of one length")
        b = into if into is not None else DeviceBatch(self, None)
        h = b.handle if b.handle else C.c_void_p()
        N.check(self._lib.fm_batch_from_pairs(self.handle, contexts.handle, candidates.handle, N.ptr(pc, C.c_int32),
                                              N.ptr(pd, C.c_int32), N.ptr(y, C.c_double), len(pc), C.byref(h)),
                "fm_batch_from_pairs")
        return self._pair_batch(b, h, contexts, candidates)

    def batch_sample_pairs(self, contexts: DeviceBatch, candidates: DeviceBatch, pos_ctx, pos_cand, n_neg: int, *,
                           exclude=None, pos_label: float = 1.0, neg_label: float = 0.0, seed: int = 0,
                           into: DeviceBatch | None = None, want_sampled: bool = False):
        """The implicit-feedback mini-batch of the positives (pos_ctx[i], pos_cand[i]), each followed by
        n_neg negatives drawn on the device uniformly over the candidate rows its context's ``exclude``
        list does not hold (fm_batch_sample_pairs; the lists as rank(exclude=) takes them).  Returns the
        batch, or (batch, sampled [n_pos, n_neg] int32 candidate rows) with want_sampled."""
        if exclude is None:
            ex = (None, None)
        elif isinstance(exclude, RowLists):
            ex = exclude
        else:
            ex = normalize_row_lists(exclude, contexts.n_rows)
        return self._sample_pairs(contexts, candidates, pos_ctx, pos_cand, n_neg, ex, pos_label, neg_label, seed, into,
                                  want_sampled)

    def _sample_pairs(self, contexts, candidates, pos_ctx, pos_cand, n_neg, ex, pos_label, neg_label, seed, into,
                      want_sampled):
        """batch_sample_pairs with the exclude lists already normalised: ex = (ptr, rows), (None, None) or a
        RowLists (fm_batch_sample_pairs_lists) -- a loop normalises its lists once, or makes them resident."""
        pc = np.ascontiguousarray(pos_ctx, dtype=np.int32)
        pd = np.ascontiguousarray(pos_cand, dtype=np.int32)
        if not (pc.ndim == pd.ndim == 1 and len(pc) == len(pd)):
            raise ValueError("pos_ctx and pos_cand must be flat and of one length")
        n_neg = int(n_neg)
        sampled = np.zeros(max(len(pc) * max(n_neg, 0), 1), dtype=np.int32) if want_sampled else None
        b = into if into is not None else DeviceBatch(self, None)
        h = b.handle if b.handle else C.c_void_p()
        head = (self.handle, contexts.handle, candidates.handle, N.ptr(pc, C.c_int32), N.ptr(pd, C.c_int32), len(pc), n_neg)
        tail = (float(pos_label), float(neg_label), int(seed) & (2**64 - 1), C.byref(h),
                N.ptr(sampled, C.c_int32) if want_sampled else None)
        if isinstance(ex, RowLists):
            N.check(self._lib.fm_batch_sample_pairs_lists(*head, ex.handle, *tail), "fm_batch_sample_pairs_lists")
        else:
            N.check(self._lib.fm_batch_sample_pairs(
                *head, None if ex[0] is None else N.ptr(ex[0], C.c_int64),
                None if ex[1] is None else N.ptr(ex[1], C.c_int32), *tail), "fm_batch_sample_pairs")
        self._pair_batch(b, h, contexts, candidates)
        return (b, sampled[: len(pc) * n_neg].reshape(len(pc), n_neg)) if want_sampled else b

    def _pair_batch(self, b: DeviceBatch, h, contexts: DeviceBatch, candidates: DeviceBatch) -> DeviceBatch:
        b.handle = h
        b.n_rows = int(self._lib.fm_batch_rows(h))
        b.nnz = int(self._lib.fm_batch_nnz(h))
        b._data = (contexts, candidates)  # the sources stay alive while this batch's gather may be queued
        return b

    @property
    def fuse_active(self) -> bool:
        """Whether prepared batches of this context take the fused step (fm_fuse_active)."""
        return int(self._lib.fm_fuse_active(self.handle)) == 1

    def step(self, csr: N.CSRHost, t: int, step_size: float, reg_param: float, sync: bool = True):
        """One iteration from a host CSR.  sync=False only enqueues (the host buffers are free on
        return; losses via loss_history), so consecutive calls overlap upload and compute."""
        if not sync:
            N.check(self._lib.fm_step(self.handle, C.byref(csr.c), int(t), float(step_size), float(reg_param), None),
                    "fm_step")
            return None
        out = N.fm_step_out()
        rc = N.check(self._lib.fm_step(self.handle, C.byref(csr.c), int(t), float(step_size), float(reg_param),
                                       C.byref(out)), "fm_step")
        if rc == N.FM_NOTHING_TO_DO:
            return StepOut(0.0, 0, 0, 0, executed=False)
        return StepOut(out.loss_sum, out.n_rows, out.n_loss_rows, out.n_unique)

    def step_batch(self, b: DeviceBatch, t: int, step_size: float, reg_param: float, sync: bool = True):
        if sync:
            out = N.fm_step_out()
            rc = N.check(self._lib.fm_step_batch(self.handle, b.handle, int(t), float(step_size), float(reg_param),
                                                 C.byref(out)), "fm_step_batch")
            if rc == N.FM_NOTHING_TO_DO:
                return StepOut(0.0, 0, 0, 0, executed=False)
            return StepOut(out.loss_sum, out.n_rows, out.n_loss_rows, out.n_unique)
        N.check(self._lib.fm_step_batch(self.handle, b.handle, int(t), float(step_size), float(reg_param), None),
                "fm_step_batch")
        return None

    def loss_history(self) -> np.ndarray:
        n = C.c_int64()
        N.check(self._lib.fm_loss_history(self.handle, None, 0, C.byref(n)), "fm_loss_history")
        out = np.zeros(max(n.value, 1))
        if n.value:
            N.check(self._lib.fm_loss_history(self.handle, N.ptr(out, C.c_double), n.value, C.byref(n)),
                    "fm_loss_history")
        return out[: n.value]

    # ------------------------------------------------------------------- inference
    def predict(self, csr: N.CSRHost, min_label: float, max_label: float) -> np.ndarray:
        out = np.zeros(max(csr.n_rows, 1))
        N.check(self._lib.fm_predict(self.handle, C.byref(csr.c), float(min_label), float(max_label),
                                     N.ptr(out, C.c_double)), "fm_predict")
        return out[: csr.n_rows]

    def predict_batch(self, b: DeviceBatch, min_label: float, max_label: float) -> np.ndarray:
        out = np.zeros(max(b.n_rows, 1))
        N.check(self._lib.fm_predict_batch(self.handle, b.handle, float(min_label), float(max_label),
                                           N.ptr(out, C.c_double)), "fm_predict_batch")
        return out[: b.n_rows]

    def evaluate(self, csr: N.CSRHost, min_label: float, max_label: float, want_pred: bool = False):
        """The error sums of predict(csr) against csr's labels, reduced on the device (fm_evaluate):
        EvalSums, or (EvalSums, predictions) with want_pred."""
        return self._evaluate(self._lib.fm_evaluate, "fm_evaluate", C.byref(csr.c), csr.n_rows, min_label, max_label,
                              True, want_pred)

    def evaluate_batch(self, b: DeviceBatch, min_label: float, max_label: float, sync: bool = True,
                       want_pred: bool = False):
        """The same over a device-resident batch (fm_evaluate_batch).  sync=False only enqueues (a
        single-table context; the record is read later through eval_history) and returns None."""
        if not sync and want_pred:
            raise ValueError("want_pred needs sync=True")
        return self._evaluate(self._lib.fm_evaluate_batch, "fm_evaluate_batch", b.handle, b.n_rows, min_label,
                              max_label, sync, want_pred)

    def _evaluate(self, fn, what, rows, n_rows, min_label, max_label, sync, want_pred):
        pred = np.zeros(max(n_rows, 1)) if want_pred else None
        pp = N.ptr(pred, C.c_double) if want_pred else None
        if not sync:
            N.check(fn(self.handle, rows, float(min_label), float(max_label), None, None), what)
            return None
        out = N.fm_eval_out()
        rc = N.check(fn(self.handle, rows, float(min_label), float(max_label), pp, C.byref(out)), what)
        sums = EvalSums.from_struct(out, executed=rc != N.FM_NOTHING_TO_DO)
        return (sums, pred[:n_rows]) if want_pred else sums

    def eval_history(self) -> list:
        """Every evaluation record of this context so far, in order (fm_eval_history; waits for the
        main stream)."""
        n = C.c_int64()
        N.check(self._lib.fm_eval_history(self.handle, None, 0, C.byref(n)), "fm_eval_history")
        if not n.value:
            return []
        buf = (N.fm_eval_out * n.value)()
        N.check(self._lib.fm_eval_history(self.handle, buf, n.value, C.byref(n)), "fm_eval_history")
        return [EvalSums.from_struct(o) for o in buf[: n.value]]

    def binary_metrics(self, score, label) -> BinarySums:
        """The binary record of host scores (logits, from any model) against labels, computed on the
        device (fm_binary_metrics); nothing is appended to the history."""
        score = np.ascontiguousarray(score, dtype=np.float64)
        label = np.ascontiguousarray(label, dtype=np.float64)
        if score.shape != label.shape or score.ndim != 1:
            raise ValueError("score and label must be 1-d arrays of one length")
        out = N.fm_binary_out()
        rc = N.check(self._lib.fm_binary_metrics(self.handle, N.ptr(score, C.c_double), N.ptr(label, C.c_double),
                                                 len(score), C.byref(out)), "fm_binary_metrics")
        return BinarySums.from_struct(out, executed=rc != N.FM_NOTHING_TO_DO)

    def evaluate_binary(self, csr: N.CSRHost, want_score: bool = False):
        """The binary record of the unclamped scores of csr's rows against its labels, on the device
        (fm_evaluate_binary): BinarySums, or (BinarySums, scores) with want_score."""
        return self._evaluate_binary(self._lib.fm_evaluate_binary, "fm_evaluate_binary", C.byref(csr.c), csr.n_rows, True,
                                     want_score)

    def evaluate_binary_batch(self, b: DeviceBatch, sync: bool = True, want_score: bool = False):
        """The same over a device-resident batch (fm_evaluate_binary_batch).  sync=False only enqueues (the
        record is read later through eval_binary_history) and returns None."""
        if not sync and want_score:
            raise ValueError("want_score needs sync=True")
        return self._evaluate_binary(self._lib.fm_evaluate_binary_batch, "fm_evaluate_binary_batch", b.handle, b.n_rows,
                                     sync, want_score)

    def _evaluate_binary(self, fn, what, rows, n_rows, sync, want_score):
        if not sync:
            N.check(fn(self.handle, rows, None, None), what)
            return None
        score = np.zeros(max(n_rows, 1)) if want_score else None
        out = N.fm_binary_out()
        rc = N.check(fn(self.handle, rows, N.ptr(score, C.c_double) if want_score else None, C.byref(out)), what)
        sums = BinarySums.from_struct(out, executed=rc != N.FM_NOTHING_TO_DO)
        return (sums, score[:n_rows]) if want_score else sums

    def eval_binary_history(self) -> list:
        """Every binary evaluation record of this context so far, in order (fm_eval_binary_history; waits
        for the main stream)."""
        n = C.c_int64()
        N.check(self._lib.fm_eval_binary_history(self.handle, None, 0, C.byref(n)), "fm_eval_binary_history")
        if not n.value:
            return []
        buf = (N.fm_binary_out * n.value)()
        N.check(self._lib.fm_eval_binary_history(self.handle, buf, n.value, C.byref(n)), "fm_eval_binary_history")
        return [BinarySums.from_struct(o) for o in buf[: n.value]]

    def rank(self, contexts: N.CSRHost, candidates: N.CSRHost, n_top: int, min_label: float, max_label: float, *,
             only=None, exclude=None):
        """For every context row the n_top candidate rows with the largest FM score of the two rows'
        entries together (fm_rank_candidates): (index [U, n_top] int32, score [U, n_top] float64), by
        the unclamped score descending, ties by ascending candidate row.

        only / exclude (one of them): per context a list of candidate rows, as a sequence of U integer
        sequences or a CSR pair (ptr [U + 1], rows).  ``only``: context u ranks the rows of its list
        alone; ``exclude``: every row except them (fm_rank_candidates_select).  The lists are sorted
        and de-duplicated here; rows outside the candidates are refused by the library.  Where fewer
        than n_top rows are eligible the remaining slots hold index -1 and score NaN."""
        return self._rank(self._lib.fm_rank_candidates, self._lib.fm_rank_candidates_select, "fm_rank_candidates",
                          C.byref(contexts.c), C.byref(candidates.c), contexts.n_rows, n_top, min_label, max_label,
                          only, exclude)

    def rank_batch(self, contexts: DeviceBatch, candidates: DeviceBatch, n_top: int, min_label: float,
                   max_label: float, *, only=None, exclude=None):
        """rank over device-resident batches of this context (fm_rank_batch / fm_rank_batch_select); only /
        exclude may be a RowLists of this context (fm_rank_batch_select_lists)."""
        return self._rank(self._lib.fm_rank_batch, self._lib.fm_rank_batch_select, "fm_rank_batch", contexts.handle,
                          candidates.handle, contexts.n_rows, n_top, min_label, max_label, only, exclude,
                          self._lib.fm_rank_batch_select_lists)

    def _rank(self, fn, fn_select, what, contexts, candidates, n_ctx, n_top, min_label, max_label, only, exclude,
              fn_lists=None):
        if only is not None and exclude is not None:
            raise ValueError("give only= or exclude=, not both")
        given = exclude if only is None else only
        if isinstance(given, RowLists) and fn_lists is None:
            raise ValueError("a RowLists goes with resident batches (rank_batch); rank takes host lists")
        n_top = int(n_top)
        n = max(n_ctx * max(n_top, 0), 1)
        idx = np.zeros(n, dtype=np.int32)
        score = np.zeros(n)
        out = (n_top, float(min_label), float(max_label), N.ptr(idx, C.c_int32), N.ptr(score, C.c_double))
        if only is None and exclude is None:
            N.check(fn(self.handle, contexts, candidates, *out), what)
        elif isinstance(given, RowLists):
            mode = N.FM_RANK_SELECT_EXCEPT if only is None else N.FM_RANK_SELECT_ONLY
            N.check(fn_lists(self.handle, contexts, candidates, mode, given.handle, *out), what + "_select_lists")
        else:
            ptr, rows = normalize_row_lists(given, n_ctx)
            mode = N.FM_RANK_SELECT_EXCEPT if only is None else N.FM_RANK_SELECT_ONLY
            N.check(fn_select(self.handle, contexts, candidates, mode, N.ptr(ptr, C.c_int64), N.ptr(rows, C.c_int32), *out),
                    what + "_select")
        m = n_ctx * n_top
        return idx[:m].reshape(n_ctx, n_top), score[:m].reshape(n_ctx, n_top)

    def rank_positions(self, contexts: N.CSRHost, candidates: N.CSRHost, targets, min_label: float, max_label: float, *,
                       exclude=None):
        """Where each context's target rows land in its order over its eligible candidate rows
        (fm_rank_positions): (ptr int64 [U + 1], rows int32, position int32, score float64), the last
        three per target, context u's at ptr[u] .. ptr[u + 1].  position is the 0-based rank among all
        candidate rows except the context's ``exclude`` list -- exact for any number of candidates --
        by rank()'s key and tie-break; score is rank()'s for the pair.  A target that is itself
        excluded has position -1 and score NaN.

        targets / exclude: per context a list of candidate rows, as rank(only= / exclude=) takes them;
        they are sorted and de-duplicated here, so ``rows`` tells which target each result belongs to."""
        return self._rank_positions(self._lib.fm_rank_positions, "fm_rank_positions", C.byref(contexts.c),
                                    C.byref(candidates.c), contexts.n_rows, targets, min_label, max_label, exclude)

    def rank_positions_batch(self, contexts: DeviceBatch, candidates: DeviceBatch, targets, min_label: float,
                             max_label: float, *, exclude=None):
        """rank_positions over device-resident batches of this context (fm_rank_positions_batch).  targets /
        exclude may be RowLists of this context (fm_rank_positions_batch_lists): resident targets come back
        as their exported (ptr, rows); where only one of the two is resident the other is made resident for
        the call."""
        if not isinstance(targets, RowLists) and not isinstance(exclude, RowLists):
            return self._rank_positions(self._lib.fm_rank_positions_batch, "fm_rank_positions_batch", contexts.handle,
                                        candidates.handle, contexts.n_rows, targets, min_label, max_label, exclude)
        if targets is None:
            raise ValueError("targets: one list of candidate rows per context")
        made = []
        try:
            tgt, ex = targets, exclude
            if not isinstance(tgt, RowLists):
                ptr, rows = normalize_row_lists(tgt, contexts.n_rows)
                tgt = self._row_lists((ptr, rows), candidates.n_rows)
                made.append(tgt)
            else:
                ptr, rows = tgt.export()
            if ex is not None and not isinstance(ex, RowLists):
                ex = self._row_lists(normalize_row_lists(ex, contexts.n_rows), candidates.n_rows)
                made.append(ex)
            n = max(len(rows), 1)
            position = np.zeros(n, dtype=np.int32)
            score = np.zeros(n)
            N.check(self._lib.fm_rank_positions_batch_lists(
                self.handle, contexts.handle, candidates.handle, tgt.handle, None if ex is None else ex.handle,
                float(min_label), float(max_label), N.ptr(position, C.c_int32), N.ptr(score, C.c_double)),
                "fm_rank_positions_batch_lists")
            return ptr, rows, position[: len(rows)], score[: len(rows)]
        finally:
            for l in made:
                l.close()

    def _rank_positions(self, fn, what, contexts, candidates, n_ctx, targets, min_label, max_label, exclude):
        if isinstance(targets, RowLists) or isinstance(exclude, RowLists):
            raise ValueError("a RowLists goes with resident batches (rank_positions_batch); rank_positions takes host lists")
        if targets is None:
            raise ValueError("targets: one list of candidate rows per context")
        ptr, rows = normalize_row_lists(targets, n_ctx)
        ex = (None, None) if exclude is None else normalize_row_lists(exclude, n_ctx)
        n = max(len(rows), 1)
        position = np.zeros(n, dtype=np.int32)
        score = np.zeros(n)
        N.check(fn(self.handle, contexts, candidates, N.ptr(ptr, C.c_int64), N.ptr(rows, C.c_int32),
                   None if ex[0] is None else N.ptr(ex[0], C.c_int64), None if ex[1] is None else N.ptr(ex[1], C.c_int32),
                   float(min_label), float(max_label), N.ptr(position, C.c_int32), N.ptr(score, C.c_double)), what)
        return ptr, rows, position[: len(rows)], score[: len(rows)]

    def loss_grad(self, csr: N.CSRHost, initial_sd: float | None = None, seed: int = 0):
        """calcLossGrad per entry (pred, loss, deltaWi, deltaVi).  initial_sd: ids the model lacks
        get their own N(0, initial_sd^2) draws per entry (fm_calc_loss_grad, keyed by seed); None:
        such ids are an error (fm_loss_grad)."""
        n = max(csr.nnz, 1)
        pred, loss, dw = np.zeros(n), np.zeros(n), np.zeros(n)
        dv = np.zeros((n, self.k))
        outs = (N.ptr(pred, C.c_double), N.ptr(loss, C.c_double), N.ptr(dw, C.c_double), N.ptr(dv, C.c_double))
        if initial_sd is None:
            N.check(self._lib.fm_loss_grad(self.handle, C.byref(csr.c), *outs), "fm_loss_grad")
        else:
            N.check(self._lib.fm_calc_loss_grad(self.handle, C.byref(csr.c), float(initial_sd), int(seed) & (2**64 - 1),
                                                *outs), "fm_calc_loss_grad")
        m = csr.nnz
        return pred[:m], loss[:m], dw[:m], dv[:m]

    def vector_sum_by_key(self, keys, vecs):
        keys = np.ascontiguousarray(keys, dtype=np.int32)
        vecs = np.ascontiguousarray(vecs, dtype=np.float64)
        n, k = vecs.shape
        ok = np.zeros(max(n, 1), dtype=np.int32)
        os_ = np.zeros((max(n, 1), k))
        nout = C.c_int64()
        N.check(self._lib.fm_vector_sum_by_key(self.handle, N.ptr(keys, C.c_int32), n, N.ptr(vecs, C.c_double), k,
                                               N.ptr(ok, C.c_int32), N.ptr(os_, C.c_double), C.byref(nout)),
                "fm_vector_sum_by_key")
        return ok[: nout.value], os_[: nout.value]

    # ------------------------------------------------------------------ profiling
    def profile_enable(self, on: bool = True):
        N.check(self._lib.fm_profile_enable(self.handle, 1 if on else 0), "fm_profile_enable")

    def profile_reset(self):
        N.check(self._lib.fm_profile_reset(self.handle), "fm_profile_reset")

    def profile_read(self) -> dict:
        n = C.c_int64()
        cap = 64
        names = C.create_string_buffer(4096)
        ms = np.zeros(cap)
        cnt = np.zeros(cap, dtype=np.int64)
        N.check(self._lib.fm_profile_read(self.handle, names, 4096, N.ptr(ms, C.c_double), N.ptr(cnt, C.c_int64),
                                          cap, C.byref(n)), "fm_profile_read")
        keys = names.value.decode().split("\n") if n.value else []
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(keys)}
