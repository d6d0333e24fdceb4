"""The forward probe (tests/native/forward_probe.hip): the ctypes wrapper of the forward's launch-size
door.

Test infrastructure, not C-ABI.  The door lives in the sort probe's library (tests/sort_probe.py builds
both sources into one .so against the built libfm_hip.so).  A cap on k_forward's blocks makes every
team walk several samples at a batch of a few hundred rows; while a cap is set the library logs each
forward launch -- (mode, GS, TEAM, U, chunk, chunks, blocks, rows) -- and the tests assert on that log
instead of keeping a copy of the dispatch table.  With no cap set nothing is logged.
"""

from __future__ import annotations

import ctypes as C
from collections import namedtuple
from contextlib import contextmanager

import numpy as np

import sort_probe

# FwdMode (fm_spark_amd/csrc/fm_internal.h)
TRAIN, PARTIAL, PREDICT, LOSS_GRAD, TRAIN_FUSED, PARTIAL64 = range(6)

Launch = namedtuple("Launch", "mode gs team u chunk chunks blocks rows")
Consts = namedtuple("Consts", "grid block fuse_ns fuse_u log_cap")

_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    lib = sort_probe.load()  # a missing probe raises with the "run build() first" message
    if not hasattr(lib, "fwd_probe_set_grid_cap"):
        raise RuntimeError(f"{sort_probe.PROBE} lacks the forward door: run build() first (__graft_entry__.build())")
    lib.fwd_probe_set_grid_cap.restype = C.c_int
    lib.fwd_probe_set_grid_cap.argtypes = [C.c_int64]
    lib.fwd_probe_clear_log.restype = C.c_int
    lib.fwd_probe_clear_log.argtypes = []
    lib.fwd_probe_read_log.restype = C.c_int
    lib.fwd_probe_read_log.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
    lib.fwd_probe_consts.restype = C.c_int
    lib.fwd_probe_consts.argtypes = [C.c_void_p]
    _lib = lib
    return lib


def _check(st, what):
    if st < 0:
        raise RuntimeError(f"{what}: status {st}")
    return st


def consts() -> Consts:
    out = np.zeros(5, dtype=np.int64)
    _check(load().fwd_probe_consts(out.ctypes.data), "fwd_probe_consts")
    return Consts(*map(int, out))


def set_grid_cap(blocks: int) -> None:
    """blocks > 0: every forward launch of the process takes at most that many blocks and is logged;
    0: the tuned grid, nothing logged."""
    _check(load().fwd_probe_set_grid_cap(int(blocks)), "fwd_probe_set_grid_cap")


def clear_log() -> None:
    _check(load().fwd_probe_clear_log(), "fwd_probe_clear_log")


def read_log() -> list[Launch]:
    """The launches made under a cap since the last clear, in launch order (the ranks of a multi-GPU
    context launch from their own threads: their records interleave).  Raises if the library's
    bounded log dropped one."""
    cap = consts().log_cap
    buf = np.zeros((cap, 8), dtype=np.int64)
    total = C.c_int64(0)
    n = _check(load().fwd_probe_read_log(buf.ctypes.data, cap, C.byref(total)), "fwd_probe_read_log")
    if total.value != n:
        raise RuntimeError(f"the forward log kept {n} of {total.value} launches: clear it more often")
    return [Launch(*map(int, row)) for row in buf[:n]]


@contextmanager
def grid_cap(blocks: int):
    """The forward capped at ``blocks`` blocks, with an empty log; the tuned grid again afterwards."""
    clear_log()
    set_grid_cap(blocks)
    try:
        yield
    finally:
        set_grid_cap(0)
