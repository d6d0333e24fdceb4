"""The update probe (tests/native/update_probe.hip): the ctypes wrapper of the update side's geometry
door.

Test infrastructure, not C-ABI.  The door lives in the sort probe's library (tests/sort_probe.py builds
its sources into one .so against the built libfm_hip.so).  geometry(k) is what fm_update.hip itself
uses at k factors -- the entries per wave, lane group and block of k_segment_update, whether closed
rows leave in paired stores, the lanes per range and the columns per pass of k_segment_combine, the
split's chunk and the scan's chunks per round -- so tests/test_gpu_update_edges.py writes its layouts
in these units and follows a retuned kernel.  The call reads host constants only: it needs no GPU.
"""

from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

import sort_probe

Geometry = namedtuple("Geometry", "wave group block paired comb_lanes comb_cols chunk round_chunks")

_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    lib = sort_probe.load()  # a missing probe raises with the "run build() first" message
    if not hasattr(lib, "upd_probe_geometry"):
        raise RuntimeError(f"{sort_probe.PROBE} lacks the update door: run build() first (__graft_entry__.build())")
    lib.upd_probe_geometry.restype = C.c_int
    lib.upd_probe_geometry.argtypes = [C.c_int, C.c_void_p]
    _lib = lib
    return lib


def geometry(k: int) -> Geometry:
    """The update side's geometry for a table of k factors (rows padded to whole float4 quads)."""
    out = np.zeros(8, dtype=np.int64)
    st = load().upd_probe_geometry((int(k) + 3) // 4 * 4, out.ctypes.data)
    if st < 0:
        raise RuntimeError(f"upd_probe_geometry: status {st}")
    g = Geometry(*map(int, out))
    return g._replace(paired=bool(g.paired))
