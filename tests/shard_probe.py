"""The shard probe (tests/native/shard_probe.hip): the ctypes wrapper of the sharded step's geometry
door.

Test infrastructure, not C-ABI.  The door lives in the sort probe's library (tests/sort_probe.py builds
its sources into one .so against the built libfm_hip.so).  geometry(k) is what fm_shard.hip itself uses
at k factors -- the samples per tile of the pair numbering, the lanes of a route team, the samples per
sweep of k_sample_mask, the tiles per trip of k_rows_scan, the entries per sweep of k_route_keys and
k_pair_table and their unroll, the owners whose pair slots the combine keeps in registers, the most
ranks, the combine's team width and samples per sweep, the pairs per sweep of k_pack_srec -- so
tests/test_gpu_shard_phases.py sizes its batches in these units and follows a retuned grid.  The call
reads host constants only: it needs no GPU.
"""

from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

import sort_probe

Geometry = namedtuple("Geometry", "pair_tile route_team mask_sweep scan_trip route_sweep route_unroll table_sweep "
                                  "table_unroll slot_regs max_r combine_team combine_sweep pack_sweep")

_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    lib = sort_probe.load()  # a missing probe raises with the "run build() first" message
    if not hasattr(lib, "shard_probe_geometry"):
        raise RuntimeError(f"{sort_probe.PROBE} lacks the shard door: run build() first (__graft_entry__.build())")
    lib.shard_probe_geometry.restype = C.c_int
    lib.shard_probe_geometry.argtypes = [C.c_int, C.c_void_p]
    _lib = lib
    return lib


def geometry(k: int) -> Geometry:
    """The sharded step's geometry for a table of k factors (rows padded to whole float4 quads)."""
    out = np.zeros(len(Geometry._fields), dtype=np.int64)
    st = load().shard_probe_geometry((int(k) + 3) // 4 * 4, out.ctypes.data)
    if st < 0:
        raise RuntimeError(f"shard_probe_geometry: status {st}")
    return Geometry(*map(int, out))
