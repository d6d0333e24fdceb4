"""The sort probe (tests/native/sort_probe.hip): its build recipe and its ctypes wrapper.

Test infrastructure, not C-ABI: a small shared library beside libfm_hip.so, linked against it, that
lets tests/test_gpu_sort.py call fmhip::radix_sort_pairs / radix_sort_pairs64 /
radix_sort_pairs64_bits of the built library directly.  __graft_entry__.build() calls
build_probe() after the library; the tests only load what was built.  The same library carries a
second source, tests/native/forward_probe.hip: the door to the forward's launch-size seam
(tests/forward_probe.py wraps it), and a third, tests/native/update_probe.hip: the door to the update
side's geometry seam (tests/update_probe.py wraps it), and a fourth, tests/native/shard_probe.hip: the
door to the sharded step's geometry seam (tests/shard_probe.py wraps it), and a fifth,
tests/native/stream_probe.hip: the delay and the stream handles with which
tests/test_gpu_stream_order.py holds one stream of a context back (tests/stream_probe.py wraps it).
"""

from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
SRC = HERE / "native" / "sort_probe.hip"
# the same library carries the forward's launch-size door (tests/forward_probe.py) and the update
# side's geometry door (tests/update_probe.py), the sharded step's (tests/shard_probe.py) and the stream
# order tests' delay door (tests/stream_probe.py)
SRCS = [SRC, HERE / "native" / "forward_probe.hip", HERE / "native" / "update_probe.hip",
        HERE / "native" / "shard_probe.hip", HERE / "native" / "stream_probe.hip"]
LIB_DIR = ROOT / "fm_spark_amd" / "lib"
PROBE = LIB_DIR / "libfm_sort_probe.so"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("FM_HIP_ARCH", "gfx950")

PAIRS32, PAIRS64, PAIRS64_BITS = 0, 1, 2
FM_ERR_ARG = -1

# key width -> (digit bits, passes) as fm_sort.hip digit_bits plans it: the fewest passes of at most
# 10 bits, spread evenly, never narrower than 9 bits.  Every plan the library can choose is here:
# 9-bit digits in 1, 2, 3 and 4 passes, 10-bit digits in 1, 2 and 3 passes.
PLAN = {1: (9, 1), 9: (9, 1), 10: (10, 1), 11: (9, 2), 18: (9, 2), 19: (10, 2), 20: (10, 2), 21: (9, 3), 27: (9, 3),
        28: (10, 3), 30: (10, 3), 31: (9, 4), 32: (9, 4)}


def build_probe(verbose: bool = False, force: bool = False, lib: Path | None = None, out: Path | None = None) -> Path:
    """Compile the probe against the built library ``lib`` (default: the tree's libfm_hip.so) into
    ``out`` (default: beside it).  The probe finds the library through its own directory."""
    lib = Path(lib) if lib else LIB_DIR / "libfm_hip.so"
    out = Path(out) if out else lib.parent / PROBE.name
    if not lib.exists():
        raise RuntimeError(f"{lib} is missing: build the library first")
    deps = [*SRCS, ROOT / "fm_spark_amd" / "csrc" / "fm_internal.h", ROOT / "fm_spark_amd" / "csrc" / "fm_context.h",
            ROOT / "include" / "fm_hip.h", lib]
    if not force and out.exists() and all(d.stat().st_mtime <= out.stat().st_mtime for d in deps):
        return out
    cmd = [HIPCC, f"--offload-arch={ARCH}", "-O2", "-std=c++17", "-fPIC", "-Wall", "-shared", *map(str, SRCS), "-o",
           str(out),
           f"-L{lib.parent}", f"-l:{lib.name}", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,/opt/rocm/lib"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    return out


class SortProbeError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"sort probe status {status}: {msg}")
        self.status = status
        self.msg = msg


_lib = None


def load() -> C.CDLL:
    """Load the probe (FM_SORT_PROBE: another build of it, beside another build of the library)."""
    global _lib
    if _lib is not None:
        return _lib
    path = Path(os.environ.get("FM_SORT_PROBE") or PROBE)
    if not path.exists():
        raise RuntimeError(f"{path} is missing: run build() first (__graft_entry__.build())")
    from fm_spark_amd import _native

    # the process's one libfm_hip.so first (and torch's HIP runtime before it): the probe's own
    # reference to the library beside it then resolves to the same loaded object (with FM_SORT_PROBE,
    # FM_HIP_LIB names the library beside that probe)
    _native.load()
    lib = C.CDLL(str(path))
    lib.sort_probe_last_error.restype = C.c_char_p
    lib.sort_probe_last_error.argtypes = []
    lib.sort_probe_create.restype = C.c_int
    lib.sort_probe_create.argtypes = [C.POINTER(C.c_void_p)]
    lib.sort_probe_destroy.restype = None
    lib.sort_probe_destroy.argtypes = [C.c_void_p]
    lib.sort_probe_sort.restype = C.c_int
    lib.sort_probe_sort.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    _lib = lib
    return lib


class SortResult:
    __slots__ = ("keys", "vals", "inputs_unchanged", "guard_ok")

    def __init__(self, keys, vals, inputs_unchanged, guard_ok):
        self.keys, self.vals, self.inputs_unchanged, self.guard_ok = keys, vals, inputs_unchanged, guard_ok


class SortHandle:
    """One fmhip::SortWork and its stream; sorts on it reuse the work buffers, as a context's do."""

    def __init__(self):
        self._lib = load()
        h = C.c_void_p()
        st = self._lib.sort_probe_create(C.byref(h))
        if st != 0:
            raise SortProbeError(st, self._lib.sort_probe_last_error().decode())
        self._h = h

    def close(self):
        if self._h is not None:
            self._lib.sort_probe_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sort(self, kind, keys, vals, *, hi_bit, lo_bit=0, misalign=0, use_final=False, n=None) -> SortResult:
        """keys uint32 [n]; vals None (kind PAIRS32: the implicit index), uint32 [n] or uint32 [n, 2]
        (the uint2 payload).  ``n`` overrides len(keys) (the error cases)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        m = len(keys)
        width = 1 if kind == PAIRS32 else 2
        if vals is not None:
            vals = np.ascontiguousarray(vals, dtype=np.uint32)
            assert vals.shape == ((m,) if width == 1 else (m, 2)), vals.shape
        out_k = np.empty(m, dtype=np.uint32)
        out_v = np.empty((m,) if width == 1 else (m, 2), dtype=np.uint32)
        same, guard = C.c_int(0), C.c_int(0)
        st = self._lib.sort_probe_sort(self._h, kind, keys.ctypes.data, None if vals is None else vals.ctypes.data,
                                       m if n is None else n, lo_bit, hi_bit, misalign, 1 if use_final else 0,
                                       out_k.ctypes.data, out_v.ctypes.data, C.byref(same), C.byref(guard))
        if st != 0:
            raise SortProbeError(st, self._lib.sort_probe_last_error().decode())
        return SortResult(out_k, out_v, bool(same.value), bool(guard.value))
