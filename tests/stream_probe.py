"""ctypes wrapper of the stream door (tests/native/stream_probe.hip, built into the sort probe's library
by sort_probe.build_probe): a bounded delay on one stream, its token, and a single-table context's
three stream handles.  tests/test_gpu_stream_order.py holds one lane back at a time with it.

Test infrastructure, not C-ABI.
"""

from __future__ import annotations

import ctypes as C

import sort_probe

MAIN, SIDE, COPY = "main", "side", "copy"
LANES = (MAIN, SIDE, COPY)

_ready = False


def load() -> C.CDLL:
    global _ready
    lib = sort_probe.load()
    if not _ready:
        lib.stream_probe_max_delay_us.restype = C.c_int64
        lib.stream_probe_max_delay_us.argtypes = []
        lib.stream_probe_delay.restype = C.c_int
        lib.stream_probe_delay.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
        lib.stream_probe_pending.restype = C.c_int
        lib.stream_probe_pending.argtypes = [C.c_void_p]
        lib.stream_probe_release.restype = None
        lib.stream_probe_release.argtypes = [C.c_void_p]
        lib.stream_probe_ctx_streams.restype = C.c_int
        lib.stream_probe_ctx_streams.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        _ready = True
    return lib


def max_delay_us() -> int:
    return int(load().stream_probe_max_delay_us())


class Token:
    """The event recorded behind a delay.  pending() is hipEventQuery; release() waits for it and
    destroys it (a token is released once, by whoever asked for the delay)."""

    def __init__(self, lib, handle):
        self._lib, self._h = lib, handle

    def pending(self) -> bool:
        st = self._lib.stream_probe_pending(self._h)
        if st < 0:
            raise RuntimeError(f"stream_probe_pending: status {st}")
        return st == 1

    def release(self):
        if self._h is not None:
            self._lib.stream_probe_release(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def delay(stream: int | None, us: int) -> Token:
    """A delay of min(us, max_delay_us()) microseconds enqueued on the hipStream_t ``stream`` (an int
    handle; 0 / None: the null stream); returns its token."""
    lib = load()
    tok = C.c_void_p()
    st = lib.stream_probe_delay(C.c_void_p(stream or None), int(us), C.byref(tok))
    if st != 0:
        raise RuntimeError(f"stream_probe_delay: status {st}")
    return Token(lib, tok)


def ctx_streams(ctx) -> dict:
    """{MAIN, SIDE, COPY: int handle} of a single-table FMContext as they stand now; 0 is the null
    stream for MAIN and "not created yet" for COPY (the first call that copies creates it)."""
    out = (C.c_void_p * 3)()
    st = load().stream_probe_ctx_streams(ctx.handle, out)
    if st != 0:
        raise RuntimeError(f"stream_probe_ctx_streams: status {st}")
    return {lane: int(out[i] or 0) for i, lane in enumerate(LANES)}
