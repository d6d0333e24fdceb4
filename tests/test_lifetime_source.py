"""The live-allocation counter (fm_device_bytes_live / fm_device_allocs_live) is exact only while
every device allocation of the library goes through DevBuf: the sources under fm_spark_amd/csrc
call hipMalloc once, in DevBuf::ensure, and hipFree once, in DevBuf::release, and both update the
counter there.  A second allocation site added later would be invisible to tests/test_gpu_lifetime.py;
this check keeps the counter complete."""

import re
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "fm_spark_amd" / "csrc"


def _sources():
    files = sorted(p for p in CSRC.iterdir() if p.suffix in (".hip", ".h", ".cpp"))
    assert len(files) >= 10
    return {p.name: p.read_text() for p in files}


def _function_body(text, signature):
    """The brace-balanced body of the function whose definition starts with `signature`."""
    at = text.index(signature)
    i = text.index("{", at)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[i:j + 1]
        j += 1


def _calls(src, name):
    return [(f, m.start()) for f, t in src.items() for m in re.finditer(r"\b%s\s*\(" % name, t)]


def test_one_device_malloc_and_one_free_both_counted():
    src = _sources()
    mallocs, frees = _calls(src, "hipMalloc"), _calls(src, "hipFree")
    assert [f for f, _ in mallocs] == ["fm_capi.hip"], mallocs
    assert [f for f, _ in frees] == ["fm_capi.hip"], frees
    capi = src["fm_capi.hip"]
    ensure = _function_body(capi, "void DevBuf::ensure(size_t n)")
    release = _function_body(capi, "void DevBuf::release()")
    assert "hipMalloc(" in ensure and "hipFree(" in release
    # no other device allocator sneaks past the counter
    for other in ("hipMallocAsync", "hipMallocManaged", "hipMallocFromPoolAsync", "hipFreeAsync", "hipExtMallocWithFlags",
                  "hipMallocPitch", "hipMalloc3D"):
        assert not _calls(src, other), other
    # both counters move where the allocation happens
    for body, op in ((ensure, "fetch_add"), (release, "fetch_sub")):
        assert len(re.findall(r"g_dev_bytes_live\.%s" % op, body)) == 1
        assert len(re.findall(r"g_dev_allocs_live\.%s" % op, body)) == 1
    # and nowhere else: the definition, the add, the sub and the exported read
    assert len(re.findall(r"\bg_dev_bytes_live\b", capi)) == 4
    assert len(re.findall(r"\bg_dev_allocs_live\b", capi)) == 4


def test_devbuf_is_move_only_and_frees_itself():
    hdr = _sources()["fm_internal.h"]
    body = _function_body(hdr, "struct DevBuf")
    assert "DevBuf(const DevBuf&) = delete;" in body
    assert "DevBuf& operator=(const DevBuf&) = delete;" in body
    assert "DevBuf(DevBuf&& o) noexcept" in body and "DevBuf& operator=(DevBuf&& o) noexcept" in body
    assert "~DevBuf() { release(); }" in body


def test_counters_exported_and_bound():
    header = (CSRC.parent.parent / "include" / "fm_hip.h").read_text()
    assert "int64_t fm_device_bytes_live(void);" in header
    assert "int64_t fm_device_allocs_live(void);" in header
    import ctypes as C

    from fm_spark_amd import _native as N

    for name in ("fm_device_bytes_live", "fm_device_allocs_live"):
        assert N.SIGNATURES[name] == (C.c_int64, [])
