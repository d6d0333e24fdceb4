"""The LSD radix sort of fm_sort.hip, called directly (tests/sort_probe.py, tests/native/sort_probe.hip)
and compared, element for element, with a stable host sort of the same field:

    order = np.argsort((keys >> lo_bit) & ((1 << (hi_bit - lo_bit)) - 1), kind="stable")
    expected keys = keys[order] (whole keys: bits outside the field ride along), payloads = vals[order]

Every comparison is exact array equality over all n elements.  The sort is what makes the step bitwise
reproducible (equal keys contiguous AND in their original order), and a sort that is deterministic
but unstable passes every tolerance and every run-twice test; only the payload order shows it.

The sizes are the smallest that cross each boundary of the implementation (wave 64, a wave's 512-key
share of a tile, the 4096-key tile, nine tiles on the eight XCD groups, the 16-tile chunk of the count
scan, more chunks than k_radix_chunk_top's eight slices, and its second load round above 64 chunks);
the key widths give every digit plan digit_bits can choose (PLAN below).

Only the probe runs here, and it treats payloads as opaque words, so this file is safe to run against
a deliberately broken build of the sort (a mutation check of these tests): a sort that leaves outputs
unwritten gives wrong words here, nothing more.  The sort's consumers, which use the payload as an
index, are tested through the public API in tests/test_gpu_sort_consumers.py.
"""

import functools

import numpy as np
import pytest

from sort_probe import PLAN  # key width -> (digit bits, passes), every plan digit_bits can choose

gpu_test = pytest.mark.gpu

TILE, CHUNK = 4096, 16 * 4096

WIDTHS = sorted(PLAN)
SIZES = [0, 1, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 8 * 4096 - 1, 8 * 4096 + 1, 65535, 65536, 65537,
         9 * 65536 + 1, 65 * 65536 + 5]
SIZE_WIDTHS = [9, 10, 20, 27, 31]  # every size at these widths
WIDTH_SIZES = [4097, 65537]        # every width at these sizes
PAYLOADS = ["index", "u32", "u2"]  # implicit index (uint32), explicit uint32, uint2 {index, hash(index)}
DISTS = ["zeros", "ones", "alternating", "ascending", "descending", "skew60", "top_digit"]


def test_digit_plans_cover_every_plan_and_agree_with_the_bench():
    """PLAN (tests/sort_probe.py) was read off a stand-alone host compile of fm_sort.hip's digit_bits
    (widths 1..32 printed); here it is held against the rule in words (the fewest passes of at most 10
    bits, spread evenly, never below 9) and against bench.sort_passes, an independent restatement."""
    import bench

    assert set(PLAN.values()) == {(9, 1), (9, 2), (9, 3), (9, 4), (10, 1), (10, 2), (10, 3)}
    for bits, (rb, passes) in PLAN.items():
        p = -(-bits // 10)
        assert rb == max(9, -(-bits // p)) and passes == -(-bits // rb), bits
        assert bench.sort_passes(1 << bits) == passes, bits
        assert rb * passes >= bits


# ------------------------------------------------------------------------------------------- inputs
def _hash32(i):
    """A payload word that depends on the index alone and shares no bits' meaning with it."""
    x = (np.asarray(i, dtype=np.uint64) + np.uint64(0x9E3779B9)) * np.uint64(0x85EBCA6B)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    return (x ^ (x >> np.uint64(16))).astype(np.uint32)


def make_keys(n, bits, dist, seed=0):
    rng = np.random.default_rng([n, bits, seed])
    top = (1 << bits) - 1
    uni = rng.integers(0, top + 1, n, dtype=np.uint64).astype(np.uint32)
    if dist == "uniform":
        return uni
    if dist == "zeros":
        return np.zeros(n, np.uint32)
    if dist == "ones":  # every key 2^bits - 1: one digit takes whole tiles in every pass
        return np.full(n, top, np.uint32)
    if dist == "alternating":
        return np.where(np.arange(n) % 2 == 0, np.uint32(top // 3), np.uint32(top - top // 5)).astype(np.uint32)
    if dist == "ascending":
        return ((np.arange(n, dtype=np.uint64) * np.uint64(top + 1)) // np.uint64(max(n, 1))).astype(np.uint32)
    if dist == "descending":
        return make_keys(n, bits, "ascending")[::-1].copy()
    if dist == "skew60":  # 60 % of the keys on one key, the rest uniform
        return np.where(rng.random(n) < 0.6, np.uint32(12345 & top), uni).astype(np.uint32)
    if dist == "top_digit":  # equal in every digit but the last pass's
        rb, passes = PLAN[bits]
        low = rb * (passes - 1)
        return (((uni >> np.uint32(low)) << np.uint32(low)) | np.uint32(0x15555555 & ((1 << low) - 1))).astype(np.uint32)
    raise ValueError(dist)


@functools.lru_cache(maxsize=6)
def problem(n, bits, dist="uniform", lo_bit=0, full_range=False):
    """Keys, the two explicit payloads, and the stable order of the field [lo_bit, bits): computed once
    per shape and shared by the payload kinds (read-only)."""
    keys = make_keys(n, 32 if full_range else bits, dist)
    field = (keys >> np.uint32(lo_bit)) & np.uint32((1 << (bits - lo_bit)) - 1)
    order = np.argsort(field, kind="stable")
    idx = np.arange(n, dtype=np.uint32)
    u32 = _hash32(idx)
    u2 = np.stack([idx, u32], axis=1)
    for a in (keys, order, u32, u2):
        a.setflags(write=False)
    return keys, order, u32, u2


def payload(kind, prob):
    """(probe kind, payload array or None, expected sorted payload)."""
    import sort_probe as sp

    keys, order, u32, u2 = prob
    if kind == "index":
        return sp.PAIRS32, None, order.astype(np.uint32)
    if kind == "u32":
        return sp.PAIRS32, u32, u32[order]
    return sp.PAIRS64, u2, u2[order]


def check(res, keys, order, want_vals, what):
    """Exact equality; on a mismatch the first wrong position with its tile and chunk."""
    assert res.inputs_unchanged, f"{what}: the sort wrote to its input buffers"
    assert res.guard_ok, f"{what}: the sort wrote outside its final buffers"
    want_keys = keys[order]
    for name, got, want in (("keys", res.keys, want_keys), ("payloads", res.vals, want_vals)):
        if np.array_equal(got, want):
            continue
        bad = np.nonzero((got != want).reshape(len(want), -1).any(axis=1))[0]
        i = int(bad[0])
        pytest.fail(f"{what}: {len(bad)} of {len(want)} {name} differ from the stable reference; first at output "
                    f"position {i} (tile {i // TILE}, chunk {i // CHUNK}): got {got[i]!r} (key {int(res.keys[i]):#x}), "
                    f"want {want[i]!r} (key {int(want_keys[i]):#x}, from input {int(order[i])}, input tile "
                    f"{int(order[i]) // TILE})")


_shared = {"handle": None}  # one SortWork for the whole file, as a context keeps its own across steps


def _close_shared():
    if _shared["handle"] is not None:
        _shared["handle"].close()
        _shared["handle"] = None


@pytest.fixture
def handle(gpu):
    import sort_probe as sp

    if _shared["handle"] is None:
        _shared["handle"] = sp.SortHandle()
    return _shared["handle"]


@pytest.fixture(scope="module", autouse=True)
def _shared_handle_ends_with_the_file():
    yield
    _close_shared()


# --------------------------------------------------------------------------------- sizes and widths
SIZE_CASES = [(n, b, p) for n in SIZES for b in SIZE_WIDTHS for p in PAYLOADS]
WIDTH_CASES = [(n, b, p) for b in WIDTHS if b not in SIZE_WIDTHS for n in WIDTH_SIZES for p in PAYLOADS]


@gpu_test
@pytest.mark.parametrize("n,bits,pay", SIZE_CASES + WIDTH_CASES, ids=lambda v: str(v))
def test_sort_is_the_stable_sort(handle, n, bits, pay):
    """Every size at widths 9, 10, 20, 27, 31 and every width at n = 4097, 65537, with each payload kind."""
    prob = problem(n, bits)
    kind, vals, want = payload(pay, prob)
    res = handle.sort(kind, prob[0], vals, hi_bit=bits)
    check(res, prob[0], prob[1], want, f"n={n} bits={bits} plan={PLAN[bits]} payload={pay}")


@gpu_test
@pytest.mark.parametrize("pay", ["index", "u2"])
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("n", WIDTH_SIZES)
@pytest.mark.parametrize("bits", [10, 20, 27])
def test_sort_key_distributions(handle, bits, n, dist, pay):
    """All keys equal (0, and 2^bits - 1: at 10 bits the worst case of the 16-bit wave histograms), two
    alternating values, ascending, descending, 60 % on one key, keys that differ in the top digit only
    (uniform keys: test_sort_is_the_stable_sort)."""
    prob = problem(n, bits, dist)
    kind, vals, want = payload(pay, prob)
    res = handle.sort(kind, prob[0], vals, hi_bit=bits)
    check(res, prob[0], prob[1], want, f"n={n} bits={bits} dist={dist} payload={pay}")


# ---------------------------------------------------------------------------------------- alignment
@gpu_test
@pytest.mark.parametrize("pay", PAYLOADS)
@pytest.mark.parametrize("bits", [10, 27])
def test_sort_keys_off_a_16_byte_boundary(handle, bits, pay):
    """Keys 1, 2 and 3 words past a 16-byte boundary (a split view starts anywhere): whole tiles take
    the count's scalar loads, the last tile is partial.  The same bits as the aligned sort."""
    n = 3 * 4096 + 17
    prob = problem(n, bits)
    kind, vals, want = payload(pay, prob)
    base = handle.sort(kind, prob[0], vals, hi_bit=bits)
    check(base, prob[0], prob[1], want, f"n={n} bits={bits} payload={pay} aligned")
    for mis in (1, 2, 3):
        res = handle.sort(kind, prob[0], vals, hi_bit=bits, misalign=mis)
        check(res, prob[0], prob[1], want, f"n={n} bits={bits} payload={pay} misalign={mis}")
        assert np.array_equal(res.keys, base.keys) and np.array_equal(res.vals, base.vals)


# ------------------------------------------------------------------------------------ final outputs
@gpu_test
@pytest.mark.parametrize("n", [0, 1, 4097, 65537])
@pytest.mark.parametrize("bits", [10, 20, 27])
def test_sort_into_final_buffers(handle, bits, n):
    """The step's sort: uint2 payload, the last pass written to final_keys / final_vals -- with one
    pass (10 bits) straight from the input.  Guards around the final buffers intact, inputs unchanged."""
    import sort_probe as sp

    assert PLAN[bits][1] == {10: 1, 20: 2, 27: 3}[bits]
    keys, order, _, u2 = problem(n, bits)
    res = handle.sort(sp.PAIRS64, keys, u2, hi_bit=bits, use_final=True)
    check(res, keys, order, u2[order], f"final n={n} bits={bits}")


# --------------------------------------------------------------------------------------- bit ranges
@gpu_test
@pytest.mark.parametrize("n", WIDTH_SIZES)
@pytest.mark.parametrize("lo,hi,all32", [(10, 11, False), (24, 27, False), (27, 32, True), (28, 32, True),
                                          (20, 32, True)])
def test_sort_by_a_bit_range(handle, lo, hi, all32, n):
    """radix_sort_pairs64_bits at the (sb, sb + ob) shapes fm_shard_route forms: stable on the field
    [lo, hi) alone, the whole key and the payload carried along.

    The fields that end at bit 32 take keys uniform over all 32 bits.  (10, 11) and (24, 27) take keys
    uniform below hi_bit, as fm_shard_route forms them (owner << sb | slot, owner < 2^ob), because that
    is the entry point's contract (fm_internal.h: nothing at hi_bit and above): every pass takes a
    whole 9- or 10-bit digit, so with bits above the field the sort orders by them as well.  Measured
    on an MI355X with keys uniform over 32 bits: [10, 11) comes out sorted by bits [10, 19) (4097 of
    4097 and 65536 of 65537 keys away from the stable sort of the field), [24, 27) by bits [24, 32)
    (4093 of 4097, 65536 of 65537).  The bits below the field are uniform in every shape."""
    import sort_probe as sp

    keys, order, _, u2 = problem(n, hi, "uniform", lo, all32)
    assert all32 or int(keys.max()) < (1 << hi)
    res = handle.sort(sp.PAIRS64_BITS, keys, u2, lo_bit=lo, hi_bit=hi)
    check(res, keys, order, u2[order], f"bits [{lo}, {hi}) n={n}")


# ------------------------------------------------------------------------------------ SortWork reuse
@gpu_test
def test_sort_work_reuse_large_then_small(gpu):
    """One SortWork through a large sort and then small ones: the count and prefix buffers hold stale
    values of the larger sorts and the chunk sums' offset moves with the tile count.  A fresh handle
    gives the same bits for the last case."""
    import sort_probe as sp

    seq = [(65 * 65536 + 5, 27), (1, 10), (4097, 27), (65537, 10), (0, 27), (4096, 10)]
    with sp.SortHandle() as h:
        for n, bits in seq:
            keys, order, _, u2 = problem(n, bits)
            last = h.sort(sp.PAIRS64, keys, u2, hi_bit=bits)
            check(last, keys, order, u2[order], f"reused handle n={n} bits={bits}")
    with sp.SortHandle() as h:
        n, bits = seq[-1]
        keys, order, _, u2 = problem(n, bits)
        fresh = h.sort(sp.PAIRS64, keys, u2, hi_bit=bits)
    assert np.array_equal(fresh.keys, last.keys) and np.array_equal(fresh.vals, last.vals)


# ------------------------------------------------------------------------------------------- errors
@gpu_test
def test_sort_errors_leave_the_handle_usable(gpu):
    """n < 0, hi_bit <= lo_bit and hi_bit > 32 come back as the probe's error status with the library's
    message (FM_REQUIRE throws; nothing crosses the boundary), and the handle still sorts.  The bit
    range is checked by radix_sort_pairs64_bits alone: radix_sort_pairs and radix_sort_pairs64 take
    key_bits as the caller's promise about its keys (bits_for of the largest key or row) and plan
    their passes from it unchecked, so they have no range error to test."""
    import sort_probe as sp

    keys, order, u32, u2 = problem(513, 20)
    with sp.SortHandle() as h:
        for kind, vals in ((sp.PAIRS32, None), (sp.PAIRS64, u2), (sp.PAIRS64_BITS, u2)):
            with pytest.raises(sp.SortProbeError, match="sort size out of range") as e:
                h.sort(kind, keys, vals, hi_bit=20, n=-1)
            assert e.value.status == sp.FM_ERR_ARG
        for lo, hi in ((5, 5), (7, 3), (0, 33), (-1, 8)):
            with pytest.raises(sp.SortProbeError, match="bad sort bit range") as e:
                h.sort(sp.PAIRS64_BITS, keys, u2, lo_bit=lo, hi_bit=hi)
            assert e.value.status == sp.FM_ERR_ARG
        res = h.sort(sp.PAIRS64, keys, u2, hi_bit=20)
        check(res, keys, order, u2[order], "after the errors")


# ------------------------------------------------------------------------------------------- memory
@gpu_test
def test_sort_memory_returns_to_its_start(gpu):
    """Every device byte of a SortWork (and of the probe's own buffers) is a DevBuf: live bytes and
    allocations are back at their starting values once every handle is freed -- the file's shared
    handle, grown to the 4.26 M-pair case, included: it is freed first and its bytes must go."""
    import sort_probe as sp
    from fm_spark_amd import _native

    lib = _native.load()
    with_shared = lib.fm_device_bytes_live(), lib.fm_device_allocs_live()
    had_shared = _shared["handle"] is not None
    _close_shared()
    bytes0, allocs0 = lib.fm_device_bytes_live(), lib.fm_device_allocs_live()
    if had_shared:  # its six work buffers
        assert bytes0 < with_shared[0] and allocs0 == with_shared[1] - 6
    bytes0, allocs0 = lib.fm_device_bytes_live(), lib.fm_device_allocs_live()
    hs = [sp.SortHandle() for _ in range(2)]
    for h, (n, bits) in zip(hs, [(65537, 27), (4097, 10)]):
        keys, order, _, u2 = problem(n, bits)
        check(h.sort(sp.PAIRS64, keys, u2, hi_bit=bits, use_final=True), keys, order, u2[order], "memory")
    assert lib.fm_device_bytes_live() > bytes0 and lib.fm_device_allocs_live() >= allocs0 + 12
    with pytest.raises(sp.SortProbeError):
        hs[0].sort(sp.PAIRS64, keys, u2, hi_bit=10, n=-1)  # the probe's buffers of a failed call go too
    for h in hs:
        h.close()
    assert (lib.fm_device_bytes_live(), lib.fm_device_allocs_live()) == (bytes0, allocs0)
