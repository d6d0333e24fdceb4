"""CPU: the host reference of fm_lists_from_pairs (tests/row_lists_ref.py) against its definition, and the
boundary of the resident row lists: every fm_lists_* / *_lists symbol declared in include/fm_hip.h and
bound in _native.SIGNATURES with the header's argument list."""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import row_lists_ref as L
from fm_spark_amd import _native as N

HEADER = Path(__file__).resolve().parents[1] / "include" / "fm_hip.h"


@pytest.mark.parametrize("seed,U,C_,n", [(0, 1, 1, 0), (1, 1, 5, 9), (2, 7, 3, 40), (3, 40, 11, 25), (4, 13, 200, 300),
                                         (5, 5, 2, 64)])
def test_reference_against_the_definition(seed, U, C_, n):
    rng = np.random.default_rng(seed)
    pc, pd = rng.integers(0, U, n), rng.integers(0, C_, n)
    if n >= 20:  # repeats for certain, and contexts without a pair (the first, the last, one inside) where U allows
        pc[:5], pd[:5] = pc[5:10], pd[5:10]
        if U >= 4:
            pc[np.isin(pc, [0, U // 2, U - 1])] = 1
    ptr, rows = L.lists_from_pairs(pc, pd, U)
    bptr, brows = L.lists_brute(pc, pd, U)
    assert ptr.dtype == np.int64 and rows.dtype == np.int32
    assert np.array_equal(ptr, bptr) and np.array_equal(rows, brows)
    assert ptr[-1] == len(rows) == len({(int(a), int(b)) for a, b in zip(pc, pd)})
    for u in range(U):
        assert np.all(np.diff(rows[ptr[u]:ptr[u + 1]]) > 0)
    if n >= 20 and U >= 4:
        assert ptr[1] == 0 and ptr[U] == ptr[U - 1] and ptr[U // 2 + 1] == ptr[U // 2]
    # the order of the pairs does not matter
    perm = rng.permutation(n)
    again = L.lists_from_pairs(pc[perm], pd[perm], U)
    assert again[0].tobytes() == ptr.tobytes() and again[1].tobytes() == rows.tobytes()


_P, _I64P, _I32P, _DP = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
EXPECTED = {
    "fm_lists_create": (C.c_int, [_P, C.c_int64, C.c_int64, _I64P, _I32P, C.POINTER(_P)]),
    "fm_lists_from_pairs": (C.c_int, [_P, C.c_int64, C.c_int64, _I32P, _I32P, C.c_int64, C.POINTER(_P)]),
    "fm_lists_destroy": (None, [_P]),
    "fm_lists_contexts": (C.c_int64, [_P]),
    "fm_lists_candidates": (C.c_int64, [_P]),
    "fm_lists_total": (C.c_int64, [_P]),
    "fm_lists_longest": (C.c_int64, [_P]),
    "fm_lists_export": (C.c_int, [_P, _P, _I64P, _I32P, C.c_int64]),
    "fm_rank_batch_select_lists": (C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int32, C.c_double, C.c_double, _I32P, _DP]),
    "fm_rank_positions_batch_lists": (C.c_int, [_P, _P, _P, _P, _P, C.c_double, C.c_double, _I32P, _DP]),
    "fm_batch_sample_pairs_lists": (C.c_int, [_P, _P, _P, _I32P, _I32P, C.c_int64, C.c_int32, _P, C.c_double, C.c_double,
                                              C.c_uint64, C.POINTER(_P), _I32P]),
}


def test_every_new_symbol_is_declared_and_bound():
    header = HEADER.read_text()
    assert "typedef struct fm_lists fm_lists;" in header
    for name, sig in EXPECTED.items():
        decl = re.search(r"^(int|void|int64_t)\s+%s\(([^;]*)\);" % name, header, re.M | re.S)
        assert decl, name
        assert len(decl.group(2).split(",")) == len(sig[1]), name  # one ctypes argument per declared parameter
        assert N.SIGNATURES[name] == sig, name
    # the resident forms take the object where the host forms take two arrays
    assert len(N.SIGNATURES["fm_rank_batch_select"][1]) == len(N.SIGNATURES["fm_rank_batch_select_lists"][1]) + 1
    assert len(N.SIGNATURES["fm_rank_positions_batch"][1]) == len(N.SIGNATURES["fm_rank_positions_batch_lists"][1]) + 2
    assert len(N.SIGNATURES["fm_batch_sample_pairs"][1]) == len(N.SIGNATURES["fm_batch_sample_pairs_lists"][1]) + 1


def test_python_layer_exports_row_lists():
    from fm_spark_amd.engine import FMContext, RowLists

    for name in ("export", "close"):
        assert callable(getattr(RowLists, name))
    for name in ("row_lists", "row_lists_from_pairs"):
        assert callable(getattr(FMContext, name))
