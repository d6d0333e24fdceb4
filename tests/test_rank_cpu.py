"""CPU: the boundary of top-N ranking (fm_rank_candidates / fm_rank_batch, include/fm_hip.h) and the
NumPy reference the GPU tests compare against (tests/rank_ref.py), pinned here to
oracle.fm_ref.predict on the explicitly concatenated rows."""

import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rank_ref as R
from fm_spark_amd import _native as N
from oracle import fm_ref

HEADER = Path(__file__).resolve().parents[1] / "include" / "fm_hip.h"
_CSRP = C.POINTER(N.fm_csr)
_I32P, _DP, _P = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_void_p


def test_header_binding_and_exports():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert re.search(r"#define\s+FM_RANK_MAX_TOP\s+1024\b", text)
    assert N.FM_RANK_MAX_TOP == 1024
    for name in ("fm_rank_candidates", "fm_rank_batch"):
        assert re.search(r"^int %s\s*\(" % name, text, flags=re.M), name
    assert N.SIGNATURES["fm_rank_candidates"] == (C.c_int, [_P, _CSRP, _CSRP, C.c_int32, C.c_double, C.c_double,
                                                            _I32P, _DP])
    assert N.SIGNATURES["fm_rank_batch"] == (C.c_int, [_P, _P, _P, C.c_int32, C.c_double, C.c_double, _I32P, _DP])
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.lib_path())], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (fm_\w+)$", out, flags=re.M))
    assert {"fm_rank_candidates", "fm_rank_batch"} <= exported


def test_null_context_is_an_error_with_a_message():
    lib = N.load()
    lib.fm_create(None, None)  # leaves another message behind
    assert lib.fm_rank_candidates(None, None, None, 1, 0.0, 1.0, None, None) == -1
    assert b"null fm_ctx" in lib.fm_last_error()
    lib.fm_create(None, None)
    assert lib.fm_rank_batch(None, None, None, 1, 0.0, 1.0, None, None) == -1
    assert b"null fm_ctx" in lib.fm_last_error()


@pytest.mark.parametrize("num_items", [0, -1, 4, 1025, 2.0, True])
def test_recommend_rejects_bad_num_items_before_any_native_call(num_items):
    from fm_spark_amd.linalg import Vectors
    from fm_spark_amd.ml import DataFrame, FactorizationMachinesModel

    class NoDevice:  # any use of the context would raise AttributeError
        pass

    model = FactorizationMachinesModel("uid", 2, 0.0, ctx=NoDevice())
    ctx_df = DataFrame.from_rows([(0, Vectors.sparse(4, [(0, 1.0)]))], ["rowId", "features"])
    cand_df = DataFrame.from_rows([(i, Vectors.sparse(4, [(i, 1.0)])) for i in range(3)], ["rowId", "features"])
    with pytest.raises(ValueError, match="numItems"):
        model.recommend(ctx_df, cand_df, num_items)


def test_recommend_bound_is_the_library_limit():
    from fm_spark_amd.linalg import Vectors
    from fm_spark_amd.ml import DataFrame, FactorizationMachinesModel

    model = FactorizationMachinesModel("uid", 2, 0.0, ctx=object())
    ctx_df = DataFrame.from_rows([(0, Vectors.sparse(4, [(0, 1.0)]))], ["rowId", "features"])
    many = DataFrame.from_rows([(i, Vectors.sparse(4, [(i % 4, 1.0)])) for i in range(1100)], ["rowId", "features"])
    with pytest.raises(ValueError, match="numItems"):
        model.recommend(ctx_df, many, 1025)  # below len(candidates), above FM_RANK_MAX_TOP


# ------------------------------------------------------------------ the reference against the oracle
def _problem(seed, F, k, w0, ctx_lens, cand_lens, id_hi):
    rng = np.random.default_rng(seed)
    w, V, present = R.make_table(rng, F, k, present_frac=0.7)
    return w, V, present, w0, R.make_rows(rng, ctx_lens, id_hi), R.make_rows(rng, cand_lens, id_hi)


@pytest.mark.parametrize("seed,F,k,w0,ctx_lens,cand_lens,id_hi", [
    (1, 40, 1, 0.0, [0, 1, 7], [0, 1, 13, 2], 40),
    (2, 64, 5, 0.75, [0, 1, 30, 3], [0, 1, 13, 13, 1, 0], 80),    # ids >= F: dropped
    (3, 300, 17, -2.5, [0, 200, 1], [13, 0, 1, 5], 300),
])
def test_reference_matches_the_oracle_on_concatenated_rows(seed, F, k, w0, ctx_lens, cand_lens, id_hi):
    w, V, present, w0, ctxs, cands = _problem(seed, F, k, w0, ctx_lens, cand_lens, id_hi)
    ref = R.pair_ref(w, V, present, w0, ctxs, cands)
    model = fm_ref.Model(k=k, w=w, V=V, present=present, w0=w0)
    rp, col, val = R.concat_rows(ctxs, cands)
    U, Cn = len(ctx_lens), len(cand_lens)
    csr = fm_ref.CSR(rp, col, val, np.zeros(U * Cn))
    for lo, hi in ((-np.inf, np.inf), (-0.25, 0.5), (w0 + 1.0, w0 + 2.0)):
        want = fm_ref.predict(model, csr, lo, hi).reshape(U, Cn)
        got = ref.score(lo, hi)
        assert np.all(np.abs(got - want) <= ref.bound), (lo, hi)
    # the w0 case, absent ids and empty rows are all in the problem
    assert (~ref.learned).any() and ref.learned.any()
    assert np.all(ref.key[~ref.learned] == w0)
    assert np.all(ref.score(w0 + 1.0, w0 + 2.0)[~ref.learned] == w0)  # unclamped
    assert (present[np.minimum(cands[1], F - 1)] == 0).any() or (cands[1] >= F).any()


def test_reference_order_is_key_descending_then_row_ascending():
    key = np.array([1.0, 3.0, -2.0, 3.0, 1.0, 0.0, -0.0])
    assert R.ref_order(key).tolist() == [1, 3, 0, 4, 5, 6, 2]
    assert R.ref_order(key, 3).tolist() == [1, 3, 0]
