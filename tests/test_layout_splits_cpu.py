"""CPU: fm_batch_layout_splits at the drop-in boundary -- exported, bound, and a null context is an
error through the error channel, not a crash (the header <-> binding equality and the export list
are test_capi.py's)."""

from fm_spark_amd import _native as N


def test_layout_splits_null_arguments_are_errors():
    lib = N.load()
    assert "fm_batch_layout_splits" in N.SIGNATURES
    assert lib.fm_batch_layout_splits(None, None, 1, None, None, None) == -1
    assert lib.fm_last_error()
