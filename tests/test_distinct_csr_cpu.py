"""DISTINCTCOUNT in the C ABI, the parts that need no device: query.sets_from_csr (the value sets of
pinot_amd_result_fetch_distinct_values as the mirror path's partials) and the aggregation type's acceptance by
pinot_amd_query_add_aggregation (libpinot_amd.so loads without a GPU, as tests/test_formats_cpu.py relies on)."""
import ctypes as C
import struct

import numpy as np
import pytest

from pinot_amd.query import DistinctSize, distinct_value, final_value, sets_from_csr


def _bits(x: float) -> int:
    return struct.unpack("<q", struct.pack("<d", x))[0]


def test_sets_from_csr_int():
    sets = sets_from_csr([0, 3, 3, 4], [7, -2, 1 << 40, 5], "LONG")
    assert sets == [frozenset([7, -2, 1 << 40]), frozenset(), frozenset([5])]
    assert all(type(v) is int for s in sets for v in s)
    assert sets_from_csr(np.array([0, 2], dtype=np.int64), np.array([3, 10], dtype=np.int64), "INT") == [frozenset([3, 10])]


def test_sets_from_csr_double_nan_and_signed_zero():
    other_nan = struct.unpack("<q", struct.pack("<Q", 0x7FF8000000000001))[0]   # a NaN with another payload
    vals = [_bits(-0.0), _bits(0.0), _bits(float("nan")), _bits(1.5), other_nan]
    sets = sets_from_csr([0, 3, 5], vals, "DOUBLE")
    assert sets[0] == frozenset(distinct_value(v) for v in (-0.0, 0.0, float("nan")))
    assert len(sets[0]) == 3                                     # -0.0 != 0.0
    assert sets[1] == frozenset([distinct_value(1.5), distinct_value(float("nan"))])
    assert sets[0] & sets[1] == frozenset([distinct_value(float("nan"))])   # every NaN is one value
    # FLOAT values arrive as the double's bits of the float
    f = float(np.float32(0.1))
    assert sets_from_csr([0, 1], [_bits(f)], "FLOAT") == [frozenset([distinct_value(f)])]


def test_sets_from_csr_string():
    strings = {0: "a", 4: "é", 9: ""}
    assert sets_from_csr([0, 0, 2, 3], [4, 0, 9], "STRING", strings) == [frozenset(), frozenset(["é", "a"]), frozenset([""])]
    with pytest.raises(ValueError):
        sets_from_csr([0, 1], [0], "STRING")


def test_sets_from_csr_empty_and_malformed():
    assert sets_from_csr([], [], "INT") == []
    assert sets_from_csr([0], [], "INT") == []                   # no groups
    assert sets_from_csr([0, 0], [], "DOUBLE") == [frozenset()]  # one group, the empty set
    for off in ([1, 2], [0, 2, 1], [0, 3]):
        with pytest.raises(ValueError):
            sets_from_csr(off, [1, 2], "INT")


def test_distinct_size_is_a_partial_known_by_its_size():
    assert final_value("DISTINCTCOUNT", DistinctSize(5)) == 5
    assert final_value("DISTINCTCOUNT", DistinctSize(0)) == 0


def test_abi_accepts_distinctcount():
    from pinot_amd import _lib
    L = _lib.lib()  # loads libpinot_amd.so; no device call
    assert "pinot_amd_result_fetch_distinct_values" in _lib.SIGNATURES
    assert "pinot_amd_result_distinct_string" in _lib.SIGNATURES
    qh = C.c_void_p()
    assert L.pinot_amd_query_create(C.byref(qh)) == 0
    try:
        idx = C.c_int32(-1)
        assert L.pinot_amd_query_add_aggregation(qh, 7, b"d0", C.byref(idx)) == 0
        assert idx.value == 0
        assert L.pinot_amd_query_add_aggregation(qh, 7, b"*", C.byref(idx)) == -1          # EINVAL
        assert L.pinot_amd_query_add_aggregation(qh, 7, None, C.byref(idx)) == -1
        assert L.pinot_amd_query_add_aggregation(qh, 8, b"d0", C.byref(idx)) == -1
        assert L.pinot_amd_query_add_aggregation_expr(qh, 7, 1, b"d0", b"d1", C.byref(idx)) == -2   # EUNSUPPORTED
    finally:
        L.pinot_amd_query_destroy(qh)
    # a handle-less call fails cleanly instead of touching a device
    total = C.c_int64()
    assert L.pinot_amd_result_fetch_distinct_values(None, 0, 0, None, None, C.byref(total)) == -1
    assert L.pinot_amd_result_distinct_string(None, 0, 0) is None


def test_engine_modes():
    from pinot_amd import engine
    assert engine.AGG_CODE["DISTINCTCOUNT"] == 7
    assert engine.ServerQueryExecutor().distinct_count == "mirror"
    assert engine.ServerQueryExecutor(distinct_count="native").distinct_count == "native"
    with pytest.raises(ValueError):
        engine.ServerQueryExecutor(distinct_count="device")
