"""Selection queries without a GPU: the SQL front end (SELECT *, OFFSET, default LIMIT, the server's schema order), the
numpy reference against the values Pinot's own test asserts over test_data-sv.avro, the C ABI's argument checks on
a query handle, and the top-K kernel shapes of the JIT selftest (compiled, not run)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import helpers
import selection_ref
from pinot_amd import _lib
from pinot_amd.query import parse_sql


# ------------------------------------------------------------------------------------------------ parser
def test_parse_selection_defaults():
    qc = parse_sql("SELECT column1, column5 FROM testTable")
    assert qc.is_selection()
    assert (qc.limit, qc.offset) == (10, 0)            # Pinot's default LIMIT
    assert qc.select_list() == ["column1", "column5"]
    assert qc.selection_columns() == ["column1", "column5"]
    assert not parse_sql("SELECT COUNT(*) FROM testTable").is_selection()
    assert not parse_sql("SELECT column1, COUNT(*) FROM testTable GROUP BY column1").is_selection()


def test_parse_offset_both_spellings():
    a = parse_sql("SELECT a FROM t ORDER BY b DESC LIMIT 7 OFFSET 3")
    b = parse_sql("SELECT a FROM t ORDER BY b DESC LIMIT 3, 7")
    for qc in (a, b):
        assert (qc.limit, qc.offset) == (7, 3)
        assert qc.order_by == [("b", False)]
    assert parse_sql("SELECT a FROM t LIMIT 0").limit == 0
    for bad in ("SELECT a FROM t LIMIT -1", "SELECT a FROM t LIMIT 5 OFFSET -2", "SELECT a FROM t LIMIT 1.5"):
        with pytest.raises(ValueError):
            parse_sql(bad)
    # aggregation queries keep their LIMIT handling and carry no offset
    g = parse_sql("SELECT a, COUNT(*) FROM t GROUP BY a LIMIT 25")
    assert (g.limit, g.offset) == (25, 0) and not g.is_selection()


def test_parse_star_and_schema_order():
    class Seg:
        columns = {"b": None, "a": None, "C": None, "d": None}

    qc = parse_sql("SELECT * FROM t LIMIT 5")
    assert qc.is_selection() and qc.select_columns == ["*"]
    assert qc.select_list(Seg) == ["C", "a", "b", "d"]  # String order
    with pytest.raises(ValueError):
        qc.select_list()
    with pytest.raises(ValueError):
        parse_sql("SELECT *, COUNT(*) FROM t")
    # the server's schema: ORDER BY columns first, deduplicated, in ORDER BY order; then the rest of the select list
    qc = parse_sql("SELECT a, b, d FROM t ORDER BY d DESC, C, d LIMIT 3")
    assert qc.selection_columns() == ["d", "C", "a", "b"]
    assert qc.select_list() == ["a", "b", "d"]
    # LIMIT 0: the ORDER BY is ignored
    assert parse_sql("SELECT a FROM t ORDER BY b LIMIT 0").selection_columns() == ["a"]
    # the parse cache returns the same context
    assert parse_sql("SELECT a, b, d FROM t ORDER BY d DESC, C, d LIMIT 3") is qc


# ------------------------------------------------------------------------------------------------ reference
def _sv_table():
    data = np.load(os.path.join(helpers.GOLDEN, "test_data_sv.npz"), allow_pickle=False)
    return {c: data[c] for c, _ in helpers.SV_COLUMNS}


def _sv_filter_mask(t):
    # helpers.SV_FILTER, spelled out
    return ((t["column1"] > 100000000) & (t["column3"] >= 20000000) & (t["column3"] <= 1000000000)
            & (t["column5"] == "gFuH") & ((t["column6"] < 500000000) | ~np.isin(t["column11"], ["t", "P"]))
            & (t["daysSinceEpoch"] == 126164076))


def load_selection_expected():
    with open(os.path.join(helpers.GOLDEN, "sv_selection_expected.json")) as f:
        return json.load(f)


def test_reference_reproduces_pinot_selection_values():
    t = _sv_table()
    mask = _sv_filter_mask(t)
    assert int(mask.sum()) == 6129
    star = sorted(t, key=lambda n: n.encode("utf-16-be"))
    for case in load_selection_expected()["cases"]:
        cols = star if case["select"] == ["*"] else case["select"]
        rows, origins, matched = selection_ref.select([t], [mask if case["filtered"] else None], cols,
                                                      [tuple(o) for o in case["order_by"]], case["limit"])
        assert len(rows) == case["limit"] and len(origins) == case["limit"], case["name"]
        row = dict(zip(cols, rows[case["row"]]))
        for c, v in case["values"].items():
            assert row[c] == v, (case["name"], c, row[c], v)
        assert matched == case["docs_matched"], case["name"]


def test_reference_order_and_ties():
    t0 = {"k": np.array([2.0, np.nan, -0.0, 0.0, 2.0], dtype=np.float64), "s": np.array(["b", "a", "b", "a", "b"])}
    t1 = {"k": np.array([-np.inf, 2.0, np.nan], dtype=np.float64), "s": np.array(["a", "b", "a"])}
    rows, origins, matched = selection_ref.select([t0, t1], None, ["k"], [("k", True)], limit=8)
    assert origins == [(1, 0), (0, 2), (0, 3), (0, 0), (0, 4), (1, 1), (0, 1), (1, 2)] and matched == 8
    rows, origins, _ = selection_ref.select([t0, t1], None, ["s", "k"], [("s", False), ("k", False)], limit=3, offset=1)
    assert origins == [(0, 0), (0, 4), (1, 1), (0, 2)]  # offset + limit rows; DESC reverses values, not the tie rule
    rows, origins, matched = selection_ref.select([t0, t1], [t0["s"] == "a", None], ["k"], (), limit=3)
    assert origins == [(0, 1), (0, 3), (1, 0)] and matched == 3
    assert selection_ref.select([t0, t1], None, ["k"], [("k", True)], limit=0) == ([], [], 0)


# ------------------------------------------------------------------------------------------------ C ABI
@pytest.fixture()
def query_handle():
    L = _lib.lib()
    q = C.c_void_p()
    assert L.pinot_amd_query_create(C.byref(q)) == 0
    yield L, q
    L.pinot_amd_query_destroy(q)


def test_abi_selection_argument_checks(query_handle):
    L, q = query_handle
    EINVAL = -1
    idx = C.c_int32(-1)
    assert L.pinot_amd_query_add_selection(q, b"a", C.byref(idx)) == 0 and idx.value == 0
    assert L.pinot_amd_query_add_selection(q, b"b", C.byref(idx)) == 0 and idx.value == 1
    assert L.pinot_amd_query_add_selection(q, b"c", None) == 0
    assert L.pinot_amd_query_add_selection(q, None, None) == EINVAL
    assert L.pinot_amd_query_add_selection(None, b"a", None) == EINVAL
    assert L.pinot_amd_query_add_selection_order_by(q, b"z", 0) == 0     # need not be selected
    assert L.pinot_amd_query_add_selection_order_by(q, None, 1) == EINVAL
    assert L.pinot_amd_query_set_selection_limit(q, 10, 5) == 0
    assert L.pinot_amd_query_set_selection_limit(q, 0, 0) == 0
    assert L.pinot_amd_query_set_selection_limit(q, -1, 0) == EINVAL
    assert L.pinot_amd_query_set_selection_limit(q, 1, -1) == EINVAL
    assert b"set_selection_limit" in L.pinot_amd_last_error()


def test_abi_selection_with_aggregation_refused(query_handle):
    """A query with selection columns and an aggregation or a GROUP BY fails at execute, before any segment is
    read (the segment handle here is never dereferenced)."""
    L, q = query_handle
    assert L.pinot_amd_query_add_selection(q, b"a", None) == 0
    assert L.pinot_amd_query_add_aggregation(q, 0, b"*", None) == 0
    fake = C.create_string_buffer(64)
    segs = (C.c_void_p * 1)(C.addressof(fake))
    r = C.c_void_p()
    assert L.pinot_amd_execute(q, segs, 1, None, C.byref(r)) == -1
    assert b"selection" in L.pinot_amd_last_error()
    # the selection result calls refuse a null result
    n = C.c_int64()
    assert L.pinot_amd_result_num_rows(None, C.byref(n)) == -1
    assert L.pinot_amd_result_selection_string(None, 0, 0) is None


def test_jit_selftest_compiles_topk_shapes():
    assert _lib.lib().pinot_amd_jit_selftest(0) == 0
