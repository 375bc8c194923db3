"""SELECT DISTINCT without a device: the parser, the numpy reference (tests/distinct_ref.py) on hand-written cases, the C
ABI's argument checks up to where a device is needed, and the distinct shapes of the JIT selftest."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import distinct_ref
import helpers
from pinot_amd import _lib
from pinot_amd.query import parse_sql

EINVAL, EUNSUPPORTED = -1, -2


# ------------------------------------------------------------------------------------------------ parser
def test_parse_distinct_spellings():
    qc = parse_sql("SELECT DISTINCT column1 FROM testTable")
    assert qc.is_distinct() and qc.distinct and not qc.is_selection()
    assert qc.group_by == ["column1"] and qc.select_columns == ["column1"]
    assert qc.limit == 10 and qc.order_by == [] and qc.filter is None and not qc.aggregations
    qc = parse_sql("select distinct a, b, c from t where a > 3 and b in ('x', 'y') order by b desc, a limit 25")
    assert qc.is_distinct() and qc.group_by == ["a", "b", "c"] and qc.limit == 25
    assert qc.order_by == [("b", False), ("a", True)]
    assert qc.order_by_targets() == [(0, 1, False), (0, 0, True)]
    assert len(qc.cnf) == 2
    # LIMIT 0, OFFSET 0 and the "offset, limit" spelling with a zero offset are what a selection parses too
    assert parse_sql("SELECT DISTINCT a FROM t LIMIT 0").limit == 0
    assert parse_sql("SELECT DISTINCT a FROM t LIMIT 7 OFFSET 0").limit == 7
    assert parse_sql("SELECT DISTINCT a FROM t LIMIT 0, 7").limit == 7
    # a column listed twice is one distinct column
    assert parse_sql("SELECT DISTINCT a, b, a FROM t").group_by == ["a", "b"]
    # a time-bucket transform and an arithmetic expression are distinct columns as they are GROUP BY keys
    qc = parse_sql("SELECT DISTINCT dateTrunc('DAY', ts), a FROM t ORDER BY a LIMIT 5")
    assert qc.is_distinct() and len(qc.group_by) == 2 and qc.group_by[1] == "a"
    g = parse_sql("SELECT dateTrunc('DAY', ts), COUNT(*) FROM t GROUP BY dateTrunc('DAY', ts)")
    assert qc.group_by[0] == g.group_by[0]
    qc = parse_sql("SELECT DISTINCT a + b FROM t")
    assert qc.is_distinct() and qc.expressions() == qc.group_by
    # queries that are not distinct queries stay what they were
    assert not parse_sql("SELECT a FROM t").is_distinct()
    assert not parse_sql("SELECT a, COUNT(*) FROM t GROUP BY a").is_distinct()
    assert not parse_sql("SELECT DISTINCTCOUNT(a) FROM t").is_distinct()
    qc = parse_sql("SELECT distinct FROM t")  # a column named "distinct"
    assert not qc.is_distinct() and qc.select_columns == ["distinct"]


@pytest.mark.parametrize("sql, cause", [
    ("SELECT DISTINCT a, COUNT(*) FROM t", "aggregation"),
    ("SELECT DISTINCT SUM(b) FROM t", "aggregation"),
    ("SELECT DISTINCT a FROM t GROUP BY a", "GROUP BY"),
    ("SELECT DISTINCT * FROM t", "*"),
    ("SELECT DISTINCT a, b FROM t ORDER BY c", "ORDER BY c"),
    ("SELECT DISTINCT a FROM t ORDER BY a, b DESC", "ORDER BY b"),
    ("SELECT DISTINCT a FROM t ORDER BY A", "ORDER BY A"),          # column names are case-sensitive
    ("SELECT DISTINCT a FROM t LIMIT 5 OFFSET 2", "OFFSET"),
    ("SELECT DISTINCT a FROM t LIMIT 2, 5", "OFFSET"),
    ("SELECT DISTINCT a FROM t LIMIT -1", "LIMIT"),
])
def test_parse_distinct_refusals(sql, cause):
    with pytest.raises(ValueError) as e:
        parse_sql(sql)
    assert cause in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------------ reference
T0 = {"k": np.array([2.0, np.nan, -0.0, 0.0, 2.0, float("nan")]), "s": np.array(["b", "a", "b", "a", "b", "a"]),
      "i": np.array([5, 5, -1, 7, 5, 5], dtype=np.int32)}
T1 = {"k": np.array([-np.inf, 2.0, np.nan]), "s": np.array(["a", "c", "a"]), "i": np.array([7, 9, 5], dtype=np.int32)}
T2 = {"k": np.array([1.5]), "s": np.array(["～"]), "i": np.array([0], dtype=np.int32)}


def test_reference_identity_and_double_order():
    rows, matched, scanned = distinct_ref.distinct([T0, T1], [None, None], ["k"], [("k", True)], limit=100)
    # one NaN, -0.0 and 0.0 apart; Double.compare: -inf < -0.0 < 0.0 < 2.0 < NaN
    assert distinct_ref.same_rows(rows, [(-np.inf,), (-0.0,), (0.0,), (2.0,), (np.nan,)])
    assert not distinct_ref.same_rows([(0.0,)], [(-0.0,)]) and distinct_ref.same_rows([(np.nan,)], [(float("nan"),)])
    assert matched == 9 and scanned == 2
    rows, _, _ = distinct_ref.distinct([T0, T1], [None, None], ["k"], [("k", False)], limit=2)
    assert distinct_ref.same_rows(rows, [(np.nan,), (2.0,)])


def test_reference_string_order_is_utf16():
    # U+FF5E sorts before U+1F600 by code point and by UTF-8 bytes, after it by UTF-16 code units (a surrogate pair)
    t = {"s": np.array(["～", "\U0001F600", "a"])}
    rows, _, _ = distinct_ref.distinct([t], [None], ["s"], [("s", True)], limit=10)
    assert rows == [("a",), ("\U0001F600",), ("～",)]
    assert sorted(["～", "\U0001F600"], key=lambda s: s.encode()) == ["～", "\U0001F600"]


def test_reference_order_by_subset_ties_by_global_key():
    # ORDER BY s only: rows equal on s come in ascending global key order -- the LAST column (i) most significant
    rows, _, _ = distinct_ref.distinct([T0, T1], [None, None], ["s", "k", "i"], [("s", False)], limit=100)
    assert distinct_ref.same_rows(rows, [("c", 2.0, 9), ("b", -0.0, -1), ("b", 2.0, 5),
                                         ("a", np.nan, 5), ("a", -np.inf, 7), ("a", 0.0, 7)])
    # DESC reverses the values of the ORDER BY column, not the tie rule
    rows, _, _ = distinct_ref.distinct([T0, T1], [None, None], ["s", "i"], [("s", True)], limit=3)
    assert rows == [("a", 5), ("a", 7), ("b", -1)]
    # mixed directions on two columns
    rows, _, _ = distinct_ref.distinct([T0, T1], [None, None], ["s", "i"], [("s", True), ("i", False)], limit=100)
    assert rows == [("a", 7), ("a", 5), ("b", 5), ("b", -1), ("c", 9)]


def test_reference_filter_limit_and_matched():
    masks = [T0["i"] == 5, T1["i"] > 100]
    rows, matched, _ = distinct_ref.distinct([T0, T1], masks, ["s"], [("s", True)], limit=10)
    assert rows == [("a",), ("b",)] and matched == 4
    assert distinct_ref.distinct([T0, T1], masks, ["s"], [("s", True)], limit=0) == ([], 0, 0)
    rows, matched, _ = distinct_ref.distinct([T0, T1], [T0["i"] > 100, T1["i"] > 100], ["s"], [], limit=10)
    assert rows == [] and matched == 0
    assert distinct_ref.distinct_set([T0, T1], masks, ["s", "i"]) == {("a", 5), ("b", 5)}


def test_reference_staged_scan_without_order_by():
    assert distinct_ref.stages(8) == [[0], [1, 2], [3, 4, 5, 6], [7]]
    assert distinct_ref.stages(1) == [[0]] and distinct_ref.stages(3) == [[0], [1, 2]]
    tables = [{"v": np.array([9, 9], dtype=np.int32)}, {"v": np.array([4], dtype=np.int32)},
              {"v": np.array([7, 4], dtype=np.int32)}, {"v": np.array([1], dtype=np.int32)}]
    none = [None] * 4
    # LIMIT 1: the first stage (segment 0) holds a row already
    assert distinct_ref.distinct(tables, none, ["v"], [], limit=1) == ([(9,)], 2, 1)
    # LIMIT 3: stage 1 holds 1 row, stage 2 (segments 1, 2) brings it to 3: stop; the rows in ascending key order
    assert distinct_ref.distinct(tables, none, ["v"], [], limit=3) == ([(4,), (7,), (9,)], 5, 3)
    # LIMIT 2: the same stages (1 < 2 after the first), 3 rows held, the first 2 by key returned
    assert distinct_ref.distinct(tables, none, ["v"], [], limit=2) == ([(4,), (7,)], 5, 3)
    # LIMIT 10: never reached, every segment scanned
    assert distinct_ref.distinct(tables, none, ["v"], [], limit=10) == ([(1,), (4,), (7,), (9,)], 6, 4)
    # a hash plan scans the whole batch
    assert distinct_ref.distinct(tables, none, ["v"], [], limit=1, staged=False) == ([(1,)], 6, 4)
    # an ORDER BY always does
    assert distinct_ref.distinct(tables, none, ["v"], [("v", True)], limit=1) == ([(1,)], 6, 4)


def test_reference_dictionary_only():
    tables = [{"v": np.array([5, 3, 5, 9], dtype=np.int32)}, {"v": np.array([1, 9], dtype=np.int32)}]
    assert distinct_ref.dictionary_only(tables, "v", True, 2) == ([(1,), (3,)], 4)
    assert distinct_ref.dictionary_only(tables, "v", False, 3) == ([(9,), (5,), (3,)], 5)
    assert distinct_ref.dictionary_only(tables, "v", True, 100) == ([(1,), (3,), (5,), (9,)], 5)
    assert distinct_ref.dictionary_only(tables, "v", True, 0) == ([], 0)


def test_reference_reproduces_pinot_distinct_counts():
    data = np.load(os.path.join(helpers.GOLDEN, "test_data_sv.npz"), allow_pickle=False)
    table = {c: data[c] for c, _ in helpers.SV_COLUMNS}
    with open(os.path.join(helpers.GOLDEN, "sv_distinct_expected.json")) as f:
        cases = json.load(f)["cases"]
    assert [c["rows"] for c in cases] == [6582, 21968]
    for case in cases:
        qc = parse_sql(case["sql"])
        rows, matched, _ = distinct_ref.distinct([table], [None], qc.group_by, [], qc.limit)
        assert len(rows) == case["rows"] and matched == 30000, case["name"]
    assert len(np.unique(table["column1"])) == 6582


# ------------------------------------------------------------------------------------------------ C ABI
@pytest.fixture()
def query_handle():
    L = _lib.lib()
    q = C.c_void_p()
    assert L.pinot_amd_query_create(C.byref(q)) == 0
    yield L, q
    L.pinot_amd_query_destroy(q)


def _execute(L, q):
    """pinot_amd_execute on a segment handle that is never dereferenced: a distinct query's own checks come first."""
    fake = C.create_string_buffer(64)
    segs = (C.c_void_p * 1)(C.addressof(fake))
    r = C.c_void_p()
    return L.pinot_amd_execute(q, segs, 1, None, C.byref(r))


def test_abi_set_distinct_argument_checks(query_handle):
    L, q = query_handle
    assert L.pinot_amd_query_set_distinct(q, -1) == EINVAL
    assert b"set_distinct" in L.pinot_amd_last_error()
    assert L.pinot_amd_query_set_distinct(None, 10) == EINVAL
    assert L.pinot_amd_query_set_distinct(q, 0) == 0
    assert L.pinot_amd_query_set_distinct(q, 10) == 0
    # no key
    assert _execute(L, q) == EINVAL
    assert b"DISTINCT" in L.pinot_amd_last_error() and b"distinct column" in L.pinot_amd_last_error()


def test_abi_distinct_beside_aggregation_refused(query_handle):
    L, q = query_handle
    assert L.pinot_amd_query_add_group_by(q, b"a") == 0
    assert L.pinot_amd_query_add_aggregation(q, 0, b"*", None) == 0
    assert L.pinot_amd_query_set_distinct(q, 10) == 0
    assert _execute(L, q) == EINVAL
    assert b"aggregation" in L.pinot_amd_last_error()


def test_abi_distinct_beside_selection_refused(query_handle):
    L, q = query_handle
    assert L.pinot_amd_query_add_group_by(q, b"a") == 0
    assert L.pinot_amd_query_add_selection(q, b"b", None) == 0
    assert L.pinot_amd_query_set_distinct(q, 10) == 0
    assert _execute(L, q) == EINVAL
    assert b"selection" in L.pinot_amd_last_error()


@pytest.mark.parametrize("call", ["set_result_limit", "set_server_options", "set_segment_trim"])
def test_abi_distinct_beside_group_by_result_options_refused(query_handle, call):
    L, q = query_handle
    assert L.pinot_amd_query_add_group_by(q, b"a") == 0
    assert L.pinot_amd_query_set_distinct(q, 10) == 0
    if call == "set_result_limit":
        assert L.pinot_amd_query_set_result_limit(q, 10, 5000, 1000000) == 0
    elif call == "set_server_options":
        assert L.pinot_amd_query_set_server_options(q, 0, 10000) == 0
    else:
        assert L.pinot_amd_query_set_segment_trim(q, 100) == 0
    assert _execute(L, q) == EINVAL
    assert call.encode() in L.pinot_amd_last_error()


def test_abi_distinct_with_key_space_unsupported(query_handle):
    L, q = query_handle
    assert L.pinot_amd_query_add_group_by(q, b"a") == 0
    vals = (C.c_int64 * 3)(1, 2, 3)
    assert L.pinot_amd_query_set_group_key_values(q, b"a", 0, 3, vals, None, None) == 0
    assert L.pinot_amd_query_set_distinct(q, 10) == 0
    assert _execute(L, q) == EUNSUPPORTED
    assert b"key space" in L.pinot_amd_last_error() and b"a" in L.pinot_amd_last_error()


def test_jit_selftest_compiles_distinct_shapes(capfd):
    """The selftest names every shape it compiled for gfx950 (verbose): each distinct table kind is among them, the
    LDS kind also with the read before the LDS atomic (shape key field |DQ<kind>.<read>)."""
    assert _lib.lib().pinot_amd_jit_selftest(1) == 0
    ok = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("JIT ok:")]
    for field in ("|DQ1.0:", "|DQ1.1:", "|DQ2.0:", "|DQ3.0:"):
        assert sum(field in ln for ln in ok) == 1, field


def test_cross_rank_merges_and_key_space_refuse_a_distinct_query():
    from pinot_amd import dist, engine
    qc = parse_sql("SELECT DISTINCT a FROM t ORDER BY a LIMIT 5")
    with pytest.raises(ValueError) as e:
        dist.merge_groups(qc, {})
    assert "DISTINCT" in str(e.value)

    class Result:
        pass
    r = Result()
    r.qc = qc
    with pytest.raises(ValueError) as e:
        dist.merge_result(r)
    assert "DISTINCT" in str(e.value)
    with pytest.raises(_lib.PinotAmdError) as e:  # refused before any segment is read
        engine.ServerQueryExecutor().execute(qc, [], key_space={"a": [1, 2]})
    assert "key_space" in str(e.value)
    # the same calls on a group-by context get past that refusal
    g = parse_sql("SELECT a, COUNT(*) FROM t GROUP BY a")
    dist._refuse_distinct(g)
