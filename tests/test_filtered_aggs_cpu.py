"""Filtered aggregations, AGG(x) FILTER (WHERE f), without a GPU: the parser (forms, result column names, ORDER BY,
the option, refusals), the per-doc restatement of filtered_aggs_ref against the unchanged CPU oracle by Pinot's own
method (FilteredAggregationsTest.testQuery: a filtered query equals its plain per-lane queries), the new entry points
of the C ABI and the query-shape compiler's filtered shapes."""
import ctypes as C
import math

import numpy as np
import pytest

import filtered_aggs_ref as ref
import helpers
import oracle
from helpers import SV_FILTER, sv_segment
from pinot_amd import _lib
from pinot_amd.query import canonical_key, final_value, parse_sql
from pinot_amd.segment import DOUBLE, INT, LONG

EINVAL, EUNSUPPORTED = -1, -2
INF = float("inf")


# ------------------------------------------------------------------------------------------------ 1: the parser
def test_parser_forms_and_names():
    qc = parse_sql("SELECT country, COUNT(*), SUM(clicks) FILTER (WHERE device = 'phone'), "
                   "SUM(impressions) FILTER (WHERE device = 'phone') AS imp, "
                   "AVG(cost) FILTER (WHERE daysSinceEpoch >= 19700 AND campaign IN (3, 7)) "
                   "FROM adAnalytics WHERE clicks > 100 GROUP BY country")
    a = qc.aggregations
    assert [(x.func, x.column, x.filter is not None) for x in a] == \
        [("COUNT", "*", False), ("SUM", "clicks", True), ("SUM", "impressions", True), ("AVG", "cost", True)]
    assert a[0].text == "count(*)" and a[0].cnf == []
    assert a[1].name == a[1].text == "sum(clicks) FILTER(WHERE device = 'phone')"
    assert a[2].name == "imp" and a[2].text == "sum(impressions) FILTER(WHERE device = 'phone')"
    assert a[3].text == "avg(cost) FILTER(WHERE (daysSinceEpoch >= '19700' AND campaign IN ('3','7')))"
    assert [[(p.type, p.column, neg) for p, neg in cl] for cl in a[3].cnf] == \
        [[("RANGE", "daysSinceEpoch", False)], [("IN", "campaign", False)]]
    assert qc.has_filtered_aggregations() and not qc.filtered_aggregations_skip_empty_groups
    assert not parse_sql("SELECT SUM(a) FROM t").has_filtered_aggregations()


def test_parser_names_of_the_reference_tests():
    """FilteredAggregationsTest.java:214, 221."""
    (a,) = parse_sql("SELECT SUM(INT_COL) FILTER(WHERE INT_COL > 9999) FROM MyTable").aggregations
    assert a.text == "sum(INT_COL) FILTER(WHERE INT_COL > '9999')"
    (a,) = parse_sql("SELECT SUM(INT_COL) FILTER(WHERE INT_COL > 9999 AND INT_COL < 1000000) FROM MyTable").aggregations
    assert a.text == "sum(INT_COL) FILTER(WHERE (INT_COL > '9999' AND INT_COL < '1000000'))"


def test_parser_every_function_and_predicate_text():
    qc = parse_sql("SELECT COUNT(*) FILTER (WHERE a <> 1), MIN(x) FILTER (WHERE a NOT IN (1, 2) OR b = 'q'), "
                   "MAX(x) FILTER (WHERE NOT a BETWEEN 1 AND 5), SUMLONG(x) FILTER (WHERE a <= 2.5), "
                   "MINMAXRANGE(x) FILTER (WHERE (a >= 1)) r, SUM(x * y) FILTER (WHERE a < 3) FROM t")
    assert [a.text for a in qc.aggregations] == [
        "count(*) FILTER(WHERE a != '1')",
        "min(x) FILTER(WHERE (a NOT IN ('1','2') OR b = 'q'))",
        "max(x) FILTER(WHERE (NOT a BETWEEN '1' AND '5'))",
        "sumlong(x) FILTER(WHERE a <= '2.5')",
        "minmaxrange(x) FILTER(WHERE a >= '1')",
        "sum(times(x,y)) FILTER(WHERE a < '3')"]
    assert qc.aggregations[4].name == "r" and qc.aggregations[5].expr == ("MUL", "x", "y")
    assert qc.aggregations[2].cnf[0][0][1] is True   # NOT BETWEEN: a negated range leaf
    assert len(qc.aggregations[1].cnf) == 1 and len(qc.aggregations[1].cnf[0]) == 2   # one OR clause


def test_parser_order_by_alias_and_text():
    qc = parse_sql("SELECT g, SUM(x) FILTER (WHERE a > 1) AS s, COUNT(*) FILTER (WHERE a > 1), SUM(x) FROM t GROUP BY g "
                   "ORDER BY s DESC, count(*) FILTER(WHERE a > 1), SUM(x) LIMIT 5")
    assert qc.order_by_targets() == [(1, 0, False), (1, 1, True), (1, 2, True)]
    qc = parse_sql("SELECT g, SUM(x) FILTER (WHERE a > 1), SUM(x) FROM t GROUP BY g ORDER BY sum(x) FILTER (WHERE a > 1) DESC")
    assert qc.order_by_targets() == [(1, 0, False)]


def test_parser_option_and_text_cache():
    sql = "SET filteredAggregationsSkipEmptyGroups = true; SELECT g, SUM(x) FILTER (WHERE a > 1) FROM t GROUP BY g"
    qc = parse_sql(sql)
    assert qc.filtered_aggregations_skip_empty_groups and parse_sql(sql) is qc
    assert not parse_sql("SET filteredAggregationsSkipEmptyGroups = false; SELECT SUM(x) FILTER (WHERE a > 1) FROM t") \
        .filtered_aggregations_skip_empty_groups
    other = parse_sql("SELECT g, SUM(x) FILTER (WHERE a > 2) FROM t GROUP BY g")
    assert other is not qc and other.aggregations[0].text != qc.aggregations[0].text


@pytest.mark.parametrize("sql", [
    "SELECT SUM(x) FILTER (WHERE) FROM t",
    "SELECT SUM(x) FILTER (WHERE ) AS s FROM t",
    "SELECT g, SUM(x) FILTER (WHERE dateTrunc('DAY', ts) > 5) FROM t GROUP BY g",
    "SELECT SUM(x) FILTER (WHERE a > 1 AND timeConvert(ts, 'MILLISECONDS', 'DAYS') = 3) FROM t",
    "SELECT SUM(x) FILTER (a > 1) FROM t",
])
def test_parser_refusals(sql):
    with pytest.raises(ValueError):
        parse_sql(sql)


# ------------------------------------------------------------- 2: the restatement against the unchanged oracle
def _with_arrays(rng, n, **kw):
    """helpers.random_segment and the per-doc arrays it was built from."""
    seen = {}
    real = helpers.build_segment

    def spy(name, cols):
        seen.update({c: np.asarray(v[0]) for c, v in cols.items()})
        return real(name, cols)
    helpers.build_segment = spy
    try:
        bufs = helpers.random_segment(rng, n, **kw)
    finally:
        helpers.build_segment = real
    return seen, bufs


def _finals(qc, groups):
    return {canonical_key(k): [float(v) if a.func in ("SUM", "AVG", "MIN", "MAX", "MINMAXRANGE") else v
                               for a, v in ((a, final_value(a.func, p, a.param)) for a, p in zip(qc.aggregations, parts))]
            for k, parts in groups.items()}


def _check_against_oracle(arrays, bufs, keys, main, lanes, skip=False):
    """main: (sql or None, mask function or None); lanes: [(plain aggregation sql, lane sql or None, lane mask function
    or None)]. The filtered query is never handed to the oracle: per lane the plain query WHERE main AND lane must
    equal the restatement's lane values for the groups it returns (the groups it does not return hold the empty
    values), and the plain query WHERE main gives the group set."""
    select = ", ".join(f"{a} FILTER (WHERE {ls})" if ls else a for a, ls, _ in lanes)
    gb = f" GROUP BY {', '.join(keys)} LIMIT 1000000" if keys else ""
    head = ("SET filteredAggregationsSkipEmptyGroups = true; " if skip else "") + "SELECT " + ", ".join(list(keys) + [select])
    qc = parse_sql(f"{head} FROM t{' WHERE ' + main[0] if main[0] else ''}{gb}")
    exp, matched = ref.reference(qc, arrays, main[1], [f for _, _, f in lanes], skip_empty=skip)

    def where(*parts):
        parts = [f"({p})" for p in parts if p]
        return " WHERE " + " AND ".join(parts) if parts else ""
    if skip and all(ls for _, ls, _ in lanes):
        group_where = where(main[0], " OR ".join(f"({ls})" for _, ls, _ in lanes))
    else:
        group_where = where(main[0])
    n_main, g_main = oracle.execute(f"SELECT {', '.join(list(keys) + ['COUNT(*)'])} FROM t{group_where}{gb}", bufs)
    assert n_main == matched
    if keys:
        assert {canonical_key(k) for k in g_main} == set(exp)
    for lane_sql in sorted({ls or "" for _, ls, _ in lanes}):
        idx = [i for i, (_, ls, _) in enumerate(lanes) if (ls or "") == lane_sql]
        plain = ", ".join(lanes[i][0] for i in idx)
        sql = f"SELECT {', '.join(list(keys) + [plain])} FROM t{where(main[0], lane_sql)}{gb}"
        pq = parse_sql(sql)
        got = _finals(pq, oracle.execute(sql, bufs)[1])
        for k, e in exp.items():
            for j, i in enumerate(idx):
                a = qc.aggregations[i]
                if k in got:
                    assert ref.same(got[k][j], e[i], a, ref.reads_floats(a, arrays[0])), (sql, k, a.text, got[k][j], e[i])
                else:  # no doc of the group in this lane: the function's empty value
                    e0 = ref.final(a, np.zeros(0, dtype=np.int64), bool(keys))
                    assert e[i] == e0 or (math.isnan(e0) and math.isnan(e[i])), (sql, k, a.text, e[i], e0)
        assert set(got) <= set(exp) or not keys
    return exp


@pytest.fixture(scope="module")
def sv():
    data = np.load(helpers.os.path.join(helpers.GOLDEN, "test_data_sv.npz"), allow_pickle=False)
    return [{c: data[c] for c in data.files}], [sv_segment()]


def test_empty_values_of_the_restatement():
    qc = parse_sql("SELECT COUNT(*) FILTER (WHERE a > 0), SUM(a) FILTER (WHERE a > 0), SUMLONG(a) FILTER (WHERE a > 0), "
                   "MIN(a) FILTER (WHERE a > 0), MAX(a) FILTER (WHERE a > 0), AVG(a) FILTER (WHERE a > 0), "
                   "MINMAXRANGE(a) FILTER (WHERE a > 0), SUM(d) FILTER (WHERE a > 0) FROM t")
    seg = {"a": np.array([-1, -2], dtype=np.int32), "d": np.array([0.5, 1.5])}
    lane = [lambda s: s["a"] > 0] * 8
    got, n = ref.reference(qc, [seg], None, lane)
    assert n == 2 and got[()] == [0, 0.0, 0, INF, -INF, -INF, -INF, 0.0]
    assert isinstance(got[()][0], int) and isinstance(got[()][1], float) and isinstance(got[()][2], int)
    # the same through query.final_value from the partials the functions start with
    assert final_value("AVG", (0.0, 0)) == -INF and final_value("MINMAXRANGE", (INF, -INF)) == -INF
    # grouped: the group of the main filter exists with every lane empty; skip mode drops it
    qg = parse_sql("SELECT g, COUNT(*) FILTER (WHERE a > 0), MIN(a) FILTER (WHERE a > 0) FROM t GROUP BY g")
    sg = dict(seg, g=np.array([7, 7], dtype=np.int32))
    assert ref.reference(qg, [sg], None, lane[:2]) == ({(7,): [0, INF]}, 2)
    assert ref.reference(qg, [sg], None, lane[:2], skip_empty=True) == ({}, 0)
    qu = parse_sql("SELECT g, COUNT(*), MIN(a) FILTER (WHERE a > 0) FROM t GROUP BY g")
    assert ref.reference(qu, [sg], None, [None, lane[0]], skip_empty=True) == ({(7,): [2, INF]}, 2)


def test_restatement_equals_oracle_sv(sv):
    """The SV segment of BaseSingleValueQueriesTest: lanes cut from SV_FILTER's own predicates."""
    arrays, bufs = sv
    main = ("column1 > 100000000 AND column3 BETWEEN 20000000 AND 1000000000",
            lambda s: (s["column1"] > 100000000) & (s["column3"] >= 20000000) & (s["column3"] <= 1000000000))
    l1 = ("column5 = 'gFuH'", lambda s: s["column5"] == "gFuH")
    l2 = ("column6 < 500000000 OR column11 NOT IN ('t', 'P')",
          lambda s: (s["column6"] < 500000000) | ~np.isin(s["column11"], ["t", "P"]))
    l3 = ("daysSinceEpoch = 126164076 AND column7 > 2000000000", lambda s: (s["daysSinceEpoch"] == 126164076) & (s["column7"] > 2000000000))
    lanes = [("COUNT(*)", None, None), ("SUM(column1)", *l1), ("MAX(column3)", *l1), ("AVG(column3)", *l2),
             ("COUNT(*)", *l2), ("MINMAXRANGE(column1)", *l3), ("SUMLONG(column3)", *l3), ("MIN(column1)", *l3)]
    assert SV_FILTER.count("column5 = 'gFuH'") == 1
    for keys in ([], ["column9"], ["column11", "column12"]):
        exp = _check_against_oracle(arrays, bufs, keys, main, lanes)
        assert exp
    # no main filter; every aggregation filtered; both group rules
    for skip in (False, True):
        _check_against_oracle(arrays, bufs, ["column9"], (None, None), lanes[1:4] + lanes[5:], skip=skip)


def test_restatement_equals_oracle_random_segments():
    """helpers.random_segment with raw, dictionary, sorted and inverted columns; two segments whose dictionaries
    differ."""
    rng = np.random.default_rng(20260101)
    parts = [_with_arrays(rng, n, name=f"fa{n}", bits_cards=(50, 7), raw_types=(INT, LONG, DOUBLE), inverted=("d1",),
                          sorted_col=True) for n in (1025, 3000)]
    arrays, bufs = [p[0] for p in parts], [p[1] for p in parts]
    main = ("r_int > -600000", lambda s: s["r_int"] > -600000)
    raw = ("r_int BETWEEN -100000 AND 400000", lambda s: (s["r_int"] >= -100000) & (s["r_int"] <= 400000))
    dic = ("d0 IN (3, 10, 17, 24, 346)", lambda s: np.isin(s["d0"], [3, 10, 17, 24, 346]))
    srt = ("ts >= 10 AND ts < 30", lambda s: (s["ts"] >= 10) & (s["ts"] < 30))
    inv = ("d1 = 17", lambda s: s["d1"] == 17)
    none = ("r_long > 4000000000000", lambda s: s["r_long"] > 4000000000000)   # matches no doc
    lanes = [("COUNT(*)", None, None), ("SUM(r_long)", None, None), ("SUM(r_int)", *raw), ("COUNT(*)", *raw),
             ("AVG(r_int)", *dic), ("MIN(r_double)", *dic), ("MAX(r_double)", *srt), ("SUM(r_int * d0)", *srt),
             ("SUMLONG(r_long)", *inv), ("MINMAXRANGE(r_double)", *inv), ("SUM(r_long)", *none), ("AVG(r_int)", *none)]
    for keys in ([], ["d1"], ["ts", "d1"]):
        _check_against_oracle(arrays, bufs, keys, main, lanes)
    exp = _check_against_oracle(arrays, bufs, ["d1"], (None, None), lanes[2:])
    assert all(v[-2:] == [0.0, -INF] for v in exp.values())
    filtered_only = lanes[2:10]
    a = _check_against_oracle(arrays, bufs, ["ts", "d0"], main, filtered_only, skip=False)
    b = _check_against_oracle(arrays, bufs, ["ts", "d0"], main, filtered_only, skip=True)
    assert set(b) < set(a)   # some group has no doc in any lane


# ------------------------------------------------------------------- the paths that do not cover a filter
def test_uncovered_paths_raise_instead_of_ignoring_the_filter():
    """dist.py, key_space= and the mirror split of the value-set functions: a clear error, never a dropped filter."""
    from pinot_amd import dist, engine
    from pinot_amd.query import split_distinct_count
    qc = parse_sql("SELECT g, SUM(x) FILTER (WHERE a > 1) FROM t GROUP BY g")
    with pytest.raises(ValueError, match="cross-rank merge"):
        dist.merge_groups(qc, {})
    with pytest.raises(_lib.PinotAmdError, match="key_space"):
        engine.ServerQueryExecutor().execute(qc, [object()], key_space={"g": [1]})
    dc = parse_sql("SELECT g, DISTINCTCOUNT(x) FILTER (WHERE a > 1), PERCENTILE50(x) FROM t GROUP BY g")
    with pytest.raises(ValueError, match="FILTER"):
        split_distinct_count(dc)
    with pytest.raises(_lib.PinotAmdError, match="DISTINCTCOUNT"):
        engine.ServerQueryExecutor().execute(dc, [object()])


# ------------------------------------------------------------------------------------- 3: the ABI, no device
def _spec(keep, column=b"c", lo=1):
    s = _lib.PredicateSpec()
    s.column = column
    s.type = 4  # PINOT_AMD_RANGE
    s.lower_unbounded, s.upper_unbounded, s.lower_inclusive, s.upper_inclusive = 0, 1, 1, 1
    s.lower_i, s.lower_d = lo, float(lo)
    keep.append(s)
    return s


def test_abi_argument_errors_and_limits():
    assert "pinot_amd_query_add_aggregation_filter_predicate" in _lib.SIGNATURES
    assert "pinot_amd_query_set_filtered_aggregations_skip_empty_groups" in _lib.SIGNATURES
    L = _lib.lib()
    assert L.pinot_amd_abi_version() == 1
    add = L.pinot_amd_query_add_aggregation_filter_predicate
    keep = []
    qh = C.c_void_p()
    assert L.pinot_amd_query_create(C.byref(qh)) == 0
    try:
        idx = C.c_int32(-1)
        assert add(qh, 0, 0, C.byref(_spec(keep)), 0) == EINVAL          # no aggregation yet
        assert L.pinot_amd_query_add_aggregation(qh, 1, b"c", C.byref(idx)) == 0 and idx.value == 0
        assert L.pinot_amd_query_add_aggregation(qh, 0, b"*", C.byref(idx)) == 0 and idx.value == 1
        assert add(qh, 2, 0, C.byref(_spec(keep)), 0) == EINVAL and b"index" in L.pinot_amd_last_error()
        assert add(qh, -1, 0, C.byref(_spec(keep)), 0) == EINVAL
        assert add(qh, 0, 0, None, 0) == EINVAL
        assert add(None, 0, 0, C.byref(_spec(keep)), 0) == EINVAL
        bad = _spec(keep)
        bad.type = 9
        assert add(qh, 0, 0, C.byref(bad), 0) == EINVAL
        assert add(qh, 0, -1, C.byref(_spec(keep)), 0) == EUNSUPPORTED
        assert add(qh, 0, 16, C.byref(_spec(keep)), 0) == EUNSUPPORTED      # a 17th clause
        assert b"16" in L.pinot_amd_last_error() and b"clause" in L.pinot_amd_last_error()
        # 16 leaves shared by the main filter and the lanes: 5 main + 6 + 5, the 17th refused on either side
        for i in range(5):
            assert L.pinot_amd_query_add_predicate(qh, i, C.byref(_spec(keep)), 0) == 0
        for i in range(6):
            assert add(qh, 0, i, C.byref(_spec(keep, lo=i)), i & 1) == 0
        for i in range(5):
            assert add(qh, 1, 15 - i, C.byref(_spec(keep, lo=i)), 0) == 0
        assert add(qh, 1, 0, C.byref(_spec(keep)), 0) == EUNSUPPORTED
        assert b"16" in L.pinot_amd_last_error() and b"predicates" in L.pinot_amd_last_error()
        assert L.pinot_amd_query_add_predicate(qh, 5, C.byref(_spec(keep)), 0) == EUNSUPPORTED
        assert L.pinot_amd_query_set_filtered_aggregations_skip_empty_groups(qh, 1) == 0
        assert L.pinot_amd_query_set_filtered_aggregations_skip_empty_groups(None, 1) == EINVAL
    finally:
        L.pinot_amd_query_destroy(qh)


# --------------------------------------------------------------------------- 4: the query-shape compiler
def test_jit_selftest_compiles_the_filtered_shapes():
    assert _lib.lib().pinot_amd_jit_selftest(0) == 0
