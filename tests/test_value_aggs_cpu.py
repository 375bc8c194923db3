"""PERCENTILE, DISTINCTSUM and DISTINCTAVG without a GPU: the parser's spellings, the rank selection, the mirror
path's fold and merge (query.py), Pinot's own expected values (tests/golden/sv_value_aggs_expected.json) through
that pure Python path over four copies of the SV segment, and the new entry points of the C ABI."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import value_aggs_ref as ref
from helpers import GOLDEN
from pinot_amd import _lib
from pinot_amd.query import (FinalValue, JavaDouble, distinct_sum, distinct_value, final_value, fold_distinct_count,
                             hists_from_csr, merge_partial, parse_sql, percentile_select, reduce_rows, server_table,
                             split_distinct_count)

EINVAL, EUNSUPPORTED = -1, -2
NAN = float("nan")


# ------------------------------------------------------------------------------------------------ the parser
def test_parser_spellings():
    for sql in ["SELECT PERCENTILE50(c) FROM t", "SELECT PERCENTILE(c, 50) FROM t", "SELECT PERCENTILE(c, '50') FROM t",
                "select percentile050(c) from t"]:
        (a,) = parse_sql(sql).aggregations
        assert (a.func, a.column, a.param, a.name) == ("PERCENTILE", "c", 50.0, "percentile50(c)"), sql
    (a,) = parse_sql("SELECT PERCENTILE(c, 99.9) AS p FROM t").aggregations
    assert (a.func, a.param, a.name, a.text) == ("PERCENTILE", 99.9, "p", "percentile(c,99.9)")
    assert [x.param for x in parse_sql("SELECT PERCENTILE0(c), PERCENTILE100(c), PERCENTILE(c, 0.0) FROM t").aggregations] \
        == [0.0, 100.0, 0.0]
    qc = parse_sql("SELECT g, DISTINCTSUM(c), DISTINCTAVG(c) v, PERCENTILE90(c), COUNT(*) FROM t WHERE x > 1 GROUP BY g "
                   "ORDER BY PERCENTILE(c, 90) DESC, distinctsum(c), v LIMIT 3")
    assert [(a.func, a.column, a.param) for a in qc.aggregations] == \
        [("DISTINCTSUM", "c", None), ("DISTINCTAVG", "c", None), ("PERCENTILE", "c", 90.0), ("COUNT", "*", None)]
    assert qc.order_by_targets() == [(1, 2, False), (1, 0, True), (1, 1, True)]


@pytest.mark.parametrize("sql", ["SELECT PERCENTILE101(c) FROM t", "SELECT PERCENTILE(c, -1) FROM t",
                                 "SELECT PERCENTILE(c, 100.5) FROM t", "SELECT PERCENTILE(c, 'nan') FROM t",
                                 "SELECT PERCENTILE(c, 'x') FROM t", "SELECT PERCENTILE(c) FROM t",
                                 "SELECT PERCENTILE50(c, 50) FROM t", "SELECT PERCENTILE(c, d) FROM t"])
def test_parser_refuses_bad_percentiles(sql):
    with pytest.raises(ValueError):
        parse_sql(sql)


# ------------------------------------------------------------------------------------------- the selection
def test_selection_on_runs_of_duplicates():
    """Docs 10 10 10 20 20 30 30 30 30 40 (n = 10): the index (int) (10 * p / 100.0) lands on the first doc of a
    run (p = 30 -> index 3, the first 20), on the last (p = 20 -> index 2, the last 10; p = 80 -> index 8, the last
    30) and inside one."""
    hist = {10: 3, 20: 2, 30: 4, 40: 1}
    docs = [10] * 3 + [20] * 2 + [30] * 4 + [40]
    for p in [0, 20, 29.9, 30, 49.9, 50, 80, 89.9, 90, 99.9, 100]:
        assert percentile_select(hist, p) == ref.percentile(docs, p) == float(docs[9 if p == 100 else int(10.0 * p / 100.0)])
    assert percentile_select(hist, 0) == 10.0 and percentile_select(hist, 100) == 40.0
    assert percentile_select(hist, 99.9) == 40.0 and percentile_select(hist, 50) == 30.0
    assert isinstance(percentile_select(hist, 50), float)
    assert percentile_select({7: 1}, 0) == percentile_select({7: 1}, 100) == 7.0
    assert percentile_select({}, 50) == float("-inf")
    # one double multiply and one double divide, truncated: 1000 docs at p = 99.9 -> index 999, not 998
    big = {i: 1 for i in range(1000)}
    assert percentile_select(big, 99.9) == float(int(1000.0 * 99.9 / 100.0))


def test_selection_orders_like_arrays_sort():
    """-0.0 < 0.0, NaN greatest and one value (two NaN payloads are one histogram key)."""
    docs = np.array([0.0, -0.0, NAN, -1.5, 0.0, -0.0, 2.0, np.float64(np.nan)], dtype=np.float64)
    hist = {}
    for x in docs.tolist():
        hist[distinct_value(x)] = hist.get(distinct_value(x), 0) + 1
    assert len(hist) == 5
    srt = ref.java_sorted(docs)
    assert [math.copysign(1, x) for x in srt[1:5]] == [-1, -1, 1, 1] and math.isnan(srt[-1]) and math.isnan(srt[-2])
    got = [percentile_select(hist, p) for p in (0, 13, 25, 38, 50, 63, 75, 100)]
    exp = [ref.percentile(docs, p) for p in (0, 13, 25, 38, 50, 63, 75, 100)]
    assert [distinct_value(x) for x in got] == [distinct_value(x) for x in exp]
    assert math.copysign(1, got[2]) == -1 and math.copysign(1, got[3]) == 1 and got[2] == got[3] == 0.0
    assert math.isnan(got[-1]) and math.isnan(got[-2]) and got[0] == -1.5


# --------------------------------------------------------------------------------- the sums and the finals
def test_distinct_sum_and_avg_finals():
    assert final_value("DISTINCTSUM", frozenset({1, 2, 3})) == 6.0 and isinstance(distinct_sum(frozenset({1})), float)
    assert final_value("DISTINCTAVG", frozenset({1, 2, 4})) == 7.0 / 3
    assert final_value("DISTINCTSUM", frozenset()) == 0.0 and math.isnan(final_value("DISTINCTAVG", frozenset()))
    big = frozenset({(1 << 53) + 1, 1})   # integers add exactly, rounded once
    assert final_value("DISTINCTSUM", big) == float((1 << 53) + 2)
    fl = frozenset(distinct_value(x) for x in (0.1, 0.2, 0.3, -0.0))
    assert final_value("DISTINCTSUM", fl) == math.fsum([0.1, 0.2, 0.3])
    assert final_value("DISTINCTAVG", fl) == math.fsum([0.1, 0.2, 0.3]) / 4
    assert math.copysign(1, final_value("DISTINCTSUM", frozenset({distinct_value(-0.0)}))) == 1   # 0.0 + -0.0
    assert math.isnan(final_value("DISTINCTSUM", frozenset({distinct_value(NAN), distinct_value(1.0)})))
    assert final_value("PERCENTILE", {5: 2, 9: 1}, 50) == 5.0 and final_value("PERCENTILE", {}, 50) == float("-inf")
    assert final_value("PERCENTILE", FinalValue(3.5), 50) == 3.5 and final_value("DISTINCTSUM", FinalValue(2.0)) == 2.0


# -------------------------------------------------------------------------------- the mirror fold and merge
def test_split_shares_one_sub_query_per_column():
    qc = parse_sql("SELECT g, PERCENTILE50(c), SUM(b), PERCENTILE99(c), DISTINCTCOUNT(c), DISTINCTAVG(c), DISTINCTSUM(d) "
                   "FROM t WHERE b > 1 GROUP BY g")
    base, subs = split_distinct_count(qc)
    assert [a.func for a in base.aggregations] == ["SUM"] and base.group_by == ["g"]
    assert [(i, s.group_by, [a.func for a in s.aggregations]) for i, s in subs] == \
        [(0, ["g", "c"], ["COUNT"]), (5, ["g", "d"], ["COUNT"])]
    assert all(s.filter == qc.filter and s.num_groups_limit >= 1 << 30 for _, s in subs)
    with pytest.raises(ValueError):
        split_distinct_count(parse_sql("SELECT DISTINCTSUM(a * b) FROM t"))


def test_mirror_fold_on_hand_made_groups():
    qc = parse_sql("SELECT g, PERCENTILE50(c), SUM(b), DISTINCTCOUNT(c), DISTINCTSUM(c), DISTINCTAVG(c), PERCENTILE100(d) "
                   "FROM t GROUP BY g")
    base = {(1,): [10.0], (2,): [4.0], (3,): [0.5]}
    sub_c = {(1, 5): [2], (1, 6): [1], (1, 9): [1], (2, 5): [7]}            # group 3: no row of this query
    sub_d = {(1, 0.5): [3], (2, JavaDouble(-0.0)): [1], (2, JavaDouble(0.0)): [1], (3, 2.5): [1]}   # (keys as groups() gives)
    groups = fold_distinct_count(qc, base, [(0, sub_c), (5, sub_d)])
    f = distinct_value
    assert groups[(1,)] == [{5: 2, 6: 1, 9: 1}, 10.0, frozenset({5, 6, 9}), frozenset({5, 6, 9}), frozenset({5, 6, 9}),
                            {f(0.5): 3}]
    assert groups[(2,)] == [{5: 7}, 4.0, frozenset({5}), frozenset({5}), frozenset({5}), {f(-0.0): 1, f(0.0): 1}]
    assert groups[(3,)] == [{}, 0.5, frozenset(), frozenset(), frozenset(), {f(2.5): 1}]
    rows = {r[0]: r[1:] for r in reduce_rows(qc, groups)}
    assert rows[1] == (6.0, 10.0, 3, 20.0, 20.0 / 3, 0.5)       # docs 5 5 6 9: index (int) (4 * 50 / 100.0) = 2
    assert rows[2] == (5.0, 4.0, 1, 5.0, 5.0, 0.0) and math.copysign(1, rows[2][5]) == 1
    assert rows[3][0] == float("-inf") and rows[3][2:4] == (0, 0.0) and math.isnan(rows[3][4]) and rows[3][5] == 2.5
    # the server table orders by the finals
    qo = parse_sql("SELECT g, PERCENTILE50(c), DISTINCTSUM(c) FROM t GROUP BY g ORDER BY PERCENTILE50(c) DESC, g LIMIT 2")
    kept = server_table(qo, {(k,): [v[0], v[3]] for (k,), v in groups.items()})
    assert list(kept) == [(1,), (2,), (3,)]                      # max(5 * LIMIT, minServerGroupTrimSize) keeps all
    assert reduce_rows(qo, kept) == [(1, 6.0, 20.0), (2, 5.0, 5.0)]


def test_merge_partial_halves_equal_the_whole():
    rng = np.random.default_rng(4)
    docs = rng.integers(0, 40, 5_000) * 3
    def hist(v):
        u, c = np.unique(v, return_counts=True)
        return dict(zip(u.tolist(), c.tolist()))
    whole, a, b = hist(docs), hist(docs[:1_777]), hist(docs[1_777:])
    merged = merge_partial("PERCENTILE", a, b)
    assert merged == whole and a == hist(docs[:1_777])           # (the operands are left alone)
    assert merge_partial("PERCENTILE", {}, b) == b
    for p in (0, 50, 99.9, 100):
        assert percentile_select(merged, p) == ref.percentile(docs, p)
    sa, sb = frozenset(a), frozenset(b)
    for fn in ("DISTINCTSUM", "DISTINCTAVG"):
        assert merge_partial(fn, sa, sb) == frozenset(whole)
        assert final_value(fn, merge_partial(fn, sa, sb)) == final_value(fn, frozenset(whole))
    assert final_value("DISTINCTSUM", frozenset(whole)) == ref.distinct_sum(docs)


def test_hists_from_csr():
    off = [0, 2, 2, 3]
    assert hists_from_csr(off, [7, 9, 4], [3, 1, 5], "LONG") == [{7: 3, 9: 1}, {}, {4: 5}]
    bits = np.array([-0.0, 0.0, 1.5]).view(np.int64)
    f = distinct_value
    assert hists_from_csr(off, bits, [1, 2, 3], "DOUBLE") == [{f(-0.0): 1, f(0.0): 2}, {}, {f(1.5): 3}]
    assert hists_from_csr([], [], [], "INT") == []
    with pytest.raises(ValueError):
        hists_from_csr([0, 5], [1], [1], "INT")


# ---------------------------------------------------- Pinot's expected values through the pure Python path
@pytest.fixture(scope="module")
def sv():
    data = np.load(os.path.join(GOLDEN, "test_data_sv.npz"), allow_pickle=False)
    return {c: data[c] for c in ("column1", "column3", "column5", "column6", "column9", "column11", "daysSinceEpoch")}


def sv_filter(s):
    """BaseSingleValueQueriesTest's FILTER (the golden file's filter_sql), restated in numpy."""
    return ((s["column1"] > 100000000) & (s["column3"] >= 20000000) & (s["column3"] <= 1000000000)
            & (s["column5"] == "gFuH") & ((s["column6"] < 500000000) | ~np.isin(s["column11"], ["t", "P"]))
            & (s["daysSinceEpoch"] == 126164076))


def load_golden():
    with open(os.path.join(GOLDEN, "sv_value_aggs_expected.json")) as f:
        return json.load(f)


def golden_cases():
    """(sql, [v1, v2], filtered) for every query, spelling and case of the golden file."""
    g = load_golden()
    out = []
    for section in ("percentile", "distinct_sum", "distinct_avg"):
        for q in g[section]["queries"]:
            for sel in q["select"]:
                for case, exp in q["cases"].items():
                    filtered = case.startswith("filter")   # no_filter | filter | group_by | filter_group_by
                    sql = sel + (" WHERE " + g["filter_sql"] if filtered else "") \
                        + (" " + g["group_by_sql"] if case.endswith("group_by") else "")
                    out.append((sql, exp, filtered))
    return out


def segment_partials(qc, seg, mask):
    """One segment's groups of qc through the mirror path's own functions: the base and value-set sub queries'
    groups (COUNT(*) per group) restated in numpy, folded by fold_distinct_count."""
    base, subs = split_distinct_count(qc)
    assert [a.func for a in base.aggregations] == ["COUNT"]

    def counted(columns):
        cols = [seg[c][mask] for c in columns]
        if not cols:
            return {(): [int(mask.sum())]}
        u, c = np.unique(np.stack(cols, axis=1), axis=0, return_counts=True)
        return {tuple(k): [n] for k, n in zip(u.tolist(), c.tolist())}
    return fold_distinct_count(qc, counted(base.group_by), [(i, counted(s.group_by)) for i, s in subs])


def test_golden_file_is_complete():
    g = load_golden()
    assert len(g["percentile"]["queries"]) == 4 and len(g["percentile"]["queries"][0]["select"]) == 3
    assert sorted(a.param for q in g["percentile"]["queries"] for a in parse_sql(q["select"][0]).aggregations) == \
        [50.0, 50.0, 90.0, 90.0, 95.0, 95.0, 99.0, 99.0]
    assert len(golden_cases()) == (3 + 1 + 1 + 1 + 1 + 1) * 4


def test_pinot_values_through_python_path(sv):
    """Four copies of the segment, as BaseQueriesTest.getBrokerResponse runs them: per copy the mirror fold's
    partials, merged with merge_partial, then the server table and the broker reduce. Every value equals Pinot's,
    and the per-doc restatement (value_aggs_ref) agrees."""
    g = load_golden()
    masks = {False: np.ones(len(sv["column1"]), dtype=bool), True: sv_filter(sv)}
    assert 4 * int(masks[True].sum()) == g["num_docs"]["filter"] and 4 * len(sv["column1"]) == g["num_docs"]["no_filter"]
    done = {}
    for sql, exp, filtered in golden_cases():
        qc = parse_sql(sql)
        what = (tuple((a.text, a.alias) for a in qc.aggregations), filtered, bool(qc.group_by))
        if what not in done:   # (the three spellings of PERCENTILE50 parse to one query)
            one = segment_partials(qc, sv, masks[filtered])
            merged = {}
            for _ in range(4):
                for k, parts in one.items():
                    merged[k] = [merge_partial(a.func, x, y) for a, x, y in zip(qc.aggregations, merged[k], parts)] \
                        if k in merged else parts
            rows = reduce_rows(qc, server_table(qc, merged) if qc.group_by else merged)
            assert len(rows) == 1, sql
            per_doc = ref.reference_rows(qc, [sv] * 4, (lambda s: masks[True]) if filtered else None)
            done[what] = (rows[0], per_doc[tuple(rows[0][:len(qc.group_by)])])
        row, restated = done[what]
        assert list(row[len(qc.group_by):]) == exp, (sql, row)
        assert restated == exp, (sql, restated)


# ------------------------------------------------------------------------------------------------- the ABI
def test_abi_symbols_and_refusals():
    assert "pinot_amd_query_add_aggregation_param" in _lib.SIGNATURES
    assert "pinot_amd_result_fetch_value_counts" in _lib.SIGNATURES
    from pinot_amd.engine import AGG_CODE
    assert AGG_CODE["PERCENTILE"] == 8 and AGG_CODE["DISTINCTSUM"] == 9 and AGG_CODE["DISTINCTAVG"] == 10
    assert AGG_CODE["DISTINCTCOUNT"] == 7 and AGG_CODE["COUNT"] == 0
    L = _lib.lib()
    assert L.pinot_amd_abi_version() == 1
    qh = C.c_void_p()
    assert L.pinot_amd_query_create(C.byref(qh)) == 0
    try:
        idx = C.c_int32(-1)
        for t in range(11):
            assert L.pinot_amd_query_add_aggregation_param(qh, t, b"c", 50.0, C.byref(idx)) == 0, t
            assert idx.value == t
        assert L.pinot_amd_query_add_aggregation_param(qh, 0, None, 7e9, C.byref(idx)) == 0    # COUNT(*): param ignored
        assert L.pinot_amd_query_add_aggregation_param(qh, 9, b"c", -5.0, C.byref(idx)) == 0   # ignored for DISTINCTSUM
        assert L.pinot_amd_query_add_aggregation_param(qh, 11, b"c", 50.0, C.byref(idx)) == EINVAL
        assert L.pinot_amd_query_add_aggregation_param(qh, -1, b"c", 50.0, C.byref(idx)) == EINVAL
        for p in (-1.0, 100.5, NAN, float("inf")):
            assert L.pinot_amd_query_add_aggregation_param(qh, 8, b"c", p, C.byref(idx)) == EINVAL, p
        for p in (0.0, 99.9, 100.0):
            assert L.pinot_amd_query_add_aggregation_param(qh, 8, b"c", p, C.byref(idx)) == 0, p
        for t in (8, 9, 10):
            assert L.pinot_amd_query_add_aggregation_param(qh, t, b"*", 50.0, C.byref(idx)) == EINVAL
            assert L.pinot_amd_query_add_aggregation_param(qh, t, None, 50.0, C.byref(idx)) == EINVAL
            assert L.pinot_amd_query_add_aggregation_expr(qh, t, 1, b"a", b"b", C.byref(idx)) == EUNSUPPORTED
            assert L.pinot_amd_query_add_aggregation(qh, t, b"c", C.byref(idx)) == EINVAL       # the old entry point
        assert L.pinot_amd_query_add_aggregation_param(None, 8, b"c", 50.0, C.byref(idx)) == EINVAL
    finally:
        L.pinot_amd_query_destroy(qh)
    n = C.c_int64()
    assert L.pinot_amd_result_fetch_value_counts(None, 0, 0, None, None, None, None) == EINVAL
    assert L.pinot_amd_result_fetch_value_counts(None, 0, 0, None, None, None, C.byref(n)) == EINVAL
