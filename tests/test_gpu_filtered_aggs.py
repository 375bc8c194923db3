"""Filtered aggregations, AGG(x) FILTER (WHERE f), evaluated inside the generated scan kernel: every lane's clauses
beside the main filter's, each accumulator guarded by its lane's mask. rows() and the finals of groups() are compared
with the per-doc restatement of filtered_aggs_ref (integers exactly, double sums within 1e-12 relative).

Inputs: 3 segments of 1, 1025 and 5000 docs (a one-doc segment, a tile tail, a tile range padded to the 4-tile group)
whose dictionaries differ; column `mix` is raw in the middle segment and dictionary-encoded in the others. Most cases
run with run-time bit widths and without packed twins (one_shape), so the three segments share one kernel shape; the
table-kind cases of the LDS tables and the register path keep the defaults (one shape per segment)."""
import math

import numpy as np
import pytest

import filtered_aggs_ref as ref
from pinot_amd import segment as S
from pinot_amd.query import canonical_key, final_value, parse_sql

pytestmark = pytest.mark.gpu

INF = float("inf")
SIZES = (1, 1025, 5000)


@pytest.fixture(scope="module")
def engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from pinot_amd import engine as E
    return E


def _columns(rng, n, si):
    """Segment si: dictionary columns drawn from different value ranges per segment (the key remaps are live; `dev`
    value 4 and `inv` value 19 are absent from the middle segment's dictionaries)."""
    lo = (36, 0, 5)[si]
    hi = (37, 30, 37)[si]
    dct = {"detect_sorted": False}
    r_double = np.round(rng.gamma(2.0, 500.0, n), 1)
    r_double[rng.random(n) < 0.02] = np.nan
    r_long = rng.integers(1 << 50, 1 << 51, n).astype(np.int64) * rng.choice([1, 1, 1, -1], n)
    return {
        "k37": ((rng.integers(lo, hi, n) * 7 + 3).astype(np.int32), S.INT, dct),
        "k50": ((rng.integers(0, 40 if si == 1 else 50, n) * 3 + 1).astype(np.int32), S.INT, dct),
        "k1000": ((rng.integers(100 if si == 1 else 0, 1000, n) * 11 + 5).astype(np.int32), S.INT, dct),
        "dev": (rng.integers(0, 4 if si == 1 else 5, n).astype(np.int32), S.INT, dict(dct, inverted=True)),
        "inv": (rng.integers(0, 19 if si == 1 else 20, n).astype(np.int32), S.INT, dict(dct, inverted=True)),
        "big": ((rng.integers(0, 300, n) * 2).astype(np.int32), S.INT, dct),
        "ts": (np.sort(rng.integers(0, 12, n)).astype(np.int32), S.INT, {}),
        "mix": (rng.integers(0, 40, n).astype(np.int32), S.INT, {"dictionary": False} if si == 1 else dct),
        "r_int": (rng.integers(-1000, 1000, n).astype(np.int32), S.INT, {"dictionary": False}),
        "r_long": (r_long, S.LONG, {"dictionary": False}),
        "r_double": (r_double, S.DOUBLE, {"dictionary": False}),
    }


@pytest.fixture(scope="module")
def data(engine):
    rng = np.random.default_rng(4242)
    arrays, segs = [], []
    for si, n in enumerate(SIZES):
        cols = _columns(rng, n, si)
        arrays.append({c: v[0] for c, v in cols.items()})
        segs.append(engine.ImmutableSegment(S.build_segment(f"fa_{n}", cols)))
    return arrays, segs


@pytest.fixture
def one_shape(monkeypatch):
    """Run-time bit widths and raw loads: the three segments run as one launch of one kernel shape."""
    monkeypatch.setenv("PINOT_AMD_GENERIC_BITS", "1")
    monkeypatch.setenv("PINOT_AMD_PACKED", "0")


# the main filters and the lanes of the cases: SQL text and the same condition over a segment's arrays
MAIN = ("r_int > -800", lambda s: s["r_int"] > -800)
L_RAW_INT = ("r_int BETWEEN -300 AND 450", lambda s: (s["r_int"] >= -300) & (s["r_int"] <= 450))
L_RAW_DBL = ("r_double > 700.5", lambda s: s["r_double"] > 700.5)
L_RAW_IN = ("r_int IN (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, -144)", lambda s: np.isin(s["r_int"], [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, -144]))
L_DICT_RANGE = ("k1000 >= 2205 AND k1000 < 8000", lambda s: (s["k1000"] >= 2205) & (s["k1000"] < 8000))
L_IN_BIG = ("big IN (0, 2, 44, 100, 250, 598, 599)", lambda s: np.isin(s["big"], [0, 2, 44, 100, 250, 598]))
L_IN_SMALL = ("dev IN (1, 3)", lambda s: np.isin(s["dev"], [1, 3]))
L_SORTED = ("ts BETWEEN 3 AND 7", lambda s: (s["ts"] >= 3) & (s["ts"] <= 7))
L_INV_EQ = ("inv = 7", lambda s: s["inv"] == 7)
L_ABSENT = ("dev = 4", lambda s: s["dev"] == 4)          # alwaysFalse in the middle segment
L_NONE = ("k50 = 2", lambda s: s["k50"] == 2)            # in no dictionary: an empty lane
L_ALL = ("r_int >= -1000", lambda s: s["r_int"] >= -1000)  # every doc
L_NEG = ("NOT mix BETWEEN 10 AND 29", lambda s: ~((s["mix"] >= 10) & (s["mix"] <= 29)))
L_OR = ("dev = 2 OR r_int < -500 OR big NOT IN (4, 6)", lambda s: (s["dev"] == 2) | (s["r_int"] < -500) | ~np.isin(s["big"], [4, 6]))
L_MIX = ("mix IN (3, 4, 5, 30)", lambda s: np.isin(s["mix"], [3, 4, 5, 30]))
L_ODD = ("r_int IN (" + ", ".join(str(v) for v in range(-999, 1000, 2)) + ")", lambda s: (s["r_int"] & 1) == 1)


def run(engine, data, select, main=MAIN, keys=(), skip=False, executor=None, tail=""):
    """select: [(aggregation sql, lane or None)]. Executes the filtered query and compares rows(), the finals of
    groups() and num_docs_matched() with the restatement. Returns (result, expected groups)."""
    arrays, segs = data
    sel = ", ".join(f"{a} FILTER (WHERE {ln[0]})" if ln else a for a, ln in select)
    gb = f" GROUP BY {', '.join(keys)}" if keys else ""
    q = (("SET filteredAggregationsSkipEmptyGroups = true; " if skip else "") +
         f"SELECT {', '.join(list(keys) + [sel])} FROM t{' WHERE ' + main[0] if main else ''}{gb}" +
         (tail or (" LIMIT 1000000" if keys else "")))
    qc = parse_sql(q)
    exp, matched = ref.reference(qc, arrays, main[1] if main else None, [ln[1] if ln else None for _, ln in select],
                                 skip_empty=skip)
    res = (executor or engine.ServerQueryExecutor()).execute(q, segs)
    assert res.num_docs_matched() == matched, (q, res.num_docs_matched(), matched)
    nk = len(keys)

    def compare(got, what):
        if not tail:
            assert set(got) == set(exp), (q, what, len(got), len(exp))
        for k, g in got.items():
            for a, x, y in zip(qc.aggregations, g, exp[k]):
                assert ref.same(x, y, a, ref.reads_floats(a, arrays[0])), (q, what, k, a.text, x, y)
    compare({canonical_key(r[:nk]): list(r[nk:]) for r in res.rows()}, "rows()")
    compare({canonical_key(k): [final_value(a.func, p, a.param) for a, p in zip(qc.aggregations, parts)]
             for k, parts in res.groups().items()}, "groups()")
    return res, exp


def lanes_of(res):
    info = res.kernel_info()
    assert " +lanes(" in info, info
    n = int(info.split(" +lanes(")[1].split(")")[0])
    return n, info.split(" table=")[1].split()[0], info


# every function in a lane; a LONG sum past 2^53, NaNs under MIN / MAX, an expression, an empty lane
# (15 accumulators beside the main count: the most one query takes)
FUNCTIONS = [("COUNT(*)", None), ("COUNT(*)", L_RAW_INT), ("AVG(r_int)", L_RAW_INT), ("SUM(r_long)", L_RAW_INT),
             ("MINMAXRANGE(r_double)", L_RAW_DBL), ("MIN(r_double)", L_RAW_IN), ("MAX(r_double)", L_RAW_IN),
             ("SUMLONG(r_long)", L_RAW_DBL), ("SUM(r_int * mix)", L_RAW_IN), ("AVG(r_double)", L_NONE),
             ("MIN(r_int)", L_NONE)]


# --------------------------------------------------------------------------------------- every table kind
def test_aggregation_only_registers(engine, data):
    res, exp = run(engine, data, FUNCTIONS)
    assert lanes_of(res)[:2] == (4, "regs"), res.kernel_info()
    e = exp[()]
    assert abs(e[3]) > 2.0 ** 53 and e[1] > 0          # the lane's exact integer sum is past 2^53
    assert e[9:] == [-INF, INF]                        # aggregation only with an empty lane
    lane = np.concatenate([L_RAW_IN[1](s) & MAIN[1](s) for s in data[0]])
    vals = np.concatenate([s["r_double"] for s in data[0]])
    assert np.isnan(vals[lane]).any() and math.isnan(e[5]) and math.isnan(e[6])   # Math.min / Math.max propagate NaN
    res.execute_again()
    assert res.rows()[0][1] == e[1]
    res.destroy()


def test_lds_table_37_keys_two_launch_shapes(engine, data):
    """The <= 40 KiB LDS-privatised table; `mix` is raw in one segment: two encodings, several launches into one table.
    Lanes: dict range, IN on a dictionary of > 64 values, accept mask (<= 64 values), a negated leaf, an OR clause, a
    literal absent from one segment; two aggregations share a lane."""
    select = [("COUNT(*)", None), ("SUM(r_int)", L_DICT_RANGE), ("MAX(r_double)", L_DICT_RANGE), ("COUNT(*)", L_IN_BIG),
              ("AVG(r_long)", L_IN_SMALL), ("SUM(r_int)", L_NEG), ("MIN(r_double)", L_OR), ("SUM(r_long)", L_ABSENT),
              ("COUNT(*)", L_MIX)]
    res, exp = run(engine, data, select, keys=("k37",))
    n, table, info = lanes_of(res)
    assert (n, table) == (7, "lds") and " x" in info, info
    assert len(exp) == 37
    res.destroy()


def test_cu_wide_table_no_main_filter(engine, data):
    """Two key columns, 1850 keys x 9 arrays (11 without the narrow sums): between 40 and 160 KiB, one CU-wide block
    per CU. No main filter at all (gate trap c); a sorted-column lane, a lane matching every doc, an empty lane: the
    group is present with the functions' empty values."""
    select = [("COUNT(*)", None), ("SUM(r_int)", L_SORTED), ("COUNT(*)", L_SORTED), ("AVG(r_int)", L_ALL),
              ("COUNT(*)", L_NONE), ("SUMLONG(r_int)", L_NONE), ("MIN(r_int)", L_NONE), ("AVG(r_double)", L_NONE)]
    res, exp = run(engine, data, select, main=None, keys=("k37", "k50"))
    n, table, _ = lanes_of(res)
    assert (n, table) == (3, "cu"), res.kernel_info()
    assert len(exp) > 1500
    assert all(v[4:] == [0, 0, INF, -INF] for v in exp.values())   # the empty values of COUNT, SUMLONG, MIN, AVG
    res.destroy()


def test_dense_hbm_table_not_partitioned(engine, data, one_shape):
    """~37000 keys: a plain query of this key space takes the partitioned plan; a filtered one keeps the dense HBM
    table with direct atomics (a partition record carries no lane mask)."""
    select = [("COUNT(*)", None), ("SUM(r_long)", L_RAW_INT), ("MAX(r_double)", L_RAW_DBL), ("AVG(r_int)", L_IN_SMALL),
              ("COUNT(*)", L_IN_SMALL), ("MINMAXRANGE(r_int)", L_NONE), ("SUM(r_long)", L_NONE), ("MAX(r_int)", L_NONE)]
    res, exp = run(engine, data, select, keys=("k37", "k1000"))
    assert all(v[5:] == [-INF, 0.0, -INF] for v in exp.values())   # the empty values of MINMAXRANGE, SUM, MAX
    n, table, info = lanes_of(res)
    assert (n, table) == (4, "hbm") and "partitioned" not in info and info.startswith("jit "), info
    plain = engine.ServerQueryExecutor().execute("SELECT k37, k1000, COUNT(*), SUM(r_long) FROM t WHERE r_int > -800 "
                                                 "GROUP BY k37, k1000 LIMIT 1000000", data[1])
    assert "partitioned" in plain.kernel_info(), plain.kernel_info()
    plain.destroy()
    res.destroy()


@pytest.mark.parametrize("hash_lds", ["1", "0"])
def test_hash_plan(engine, data, one_shape, monkeypatch, hash_lds):
    monkeypatch.setenv("PINOT_AMD_GROUP_PLAN", "hash")
    monkeypatch.setenv("PINOT_AMD_HASH_LDS", hash_lds)
    select = [("COUNT(*)", None), ("SUM(r_long)", L_RAW_INT), ("COUNT(*)", L_RAW_INT), ("MIN(r_double)", L_IN_BIG),
              ("AVG(r_double)", L_SORTED), ("SUM(r_int * mix)", L_SORTED)]
    res, _ = run(engine, data, select, keys=("k37", "k50"))
    n, table, info = lanes_of(res)
    assert (n, table) == (3, "hash+lds" if hash_lds == "1" else "hash"), info
    assert info.startswith("jit-hash ") and "+nolds" not in info and "+direct" not in info, info   # no second level
    res.execute_again()   # (a second level would switch modes on the re-execution)
    assert "+nolds" not in res.kernel_info() and "+direct" not in res.kernel_info()
    res.destroy()


def test_selective_main_filter_takes_no_selection_vector(engine, data, one_shape):
    main = ("r_int BETWEEN 70 AND 79", lambda s: (s["r_int"] >= 70) & (s["r_int"] <= 79))
    select = [("COUNT(*)", None), ("SUM(r_long)", None), ("SUM(r_long)", L_IN_SMALL), ("MAX(r_double)", L_SORTED)]
    res, exp = run(engine, data, select, main=main, keys=("k37",))
    assert "select" not in res.kernel_info() and lanes_of(res)[:2] == (2, "lds"), res.kernel_info()
    assert 0 < len(exp) < 37
    res.destroy()


# ------------------------------------------------------------------- inverted-index leaves and the gate traps
@pytest.mark.parametrize("policy", ["always", "never"])
def test_lane_of_one_inverted_leaf_under_scanned_main(engine, data, one_shape, monkeypatch, policy):
    """Gate trap b: the lane is one inverted-index EQ, the main filter reads scanned columns. Docs failing the lane
    still count in COUNT(*) and create their groups."""
    monkeypatch.setenv("PINOT_AMD_INV_POLICY", policy)
    select = [("COUNT(*)", None), ("SUM(r_int)", L_INV_EQ), ("COUNT(*)", L_INV_EQ), ("MAX(r_long)", L_ABSENT)]
    res, exp = run(engine, data, select, keys=("k37",))
    assert len(exp) == 37 and sum(v[0] for v in exp.values()) > 10 * sum(v[2] for v in exp.values()) > 0
    res.destroy()


def test_main_of_inverted_leaves_lane_on_scanned_column(engine, data, one_shape, monkeypatch):
    """Gate trap a: the main filter is made only of inverted-index leaves (it gates the loads), the lanes read scanned
    columns."""
    monkeypatch.setenv("PINOT_AMD_INV_POLICY", "always")
    main = ("inv IN (3, 7, 11) AND dev = 1", lambda s: np.isin(s["inv"], [3, 7, 11]) & (s["dev"] == 1))
    select = [("COUNT(*)", None), ("SUM(r_long)", L_RAW_INT), ("AVG(r_double)", L_RAW_DBL), ("COUNT(*)", L_NEG)]
    res, exp = run(engine, data, select, main=main, keys=("k37",))
    assert exp
    res.destroy()


# ------------------------------------------------------------------------------- wave-uniform fast path
def test_sorted_key_lane_splits_each_wave(engine, data):
    """GROUP BY a sorted column: whole waves share a key (the wave-uniform reductions), the lane takes the odd values
    of r_int inside each wave."""
    select = [("COUNT(*)", None), ("SUM(r_int)", None), ("COUNT(*)", L_ODD), ("SUM(r_long)", L_ODD), ("MIN(r_double)", L_ODD),
              ("MAX(r_double)", L_RAW_DBL), ("AVG(r_double)", L_RAW_DBL), ("SUM(r_int * mix)", L_ODD)]
    res, exp = run(engine, data, select, main=None, keys=("ts",))
    assert len(exp) == 12 and lanes_of(res)[:2] == (2, "lds")
    assert all(0 < v[2] < v[0] for v in exp.values())
    res.destroy()


# ------------------------------------------------------------------------------------------ the skip option
def test_skip_empty_groups(engine, data, one_shape):
    lanes = [("SUM(r_long)", L_INV_EQ), ("COUNT(*)", L_INV_EQ), ("MAX(r_double)", L_RAW_IN)]
    keep, all_groups = run(engine, data, lanes, keys=("k37", "k50"))
    skip, some_groups = run(engine, data, lanes, keys=("k37", "k50"), skip=True)
    assert set(some_groups) < set(all_groups) and skip.num_docs_matched() < keep.num_docs_matched()
    assert some_groups and any(v[1] == 0 for v in some_groups.values())   # (a group kept by the other lane alone)
    # with one unfiltered aggregation the option changes nothing
    mixed = [("COUNT(*)", None)] + lanes
    a, ga = run(engine, data, mixed, keys=("k37", "k50"))
    b, gb = run(engine, data, mixed, keys=("k37", "k50"), skip=True)
    assert ga == gb and a.num_docs_matched() == b.num_docs_matched() == keep.num_docs_matched()
    for r in (keep, skip, a, b):
        r.destroy()


# ------------------------------------------------------------------------------------------ the server table
def test_server_table_orders_by_a_filtered_aggregation(engine, data, one_shape):
    ex = engine.ServerQueryExecutor(server_trim=True)
    arrays, segs = data
    sel = (f"COUNT(*), SUM(r_int) FILTER (WHERE {L_DICT_RANGE[0]}) AS s, AVG(r_int) FILTER (WHERE {L_IN_SMALL[0]})")
    lanes = [None, L_DICT_RANGE[1], L_IN_SMALL[1]]
    for idx, order in ((1, "s DESC"), (2, f"avg(r_int) FILTER (WHERE {L_IN_SMALL[0]}) DESC, k37")):
        q = (f"SET serverReturnFinalResult = true; SELECT k37, {sel} FROM t WHERE {MAIN[0]} GROUP BY k37 "
             f"ORDER BY {order} LIMIT 5")
        exp, _ = ref.reference(parse_sql(q), arrays, MAIN[1], lanes)
        res = ex.execute(q, segs)
        rows = res.rows()
        top = sorted(exp.items(), key=lambda kv: (-kv[1][idx], kv[0]))[:5]   # its final value DESC, ties by key
        assert len(rows) == 5 and [canonical_key(r[:1]) for r in rows] == [k for k, _ in top], (q, rows, top)
        for r, (k, e) in zip(rows, top):
            assert list(r[1:]) == e, (q, r, e)
        assert lanes_of(res)[0] == 2
        res.destroy()


# ---------------------------------------------------------------------------------------------- plan reuse
def test_plan_identity_includes_the_lane_literals(engine, data, one_shape):
    """Two queries that differ only in a lane's literal, back to back with the first result destroyed (its prepared
    plan goes back to the cache): the second must match its own reference."""
    first = L_RAW_INT
    second = ("r_int BETWEEN -300 AND 451", lambda s: (s["r_int"] >= -300) & (s["r_int"] <= 451))
    got = []
    for lane in (first, second, first):
        res, exp = run(engine, data, [("COUNT(*)", None), ("COUNT(*)", lane), ("SUM(r_long)", lane)], keys=("k37",))
        res.execute_again()
        got.append((sum(v[1] for v in exp.values()), sum(r[2] for r in res.rows())))
        res.destroy()
    assert got[0][0] == got[0][1] == got[2][1] and got[1][0] == got[1][1] and got[1][0] > got[0][0]


# ---------------------------------------------------------------------------------------------- refusals
def _refused(engine, q, segs, code, *words, executor=None):
    from pinot_amd._lib import PinotAmdError
    with pytest.raises(PinotAmdError) as e:
        (executor or engine.ServerQueryExecutor()).execute(q, segs)
    msg = str(e.value)
    assert all(w in msg for w in words), msg
    assert code is None or f"failed ({code})" in msg, msg


def test_refusals(engine, data, one_shape):
    _, segs = data
    f = f"FILTER (WHERE {L_RAW_INT[0]})"
    _refused(engine, f"SET numGroupsLimit = 10; SELECT k37, COUNT(*), SUM(r_int) {f} FROM t GROUP BY k37 LIMIT 100", segs, -2,
             "numGroupsLimit")
    trim = engine.ServerQueryExecutor(server_trim=True)
    _refused(engine, f"SET minSegmentGroupTrimSize = 5; SELECT k37, SUM(r_int) {f} AS s FROM t GROUP BY k37 ORDER BY s LIMIT 3",
             segs, -2, "segment-level trim", executor=trim)
    _refused(engine, f"SET sortAggregateLimitThreshold = 2; SELECT k37, SUM(r_int) {f} FROM t GROUP BY k37 ORDER BY k37 LIMIT 3",
             segs, -2, "segment-level safe trim", executor=trim)
    native = engine.ServerQueryExecutor(distinct_count="native")
    _refused(engine, f"SELECT k37, DISTINCTCOUNT(k50) {f} FROM t GROUP BY k37", segs, -2, "DISTINCTCOUNT", executor=native)
    _refused(engine, f"SELECT k37, DISTINCTCOUNT(k50) {f} FROM t GROUP BY k37", segs, None, "DISTINCTCOUNT")   # the mirror path
    many = ", ".join(f"COUNT(*) FILTER (WHERE r_int > {i} AND mix < {i})" for i in range(9))   # 18 leaves
    _refused(engine, f"SELECT {many} FROM t", segs, -2, "16", "predicates")
