"""PERCENTILE, DISTINCTSUM and DISTINCTAVG executed by the library (PINOT_AMD_AGG_PERCENTILE / DISTINCTSUM /
DISTINCTAVG through pinot_amd_query_add_aggregation_param; engine.ServerQueryExecutor(distinct_count="native")): the
value-set query's COUNT rides through the fold, a percentile is a rank selection in each group's cumulative doc
counts (value_count_*_kernel, percentile_select_kernel), the sums are segmented sums of the dictionary's values
(distinct_fold_sum_*_kernel). Every case is compared with the per-doc numpy restatement of value_aggs_ref (gather the
matching docs' values per group, sort, index -- no histogram), rows() (pinot_amd_result_fetch alone) and groups()
(the histograms / sets as CSR) alike, and where cheap with the mirror path."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import value_aggs_ref as ref
from helpers import GOLDEN, SV_FILTER, sv_segment
from pinot_amd import segment as S
from pinot_amd.query import VALUE_SET_FUNCS, canonical_key, final_value, parse_sql

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED, EOVERFLOW = -1, -2, -5
AGG_PERCENTILE, AGG_DISTINCTSUM, AGG_DISTINCTAVG = 8, 9, 10
INT64_MIN = -(1 << 63)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def engine(torch_cuda):
    from pinot_amd import engine as E
    return E


def build(engine, name, cols):
    """cols: column -> (array, type, options). Returns (the per-doc arrays, the device segment)."""
    return {c: v[0] for c, v in cols.items()}, engine.ImmutableSegment(S.build_segment(name, cols))


def is_float_col(arrays, a):
    return a.column != "*" and np.asarray(arrays[0][a.column]).dtype.kind == "f"


def assert_rows(qc, arrays, got, exp, what):
    assert set(got) == set(exp), (what, len(got), len(exp))
    for k, e in exp.items():
        for a, x, y in zip(qc.aggregations, got[k], e):
            assert ref.same(x, y, a.func, is_float_col(arrays, a)), (what, k, a.name, x, y)


def check(engine, q, segs, arrays, flt=None, mirror=False, executor=None):
    """The native result of q against the per-doc restatement: rows() and the finals of groups()'s partials (and the
    mirror path's rows). Queries carry a LIMIT above their group count. Returns the native result."""
    qc = parse_sql(q)
    nk = len(qc.group_by)
    exp = ref.reference_rows(qc, arrays, flt)
    res = (executor or engine.ServerQueryExecutor(distinct_count="native")).execute(q, segs)
    rows = res.rows()
    assert len(rows) == len(exp), (q, len(rows), len(exp))
    assert_rows(qc, arrays, {canonical_key(r[:nk]): list(r[nk:]) for r in rows}, exp, q)
    finals = {canonical_key(k): [final_value(a.func, p, a.param) for a, p in zip(qc.aggregations, parts)]
              for k, parts in res.groups().items()}
    assert_rows(qc, arrays, finals, exp, q + " [groups()]")
    if mirror:
        m = engine.ServerQueryExecutor().execute(q, segs)
        assert_rows(qc, arrays, {canonical_key(r[:nk]): list(r[nk:]) for r in m.rows()}, exp, q + " [mirror]")
        m.destroy()
    return res


# ------------------------------------------------------------------------------ 1: Pinot's own expected values
@pytest.fixture(scope="module")
def sv(engine):
    data = np.load(os.path.join(GOLDEN, "test_data_sv.npz"), allow_pickle=False)
    bufs = sv_segment()
    return {c: data[c] for c in data.files}, [engine.ImmutableSegment(bufs) for _ in range(4)]


def test_pinot_golden_values_native(engine, sv):
    """InterSegmentAggregationSingleValueQueriesTest's testPercentile / testDistinctSum / testDistinctAvg on four
    copies of its segment: no filter, FILTER, GROUP BY column9 ORDER BY v1 DESC, v2 DESC LIMIT 1 (the server table
    orders by the two aggregations) and both."""
    arrays, segs = sv
    with open(os.path.join(GOLDEN, "sv_value_aggs_expected.json")) as f:
        g = json.load(f)
    assert " WHERE " + g["filter_sql"] == SV_FILTER
    ex = engine.ServerQueryExecutor(server_trim=True, distinct_count="native")
    n = 0
    for section in ("percentile", "distinct_sum", "distinct_avg"):
        for query in g[section]["queries"]:
            for sel in query["select"]:
                for case, exp in query["cases"].items():
                    filtered = case.startswith("filter")
                    sql = sel + (SV_FILTER if filtered else "") + (" " + g["group_by_sql"] if case.endswith("group_by") else "")
                    res = ex.execute(sql, segs)
                    assert res.num_docs_matched() == g["num_docs"]["filter" if filtered else "no_filter"]
                    rows = res.rows()
                    assert len(rows) == 1 and list(rows[0][-2:]) == exp, (sql, rows)
                    assert res.kernel_info().count("+distinct(") == 2, res.kernel_info()
                    res.destroy()
                    n += 1
    assert n == 32


# ------------------------------------------------------------------------------------- 2: the two-segment fixture
def _two_segment_columns(rng, n):
    """The columns of helpers.random_segment (dictionary INT d0 / d1 with values != dictIds, raw INT / LONG / DOUBLE)
    plus a sorted column, a dictionary LONG and a dictionary DOUBLE; the dictionaries differ per segment."""
    return {
        "d0": ((rng.integers(0, 1000, n) * 7 + 3).astype(np.int32), S.INT, {}),
        "d1": ((rng.integers(0, 37, n) * 7 + 3).astype(np.int32), S.INT, {}),
        "r_int": (rng.integers(-1000000, 1000000, n).astype(np.int32), S.INT, {"dictionary": False}),
        "r_long": (rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64), S.LONG, {"dictionary": False}),
        # (positive: a sum that cancels to nearly nothing has no meaningful relative error)
        "r_double": (np.round(rng.gamma(2.0, 500.0, n), 1), S.DOUBLE, {"dictionary": False}),
        "ts": (np.sort(rng.integers(0, 50, n)).astype(np.int32), S.INT, {}),
        "dl": ((rng.integers(0, 300, n).astype(np.int64) << 33) - 11, S.LONG, {}),
        "fd": ((rng.integers(-40, 40, n) * 0.375).astype(np.float64), S.DOUBLE, {}),
    }


@pytest.fixture(scope="module")
def two_segments(engine):
    rng = np.random.default_rng(91)
    built = [build(engine, f"va{i}", _two_segment_columns(rng, n)) for i, n in enumerate([20_000, 7_001])]
    return [b[0] for b in built], [b[1] for b in built]


TWO_SEGMENT_QUERIES = [
    ("SELECT PERCENTILE50(d0), DISTINCTSUM(d0), DISTINCTAVG(d0), PERCENTILE(ts, 99.9), DISTINCTSUM(ts) FROM t "
     "WHERE d1 < 100", lambda s: s["d1"] < 100),
    ("SELECT PERCENTILE90(r_int), DISTINCTAVG(r_int), PERCENTILE0(r_long), PERCENTILE100(r_long), DISTINCTSUM(r_long), "
     "PERCENTILE(r_double, 37.5), DISTINCTSUM(r_double), DISTINCTAVG(r_double), COUNT(*) FROM t", None),
    ("SELECT d1, PERCENTILE95(r_int), DISTINCTSUM(r_int), SUM(r_long), COUNT(*) FROM t WHERE r_int > 0 GROUP BY d1 "
     "LIMIT 100", lambda s: s["r_int"] > 0),
    ("SELECT d1, PERCENTILE50(r_double), DISTINCTAVG(r_double), DISTINCTSUM(fd), PERCENTILE(fd, 12.5) FROM t "
     "GROUP BY d1 LIMIT 100", None),
    ("SELECT ts, PERCENTILE50(dl), DISTINCTSUM(dl), DISTINCTAVG(dl), PERCENTILE99(d0) FROM t WHERE d0 > 500 "
     "GROUP BY ts LIMIT 100", lambda s: s["d0"] > 500),
    ("SELECT d1, fd, PERCENTILE50(ts), DISTINCTSUM(r_long) FROM t GROUP BY d1, fd LIMIT 100000", None),
]


@pytest.mark.parametrize("qi", range(len(TWO_SEGMENT_QUERIES)))
def test_two_segments_vs_restatement_and_mirror(engine, two_segments, qi):
    arrays, segs = two_segments
    q, flt = TWO_SEGMENT_QUERIES[qi]
    res = check(engine, q, segs, arrays, flt, mirror=True)
    assert res.kernel_info().count("+distinct(") == len({a.column for a in res.qc.aggregations
                                                         if a.func in VALUE_SET_FUNCS}), res.kernel_info()
    res.destroy()


def test_one_value_set_query_per_column(engine, two_segments):
    """Several percentiles, DISTINCTCOUNT, DISTINCTSUM and DISTINCTAVG of one column share one value-set query; of a
    GROUP BY column they run none (each is the key's value)."""
    arrays, segs = two_segments
    q = ("SELECT d1, PERCENTILE50(d0), PERCENTILE99(d0), PERCENTILE(d0, 0.1), DISTINCTCOUNT(d0), DISTINCTSUM(d0), "
         "DISTINCTAVG(d0), COUNT(*), PERCENTILE100(d0) FROM t WHERE r_int > -500000 GROUP BY d1 LIMIT 100")
    res = check(engine, q, segs, arrays, lambda s: s["r_int"] > -500000, mirror=True)
    info = res.kernel_info()
    assert info.count("+distinct(") == 1 and " +distinct(d0:" in info, info
    res.destroy()
    q = "SELECT d1, PERCENTILE50(d1), DISTINCTSUM(d1), DISTINCTAVG(d1), DISTINCTCOUNT(d1), COUNT(*) FROM t GROUP BY d1 LIMIT 100"
    res = check(engine, q, segs, arrays, mirror=True)
    assert "+distinct(" not in res.kernel_info()
    assert all(r[1] == r[2] == r[3] == float(r[0]) and r[4] == 1 for r in res.rows())
    res.destroy()


# ----------------------------------------------------------------------------------------------- 3: fold shapes
def _shape(engine, name, g, c, extra=None):
    cols = {"g": (np.asarray(g, dtype=np.int32), S.INT, {}), "c": (np.asarray(c, dtype=np.int32), S.INT, {}),
            "m": ((np.arange(len(g)) % 10).astype(np.int32), S.INT, {"dictionary": False})}
    cols.update(extra or {})
    arrays, seg = build(engine, name, cols)
    return [arrays], [seg]


SHAPE_AGGS = "PERCENTILE0(c), PERCENTILE50(c), PERCENTILE(c, 99.9), PERCENTILE100(c), DISTINCTSUM(c), DISTINCTAVG(c), COUNT(*)"


def test_fold_one_group_many_values(engine):
    """One group of 5003 distinct values, one of them held by ~70 000 docs: cumulative counts are far from row
    indexes, the group's slice spans many tiles of the sum and the rank search runs over the whole slice."""
    rng = np.random.default_rng(3)
    c = np.concatenate([np.arange(5003) * 3, np.full(70_001, 2500 * 3), rng.integers(0, 5003, 4_000) * 3])
    g = np.full(len(c), 7)
    g[-40:] = 9
    g[-3:] = 2
    arrays, segs = _shape(engine, "vone", g, c)
    res = check(engine, f"SELECT g, {SHAPE_AGGS} FROM t GROUP BY g LIMIT 10", segs, arrays)
    row = {r[0]: r for r in res.rows()}[7]
    assert row[2] == 2500 * 3.0 and row[4] == 5002 * 3.0   # the median sits in the long run
    res.destroy()
    res = check(engine, f"SELECT {SHAPE_AGGS} FROM t", segs, arrays)   # aggregation-only: one group holds every row
    res.destroy()


def test_fold_many_groups_one_value(engine):
    """5001 groups of exactly one value each: every slice one row, every percentile that row."""
    ng = 5001
    g = np.repeat(np.arange(ng), 3)
    c = np.repeat((np.arange(ng) * 7919) % 6007, 3)
    arrays, segs = _shape(engine, "vmany", g, c)
    res = check(engine, f"SELECT g, {SHAPE_AGGS} FROM t GROUP BY g LIMIT 100000", segs, arrays)
    assert all(r[1] == r[2] == r[3] == r[4] == r[5] == r[6] and r[7] == 3 for r in res.rows())
    res.destroy()


def test_fold_scan_spans_many_blocks(engine):
    """~86 000 (group, value) rows over 397 groups: the count scan runs over many blocks with carried totals, the
    sums' tiles cut most groups, and the row count is no multiple of the tile."""
    rng = np.random.default_rng(8)
    n = 150_000
    g = rng.integers(0, 397, n)
    c = rng.integers(0, 307, n) * 5 - 600
    pairs = len(set(zip(g.tolist(), c.tolist())))
    assert pairs > 80_000 and pairs % 256 != 0
    arrays, segs = _shape(engine, "vscan", g, c)
    check(engine, f"SELECT g, {SHAPE_AGGS}, SUM(m) FROM t GROUP BY g LIMIT 1000", segs, arrays).destroy()


def test_fold_cardinality_one_and_no_match(engine):
    """A column of cardinality 1; a filter matching nothing: no groups with GROUP BY, and without it the one group
    with PERCENTILE = -inf (DEFAULT_FINAL_RESULT), DISTINCTSUM = 0.0, DISTINCTAVG = NaN."""
    rng = np.random.default_rng(13)
    n = 7_001
    arrays, segs = _shape(engine, "vcard1", rng.integers(0, 50, n), np.full(n, 42))
    res = check(engine, f"SELECT g, {SHAPE_AGGS} FROM t GROUP BY g LIMIT 100", segs, arrays)
    assert all(r[1:7] == (42.0,) * 6 for r in res.rows())
    res.destroy()
    check(engine, f"SELECT {SHAPE_AGGS} FROM t", segs, arrays).destroy()
    res = check(engine, f"SELECT g, {SHAPE_AGGS} FROM t WHERE m > 100 GROUP BY g LIMIT 100", segs, arrays, lambda s: s["m"] > 100)
    assert res.rows() == [] and res.groups() == {}
    res.destroy()
    res = check(engine, "SELECT PERCENTILE50(c), DISTINCTSUM(c), DISTINCTAVG(c), PERCENTILE100(g) FROM t WHERE m > 100", segs,
                arrays, lambda s: s["m"] > 100)
    (row,) = res.rows()
    assert row[0] == row[3] == float("-inf") and row[1] == 0.0 and math.copysign(1, row[1]) == 1 and math.isnan(row[2])
    assert res.groups()[()][0] == {} and res.groups()[()][1] == frozenset()
    vals, vals_i = res.fetch_arrays()[2:4]
    assert vals_i[:4].tolist() == [INT64_MIN, 0, INT64_MIN, INT64_MIN] and vals[1] == 0.0
    res.destroy()


# ------------------------------------------------------------------------ 4: NaN and signed zeros, beyond 2^53
def test_double_nan_and_signed_zero(engine):
    """A raw DOUBLE column with NaN, -0.0 and 0.0: p = 0, p = 100 (NaN, greatest) and ranks that fall on the last
    -0.0 and on the first 0.0. docs: 100 x -2.5, 300 x -0.0, 200 x 0.0, 250 x 1.25, 150 x NaN (n = 1000)."""
    x = np.concatenate([np.full(100, -2.5), np.full(300, -0.0), np.full(200, 0.0), np.full(250, 1.25), np.full(150, np.nan)])
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(x))
    g = (np.arange(len(x)) % 3).astype(np.int32)
    arrays, seg = build(engine, "vnan", {"x": (x[perm], S.DOUBLE, {"dictionary": False}),
                                         "f": (x[perm].astype(np.float32), S.FLOAT, {"dictionary": False}),
                                         "g": (g, S.INT, {})})
    q = ("SELECT PERCENTILE0(x), PERCENTILE(x, 39.9), PERCENTILE40(x), PERCENTILE(x, 59.9), PERCENTILE60(x), PERCENTILE(x, 84.9), "
         "PERCENTILE85(x), PERCENTILE100(x), DISTINCTSUM(x), DISTINCTAVG(x), DISTINCTCOUNT(x) FROM t")
    res = check(engine, q, [seg], [arrays], mirror=True)
    (row,) = res.rows()
    assert row[0] == -2.5 and [math.copysign(1, v) for v in row[1:5]] == [-1, 1, 1, 1] and row[1:4] == (0.0, 0.0, 0.0)
    assert row[4] == row[5] == 1.25 and math.isnan(row[6]) and math.isnan(row[7]) and math.isnan(row[8]) and row[10] == 5
    res.destroy()
    q = ("SELECT g, PERCENTILE0(f), PERCENTILE50(f), PERCENTILE100(f), PERCENTILE50(x), DISTINCTSUM(f) FROM t WHERE g < 2 "
         "GROUP BY g LIMIT 10")
    check(engine, q, [seg], [arrays], lambda s: s["g"] < 2, mirror=True).destroy()
    q = "SELECT x, PERCENTILE50(g), DISTINCTSUM(g), PERCENTILE100(x) FROM t GROUP BY x LIMIT 10"
    res = check(engine, q, [seg], [arrays])   # FLOAT keys -0.0 / 0.0 / NaN; PERCENTILE of the GROUP BY column
    assert len(res.rows()) == 5
    res.destroy()


def test_long_above_2_53(engine):
    """Epoch nanoseconds (LONG beyond 2^53, adjacent values one double apart or less): the selected value is exact
    in h_values_i64 and rounded once in h_values; the sums stay below 2^53 for a second, small column only."""
    rng = np.random.default_rng(29)
    n = 9_001
    base = 1_760_000_000_000_000_000
    t = base + rng.integers(0, 4_000, n).astype(np.int64)
    small = rng.integers(-(1 << 30), 1 << 30, n).astype(np.int64)
    g = rng.integers(0, 11, n).astype(np.int32)
    arrays, seg = build(engine, "vnanos", {"t": (t, S.LONG, {"dictionary": False}), "small": (small, S.LONG, {}),
                                           "g": (g, S.INT, {})})
    q = "SELECT g, PERCENTILE50(t), PERCENTILE(t, 99.9), PERCENTILE0(t), DISTINCTSUM(small), DISTINCTAVG(small) " \
        "FROM t GROUP BY g LIMIT 100"
    check(engine, q, [seg], [arrays], mirror=True).destroy()
    # the same with DISTINCTSUM(t), whose sums are far above 2^53 (not compared for equality)
    res = engine.ServerQueryExecutor(distinct_count="native").execute(
        q.replace(" FROM t", ", DISTINCTSUM(t) FROM t"), [seg])
    got, keys, vals, vals_i, _ = res.fetch_arrays()
    na = 6
    assert got.value == 11
    for i in range(got.value):
        grp = np.sort(t[g == keys[i]])
        small_d = np.unique(small[g == keys[i]])
        for j, p in enumerate((50.0, 99.9, 0.0)):
            exact = int(grp[int(float(len(grp)) * p / 100.0)])
            assert vals_i[i * na + j] == exact and vals[i * na + j] == float(exact)
            assert exact > (1 << 53)
        assert vals_i[i * na + 3] == int(small_d.sum()) and vals[i * na + 3] == float(int(small_d.sum()))
        assert vals_i[i * na + 4] == INT64_MIN
        # hundreds of distinct values near 1.76e18: the exact sum is beyond int64, so it is the double sum alone
        exact_t = sum(int(v) for v in np.unique(grp))
        assert exact_t > (1 << 63) and vals_i[i * na + 5] == INT64_MIN
        assert abs(vals[i * na + 5] - float(exact_t)) <= 1e-12 * float(exact_t)
    res.destroy()
    # a sum of LONGs that fits int64 but not 2^53: the integer leg is exact, the double is it rounded once
    few = np.array([base, base + 1, base + 3, 5], dtype=np.int64)
    arrays, seg = build(engine, "vfew", {"t": (few[rng.integers(0, 4, 3_001)], S.LONG, {})})
    res = engine.ServerQueryExecutor(distinct_count="native").execute("SELECT DISTINCTSUM(t), DISTINCTAVG(t) FROM t", [seg])
    _, _, vals, vals_i, _ = res.fetch_arrays()
    exact = int(sum(int(v) for v in np.unique(arrays["t"])))
    assert vals_i[0] == exact and vals[0] == float(exact) and vals[1] == float(exact) / len(np.unique(arrays["t"]))
    res.destroy()


# ------------------------------------------------------------------------------------------- 5: plan coverage
def _parts(res):
    info = res.kernel_info()
    return info, info.split(" +distinct(")[1:]


def test_child_plans_dense_partitioned_hash(engine, two_segments):
    """The value-set query as a dense plan (50 x 40 keys), as a partitioned plan (37 x ~27k raw values) and as a
    hash plan (a key space above 2^28) under a dense base."""
    rng = np.random.default_rng(31)
    n = 7_001
    arrays, segs = _shape(engine, "vdense", rng.integers(0, 50, n), rng.integers(0, 40, n) * 5)
    res = check(engine, f"SELECT g, {SHAPE_AGGS} FROM t GROUP BY g LIMIT 50", segs, arrays)
    info, parts = _parts(res)
    assert len(parts) == 1 and parts[0].startswith("c:jit") and "partitioned" not in info and "hash" not in info, info
    res.destroy()
    arrays, segs = two_segments
    res = check(engine, "SELECT d1, PERCENTILE50(r_int), DISTINCTSUM(r_int), COUNT(*) FROM t GROUP BY d1 LIMIT 50", segs, arrays)
    info, parts = _parts(res)
    assert len(parts) == 1 and parts[0].startswith("r_int:jit-partitioned"), info
    assert "partitioned" not in info.split(" +distinct(")[0], info
    res.destroy()
    rng = np.random.default_rng(77)
    n = 200_000
    arrays, seg = build(engine, "vhash", {"g": (rng.integers(0, 3200, n).astype(np.int32), S.INT, {}),
                                          "k": (rng.integers(0, 150_000, n).astype(np.int64) * 3 - 10**12, S.LONG,
                                                {"dictionary": False})})
    res = check(engine, "SELECT g, PERCENTILE50(k), PERCENTILE100(k), DISTINCTSUM(k), DISTINCTAVG(k) FROM t GROUP BY g LIMIT 5000",
                [seg], [arrays])
    info, parts = _parts(res)
    assert len(parts) == 1 and parts[0].startswith("k:jit-hash") and "hash" not in info.split(" +distinct(")[0], info
    res.destroy()


def test_forced_hash_base(engine, two_segments, monkeypatch):
    monkeypatch.setenv("PINOT_AMD_GROUP_PLAN", "hash")
    arrays, segs = two_segments
    q = ("SELECT d1, d0, PERCENTILE50(r_int), DISTINCTSUM(r_int), DISTINCTAVG(fd), SUM(r_long) FROM t WHERE r_int > 0 "
         "GROUP BY d1, d0 LIMIT 100000")
    res = check(engine, q, segs, arrays, lambda s: s["r_int"] > 0)
    info, parts = _parts(res)
    assert info.startswith("jit-hash") and parts[0].startswith("r_int:jit-hash"), info
    res.destroy()


# ------------------------------------------------------------------------------------------- 6: numGroupsLimit
def test_num_groups_limit(engine, two_segments):
    """SET numGroupsLimit = 40 over two segments with different dictionaries, as for DISTINCTCOUNT: the groups are
    the ones the base query admitted, each with its values over every matching doc of the batch, and the flag is
    set."""
    arrays, segs = two_segments
    q = ("SET numGroupsLimit = 40; SELECT d0, PERCENTILE50(d1), DISTINCTSUM(d1), DISTINCTAVG(d1), PERCENTILE100(d1) FROM t "
         "GROUP BY d0 LIMIT 100000")
    qc = parse_sql(q)
    full = ref.reference_rows(qc, arrays)
    res = engine.ServerQueryExecutor(distinct_count="native").execute(q, segs)
    assert res.num_groups_limit_reached()
    got = {canonical_key(r[:1]): list(r[1:]) for r in res.rows()}
    assert 40 <= len(got) <= 80 < len(full)
    assert_rows(qc, arrays, got, {k: full[k] for k in got}, q)
    m = engine.ServerQueryExecutor().execute(q, segs)
    assert {canonical_key(r[:1]): list(r[1:]) for r in m.rows()} == got
    m.destroy()
    res.destroy()


# -------------------------------------------------------------------- 7: execute_again and the plan cache
def test_execute_again_and_percentile_is_no_plan_identity(engine, two_segments):
    arrays, segs = two_segments
    ex = engine.ServerQueryExecutor(distinct_count="native")
    q50 = "SELECT d1, PERCENTILE50(r_int), DISTINCTSUM(r_double), COUNT(*) FROM t WHERE d0 < 5000 GROUP BY d1 LIMIT 100"
    res = check(engine, q50, segs, arrays, lambda s: s["d0"] < 5000)
    before = [a.tobytes() for a in res.fetch_arrays()[1:4]]
    hists = res.groups()
    ms, by, info = res.last_kernel_ms(), res.algorithmic_bytes(), res.kernel_info()
    res.execute_again()
    assert [a.tobytes() for a in res.fetch_arrays()[1:4]] == before    # the sums too: a fixed reduction order
    assert res.groups() == hists and res.last_kernel_ms() > 0 and res.algorithmic_bytes() == by
    assert ms > 0
    res.destroy()
    # the same plans (cached under the base's and the value-set query's identities) with another percentile
    q90 = q50.replace("PERCENTILE50", "PERCENTILE90")
    r90 = check(engine, q90, segs, arrays, lambda s: s["d0"] < 5000)
    assert r90.kernel_info() == info
    r50 = ex.execute(q50, segs)
    p50 = {r[0]: r[1] for r in r50.rows()}
    p90 = {r[0]: r[1] for r in r90.rows()}
    assert all(p90[k] > p50[k] for k in p50)
    r50.destroy()
    r90.destroy()


# --------------------------------------------------------------------------------- 8: fetch_value_counts
def _raw_counts(L, h, agg, cap, ngroups, with_values=True):
    total = C.c_int64(-1)
    off = np.full(ngroups + 1, -1, dtype=np.int64)
    vals = np.full(max(cap, 1), -1, dtype=np.int64)
    cnts = np.full(max(cap, 1), -1, dtype=np.int64)
    p64 = C.POINTER(C.c_int64)
    rc = L.pinot_amd_result_fetch_value_counts(h, agg, cap, off.ctypes.data_as(p64),
                                               vals.ctypes.data_as(p64) if with_values else None,
                                               cnts.ctypes.data_as(p64) if with_values else None, C.byref(total))
    return rc, total.value, off, vals, cnts


def _numpy_hist(values):
    u, c = np.unique(values, return_counts=True)
    return u.tolist(), c.tolist()


def test_fetch_value_counts(engine):
    rng = np.random.default_rng(17)
    n = 7_001
    cols = {"g": (rng.integers(0, 23, n).astype(np.int32), S.INT, {}),
            "r": (rng.integers(0, 300, n).astype(np.int32) * 3 - 100, S.INT, {"dictionary": False}),
            "s": (np.array([f"v{i:02d}" for i in range(30)], dtype=object)[rng.integers(0, 30, n)], S.STRING, {})}
    arrays, seg = build(engine, "vcsr", cols)
    L = engine.lib()
    # library aggregations: 0 PERCENTILE50(r), 1 SUM(r), 2 DISTINCTSUM(r), 3 DISTINCTCOUNT(g) (the GROUP BY column)
    q = "SELECT g, PERCENTILE50(r), SUM(r), DISTINCTSUM(r), DISTINCTCOUNT(g) FROM t WHERE r < 700 GROUP BY g LIMIT 100"
    m = arrays["r"] < 700
    res = check(engine, q, [seg], [arrays], lambda s: s["r"] < 700, mirror=True)
    h, ng = res._h, 23
    rc, total, off, _, _ = _raw_counts(L, h, 0, 0, ng, with_values=False)       # sizes only
    assert rc == 0 and off[0] == 0 and off[-1] == total > ng
    rc, t2, off, vals, cnts = _raw_counts(L, h, 0, total, ng)
    assert rc == 0 and t2 == total
    keys = sorted(np.unique(arrays["g"][m]).tolist())
    for i, k in enumerate(keys):   # ascending values (merged-dictionary order), each with its matching docs
        u, c = _numpy_hist(arrays["r"][m & (arrays["g"] == k)])
        assert vals[off[i]:off[i + 1]].tolist() == u and cnts[off[i]:off[i + 1]].tolist() == c
    rc, t3, _, _, _ = _raw_counts(L, h, 0, total - 1, ng)
    assert rc == EOVERFLOW and t3 == total
    assert _raw_counts(L, h, 1, total, ng)[0] == EINVAL                            # SUM(r) has no value set
    # DISTINCTSUM shares the PERCENTILE's value-set query: the same CSR, from both entry points
    rc, t4, off2, vals2, cnts2 = _raw_counts(L, h, 2, total, ng)
    assert rc == 0 and t4 == total and off2.tolist() == off.tolist() and vals2.tolist() == vals.tolist() \
        and cnts2.tolist() == cnts.tolist()
    assert res.distinct_sets(2, "INT", ng) == [frozenset(vals[off[i]:off[i + 1]].tolist()) for i in range(ng)]
    assert res.distinct_sets(0, "INT", ng) == res.distinct_sets(2, "INT", ng)
    # of a GROUP BY column: the key's value with the group's doc count
    rc, t5, off5, vals5, cnts5 = _raw_counts(L, h, 3, ng, ng)
    assert rc == 0 and t5 == ng and vals5[:ng].tolist() == keys
    assert cnts5[:ng].tolist() == [int((m & (arrays["g"] == k)).sum()) for k in keys]
    # the calls that stay refused for value sets
    nsl, nks = C.c_int32(), C.c_int64()
    assert L.pinot_amd_result_accumulators(h, C.byref(nsl), C.byref(nks), None, None) == EUNSUPPORTED
    kw, na, ngr = C.c_int32(), C.c_int32(), C.c_int64()
    assert L.pinot_amd_result_export_groups(h, None, None, 0, C.byref(kw), C.byref(na), C.byref(ngr), None) == EUNSUPPORTED
    assert L.pinot_amd_result_merge_groups(h, None, None, 0, None) == EUNSUPPORTED
    pairs = np.zeros(ng * 4 * 2, dtype=np.float64)
    got = C.c_int64()
    assert L.pinot_amd_result_fetch_intermediate(h, ng, pairs.ctypes.data_as(C.POINTER(C.c_double)), C.byref(got)) == 0
    pr = pairs.reshape(ng, 4, 2)
    rows = sorted(res.rows())
    assert pr[:, 0, 0].tolist() == [r[1] for r in rows] and pr[:, 2, 0].tolist() == [r[3] for r in rows]
    assert not pr[:, 0, 1].any() and not pr[:, 2, 1].any()                           # (final value, 0)
    res.destroy()
    # without a PERCENTILE the fold carries no doc counts until fetch_value_counts asks: DISTINCTCOUNT / DISTINCTAVG
    q = "SELECT g, DISTINCTCOUNT(r), DISTINCTAVG(r) FROM t WHERE r < 700 GROUP BY g LIMIT 100"
    res = check(engine, q, [seg], [arrays], lambda s: s["r"] < 700)
    rows_before = res.rows()
    for agg in (0, 1):
        rc, t6, off6, vals6, cnts6 = _raw_counts(L, res._h, agg, total, ng)
        assert rc == 0 and t6 == total and off6.tolist() == off.tolist() and vals6.tolist() == vals.tolist() \
            and cnts6.tolist() == cnts.tolist()
    assert res.rows() == rows_before
    res.execute_again()
    assert _raw_counts(L, res._h, 0, total, ng)[4].tolist() == cnts.tolist() and res.rows() == rows_before
    res.destroy()


def test_fetch_value_counts_after_server_table(engine):
    """ORDER BY a percentile with a server table keeping 10 of 23 groups: the CSR follows the kept groups in the
    table's order."""
    rng = np.random.default_rng(19)
    n = 9_001
    g = rng.integers(0, 23, n).astype(np.int32)
    r = (rng.integers(0, 200, n) + g * 7).astype(np.int64)
    arrays, seg = build(engine, "vsrv", {"g": (g, S.INT, {}), "r": (r, S.LONG, {})})
    q = ("SET minServerGroupTrimSize = 3; SELECT g, PERCENTILE(r, 62.5), DISTINCTAVG(r), COUNT(*) FROM t GROUP BY g "
         "ORDER BY PERCENTILE(r, 62.5) DESC, DISTINCTAVG(r) LIMIT 2")
    qc = parse_sql(q)
    full = ref.reference_rows(qc, [arrays])
    order = sorted(full, key=lambda k: (-full[k][0], full[k][1], k))[:10]             # max(5 * LIMIT, 3) groups
    for plan in ("native", "mirror"):
        res = engine.ServerQueryExecutor(server_trim=True, distinct_count=plan).execute(q, [seg])
        got = res.groups()
        assert [canonical_key(k) for k in got] == order, plan
        for k, parts in got.items():
            u, c = _numpy_hist(r[g == k[0]])
            assert parts[0] == dict(zip(u, c)) and parts[1] == frozenset(u) and parts[2] == sum(c), (plan, k)
        assert [canonical_key(x[:1]) for x in res.rows()] == order[:2]
        assert [list(x[1:]) for x in res.rows()] == [full[k] for k in order[:2]]
        res.destroy()


# -------------------------------------------------------------------------------------------- 9: refusals
def test_refusals(engine, two_segments):
    arrays, segs = two_segments
    rng = np.random.default_rng(23)
    n = 3_001
    _, sseg = build(engine, "vstr", {"g": (rng.integers(0, 5, n).astype(np.int32), S.INT, {}),
                                     "s": (np.array(["a", "b", "c"], dtype=object)[rng.integers(0, 3, n)], S.STRING, {})})
    ex = engine.ServerQueryExecutor(distinct_count="native")
    for fn in ("PERCENTILE50(s)", "DISTINCTSUM(s)", "DISTINCTAVG(s)"):
        with pytest.raises(engine._lib.PinotAmdError, match="STRING"):
            ex.execute(f"SELECT g, {fn} FROM t GROUP BY g", [sseg])
    L = engine.lib()
    qh = C.c_void_p()
    assert L.pinot_amd_query_create(C.byref(qh)) == 0
    try:
        idx = C.c_int32()
        assert L.pinot_amd_query_add_aggregation_param(qh, AGG_PERCENTILE, b"s", 50.0, C.byref(idx)) == 0
        arr = (C.c_void_p * 1)(sseg.handle.value)
        rh = C.c_void_p()
        assert L.pinot_amd_execute(qh, arr, 1, None, C.byref(rh)) == EINVAL            # the STRING column
        for t in (AGG_PERCENTILE, AGG_DISTINCTSUM, AGG_DISTINCTAVG):
            assert L.pinot_amd_query_add_aggregation_expr(qh, t, 1, b"g", b"g", C.byref(idx)) == EUNSUPPORTED
    finally:
        L.pinot_amd_query_destroy(qh)
    with pytest.raises(ValueError, match="one column"):
        ex.execute("SELECT PERCENTILE50(d0 * d1) FROM t", segs)
    exs = engine.ServerQueryExecutor(server_trim=True, distinct_count="native")
    with pytest.raises(engine._lib.PinotAmdError, match="segment-level"):
        exs.execute("SET sortAggregateLimitThreshold = 5; SELECT d1, PERCENTILE50(d0) FROM t GROUP BY d1 ORDER BY d1 LIMIT 8",
                    segs)
    with pytest.raises(engine._lib.PinotAmdError, match="segment-level"):
        exs.execute("SET minSegmentGroupTrimSize = 10; SELECT d1, DISTINCTSUM(d0) FROM t GROUP BY d1 "
                    "ORDER BY DISTINCTSUM(d0) LIMIT 2", segs)
    with pytest.raises(engine._lib.PinotAmdError, match="mirror"):
        ex.execute("SELECT d1, DISTINCTAVG(d0) FROM t GROUP BY d1", segs, key_space={"d1": [3, 10]})
    res = ex.execute("SELECT d1, PERCENTILE50(d0) FROM t GROUP BY d1 LIMIT 100", segs)
    with pytest.raises(engine._lib.PinotAmdError):
        res.export_groups()
    res.destroy()
