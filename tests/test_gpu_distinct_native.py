"""DISTINCTCOUNT executed by the library (PINOT_AMD_AGG_DISTINCTCOUNT; engine.ServerQueryExecutor(distinct_count=
"native")): the base query and one (group, value) query per DISTINCTCOUNT column run inside pinot_amd_execute and
are folded into per-group value sets on the device (distinct_fold_count_kernel / distinct_fold_fill_kernel).
Every case compares groups() -- the sets, read as CSR through pinot_amd_result_fetch_distinct_values -- with the
CPU oracle's per-doc restatement (oracle._distinct_count), and rows() -- the counts, read from pinot_amd_result_fetch
alone -- with the sets' sizes."""
import ctypes as C

import numpy as np
import pytest

import oracle
from helpers import random_segment
from oracle_reduce import server_table
from pinot_amd import segment as S
from pinot_amd.query import canonical_key, parse_sql

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED, EOVERFLOW = -1, -2, -5
AGG_DISTINCTCOUNT = 7


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def engine(torch_cuda):
    from pinot_amd import engine as E
    return E


@pytest.fixture(scope="module")
def two_segments(engine):
    """The segments of test_gpu_parity.test_distinct_count_vs_oracle: different dictionaries per segment."""
    rng = np.random.default_rng(91)
    bufs = [random_segment(rng, n, name=f"dn{i}") for i, n in enumerate([20_000, 7_001])]
    return bufs, [engine.ImmutableSegment(b) for b in bufs]


def canon(groups):
    return {canonical_key(k): v for k, v in groups.items()}


def check_native(engine, q, segs, bufs, mirror=False):
    """Native result of q against the oracle: matched docs, groups() (keys, sets, other partials), and the counts
    of rows() against the sizes of the oracle's sets. Returns the native result."""
    res = engine.ServerQueryExecutor(distinct_count="native").execute(q, segs)
    nm, og = oracle.execute(q, bufs)
    assert res.num_docs_matched() == nm, q
    got = res.groups()
    assert canon(got) == canon(og), q
    qc = res.qc
    nk = len(qc.group_by)
    exp = canon(og)
    rows = res.rows()
    assert len(rows) == min(len(og), qc.limit), q
    for row in rows:
        parts = exp[canonical_key(row[:nk])]
        for i, a in enumerate(qc.aggregations):
            if a.func == "DISTINCTCOUNT":
                assert row[nk + i] == len(parts[i]), (q, row)
    if mirror:
        m = engine.ServerQueryExecutor().execute(q, segs)
        assert canon(m.groups()) == canon(got), q
        m.destroy()
    return res


def distinct_part(res):
    info = res.kernel_info()
    return info, info.split(" +distinct(")[1:]


# ----------------------------------------------------------------------------------------------- 1: the ABI
def test_abi_accepts_distinctcount(engine):
    L = engine.lib()
    qh = C.c_void_p()
    assert L.pinot_amd_query_create(C.byref(qh)) == 0
    try:
        idx = C.c_int32(-1)
        assert L.pinot_amd_query_add_aggregation(qh, AGG_DISTINCTCOUNT, b"d0", C.byref(idx)) == 0
        assert idx.value == 0
        assert L.pinot_amd_query_add_aggregation(qh, AGG_DISTINCTCOUNT, b"*", C.byref(idx)) == EINVAL
        assert L.pinot_amd_query_add_aggregation(qh, AGG_DISTINCTCOUNT, None, C.byref(idx)) == EINVAL
        assert L.pinot_amd_query_add_aggregation(qh, AGG_DISTINCTCOUNT + 1, b"d0", C.byref(idx)) == EINVAL
        assert L.pinot_amd_query_add_aggregation_expr(qh, AGG_DISTINCTCOUNT, 1, b"d0", b"d1",
                                                      C.byref(idx)) == EUNSUPPORTED
    finally:
        L.pinot_amd_query_destroy(qh)


# ------------------------------------------------------------- 2: the mirror path's queries, in native mode
@pytest.mark.parametrize("q", ["SELECT DISTINCTCOUNT(d0), DISTINCTCOUNT(r_int) FROM t WHERE d1 < 100",
                               "SELECT d1, DISTINCTCOUNT(d0), SUM(r_long), COUNT(*) FROM t WHERE r_int > 0 GROUP BY d1",
                               "SELECT d1, DISTINCTCOUNT(r_int) FROM t GROUP BY d1"])
def test_native_vs_oracle_and_mirror(engine, two_segments, q):
    bufs, segs = two_segments
    res = check_native(engine, q, segs, bufs, mirror=True)
    assert res.kernel_info().count("+distinct(") == len({a.column for a in res.qc.aggregations
                                                         if a.func == "DISTINCTCOUNT"})
    res.destroy()


def test_native_nan_and_signed_zero(engine):
    """The segment and queries of test_gpu_parity.test_distinct_count_nan_and_signed_zero: every NaN one value,
    -0.0 != 0.0, as a group key and as a counted value."""
    rng = np.random.default_rng(5)
    n = 12_007
    g = (rng.integers(-2, 3, n) * 0.5).astype(np.float64)
    g[::7] = -0.0
    g[::11] = np.nan
    x = (rng.integers(-3, 4, n) * 0.25).astype(np.float32)
    x[::5] = -0.0
    x[::13] = np.nan
    bufs = S.build_segment("dnnan", {"g": (g, S.DOUBLE, {"dictionary": False}),
                                     "x": (x, S.FLOAT, {"dictionary": False}),
                                     "m": (rng.integers(0, 10, n).astype(np.int32), S.INT, {})})
    seg = engine.ImmutableSegment(bufs)
    for q in ["SELECT DISTINCTCOUNT(x), DISTINCTCOUNT(g) FROM t",
              "SELECT g, DISTINCTCOUNT(x), COUNT(*) FROM t GROUP BY g",
              "SELECT m, DISTINCTCOUNT(g) FROM t WHERE m < 7 GROUP BY m"]:
        check_native(engine, q, [seg], [bufs], mirror=True).destroy()
    res = engine.ServerQueryExecutor(distinct_count="native").execute(
        "SELECT DISTINCTCOUNT(x), DISTINCTCOUNT(g) FROM t", [seg])
    sx, sg = res.groups()[()]
    assert len(sx) == 7 + 1 + 1 and len(sg) == 5 + 1 + 1   # values, -0.0 (x: 0.0 also drawn), NaN
    assert res.rows() == [(9, 7)]


# --------------------------------------------------------------------------------------------- 3: fold shapes
def _shape_segment(name, g, c, extra=None):
    cols = {"g": (np.asarray(g, dtype=np.int32), S.INT, {}), "c": (np.asarray(c, dtype=np.int32), S.INT, {}),
            "m": (np.arange(len(g), dtype=np.int32) % 10, S.INT, {"dictionary": False})}
    cols.update(extra or {})
    return S.build_segment(name, cols)


def test_fold_one_group_many_values(engine):
    """One group holding 5003 distinct values (its rows span many blocks of the fold), next to two small ones."""
    n = 12_000
    rng = np.random.default_rng(3)
    g = np.full(n, 7)
    c = rng.integers(0, 5003, n) * 3
    c[:5003] = np.arange(5003) * 3
    g[-40:] = 9
    g[-3:] = 2
    b = _shape_segment("one", g, c)
    res = check_native(engine, "SELECT g, DISTINCTCOUNT(c), COUNT(*) FROM t GROUP BY g", [engine.ImmutableSegment(b)], [b])
    assert len(res.groups()[(7,)][0]) == 5003


def test_fold_many_groups_one_value(engine):
    """5001 groups of exactly one value each (every count 1, every CSR range one entry)."""
    ng = 5001
    g = np.repeat(np.arange(ng), 3)
    c = np.repeat((np.arange(ng) * 7919) % 6007, 3)
    b = _shape_segment("many", g, c)
    res = check_native(engine, "SELECT g, DISTINCTCOUNT(c) FROM t GROUP BY g LIMIT 100000", [engine.ImmutableSegment(b)], [b])
    assert all(len(v[0]) == 1 for v in res.groups().values())


def test_fold_grid_strides(engine):
    """More than 70_000 (group, value) pairs, a count that is no multiple of 64: rows past the first wave of blocks
    and a ragged last wave."""
    rng = np.random.default_rng(8)
    n = 90_000
    g = rng.integers(0, 997, n)
    c = rng.integers(0, 1009, n)
    pairs = len(set(zip(g.tolist(), c.tolist())))
    assert pairs > 70_000 and pairs % 64 != 0
    b = _shape_segment("stride", g, c)
    check_native(engine, "SELECT g, DISTINCTCOUNT(c), SUM(m) FROM t GROUP BY g LIMIT 2000", [engine.ImmutableSegment(b)], [b])


def test_fold_cardinality_one_and_no_match(engine):
    """A DISTINCTCOUNT column of cardinality 1; a filter matching nothing, with GROUP BY (no groups) and without
    (one group: count 0, the empty set)."""
    rng = np.random.default_rng(13)
    n = 7_001
    b = _shape_segment("card1", rng.integers(0, 50, n), np.full(n, 42))
    seg = engine.ImmutableSegment(b)
    res = check_native(engine, "SELECT g, DISTINCTCOUNT(c), COUNT(*) FROM t GROUP BY g LIMIT 100", [seg], [b])
    assert all(v[0] == frozenset([42]) for v in res.groups().values())
    check_native(engine, "SELECT DISTINCTCOUNT(c) FROM t", [seg], [b])
    res = check_native(engine, "SELECT g, DISTINCTCOUNT(c) FROM t WHERE m > 100 GROUP BY g", [seg], [b])
    assert res.groups() == {} and res.rows() == []
    res = check_native(engine, "SELECT DISTINCTCOUNT(c), DISTINCTCOUNT(g) FROM t WHERE m > 100", [seg], [b])
    assert res.groups() == {(): [frozenset(), frozenset()]} and res.rows() == [(0, 0)]


# ----------------------------------------------------------------------------------------- 4: plan coverage
def test_child_plans_dense_and_partitioned(engine, two_segments):
    """The value-set query as a dense plan ((g, c): 50 x 40 keys, an LDS table) and as a partitioned plan ((d1, d0):
    37 x 1000 keys and (d1, r_int): ~37 x 27k keys, past the LDS tables), seen through kernel_info's +distinct(...)
    part."""
    rng = np.random.default_rng(31)
    n = 7_001
    b = _shape_segment("dense", rng.integers(0, 50, n), rng.integers(0, 40, n) * 5)
    res = check_native(engine, "SELECT g, DISTINCTCOUNT(c) FROM t GROUP BY g LIMIT 50", [engine.ImmutableSegment(b)], [b])
    info, parts = distinct_part(res)
    assert len(parts) == 1 and parts[0].startswith("c:jit"), info
    assert "partitioned" not in info and "hash" not in info, info
    bufs, segs = two_segments
    res = check_native(engine, "SELECT d1, DISTINCTCOUNT(d0) FROM t GROUP BY d1 LIMIT 50", segs, bufs)
    info, parts = distinct_part(res)
    assert len(parts) == 1 and parts[0].startswith("d0:jit-partitioned"), info
    res = check_native(engine, "SELECT d1, DISTINCTCOUNT(r_int), COUNT(*) FROM t GROUP BY d1 LIMIT 50", segs, bufs)
    info, parts = distinct_part(res)
    assert len(parts) == 1 and parts[0].startswith("r_int:jit-partitioned"), info
    assert "partitioned" not in info.split(" +distinct(")[0], info   # the base: a dense table of 37 keys


def test_child_plan_hash_by_key_space(engine):
    """A (group, value) key space above 2^28 (3200 groups x ~110k distinct raw values): the value-set query runs
    the hash plan while the base stays dense -- the two sides meet in the export layout."""
    rng = np.random.default_rng(77)
    n = 200_000
    b = S.build_segment("dnhash", {"g": (rng.integers(0, 3200, n).astype(np.int32), S.INT, {}),
                                   "k": (rng.integers(0, 150_000, n).astype(np.int64) * 3 - 10**12, S.LONG,
                                         {"dictionary": False})})
    res = check_native(engine, "SELECT g, DISTINCTCOUNT(k) FROM t GROUP BY g LIMIT 5000", [engine.ImmutableSegment(b)], [b])
    info, parts = distinct_part(res)
    assert len(parts) == 1 and parts[0].startswith("k:jit-hash"), info
    assert "hash" not in info.split(" +distinct(")[0], info


def test_forced_hash_base_and_child(engine, two_segments, monkeypatch):
    """PINOT_AMD_GROUP_PLAN=hash: the base's groups come from a hash table too (sorted on the device first)."""
    monkeypatch.setenv("PINOT_AMD_GROUP_PLAN", "hash")
    bufs, segs = two_segments
    res = check_native(engine, "SELECT d1, d0, DISTINCTCOUNT(r_int), SUM(r_long) FROM t WHERE r_int > 0 GROUP BY d1, d0 "
                               "LIMIT 100000", segs, bufs)
    info, parts = distinct_part(res)
    assert info.startswith("jit-hash") and parts[0].startswith("r_int:jit-hash"), info


def test_base_key_of_two_words(engine):
    """Five GROUP BY columns of 13 bits each (5000 distinct values): 65 bits of key, so the packed base key spills
    into a second 64-bit word; the value-set query's c joins that second word. 5000 groups of 4 docs each."""
    rng = np.random.default_rng(21)
    nb, rep = 5_000, 4
    cols = {}
    for j in range(5):
        cols[f"g{j}"] = (np.tile(rng.permutation(9_000)[:nb] + j, rep).astype(np.int32), S.INT, {})
    cols["c"] = (rng.integers(0, 7, nb * rep).astype(np.int32), S.INT, {})
    b = S.build_segment("wide", cols)
    for j in range(5):
        assert b.columns[f"g{j}"].cardinality > (1 << 12)   # 13 bits each: 65 bits of key
    q = "SELECT g0, g1, g2, g3, g4, DISTINCTCOUNT(c), COUNT(*) FROM t GROUP BY g0, g1, g2, g3, g4 LIMIT 100000"
    res = check_native(engine, q, [engine.ImmutableSegment(b)], [b])
    info, parts = distinct_part(res)
    assert info.startswith("jit-hash") and parts[0].startswith("c:jit-hash"), info
    assert len(res.groups()) == nb and max(len(v[0]) for v in res.groups().values()) > 1


# --------------------------------------------------------------------------- 5: several DISTINCTCOUNTs at once
def test_two_distinctcounts_with_other_aggregations(engine, two_segments):
    bufs, segs = two_segments
    q = ("SELECT d1, DISTINCTCOUNT(d0), SUM(r_long), DISTINCTCOUNT(r_int), COUNT(*), AVG(r_int), DISTINCTCOUNT(d0) "
         "FROM t WHERE r_int > -500000 GROUP BY d1 LIMIT 50")
    res = check_native(engine, q, segs, bufs, mirror=True)
    info, parts = distinct_part(res)
    assert [p.split(":")[0] for p in parts] == ["d0", "r_int"], info   # one value-set query per distinct column


def test_distinctcount_of_a_group_by_column(engine, two_segments):
    bufs, segs = two_segments
    res = check_native(engine, "SELECT d1, DISTINCTCOUNT(d1), COUNT(*) FROM t GROUP BY d1 LIMIT 50", segs, bufs, mirror=True)
    assert "+distinct(" not in res.kernel_info()
    assert all(v[0] == frozenset([k[0]]) for k, v in res.groups().items())
    assert all(r[1] == 1 for r in res.rows())
    res = check_native(engine, "SELECT d1, DISTINCTCOUNT(d1), DISTINCTCOUNT(d0) FROM t GROUP BY d1 LIMIT 50", segs, bufs)
    info, parts = distinct_part(res)
    assert [p.split(":")[0] for p in parts] == ["d0"], info


# ------------------------------------------------------------------------------------------ 6: numGroupsLimit
def test_num_groups_limit(engine, two_segments):
    """SET numGroupsLimit = 40 over two segments with different dictionaries: the groups are the ones the base
    query admitted, each with its values over every matching doc, and the flag is set."""
    bufs, segs = two_segments
    q = "SET numGroupsLimit = 40; SELECT d0, DISTINCTCOUNT(d1), COUNT(*) FROM t GROUP BY d0 LIMIT 100000"
    res = check_native(engine, q, segs, bufs, mirror=True)
    assert res.num_groups_limit_reached()
    _, full = oracle.execute(q.split(";")[1], bufs)
    assert 40 <= len(res.groups()) <= 80 < len(full)


# -------------------------------------------------------------------------------------------- 7: server table
SERVER_QUERIES = [
    "SET minServerGroupTrimSize = 3; SELECT d0, DISTINCTCOUNT(d1), COUNT(*) FROM t GROUP BY d0 "
    "ORDER BY DISTINCTCOUNT(d1) DESC LIMIT 2",
    "SELECT d0, DISTINCTCOUNT(d1) FROM t GROUP BY d0 LIMIT 5",
]


@pytest.mark.parametrize("plan", ["auto", "hash"])
@pytest.mark.parametrize("qi", range(len(SERVER_QUERIES)))
def test_server_table_orders_by_distinctcount(engine, qi, plan, monkeypatch):
    """The two DISTINCTCOUNT queries of test_gpu_server_trim.QUERIES on its segments, against its expectation
    (oracle_reduce.server_table over the oracle's groups): the fold runs before the table, the table may order by
    the count, and the CSR follows the kept groups in the table's order."""
    from test_gpu_parity import assert_same_groups
    if plan == "hash":
        monkeypatch.setenv("PINOT_AMD_GROUP_PLAN", "hash")
    q = SERVER_QUERIES[qi]
    rng = np.random.default_rng(50 + 7 + qi)
    bufs = [random_segment(rng, 30_000 + 1_000 * i, name=f"dst{i}", bits_cards=(300, 37)) for i in range(3)]
    segs = [engine.ImmutableSegment(b) for b in bufs]
    qc = parse_sql(q)
    res = engine.ServerQueryExecutor(server_trim=True, distinct_count="native").execute(qc, segs)
    got = res.groups()
    _, full = oracle.execute(q, bufs)
    exp = server_table(oracle.parse_sql(q), full)
    assert len(got) == len(exp) < len(full)
    assert_same_groups(got, exp, set())
    if qc.order_by:
        assert list(got) == list(exp)
    for row in res.rows():
        assert row[1] == len(exp[row[:1]][0])
    mirror = engine.ServerQueryExecutor(server_trim=True).execute(qc, segs).groups()
    assert list(mirror) == list(got) and mirror == got


def test_segment_level_trims_are_refused(engine, two_segments):
    _, segs = two_segments
    ex = engine.ServerQueryExecutor(server_trim=True, distinct_count="native")
    with pytest.raises(engine._lib.PinotAmdError, match="segment-level"):
        ex.execute("SET sortAggregateLimitThreshold = 5; SELECT d1, DISTINCTCOUNT(d0) FROM t GROUP BY d1 ORDER BY d1 "
                   "LIMIT 8", segs)
    with pytest.raises(engine._lib.PinotAmdError, match="segment-level"):
        ex.execute("SET minSegmentGroupTrimSize = 10; SELECT d1, DISTINCTCOUNT(d0) FROM t GROUP BY d1 "
                   "ORDER BY DISTINCTCOUNT(d0) LIMIT 2", segs)
    with pytest.raises(engine._lib.PinotAmdError, match="mirror"):
        engine.ServerQueryExecutor(distinct_count="native").execute(
            "SELECT d1, DISTINCTCOUNT(d0) FROM t GROUP BY d1", segs, key_space={"d1": [3, 10]})


# -------------------------------------------------------------------------------------------- 8: result calls
def _raw_csr(L, h, agg, cap, ngroups):
    total = C.c_int64(-1)
    off = np.full(ngroups + 1, -1, dtype=np.int64)
    vals = np.full(max(cap, 1), -1, dtype=np.int64)
    rc = L.pinot_amd_result_fetch_distinct_values(h, agg, cap, off.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  vals.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(total))
    return rc, total.value, off, vals


def test_result_calls(engine):
    rng = np.random.default_rng(17)
    n = 7_001
    names = np.array([f"v{i:03d}é" for i in range(61)], dtype=object)
    b = S.build_segment("dnres", {"g": (rng.integers(0, 23, n).astype(np.int32), S.INT, {}),
                                  "s": (names[rng.integers(0, 61, n)], S.STRING, {}),
                                  "r": (rng.integers(0, 300, n).astype(np.int32), S.INT, {"dictionary": False})})
    seg = engine.ImmutableSegment(b)
    L = engine.lib()
    q = "SELECT g, DISTINCTCOUNT(s), SUM(r), DISTINCTCOUNT(r) FROM t WHERE r < 250 GROUP BY g LIMIT 100"
    res = check_native(engine, q, [seg], [b], mirror=True)   # the STRING sets round-trip through distinct_string
    h = res._h
    ng = len(res.groups())
    assert ng == 23
    # library aggregations: 0 DISTINCTCOUNT(s), 1 SUM(r), 2 DISTINCTCOUNT(r)
    sizing = C.c_int64()
    assert L.pinot_amd_result_fetch_distinct_values(h, 0, 0, None, None, C.byref(sizing)) == 0
    total = sizing.value
    counts = [r[1] for r in sorted(res.rows())]
    assert total == sum(counts) > ng
    rc, t2, off, vals = _raw_csr(L, h, 0, total, ng)
    assert rc == 0 and t2 == total and off[0] == 0 and off[-1] == total
    assert np.diff(off).tolist() == counts
    for g in range(ng):   # ascending merged-dictionary ids within a group, every id a string of the column
        ids = vals[off[g]:off[g + 1]]
        assert np.all(np.diff(ids) > 0)
    assert L.pinot_amd_result_distinct_string(h, 0, int(vals[0])).decode() in set(names.tolist())
    assert L.pinot_amd_result_distinct_string(h, 0, 61) is None
    assert L.pinot_amd_result_distinct_string(h, 2, 0) is None      # an INT column
    rc, t3, _, _ = _raw_csr(L, h, 0, total - 1, ng)
    assert rc == EOVERFLOW and t3 == total
    assert _raw_csr(L, h, 1, total, ng)[0] == EINVAL                 # SUM(r) is no DISTINCTCOUNT
    # fetch_intermediate: (count, 0)
    pairs = np.zeros(ng * 3 * 2, dtype=np.float64)
    got = C.c_int64()
    assert L.pinot_amd_result_fetch_intermediate(h, ng, pairs.ctypes.data_as(C.POINTER(C.c_double)), C.byref(got)) == 0
    pr = pairs.reshape(ng, 3, 2)
    assert pr[:, 0, 0].tolist() == [float(c) for c in counts] and not pr[:, 0, 1].any()
    # execute_again: identical bytes from the fetch and from the CSR
    before = [a.tobytes() for a in res.fetch_arrays()[1:4]] + [_raw_csr(L, h, a, 10_000, ng) for a in (0, 2)]
    ms, by = res.last_kernel_ms(), res.algorithmic_bytes()
    res.execute_again()
    after = [a.tobytes() for a in res.fetch_arrays()[1:4]] + [_raw_csr(L, h, a, 10_000, ng) for a in (0, 2)]
    for x, y in zip(before, after):
        if isinstance(x, bytes):
            assert x == y
        else:
            assert x[:2] == y[:2] and x[2].tobytes() == y[2].tobytes() and x[3].tobytes() == y[3].tobytes()
    assert ms > 0 and res.algorithmic_bytes() == by
    # the dense accumulators and the by-value merge are not offered for value sets
    nsl, nks = C.c_int32(), C.c_int64()
    assert L.pinot_amd_result_accumulators(h, C.byref(nsl), C.byref(nks), None, None) == EUNSUPPORTED
    kw, na, ngr = C.c_int32(), C.c_int32(), C.c_int64()
    assert L.pinot_amd_result_export_groups(h, None, None, 0, C.byref(kw), C.byref(na), C.byref(ngr), None) == EUNSUPPORTED
    assert L.pinot_amd_result_merge_groups(h, None, None, 0, None) == EUNSUPPORTED
    res.destroy()
    # the destroyed result's plans were kept under their own identities: the same query again, and its base alone
    res = check_native(engine, q, [seg], [b])
    res.destroy()
    plain = engine.ServerQueryExecutor().execute("SELECT g, SUM(r) FROM t WHERE r < 250 GROUP BY g LIMIT 100", [seg])
    _, og = oracle.execute("SELECT g, SUM(r) FROM t WHERE r < 250 GROUP BY g LIMIT 100", [b])
    assert plain.groups() == og
