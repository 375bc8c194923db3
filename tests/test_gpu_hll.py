"""DISTINCTCOUNTHLL on the device (PINOT_AMD_AGG_DISTINCTCOUNTHLL): the twins hll_hash_kernel builds,
the register query, and the fold (hll_fold_place_kernel / hll_estimate_kernel). Every case compares the registers
pinot_amd_result_fetch_hll hands out, byte for byte, and the estimates of pinot_amd_result_fetch, exactly, with the
per-doc restatement tests/hll_ref.py; the mirror path (the distinct values hashed on the host) must give the same."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import hll_ref as H
from helpers import GOLDEN, SV_FILTER, sv_segment
from pinot_amd import segment as S
from pinot_amd.query import canonical_key

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED, EOVERFLOW = -1, -2, -5


@pytest.fixture(scope="module")
def engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from pinot_amd import engine as E
    return E


def make(engine, name, cols):
    """cols: column -> (values, type, options). -> (column -> values, ImmutableSegment)"""
    b = S.build_segment(name, cols)
    return {c: v[0] for c, v in cols.items()}, engine.ImmutableSegment(b)


def concat(datas, col, stype):
    if stype == "STRING":
        return [x for d in datas for x in d[col]]
    return np.concatenate([np.asarray(d[col]) for d in datas])


def reference(datas, aggs, keys=(), mask=None):
    """aggs: [(column, stored type, log2m)] -> {key: [registers per aggregation]} over the concatenated docs."""
    n = sum(len(d[aggs[0][0]]) for d in datas)
    m = np.ones(n, dtype=bool) if mask is None else mask(lambda c: np.concatenate([np.asarray(d[c]) for d in datas]))
    kcols = [np.concatenate([np.asarray(d[k]) for d in datas]) for k in keys]
    per = [H.grouped(concat(datas, c, t), t, l, kcols, m) for c, t, l in aggs]
    return {k: [p[k] for p in per] for k in per[0]}


def check(engine, q, segs, datas, aggs, keys=(), mask=None, mirror=True, executor=None):
    """q's DISTINCTCOUNTHLL aggregations (in `aggs` order, the query's first aggregations) against the reference:
    registers from groups() (fetch_hll), estimates from rows() (fetch). Returns the native result."""
    ex = executor or engine.ServerQueryExecutor(distinct_count="native")
    res = ex.execute(q, segs)
    exp = reference(datas, aggs, keys, mask)
    got = res.groups()
    assert {canonical_key(k) for k in got} == {canonical_key(k) for k in exp}, q
    for k, parts in got.items():
        for i, (c, t, l) in enumerate(aggs):
            assert parts[i][0] == l, (q, k)
            assert parts[i][1] == exp[k][i], (q, k, c)
    nk = len(keys)
    rows = res.rows()
    assert len(rows) == min(len(exp), res.qc.limit)
    for row in rows:
        for i in range(len(aggs)):
            assert row[nk + i] == H.cardinality(exp[tuple(row[:nk])][i]), (q, row)
    if mirror:
        m = engine.ServerQueryExecutor().execute(q, segs)
        mg = m.groups()
        assert set(mg) == set(got)
        for k in got:
            for i in range(len(aggs)):
                assert tuple(mg[k][i]) == tuple(got[k][i]), (q, k)
        assert sorted(m.rows()) == sorted(rows)
        m.destroy()
    return res


def hll_parts(res):
    info = res.kernel_info()
    return info, info.split(" +hll(")[1:]


# ------------------------------------------------------------------------------------------------ 1: the pins
def test_pinot_pins_native_and_mirror(engine):
    with open(os.path.join(GOLDEN, "sv_hll_expected.json")) as f:
        pins = json.load(f)
    seg = engine.ImmutableSegment(sv_segment())
    assert pins["filter"] == SV_FILTER
    for case in pins["cases"]:
        q = pins["query"] + (pins["filter"] if case["filter"] else "") + (pins["group_by"] if case["group_by"] else "")
        for ex in (engine.ServerQueryExecutor(distinct_count="native", server_trim=True),
                   engine.ServerQueryExecutor(server_trim=True)):
            # "inter": four copies of the segment
            res = ex.execute(q, [seg, seg, seg, seg])
            rows = res.rows()
            assert [list(r[-2:]) for r in rows] == [case["expected"]], (q, rows)
            res.destroy()


# --------------------------------------------------------------------------------------- 2: shapes and sources
@pytest.fixture(scope="module")
def mixed(engine):
    """Segments of 4099, 1, 0 and 2500 docs; c: an INT column dictionary-encoded in two and raw in two (the mirror
    path's (g, c) query refuses such a batch: only the native path reads it); cu / ru: the same values
    dictionary-encoded / raw in every segment; g: ~300 groups."""
    rng = np.random.default_rng(41)
    out = []
    for i, (n, raw) in enumerate([(4099, False), (1, True), (0, False), (2500, True)]):
        c = rng.integers(-50_000, 50_000, n).astype(np.int32)
        if n > 10:
            c[:3] = [0, -(1 << 31), (1 << 31) - 1]
        out.append(make(engine, f"hm{i}", {
            "c": (c, S.INT, {"dictionary": not raw}),
            "cu": (c, S.INT, {}), "ru": (c, S.INT, {"dictionary": False}),
            "g": (rng.integers(0, 300, n).astype(np.int32), S.INT, {}),
            "one": (np.full(n, 5, dtype=np.int32), S.INT, {}),
            "x": (rng.integers(0, 100, n).astype(np.int32), S.INT, {"dictionary": False})}))
    return [d for d, _ in out], [s for _, s in out]


@pytest.mark.parametrize("log2m", [4, 8, 12, 16])
def test_batch_of_mixed_segments(engine, mixed, log2m):
    """Every log2m over the batch (one column raw in two segments and dictionary-encoded in the others, segments of
    1 and 0 docs): no GROUP BY, one group, ~300 groups."""
    datas, segs = mixed
    a = [("c", "INT", log2m)]
    check(engine, f"SELECT DISTINCTCOUNTHLL(c, {log2m}) FROM t", segs, datas, a, mirror=False)
    check(engine, f"SELECT one, DISTINCTCOUNTHLL(c, {log2m}) FROM t WHERE x < 70 GROUP BY one", segs, datas, a, ["one"],
          lambda col: col("x") < 70, mirror=False)
    for c in ("cu", "ru"):   # uniformly stored: the mirror path too
        check(engine, f"SELECT DISTINCTCOUNTHLL({c}, {log2m}) FROM t WHERE x < 70", segs, datas, [(c, "INT", log2m)],
              mask=lambda col: col("x") < 70)
    if log2m <= 12:
        res = check(engine, f"SELECT g, DISTINCTCOUNTHLL(c, {log2m}), COUNT(*) FROM t GROUP BY g LIMIT 1000", segs, datas, a,
                    ["g"], mirror=False)
        assert len(res.groups()) == 300
        if log2m == 8:
            check(engine, "SELECT g, DISTINCTCOUNTHLL(ru), COUNT(*) FROM t GROUP BY g LIMIT 1000", segs, datas,
                  [("ru", "INT", 8)], ["g"])


def test_single_segments_and_no_match(engine, mixed):
    datas, segs = mixed
    a = [("c", "INT", 8)]
    for i in (0, 1, 2):   # 4099 docs, one doc, no doc
        check(engine, "SELECT DISTINCTCOUNTHLL(c) FROM t", [segs[i]], [datas[i]], a)
    res = check(engine, "SELECT DISTINCTCOUNTHLL(c) FROM t WHERE x > 1000", segs, datas, a, mask=lambda col: col("x") > 1000,
                mirror=False)
    assert res.rows() == [(0,)] and res.groups() == {(): [(8, bytes(256))]}
    res = check(engine, "SELECT g, DISTINCTCOUNTHLL(c) FROM t WHERE x > 1000 GROUP BY g", segs, datas, a, ["g"],
                lambda col: col("x") > 1000, mirror=False)
    assert res.groups() == {} and res.rows() == []


def test_value_types(engine):
    """LONG raw near +-2^62, FLOAT / DOUBLE with -0.0 and NaN (raw and dictionary-encoded), STRING with non-ASCII and
    empty values, a sorted column."""
    rng = np.random.default_rng(43)
    n = 4099
    lng = rng.integers(-(1 << 62) - 1000, -(1 << 62) + 1000, n)
    lng[::2] = rng.integers((1 << 62) - 1000, (1 << 62) + 1000, (n + 1) // 2)
    f = (rng.integers(-40, 40, n) * 0.25).astype(np.float32)
    f[::5], f[::13] = -0.0, np.nan
    d = rng.integers(-40, 40, n) * 0.125
    d[::7], d[::11] = -0.0, np.nan
    words = np.array(["", "a", "é", "aé", "éa", "abÿ", "日本語", "abc\U0001F600"] + [f"w{i}é" * (i % 4) + "x" * (i % 9)
                                                                              for i in range(200)], dtype=object)
    cols = {
        "lr": (lng.astype(np.int64), S.LONG, {"dictionary": False}), "ld": (lng.astype(np.int64), S.LONG, {}),
        # (the segment builder's dictionaries hold one zero: the dictionary-encoded copies carry -0.0 alone)
        "fr": (f, S.FLOAT, {"dictionary": False}), "fd": (np.where(f == 0, np.float32(-0.0), f), S.FLOAT, {}),
        "dr": (d, S.DOUBLE, {"dictionary": False}), "dd": (np.where(d == 0, -0.0, d), S.DOUBLE, {}),
        "s": (words[rng.integers(0, len(words), n)], S.STRING, {}),
        "ts": (np.sort(rng.integers(0, 900, n)).astype(np.int32), S.INT, {}),
        "g": (rng.integers(0, 7, n).astype(np.int32), S.INT, {}),
    }
    data, seg = make(engine, "hv", cols)
    for c, t in [("lr", "LONG"), ("ld", "LONG"), ("fr", "FLOAT"), ("fd", "FLOAT"), ("dr", "DOUBLE"), ("dd", "DOUBLE"),
                 ("s", "STRING"), ("ts", "INT")]:
        a = [(c, t, 8)]
        check(engine, f"SELECT DISTINCTCOUNTHLL({c}) FROM t", [seg], [data], a)
        check(engine, f"SELECT g, DISTINCTCOUNTHLL({c}, 5) FROM t WHERE g <> 3 GROUP BY g", [seg], [data], [(c, t, 5)], ["g"],
              lambda col: col("g") != 3)
    assert H.registers(data["fr"], "FLOAT", 8) != H.registers(data["fr"].astype(np.float64), "DOUBLE", 8)


# ------------------------------------------------------------------------------------------- 3: plan coverage
def test_child_table_kinds(engine, mixed, monkeypatch):
    datas, segs = mixed
    res = check(engine, "SELECT one, DISTINCTCOUNTHLL(c, 4) FROM t GROUP BY one", segs, datas, [("c", "INT", 4)], ["one"],
                mirror=False)
    info, parts = hll_parts(res)
    assert len(parts) == 1 and parts[0].startswith("c,4:jit") and "partitioned" not in parts[0] and "hash" not in parts[0], info
    res = check(engine, "SELECT g, DISTINCTCOUNTHLL(c, 12) FROM t GROUP BY g LIMIT 1000", segs, datas, [("c", "INT", 12)],
                ["g"], mirror=False)
    info, parts = hll_parts(res)
    assert parts[0].startswith("c,12:jit-partitioned"), info
    monkeypatch.setenv("PINOT_AMD_GROUP_PLAN", "hash")
    res = check(engine, "SELECT g, DISTINCTCOUNTHLL(c, 10), SUM(x) FROM t GROUP BY g LIMIT 1000", segs, datas,
                [("c", "INT", 10)], ["g"], mirror=False)
    info, parts = hll_parts(res)
    assert info.startswith("jit-hash") and parts[0].startswith("c,10:jit-hash"), info


def test_two_hlls_beside_other_aggregations(engine, mixed):
    datas, segs = mixed
    q = ("SELECT g, DISTINCTCOUNTHLL(cu), DISTINCTCOUNTHLL(cu, 12), DISTINCTCOUNT(cu), SUM(x), DISTINCTCOUNTHLL(cu, 8) "
         "FROM t WHERE x >= 10 GROUP BY g LIMIT 1000")
    res = check(engine, q, segs, datas, [("cu", "INT", 8), ("cu", "INT", 12)], ["g"], lambda col: col("x") >= 10)
    info, parts = hll_parts(res)
    assert [p.split(":")[0] for p in parts] == ["cu,8", "cu,12"] and info.count("+distinct(cu:") == 1, info
    cc = np.concatenate([d["c"] for d in datas]); gg = np.concatenate([d["g"] for d in datas])
    xx = np.concatenate([d["x"] for d in datas])
    for k, parts_ in res.groups().items():
        sel = (gg == k[0]) & (xx >= 10)
        assert parts_[2] == frozenset(cc[sel].tolist()) and parts_[3] == float(xx[sel].sum())
        assert parts_[4] == parts_[0]
    # differing log2m shares no plan; the same (column, log2m) one
    assert parts[0].split(":", 1)[1] != "" and res.kernel_info().count("+hll(") == 2


def test_server_table_ordered_by_the_hll(engine, mixed):
    datas, segs = mixed
    q = ("SET minServerGroupTrimSize = 3; SELECT g, DISTINCTCOUNTHLL(cu, 6), COUNT(*) FROM t GROUP BY g "
         "ORDER BY DISTINCTCOUNTHLL(cu, 6) DESC, g LIMIT 4")
    exp = reference(datas, [("cu", "INT", 6)], ["g"])
    order = sorted(exp, key=lambda k: (-H.cardinality(exp[k][0]), k[0]))[:12]   # max(5 * LIMIT, 3) kept, LIMIT rows
    for ex in (engine.ServerQueryExecutor(server_trim=True, distinct_count="native"),
               engine.ServerQueryExecutor(server_trim=True)):
        res = ex.execute(q, segs)
        got = res.groups()
        assert list(got)[:4] == order[:4]
        for k, parts in got.items():
            assert parts[0] == (6, exp[k][0])
        assert [r[:2] for r in res.rows()] == [(k[0], H.cardinality(exp[k][0])) for k in order[:4]]
        res.destroy()


def test_num_groups_limit(engine, mixed):
    datas, segs = mixed
    q = "SET numGroupsLimit = 40; SELECT g, DISTINCTCOUNTHLL(cu), COUNT(*) FROM t GROUP BY g LIMIT 100000"
    nat = engine.ServerQueryExecutor(distinct_count="native").execute(q, segs)
    mir = engine.ServerQueryExecutor().execute(q, segs)
    assert nat.num_groups_limit_reached() and mir.num_groups_limit_reached()
    gn, gm = nat.groups(), mir.groups()
    exp = reference(datas, [("cu", "INT", 8)], ["g"])
    assert set(gn) == set(gm) and 40 <= len(gn) < 300
    for k in gn:   # the admitted groups, each over every matching doc
        assert gn[k][0] == (8, exp[k][0]) and tuple(gm[k][0]) == gn[k][0]


# --------------------------------------------------------------------------------------------- 4: result calls
def test_result_calls_and_twin_reuse(engine):
    rng = np.random.default_rng(47)
    n = 4099
    data, seg = make(engine, "hr", {"c": (rng.integers(0, 3000, n).astype(np.int64) * 77, S.LONG, {"dictionary": False}),
                                    "g": (rng.integers(0, 23, n).astype(np.int32), S.INT, {})})
    L = engine.lib()
    bytes0 = seg.device_bytes()
    q = "SELECT g, DISTINCTCOUNTHLL(c, 9), COUNT(*) FROM t GROUP BY g LIMIT 100"
    res = check(engine, q, [seg], [data], [("c", "LONG", 9)], ["g"])
    bytes1 = seg.device_bytes()
    # the twins: 9 + 5 bits per doc and the two identity dictionaries
    assert bytes1 - bytes0 >= (n * 14) // 8 + (512 + 25) * 4
    h, ng, m = res._h, 23, 512
    log2m, groups = C.c_int32(), C.c_int64()
    assert L.pinot_amd_result_fetch_hll(h, 0, 0, None, C.byref(log2m), C.byref(groups)) == 0
    assert (log2m.value, groups.value) == (9, ng)
    buf = np.zeros(ng * m, dtype=np.uint8)
    assert L.pinot_amd_result_fetch_hll(h, 0, ng * m - 1, buf.ctypes.data, C.byref(log2m), C.byref(groups)) == EOVERFLOW
    assert L.pinot_amd_result_fetch_hll(h, 1, buf.size, buf.ctypes.data, C.byref(log2m), C.byref(groups)) == EINVAL
    assert L.pinot_amd_result_fetch_hll(h, 0, buf.size, buf.ctypes.data, C.byref(log2m), C.byref(groups)) == 0
    total = C.c_int64()
    assert L.pinot_amd_result_fetch_distinct_values(h, 0, 0, None, None, C.byref(total)) == EINVAL
    # fetch_intermediate: (estimate, 0)
    pairs = np.zeros(ng * 2 * 2, dtype=np.float64)
    got = C.c_int64()
    assert L.pinot_amd_result_fetch_intermediate(h, ng, pairs.ctypes.data_as(C.POINTER(C.c_double)), C.byref(got)) == 0
    est = [r[1] for r in sorted(res.rows())]
    assert pairs.reshape(ng, 2, 2)[:, 0, 0].tolist() == [float(e) for e in est] and not pairs.reshape(ng, 2, 2)[:, 0, 1].any()
    # execute_again: identical bytes
    before = [a.tobytes() for a in res.fetch_arrays()[1:4]]
    res.execute_again()
    buf2 = np.zeros(ng * m, dtype=np.uint8)
    assert L.pinot_amd_result_fetch_hll(h, 0, buf2.size, buf2.ctypes.data, C.byref(log2m), C.byref(groups)) == 0
    assert buf2.tobytes() == buf.tobytes() and [a.tobytes() for a in res.fetch_arrays()[1:4]] == before
    # the dense accumulators and the by-value merge are not offered
    nsl, nks = C.c_int32(), C.c_int64()
    assert L.pinot_amd_result_accumulators(h, C.byref(nsl), C.byref(nks), None, None) == EUNSUPPORTED
    kw, na, ngr = C.c_int32(), C.c_int32(), C.c_int64()
    assert L.pinot_amd_result_export_groups(h, None, None, 0, C.byref(kw), C.byref(na), C.byref(ngr), None) == EUNSUPPORTED
    res.destroy()
    # the second query builds nothing
    res = check(engine, q, [seg], [data], [("c", "LONG", 9)], ["g"], mirror=False)
    assert seg.device_bytes() == bytes1
    res.destroy()
    res = check(engine, "SELECT DISTINCTCOUNTHLL(c, 9) FROM t WHERE g < 5", [seg], [data], [("c", "LONG", 9)],
                mask=lambda col: col("g") < 5, mirror=False)
    assert seg.device_bytes() == bytes1
    with pytest.raises(engine._lib.PinotAmdError, match="mirror"):
        engine.ServerQueryExecutor(distinct_count="native").execute(q, [seg], key_space={"g": list(range(23))})


# ------------------------------------------------------------------------------------------------ 5: refusals
def test_refusals_stage_nothing(engine):
    rng = np.random.default_rng(53)
    n = 1000
    mv = np.empty(n, dtype=object)
    for i in range(n):
        mv[i] = rng.integers(0, 50, 1 + i % 3).astype(np.int32)
    b = S.build_segment("hx", {"c": (rng.integers(0, 500, n).astype(np.int32), S.INT, {}),
                               "a": (rng.integers(0, 500, n).astype(np.int32), S.INT, {"dictionary": False}),
                               "g": (rng.integers(0, 9, n).astype(np.int32), S.INT, {}),
                               "mv": (mv, S.INT, {"multi_value": True})})
    seg = engine.ImmutableSegment(b)
    bytes0 = seg.device_bytes()
    ex = engine.ServerQueryExecutor(distinct_count="native")
    for q, what in [("SELECT DISTINCTCOUNTHLL(c) FILTER (WHERE g > 2) FROM t", "FILTER"),
                    ("SELECT DISTINCTCOUNTHLL(c), SUM(a) FILTER (WHERE g > 2) FROM t", "filtered"),
                    ("SELECT DISTINCTCOUNTHLL(mv) FROM t", "mv"),
                    ("SELECT g, DISTINCTCOUNTHLL(nope) FROM t GROUP BY g", "nope")]:
        with pytest.raises(engine._lib.PinotAmdError, match=what):
            ex.execute(q, [seg])
    for q in ["SELECT DISTINCTCOUNTHLL(c + a) FROM t", "SELECT DISTINCTCOUNTHLLMV(mv) FROM t",
              "SELECT DISTINCTCOUNTHLL(c, 17) FROM t", "SELECT DISTINCTCOUNTRAWHLL(c) FROM t",
              "SELECT DISTINCTCOUNTHLLPLUS(c) FROM t", "SELECT DISTINCTCOUNTSMARTHLL(c) FROM t"]:
        with pytest.raises(ValueError):
            ex.execute(q, [seg])
    # through the ABI: an expression as the column
    L = engine.lib()
    qh = C.c_void_p()
    assert L.pinot_amd_query_create(C.byref(qh)) == 0
    try:
        idx = C.c_int32()
        for log2m in (3, 17):
            assert L.pinot_amd_query_add_aggregation_hll(qh, b"c", log2m, C.byref(idx)) == EINVAL
        assert L.pinot_amd_query_add_aggregation_mv(qh, 17, b"mv", C.byref(idx)) == EINVAL
    finally:
        L.pinot_amd_query_destroy(qh)
    assert seg.device_bytes() == bytes0
