"""SELECT DISTINCT on the device: the presence-bitmap scan (LDS, CU-wide LDS and HBM bitmaps), the COUNT-only hash plan,
the dictionary-only answer, ORDER BY / LIMIT and the staged scan without ORDER BY. Every case compares rows() and
num_docs_matched() exactly with tests/distinct_ref.py (a per-doc restatement); every unlimited query's row set is also
checked against the key set of the C oracle's GROUP BY over the same docs."""
import json
import os
import re

import numpy as np
import pytest

import distinct_ref as ref
import helpers
import oracle
import time_transform_ref
from pinot_amd import _lib
from pinot_amd import segment as S
from pinot_amd.query import key_transform, parse_sql

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 1023, 1025, 5000, 70_000)
DAY = 86_400_000
STRINGS = ["a", "B", "zz", "～", "\U0001F600", "é", "", "a b"]       # U+FF5E / U+1F600: UTF-16 order != byte order
DOUBLES = np.array([np.nan, -0.0, 0.0, 1.5, -np.inf, 2.25, -7.0, 1e300])
RAW, DIC = {"dictionary": False}, {"detect_sorted": False}


@pytest.fixture(scope="module")
def engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from pinot_amd import engine as E
    return E


def launches(info: str) -> int:
    m = re.search(r" x(\d+)", info)
    return int(m.group(1)) if m else 1


def draw(rng, n, i):
    """One segment's columns. Dictionaries differ by segment (values offset by the segment index, cardinalities from 1
    to 1000: other bit widths, live remaps)."""
    card = (1, 1, 5, 40, 300, 1000)[i % 6]
    lens = rng.integers(1, 4, n)
    cut = np.r_[0, np.cumsum(lens)].astype(np.int64)
    flat = rng.integers(0, 12, int(lens.sum())).astype(np.int32)
    t = {"di": (rng.integers(0, card, n) * 3 + i).astype(np.int32),
         "ds": np.array([STRINGS[(v + i) % len(STRINGS)] for v in rng.integers(0, 3 + i, n)], dtype=object),
         "ts": (np.sort(rng.integers(0, 30, n)) + i).astype(np.int32),
         "ri": rng.integers(-50, 50, n).astype(np.int32),
         "rl": (rng.integers(0, 40, n) * (1 << 33) - (1 << 35)).astype(np.int64),
         "rd": DOUBLES[rng.integers(0, len(DOUBLES), n)],
         "f": rng.integers(0, 100, n).astype(np.int32),
         "tms": rng.integers(0, 10 * DAY, n).astype(np.int64)}
    t["tags"] = [flat[cut[k]:cut[k + 1]].tolist() for k in range(n)]
    # materialised for the reference and the oracle: the expression, the time bucket, the ANY-match leaf
    t["plus(ri,di)"] = t["ri"].astype(np.float64) + t["di"].astype(np.float64)
    t["mvany"] = np.array([int(6 in d) for d in t["tags"]], dtype=np.int32)
    return t


SPECS = {"di": (S.INT, DIC), "ds": (S.STRING, DIC), "ts": (S.INT, {}), "ri": (S.INT, RAW), "rl": (S.LONG, RAW),
         "rd": (S.DOUBLE, RAW), "f": (S.INT, {"detect_sorted": False, "inverted": True}), "tms": (S.LONG, RAW)}
DAY_KEY = "dateTrunc('DAY', tms)"


def build(engine, tables, prefix):
    """(staged segments, the oracle's segments: the single-value columns plus the materialised ones as raw columns)."""
    segs, obufs = [], []
    kt = key_transform(parse_sql(f"SELECT DISTINCT {DAY_KEY} FROM t").group_by[0])
    for i, t in enumerate(tables):
        n = len(t["di"])
        cols = {c: (t[c], SPECS[c][0], SPECS[c][1]) for c in SPECS}
        cols["tags"] = (t["tags"], S.INT, {"multi_value": True})
        bufs = S.build_segment(f"{prefix}{i}", cols)
        if n > 1:
            assert bufs.columns["ts"].encoding == "SORTED" and bufs.columns["di"].encoding == "FIXED_BIT"
        segs.append(engine.ImmutableSegment(bufs))
        t["kday"] = time_transform_ref.evaluate(kt, t["tms"]) if n else np.zeros(0, np.int64)
        ocols = {c: (t[c], SPECS[c][0], SPECS[c][1]) for c in SPECS}
        ocols["kx"] = (t["plus(ri,di)"], S.DOUBLE, RAW)
        ocols["kday"] = (t["kday"], S.LONG, RAW)
        ocols["mvany"] = (t["mvany"], S.INT, DIC)
        obufs.append(S.build_segment(f"o{prefix}{i}", ocols))
    return segs, obufs


@pytest.fixture(scope="module")
def mix(engine):
    rng = np.random.default_rng(160_016)
    tables = [draw(rng, n, i) for i, n in enumerate(SIZES)]
    segs, obufs = build(engine, tables, "dq")
    widths = {b.columns["di"].bits_per_element for b in obufs if b.num_docs}
    assert len(widths) >= 3                                       # several launch shapes write one bitmap
    yield tables, segs, obufs
    for s in segs:
        s.destroy()


def named(tables, columns):
    """The tables with the query's key texts as column names (a transform's text names its materialised bucket)."""
    out = []
    for t in tables:
        u = dict(t)
        for c in columns:
            if c not in u and key_transform(c) is not None:
                u[c] = t["kday"]
        out.append(u)
    return out


def check(engine, sql, segs, tables, masks, staged=True, oracle_q=None, obufs=None):
    """Run `sql`, compare with the reference, check the invariants; -> (rows, kernel_info)."""
    qc = parse_sql(sql)
    columns, limit = list(qc.group_by), qc.limit
    tables = named(tables, columns)
    res = engine.ServerQueryExecutor().execute(sql, segs)
    try:
        exp_rows, exp_matched, _ = ref.distinct(tables, masks, columns, qc.order_by, limit, staged)
        rows = res.rows()
        assert ref.same_rows(rows, exp_rows), (sql, rows[:5], exp_rows[:5], len(rows), len(exp_rows))
        assert res.num_docs_matched() == exp_matched, sql
        assert res.columns == columns
        true = ref.distinct_set(tables, masks, columns)
        assert all(ref.row_ident(r) in true for r in rows) and len(rows) == min(limit, len(true)), sql
        assert len({ref.row_ident(r) for r in rows}) == len(rows), sql
        if oracle_q is not None:  # unlimited: the row set is the key set of the oracle's GROUP BY over the same docs
            assert limit >= len(true), sql
            nm, groups = oracle.execute(oracle_q, obufs)
            assert {ref.row_ident(k) for k in groups} == {ref.row_ident(r) for r in rows}, sql
            assert nm == res.num_docs_matched() or not staged, sql
        return rows, res.kernel_info()
    finally:
        res.destroy()


def none(tables):
    return [None] * len(tables)


# ------------------------------------------------------------------------------------------------ 1. columns
COLUMN_CASES = [
    # (distinct list, filter SQL, mask builder, ORDER BY, the oracle's keys)
    ("di", "f < 50", "di", "di"),
    ("ds", "f < 50", "ds DESC", "ds"),
    ("ts", "f < 50", "ts", "ts"),
    ("ri", "f < 50", "ri DESC", "ri"),
    ("rl", "f < 50", "rl", "rl"),
    ("rd", "f < 50", "rd", "rd"),
    ("rd", "f < 50", "rd DESC", "rd"),
    ("ri + di, ds", "f < 50", "ds DESC", "kx, ds"),
    (f"{DAY_KEY}", "f < 50", f"{DAY_KEY} DESC", "kday"),
    ("di, ds", "f < 50", "ds, di DESC", "di, ds"),
    ("ds, ts, ri", "f < 50", "ri DESC, ds", "ds, ts, ri"),
    ("ts, rd, ds", "f < 50", "rd", "ts, rd, ds"),          # ORDER BY a subset: the tie rule orders the rest
]


@pytest.mark.parametrize("cols, where, order, okeys", COLUMN_CASES)
def test_columns_and_order_by(engine, mix, cols, where, order, okeys):
    tables, segs, obufs = mix
    masks = [t["f"] < 50 for t in tables]
    sql = f"SELECT DISTINCT {cols} FROM t WHERE {where} ORDER BY {order} LIMIT 1000000"
    oq = f"SELECT {okeys}, COUNT(*) FROM t WHERE {where} GROUP BY {okeys} LIMIT 10000000"
    rows, info = check(engine, sql, segs, tables, masks, oracle_q=oq, obufs=obufs)
    assert info.startswith("jit-distinct-") and rows
    if cols == "rd":  # one NaN, both zeros
        idents = {ref.row_ident(r) for r in rows}
        assert {ref.row_ident((np.nan,)), ref.row_ident((-0.0,)), ref.row_ident((0.0,))} <= idents
    if cols == "ds":  # String.compareTo: the surrogate pair before U+FF5E, descending here
        flat = [r[0] for r in rows]
        assert flat.index("～") < flat.index("\U0001F600")


@pytest.mark.parametrize("limit", [0, 1, 7, None])
def test_limits_on_a_two_column_order(engine, mix, limit):
    """LIMIT 0, 1, one inside the result and Pinot's default (10), mixed directions."""
    tables, segs, _ = mix
    masks = [t["f"] < 50 for t in tables]
    sql = "SELECT DISTINCT ds, ts FROM t WHERE f < 50 ORDER BY ts DESC, ds" + ("" if limit is None else f" LIMIT {limit}")
    rows, info = check(engine, sql, segs, tables, masks)
    assert len(rows) == (10 if limit is None else limit)
    if limit == 0:
        assert launches(info) == 0


def test_limit_exactly_and_above_the_distinct_count(engine, mix):
    tables, segs, obufs = mix
    masks = [t["f"] < 50 for t in tables]
    count = len(ref.distinct_set(tables, masks, ["ts"]))
    for limit in (count, count + 1):
        rows, _ = check(engine, f"SELECT DISTINCT ts FROM t WHERE f < 50 ORDER BY ts DESC LIMIT {limit}", segs, tables, masks,
                        oracle_q="SELECT ts, COUNT(*) FROM t WHERE f < 50 GROUP BY ts LIMIT 100000", obufs=obufs)
        assert len(rows) == count
    rows, _ = check(engine, f"SELECT DISTINCT ts FROM t WHERE f < 50 ORDER BY ts DESC LIMIT {count - 1}", segs, tables, masks)
    assert len(rows) == count - 1


# ------------------------------------------------------------------------------------------------ 2. filters
def test_filters(engine, mix):
    tables, segs, obufs = mix
    oq = "SELECT di, ds, COUNT(*) FROM t WHERE {w} GROUP BY di, ds LIMIT 10000000"
    q = "SELECT DISTINCT di, ds FROM t WHERE {w} ORDER BY di, ds LIMIT 1000000"
    # selective; matching nothing; an inverted-index leaf (f is inverted); raw range AND NOT IN
    for w, mk in (("f < 3", lambda t: t["f"] < 3), ("f > 1000", lambda t: t["f"] > 1000), ("f = 7", lambda t: t["f"] == 7),
                  ("ri BETWEEN -10 AND 10 AND f NOT IN (1, 2, 3)",
                   lambda t: (t["ri"] >= -10) & (t["ri"] <= 10) & ~np.isin(t["f"], [1, 2, 3]))):
        rows, info = check(engine, q.format(w=w), segs, tables, [mk(t) for t in tables], oracle_q=oq.format(w=w), obufs=obufs)
        assert (rows == []) == (w == "f > 1000")
    # no filter on two columns (one column alone would be answered from the dictionary)
    check(engine, "SELECT DISTINCT di, ds FROM t ORDER BY di, ds LIMIT 1000000", segs, tables, none(tables),
          oracle_q="SELECT di, ds, COUNT(*) FROM t GROUP BY di, ds LIMIT 10000000", obufs=obufs)


def test_any_match_leaf_on_a_multi_value_column(engine, mix):
    tables, segs, obufs = mix
    masks = [t["mvany"] == 1 for t in tables]
    rows, _ = check(engine, "SELECT DISTINCT di, ts FROM t WHERE tags = 6 ORDER BY ts, di LIMIT 1000000", segs, tables, masks,
                    oracle_q="SELECT di, ts, COUNT(*) FROM t WHERE mvany = 1 GROUP BY di, ts LIMIT 10000000", obufs=obufs)
    assert rows


def test_multi_value_distinct_column_is_unsupported(engine, mix):
    _, segs, _ = mix
    with pytest.raises(_lib.PinotAmdError) as e:
        engine.ServerQueryExecutor().execute("SELECT DISTINCT tags FROM t WHERE f < 50", segs)
    assert "tags" in str(e.value)
    with pytest.raises(_lib.PinotAmdError) as e:
        engine.ServerQueryExecutor().execute("SELECT DISTINCT di, tags FROM t ORDER BY di", segs)
    assert "tags" in str(e.value)


# ------------------------------------------------------------------------------------------------ 3. table kinds
@pytest.mark.parametrize("plan", ["lds", "wide", "hbm", "hash"])
def test_every_table_kind_on_the_mixed_batch(engine, mix, monkeypatch, plan):
    """Each kind pinned on the batch with the 70 000-doc segment: the same rows from all of them (each is compared
    with the one reference), with and without ORDER BY (a hash plan scans the whole batch)."""
    tables, segs, obufs = mix
    monkeypatch.setenv("PINOT_AMD_DISTINCT_PLAN", plan)
    masks = [t["f"] < 50 for t in tables]
    rows, info = check(engine, "SELECT DISTINCT di, ds FROM t WHERE f < 50 ORDER BY ds DESC, di LIMIT 1000000", segs, tables,
                       masks, oracle_q="SELECT di, ds, COUNT(*) FROM t WHERE f < 50 GROUP BY di, ds LIMIT 10000000", obufs=obufs)
    assert info.startswith("jit-hash" if plan == "hash" else f"jit-distinct-{plan}"), info
    rows, info = check(engine, "SELECT DISTINCT ri, ts FROM t WHERE f < 50 LIMIT 25", segs, tables, masks, staged=plan != "hash")
    assert info.startswith("jit-hash" if plan == "hash" else f"jit-distinct-{plan}"), info
    rows, _ = check(engine, "SELECT DISTINCT ri, ts FROM t WHERE f < 50 ORDER BY ri LIMIT 0", segs, tables, masks)
    assert rows == []


def key_space_tables(n, card_a, card_b, seed):
    """One segment whose (a, b) key space is card_a x card_b exactly, every value of both columns present and the
    last key of the space -- (card_a - 1, card_b - 1) -- among the docs."""
    rng = np.random.default_rng(seed)
    assert n >= max(card_a, card_b)
    a = (np.arange(n) % card_a).astype(np.int32)
    b = ((np.arange(n) * 7 + rng.integers(0, card_b)) % card_b).astype(np.int32) if card_b > 1 else np.zeros(n, np.int32)
    b[:card_b] = np.arange(card_b, dtype=np.int32)
    a[n - 1], b[n - 1] = card_a - 1, card_b - 1
    a[:card_a] = np.arange(card_a, dtype=np.int32)
    return [{"a": a, "b": b, "f": rng.integers(0, 100, n).astype(np.int32)}]


def run_key_space(engine, n, card_a, card_b, kind, seed):
    tables = key_space_tables(n, card_a, card_b, seed)
    t = tables[0]
    assert len(np.unique(t["a"])) == card_a and len(np.unique(t["b"])) == card_b
    bufs = S.build_segment(f"ks{card_a}x{card_b}", {"a": (t["a"], S.INT, DIC), "b": (t["b"], S.INT, DIC), "f": (t["f"], S.INT, RAW)})
    seg = engine.ImmutableSegment(bufs)
    try:
        masks = [t["f"] >= 0]  # every doc, through a raw-range leaf (no filter at all could answer from the dictionary)
        cols = "a, b" if card_b > 1 else "a"
        oq = f"SELECT {cols}, COUNT(*) FROM t WHERE f >= 0 GROUP BY {cols} LIMIT 10000000"
        rows, info = check(engine, f"SELECT DISTINCT {cols} FROM t WHERE f >= 0 ORDER BY a DESC LIMIT 10000000", [seg], tables,
                           masks, oracle_q=oq, obufs=[bufs])
        assert info.startswith(kind), (info, card_a, card_b)
        last = (card_a - 1, card_b - 1) if card_b > 1 else (card_a - 1,)
        assert last in rows
        rows, info = check(engine, f"SELECT DISTINCT {cols} FROM t WHERE f >= 0 LIMIT 10000000", [seg], tables, masks)
        assert info.startswith(kind) and rows[-1] == last      # ascending key order: the space's last key comes last
    finally:
        seg.destroy()


@pytest.mark.parametrize("card", [1, 63, 64, 65])
def test_word_edges(engine, card):
    run_key_space(engine, 1025, card, 1, "jit-distinct-lds", card)


@pytest.mark.parametrize("n, card_a, card_b, kind", [
    (5000, 640, 512, "jit-distinct-lds"),        # 327 680 keys: the last that fit a 256-thread block's 40 KiB
    (5000, 641, 512, "jit-distinct-wide"),       # just above
    (5000, 1280, 1024, "jit-distinct-wide"),     # 1 310 720 keys: the last that fit one CU-wide block's 160 KiB
    (5000, 1281, 1024, "jit-distinct-hbm"),      # just above
    (70_000, 65_536, 32_768, "jit-distinct-hbm"),  # 2^31 keys: the last key space the 32-bit kernel keys index
    (70_000, 65_537, 32_768, "jit-hash"),        # just above: the hash plan
])
def test_table_kind_capacities(engine, n, card_a, card_b, kind):
    run_key_space(engine, n, card_a, card_b, kind, card_a)


# ------------------------------------------------------------------------------------------------ 4. no ORDER BY
def test_staged_scan_without_order_by(engine):
    """8 segments, LIMIT 3: the first stage (1 segment) holds 1 row, the second (2 segments) brings it to 3 and the scan
    stops: 3 of 8 segments scanned, fewer launches than the whole batch takes."""
    rng = np.random.default_rng(8)
    vals = [[40], [10, 40], [30], [5, 6], [7], [8], [9], [1]]
    tables = [{"v": rng.choice(np.array(v, dtype=np.int32), 300 + 17 * i), "f": rng.integers(0, 10, 300 + 17 * i).astype(np.int32)}
              for i, v in enumerate(vals)]
    bufs = [S.build_segment(f"st{i}", {"v": (t["v"], S.INT, DIC), "f": (t["f"], S.INT, RAW)}) for i, t in enumerate(tables)]
    segs = [engine.ImmutableSegment(b) for b in bufs]
    try:
        masks = [t["f"] >= 0 for t in tables]
        exp, matched, scanned = ref.distinct(tables, masks, ["v"], [], 3)
        assert scanned == 3 and exp == [(10,), (30,), (40,)] and matched == sum(len(t["v"]) for t in tables[:3])
        rows, info = check(engine, "SELECT DISTINCT v FROM t WHERE f >= 0 LIMIT 3", segs, tables, masks)
        assert rows == [(10,), (30,), (40,)]
        full_rows, full_info = check(engine, "SELECT DISTINCT v FROM t WHERE f >= 0 LIMIT 1000", segs, tables, masks,
                                     oracle_q="SELECT v, COUNT(*) FROM t WHERE f >= 0 GROUP BY v LIMIT 1000", obufs=bufs)
        assert len(full_rows) == len({v for vs in vals for v in vs}) == 9
        assert info.startswith("jit-distinct-lds") and launches(info) < launches(full_info), (info, full_info)
        # LIMIT 1: the first stage answers
        rows, info1 = check(engine, "SELECT DISTINCT v FROM t WHERE f >= 0 LIMIT 1", segs, tables, masks)
        assert rows == [(40,)] and launches(info1) == 1
    finally:
        for s in segs:
            s.destroy()


# ------------------------------------------------------------------------------------------------ 5. re-execution, plans
def test_execute_again_and_prepared_plans(engine, mix):
    tables, segs, _ = mix
    masks = [t["f"] < 20 for t in tables]
    sql = "SELECT DISTINCT ri, ds FROM t WHERE f < 20 ORDER BY ri, ds DESC LIMIT 50"
    exp, matched, _ = ref.distinct(tables, masks, ["ri", "ds"], [("ri", True), ("ds", False)], 50)
    ex = engine.ServerQueryExecutor()
    res = ex.execute(sql, segs)
    first = res.rows()
    assert ref.same_rows(first, exp)
    assert "plan_cache" not in res.plan_timing()
    for _ in range(2):  # the bitmap is re-zeroed: the same rows, the same count
        res.execute_again()
        assert ref.same_rows(res.rows(), exp) and res.num_docs_matched() == matched
        assert res.last_kernel_ms() > 0 and res.algorithmic_bytes() > 0
    res.destroy()
    again = ex.execute(sql, segs)  # the re-issued query takes its prepared plan
    assert "plan_cache" in again.plan_timing() and ref.same_rows(again.rows(), exp)
    again.destroy()
    other = ex.execute(sql.replace("LIMIT 50", "LIMIT 49"), segs)  # another LIMIT: another plan
    assert "plan_cache" not in other.plan_timing() and ref.same_rows(other.rows(), exp[:49])
    other.destroy()
    # without ORDER BY: the staged scan again and again
    sql = "SELECT DISTINCT ts FROM t WHERE f < 20 LIMIT 4"
    exp, matched, _ = ref.distinct(tables, masks, ["ts"], [], 4)
    res = ex.execute(sql, segs)
    for _ in range(3):
        assert ref.same_rows(res.rows(), exp) and res.num_docs_matched() == matched
        res.execute_again()
    res.destroy()


# ------------------------------------------------------------------------------------------------ 6. dictionary only
def test_dictionary_only_path(engine, mix):
    tables, segs, _ = mix
    for col in ("di", "ts", "ds"):
        for order, asc in (("", True), (f" ORDER BY {col}", True), (f" ORDER BY {col} DESC", False)):
            for limit in (None, 3, 100000):
                sql = f"SELECT DISTINCT {col} FROM t{order}" + ("" if limit is None else f" LIMIT {limit}")
                exp, scanned = ref.dictionary_only(tables, col, asc, 10 if limit is None else limit)
                res = engine.ServerQueryExecutor().execute(sql, segs)
                try:
                    assert ref.same_rows(res.rows(), exp), sql
                    assert res.num_docs_matched() == scanned, sql
                    assert res.kernel_info() == "distinct-dictionary", sql
                    assert res.algorithmic_bytes() == 0
                finally:
                    res.destroy()
    # a raw column has no dictionary of its own: scanned
    rows, info = check(engine, "SELECT DISTINCT ri FROM t ORDER BY ri LIMIT 1000", segs, tables, none(tables))
    assert info.startswith("jit-distinct-")
    # LIMIT 0
    res = engine.ServerQueryExecutor().execute("SELECT DISTINCT di FROM t LIMIT 0", segs)
    assert res.rows() == [] and res.num_docs_matched() == 0
    res.destroy()


# ------------------------------------------------------------------------------------------------ 7. pinned by Pinot
def test_pinot_pinned_counts(engine):
    """InnerSegmentDistinctSingleValueQueriesTest: 6582 distinct column1 values, 21968 distinct (column1, column3) rows."""
    with open(os.path.join(helpers.GOLDEN, "sv_distinct_expected.json")) as f:
        cases = json.load(f)["cases"]
    bufs = helpers.sv_segment(name="sv_distinct")
    seg = engine.ImmutableSegment(bufs)
    data = np.load(os.path.join(helpers.GOLDEN, "test_data_sv.npz"), allow_pickle=False)
    table = {c: data[c] for c, _ in helpers.SV_COLUMNS}
    try:
        for case in cases:
            qc = parse_sql(case["sql"])
            res = engine.ServerQueryExecutor().execute(case["sql"], [seg])
            rows = res.rows()
            assert len(rows) == case["rows"], case["name"]
            assert {ref.row_ident(r) for r in rows} == ref.distinct_set([table], [None], qc.group_by), case["name"]
            keys = ", ".join(qc.group_by)
            _, groups = oracle.execute(f"SELECT {keys}, COUNT(*) FROM testTable GROUP BY {keys} LIMIT 1000000", [bufs])
            assert set(groups) == set(rows), case["name"]
            res.destroy()
        # with Pinot's filter, through the scan
        mask = ((table["column1"] > 100000000) & (table["column3"] >= 20000000) & (table["column3"] <= 1000000000)
                & (table["column5"] == "gFuH") & ((table["column6"] < 500000000) | ~np.isin(table["column11"], ["t", "P"]))
                & (table["daysSinceEpoch"] == 126164076))
        check(engine, "SELECT DISTINCT column1, column3 FROM testTable" + helpers.SV_FILTER + " ORDER BY column3 DESC LIMIT 1000000",
              [seg], [table], [mask],
              oracle_q="SELECT column1, column3, COUNT(*) FROM testTable" + helpers.SV_FILTER + " GROUP BY column1, column3 LIMIT 1000000",
              obufs=[bufs])
    finally:
        seg.destroy()


def test_result_calls_refused_like_a_selection(engine, mix):
    import ctypes as C
    import torch
    tables, segs, _ = mix
    ex = engine.ServerQueryExecutor()
    sql = "SELECT DISTINCT ri FROM t WHERE f < 5 ORDER BY ri LIMIT 5"
    res = ex.execute(sql, segs)
    L, h = _lib.lib(), res._h
    try:
        n32, n64 = C.c_int32(), C.c_int64()
        assert L.pinot_amd_result_num_groups(h, C.byref(n64)) == 0 and n64.value == 5
        assert L.pinot_amd_result_fetch(h, 4, (C.c_int64 * 4)(), None, None, C.byref(n64)) == -5       # EOVERFLOW
        assert L.pinot_amd_result_fetch_intermediate(h, 8, (C.c_double * 64)(), C.byref(n64)) == -1
        assert L.pinot_amd_result_fetch_distinct_values(h, 0, 0, None, None, C.byref(n64)) == -1
        assert L.pinot_amd_result_fetch_value_counts(h, 0, 0, None, None, None, C.byref(n64)) == -1
        assert L.pinot_amd_result_accumulators(h, C.byref(n32), C.byref(n64), None, None) == -2
        assert L.pinot_amd_result_export_groups(h, None, None, 0, C.byref(n32), C.byref(n32), C.byref(n64), None) == -2
        assert b"DISTINCT" in L.pinot_amd_last_error()
        assert L.pinot_amd_result_merge_groups(h, None, None, 0, None) == -2
        assert b"DISTINCT" in L.pinot_amd_last_error()
        word = C.c_void_p()
        assert L.pinot_amd_result_check_word(h, C.byref(word)) == 0 and word.value
        assert int(torch.as_tensor(engine._DeviceWord(word.value), device="cuda").item()) == 0     # reads 0
        res.execute_again()
        assert int(torch.as_tensor(engine._DeviceWord(word.value), device="cuda").item()) == 0
        # the selection calls refuse a distinct result
        assert L.pinot_amd_result_num_rows(h, C.byref(n64)) == -1
        # no key space, no cross-rank merge
        with pytest.raises(_lib.PinotAmdError) as e:
            ex.execute(sql, segs, key_space={})
        assert "key_space" in str(e.value)
        from pinot_amd import dist
        with pytest.raises(ValueError) as e:
            dist.merge_result(res)
        assert "DISTINCT" in str(e.value)
    finally:
        res.destroy()
