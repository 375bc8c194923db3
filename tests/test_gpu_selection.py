"""Selection queries on the device (SELECT columns [ORDER BY ...] LIMIT n [OFFSET m]): the top-K scan, the candidate
sort, the gather by docId and the combine. Every case compares rows() and origins() exactly with tests/selection_ref.py
(a per-doc numpy restatement: boolean masks and one lexsort, ties by ascending (segment, docId))."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import helpers
import selection_ref
from pinot_amd import _lib
from pinot_amd import segment as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from pinot_amd import engine as E
    return E


def stage(engine, tables, specs, prefix):
    """tables: per segment a dict column -> numpy array; specs: column -> (stored type, build options)."""
    segs = []
    for i, t in enumerate(tables):
        cols = {c: (t[c].astype(object) if specs[c][0] == S.STRING else t[c], specs[c][0], specs[c][1]) for c in specs}
        segs.append(engine.ImmutableSegment(S.build_segment(f"{prefix}_{i}", cols)))
    return segs


def check(engine, sql, segs, tables, masks, columns, order_by, limit, offset=0, executor=None):
    """Run `sql` and compare with the reference; returns (rows, kernel_info)."""
    ex = executor or engine.ServerQueryExecutor()
    res = ex.execute(sql, segs)
    try:
        exp_rows, exp_origins, exp_matched = selection_ref.select(tables, masks, columns, order_by, limit, offset)
        rows, origins = res.rows(), res.origins()
        assert origins == exp_origins, (sql, origins[:8], exp_origins[:8])
        assert selection_ref.same_rows(rows, exp_rows), (sql, rows[:4], exp_rows[:4])
        assert res.num_docs_matched() == exp_matched, sql
        assert res.columns == list(columns)
        return rows, res.kernel_info()
    finally:
        res.destroy()


# ------------------------------------------------------------------------------------------------ 1. golden
@pytest.fixture(scope="module")
def sv(engine):
    data = np.load(os.path.join(helpers.GOLDEN, "test_data_sv.npz"), allow_pickle=False)
    table = {c: data[c] for c, _ in helpers.SV_COLUMNS}
    segs = [engine.ImmutableSegment(helpers.sv_segment(name=f"sv_sel_{i}")) for i in range(4)]
    mask = ((table["column1"] > 100000000) & (table["column3"] >= 20000000) & (table["column3"] <= 1000000000)
            & (table["column5"] == "gFuH") & ((table["column6"] < 500000000) | ~np.isin(table["column11"], ["t", "P"]))
            & (table["daysSinceEpoch"] == 126164076))
    yield segs, table, mask
    for s in segs:
        s.destroy()


def test_golden_four_copies(engine, sv):
    """Pinot's own asserted values (InnerSegmentSelectionSingleValueQueriesTest) over four copies of its segment:
    with ORDER BY each of Pinot's rows comes four times (ties by segment index), so its row 9 is rows 36..39 of
    LIMIT 40, and every matching doc of every copy is counted; without ORDER BY the first segment answers."""
    segs, table, mask = sv
    with open(os.path.join(helpers.GOLDEN, "sv_selection_expected.json")) as f:
        cases = json.load(f)["cases"]
    star = sorted(table, key=lambda n: n.encode("utf-16-be"))
    for case in cases:
        cols = star if case["select"] == ["*"] else case["select"]
        order = [tuple(o) for o in case["order_by"]]
        limit = case["limit"] * 4 if order else case["limit"]
        sql = "SELECT " + ", ".join(case["select"]) + " FROM testTable" + (helpers.SV_FILTER if case["filtered"] else "")
        if order:
            sql += " ORDER BY " + ", ".join(f"{c}{'' if asc else ' DESC'}" for c, asc in order)
        sql += f" LIMIT {limit}"
        res = engine.ServerQueryExecutor().execute(sql, segs)
        try:
            rows, origins = res.rows(), res.origins()
            exp_rows, exp_origins, exp_matched = selection_ref.select(
                [table] * 4, [mask if case["filtered"] else None] * 4, cols, order, limit)
            assert origins == exp_origins, case["name"]
            assert selection_ref.same_rows(rows, exp_rows), case["name"]
            picks = range(case["row"] * 4, case["row"] * 4 + 4) if order else [case["row"]]
            for i in picks:
                row = dict(zip(cols, rows[i]))
                for c, v in case["values"].items():
                    assert row[c] == v, (case["name"], i, c, row[c], v)
            want = case["docs_matched"] * 4 if order else case["docs_matched"]
            assert res.num_docs_matched() == want == exp_matched, case["name"]
        finally:
            res.destroy()


# ------------------------------------------------------------------------------------------------ 2. tile edges
@pytest.fixture(scope="module")
def edges(engine):
    rng = np.random.default_rng(7)
    tables = []
    for n in (1, 3, 0, 1023, 1024, 1025, 4097):
        tables.append({"v": rng.integers(-500, 500, n).astype(np.int32),           # many duplicates: ties
                       "f": rng.integers(0, 100, n).astype(np.int32),
                       "d": (rng.integers(0, 9, n) * 11).astype(np.int32)})
    specs = {"v": (S.INT, {"dictionary": False}), "f": (S.INT, {"dictionary": False}), "d": (S.INT, {})}
    segs = stage(engine, tables, specs, "edge")
    yield segs, tables
    for s in segs:
        s.destroy()


@pytest.mark.parametrize("desc", [False, True])
def test_tile_edges(engine, edges, desc):
    segs, tables = edges
    masks = [t["f"] < 70 for t in tables]
    matched = int(sum(m.sum() for m in masks))
    for k in (1, 10, matched + 1):
        sql = f"SELECT v, d FROM t WHERE f < 70 ORDER BY v{' DESC' if desc else ''} LIMIT {k}"
        rows, info = check(engine, sql, segs, tables, masks, ["v", "d"], [("v", not desc)], k)
        assert len(rows) == min(k, matched)
        assert info.startswith("jit-topk-sort" if k > 1024 else "jit-topk")
    # no filter, every doc of every segment (the empty one included)
    total = sum(len(t["v"]) for t in tables)
    check(engine, f"SELECT d, v FROM t ORDER BY v{' DESC' if desc else ''}, d LIMIT 5 OFFSET 1000", segs, tables, None,
          ["d", "v"], [("v", not desc), ("d", True)], 5, 1000)
    assert total == 1 + 3 + 1023 + 1024 + 1025 + 4097


# ------------------------------------------------------------------------------------------------ 3. per-segment keys
SPECIALS = [np.nan, -0.0, 0.0, np.inf, -np.inf, 1.5, -1.5]


@pytest.fixture(scope="module")
def mixed(engine):
    rng = np.random.default_rng(11)
    words = [f"w{i:03d}" for i in range(400)] + ["Zeta", "alpha", "été", "\U0001F600x"]
    tables = []
    # the same values get different dictIds and bit widths per segment: dictionaries of 40, 600 and 5 values
    for n, (lo, hi), nwords in ((5000, (100, 140), 30), (4999, (0, 600), 404), (5003, (120, 125), 7)):
        dbl = rng.normal(0, 10, n)
        dbl[rng.integers(0, n, 60)] = rng.choice(SPECIALS, 60)
        flt = rng.normal(0, 10, n).astype(np.float32)
        flt[rng.integers(0, n, 60)] = rng.choice(SPECIALS, 60).astype(np.float32)
        tables.append({
            "lc": rng.integers(0, 3, n).astype(np.int32),                            # low cardinality: most rows tie
            "di": rng.integers(lo, hi, n).astype(np.int32),
            "ds": np.array(rng.choice(words[-nwords:], n)),
            "ts": np.sort(rng.integers(1000 * len(tables), 1000 * len(tables) + 50, n)).astype(np.int32),
            "rl": rng.integers(-(1 << 62), 1 << 62, n).astype(np.int64),
            "rl2": rng.integers(-3, 3, n).astype(np.int64),
            "rl3": rng.integers(-3, 3, n).astype(np.int64),
            "rd": dbl, "rf": flt})
    specs = {"lc": (S.INT, {}), "di": (S.INT, {}), "ds": (S.STRING, {}), "ts": (S.INT, {}),
             "rl": (S.LONG, {"dictionary": False}), "rl2": (S.LONG, {"dictionary": False}),
             "rl3": (S.LONG, {"dictionary": False}), "rd": (S.DOUBLE, {"dictionary": False}),
             "rf": (S.FLOAT, {"dictionary": False})}
    segs = stage(engine, tables, specs, "mixed")
    yield segs, tables
    for s in segs:
        s.destroy()


MIXED_ORDERS = [
    [("di", True)],                        # one dictionary column whose dictionaries differ per segment
    [("lc", True), ("rd", False)],         # ties on the first key; raw DOUBLE DESC with NaN, +-0.0, +-inf
    [("ds", False), ("di", True)],         # dictionary STRING DESC (UTF-16 order), then dictionary INT
    [("ts", True), ("rf", False)],         # a sorted column, then raw FLOAT DESC
    [("rl", False)],                       # raw LONG with negatives
    [("di", False), ("rl", True)],         # 32 + 64 bits: two key words, a 64-bit field across them
    [("rd", True), ("rl2", False)],        # 128 bits
    [("lc", False), ("rl2", True), ("ts", False)],
]


@pytest.mark.parametrize("order", MIXED_ORDERS, ids=lambda o: "_".join(f"{c}{'' if a else '-'}" for c, a in o))
def test_per_segment_keys(engine, mixed, order):
    segs, tables = mixed
    cols = ["rf", "ds", "rl", "lc", "rd", "di", "ts"]
    masks = [(t["rl2"] >= -2) & (t["di"] != 121) for t in tables]
    ob = ", ".join(f"{c}{'' if a else ' DESC'}" for c, a in order)
    for limit, offset in ((25, 0), (3, 40)):
        sql = f"SELECT {', '.join(cols)} FROM t WHERE rl2 >= -2 AND di <> 121 ORDER BY {ob} LIMIT {limit} OFFSET {offset}"
        _, info = check(engine, sql, segs, tables, masks, cols, order, limit, offset)
        assert info.startswith("jit-topk") and " x" in info, info  # differing dictionary widths: several launches


def test_three_long_order_by_unsupported(engine, mixed):
    segs, _ = mixed
    with pytest.raises(_lib.PinotAmdError, match=r"\(-2\)"):
        engine.ServerQueryExecutor().execute("SELECT lc FROM t ORDER BY rl, rl2, rl3 LIMIT 5", segs)


# ------------------------------------------------------------------------------------------------ 4. worst case
@pytest.fixture(scope="module")
def ascending(engine):
    tables = [{"a": (np.arange(20000) * 3 + 7 * i).astype(np.int32), "b": (np.arange(20000) % 17).astype(np.int32)}
              for i in range(3)]
    segs = stage(engine, tables, {"a": (S.INT, {"dictionary": False}), "b": (S.INT, {})}, "asc")
    yield segs, tables
    for s in segs:
        s.destroy()


def test_worst_case_every_doc_beats_the_threshold(engine, ascending, monkeypatch):
    """ORDER BY a DESC over a column ascending in docId: every doc beats the threshold, so every step appends all its
    docs and the buffer is reduced again and again; two blocks walk all three segments (segment changes inside a
    block) with the smallest buffer (512 records: the LDS bound is 256 rows)."""
    segs, tables = ascending
    monkeypatch.setenv("PINOT_AMD_TOPK_BLOCKS", "2")
    monkeypatch.setenv("PINOT_AMD_TOPK_LDS_ROWS", "512")
    for k, plan in ((1, "jit-topk"), (256, "jit-topk"), (257, "jit-topk-sort")):
        _, info = check(engine, f"SELECT a, b FROM t ORDER BY a DESC LIMIT {k}", segs, tables, None, ["a", "b"],
                        [("a", False)], k)
        assert info == plan, (k, info)
    _, info = check(engine, "SELECT b, a FROM t WHERE b <> 3 ORDER BY b DESC, a DESC LIMIT 200 OFFSET 56", segs, tables,
                    [t["b"] != 3 for t in tables], ["b", "a"], [("b", False), ("a", False)], 200, 56)
    assert info == "jit-topk"
    monkeypatch.setenv("PINOT_AMD_TOPK_SORT_MAX_BYTES", "4096")
    with pytest.raises(_lib.PinotAmdError, match=r"\(-2\).*PINOT_AMD_TOPK_SORT_MAX_BYTES"):
        engine.ServerQueryExecutor().execute("SELECT a FROM t ORDER BY a DESC LIMIT 300", segs)


# ------------------------------------------------------------------------------------------------ 5. no ORDER BY
@pytest.fixture(scope="module")
def eight(engine):
    rng = np.random.default_rng(3)
    tables = [{"x": rng.integers(0, 10, 300 + i).astype(np.int32), "y": rng.integers(0, 1 << 40, 300 + i).astype(np.int64)}
              for i in range(8)]
    segs = stage(engine, tables, {"x": (S.INT, {"dictionary": False}), "y": (S.LONG, {"dictionary": False})}, "eight")
    yield segs, tables
    for s in segs:
        s.destroy()


def test_no_order_by(engine, eight):
    segs, tables = eight
    masks = [t["x"] == 4 for t in tables]
    first, total = int(masks[0].sum()), int(sum(m.sum() for m in masks))
    assert first >= 6
    runs = {}
    for limit, offset in ((5, 0), (first - 2, 4), (total + 10, 0), (0, 0), (0, 7)):
        rows, info = check(engine, f"SELECT y, x FROM t WHERE x = 4 LIMIT {limit} OFFSET {offset}", segs, tables, masks,
                           ["y", "x"], [], limit, offset)
        assert len(rows) == min(limit + offset, total)   # num_docs_matched == the rows: checked against the reference
        runs[(limit, offset)] = info
    # segments launch in groups of 1, 2, 4, 1: LIMIT 5 is answered by the first group, the later ones never launch
    assert runs[(5, 0)] == "jit-topk"
    assert runs[(first - 2, 4)] == "jit-topk x2"
    assert runs[(total + 10, 0)] == "jit-topk x4"
    assert runs[(0, 0)] == "jit-topk x0"
    rows, _ = check(engine, "SELECT x FROM t WHERE x = 77 LIMIT 5", segs, tables, [t["x"] == 77 for t in tables], ["x"],
                    [], 5)
    assert rows == []
    # LIMIT 0 ignores the ORDER BY
    check(engine, "SELECT x FROM t ORDER BY y LIMIT 0", segs, tables, None, ["x"], [("y", True)], 0)


# ------------------------------------------------------------------------------------------------ 6. filters
@pytest.mark.parametrize("policy", ["always", "never"])
def test_inverted_index_leaf(engine, sv, monkeypatch, policy):
    segs, table, _ = sv
    monkeypatch.setenv("PINOT_AMD_INV_POLICY", policy)
    mask = np.isin(table["column11"], ["t", "P"]) & (table["column6"] > 1000000)
    check(engine, "SELECT column1, column11 FROM testTable WHERE column11 IN ('t', 'P') AND column6 > 1000000 "
                  "ORDER BY column1 DESC, column6 LIMIT 12", segs[:2], [table] * 2, [mask] * 2, ["column1", "column11"],
          [("column1", False), ("column6", True)], 12)


def test_packed_twin_and_raw_bytes_agree(engine, ascending, monkeypatch):
    segs, tables = ascending
    sql = "SELECT a FROM t WHERE a > 100 ORDER BY a LIMIT 20"
    masks = [t["a"] > 100 for t in tables]
    res = engine.ServerQueryExecutor().execute(sql, segs)
    assert "a:" in res.packed_info()   # the ORDER BY column streams through its packed twin
    res.destroy()
    rows_default, _ = check(engine, sql, segs, tables, masks, ["a"], [("a", True)], 20)
    monkeypatch.setenv("PINOT_AMD_PACKED", "0")
    res = engine.ServerQueryExecutor().execute(sql, segs)
    assert res.packed_info() == ""
    res.destroy()
    rows_raw, _ = check(engine, sql, segs, tables, masks, ["a"], [("a", True)], 20)
    assert rows_raw == rows_default


# ------------------------------------------------------------------------------------------------ 7. plans
def test_plans_and_result_calls(engine, eight):
    segs, tables = eight
    ex = engine.ServerQueryExecutor()
    sql = "SELECT x, y FROM t WHERE x > 2 ORDER BY y DESC LIMIT 9 OFFSET 2"
    res = ex.execute(sql, segs)
    rows, origins = res.rows(), res.origins()
    res.execute_again()
    assert res.rows() == rows and res.origins() == origins
    assert res.last_kernel_ms() > 0 and res.algorithmic_bytes() > 0
    # the group-by calls on a selection result
    L, h = _lib.lib(), res._h
    n64, n32, d = C.c_int64(), C.c_int32(), C.c_double()
    k64 = (C.c_int64 * 4)()
    assert L.pinot_amd_result_num_groups(h, C.byref(n64)) == -1
    assert L.pinot_amd_result_fetch(h, 4, k64, (C.c_double * 4)(), None, C.byref(n64)) == -1
    assert L.pinot_amd_result_fetch_intermediate(h, 4, (C.c_double * 8)(), C.byref(n64)) == -1
    assert L.pinot_amd_result_fetch_distinct_values(h, 0, 0, None, None, C.byref(n64)) == -1
    assert L.pinot_amd_result_fetch_value_counts(h, 0, 0, None, None, None, C.byref(n64)) == -1
    assert L.pinot_amd_result_accumulators(h, C.byref(n32), C.byref(n64), None, None) == -2
    assert L.pinot_amd_result_export_groups(h, None, None, 0, C.byref(n32), C.byref(n32), C.byref(n64), None) == -2
    assert L.pinot_amd_result_merge_groups(h, None, None, 0, None) == -2
    assert L.pinot_amd_result_fetch_rows(h, 3, None, None, None, C.byref(n64)) == -5   # EOVERFLOW
    word = C.c_void_p()
    assert L.pinot_amd_result_check_word(h, C.byref(word)) == 0 and word.value
    import torch
    assert int(torch.as_tensor(engine._DeviceWord(word.value), device="cuda").item()) == 0
    assert L.pinot_amd_result_selection_num_columns(h, C.byref(n32)) == 0 and n32.value == 2
    res.destroy()
    # re-issued: the prepared plan answers the same
    again = ex.execute(sql, segs)
    assert again.rows() == rows and again.origins() == origins
    again.destroy()
    # queries differing only in LIMIT, OFFSET or direction are other plans: each answers as the reference says
    masks = [t["x"] > 2 for t in tables]
    for limit, offset, asc in ((9, 3, False), (8, 2, False), (9, 2, True), (9, 2, False)):
        check(engine, f"SELECT x, y FROM t WHERE x > 2 ORDER BY y{'' if asc else ' DESC'} LIMIT {limit} OFFSET {offset}",
              segs, tables, masks, ["x", "y"], [("y", asc)], limit, offset, executor=ex)
    # a selection query takes no key space, and the selection calls refuse an aggregation result
    with pytest.raises(_lib.PinotAmdError):
        ex.execute(sql, segs, key_space={})
    agg = ex.execute("SELECT COUNT(*) FROM t", segs)
    assert L.pinot_amd_result_num_rows(agg._h, C.byref(n64)) == -1
    agg.destroy()
