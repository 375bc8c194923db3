"""GROUP BY time buckets on the device (pinot_amd_query_add_group_by_transform): dateTrunc / timeConvert /
dateTimeConvert keys over raw LONG, raw INT, dictionary and sorted source columns, alone and mixed in one batch.

The oracle cannot evaluate transforms, so parity is against the oracle's GROUP BY k where k is a raw LONG column the
test materialised from the numpy restatement (time_transform_ref.py) on the same docs; Pinot's own asserted values
(tests/golden/time_transforms_expected.json) are also checked on the device directly. Integers compare exactly,
double sums within the project's 1e-12 relative rule (assert_same_groups)."""
import collections
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle
import time_transform_ref as R
import value_aggs_ref as vref
from helpers import GOLDEN
from oracle_reduce import server_table
from pinot_amd import segment as S
from pinot_amd.query import TRUNC_UNITS, canonical_key, key_transform, parse_sql

pytestmark = pytest.mark.gpu

from test_gpu_parity import assert_same_groups  # noqa: E402

DAY = 86_400_000
SIZES = [1, 4099, 5000, 0]
EINVAL, EUNSUPPORTED = -1, -2

with open(os.path.join(GOLDEN, "time_transforms_expected.json")) as f:
    EXPECTED = json.load(f)


@pytest.fixture(scope="module")
def engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from pinot_amd import engine as E
    return E


def draw_ts(rng, n):
    """Epoch milliseconds: most within a few days of 1970-01-01 on both sides (many docs per hour, every segment
    draws from the same hours), the rest anywhere in 1965..2030 (months, quarters and years on both sides of 0)."""
    near = rng.integers(-3 * DAY, 5 * DAY, n)
    far = rng.integers(-5 * 365 * DAY, 61 * 365 * DAY, n)
    return np.where(rng.random(n) < 0.7, near, far).astype(np.int64)


@pytest.fixture(scope="module")
def data(engine):
    """(per-segment column arrays, staged segments). ts: raw LONG ms; tsi: raw INT seconds; tsd: dictionary LONG;
    tss: sorted dictionary LONG; tsm: raw / dictionary / sorted / raw by segment."""
    rng = np.random.default_rng(20260)
    arrays, segs = [], []
    for i, n in enumerate(SIZES):
        ts = np.array([-1], dtype=np.int64) if n == 1 else draw_ts(rng, n)
        a = {"ts": ts, "tsi": (ts // 1000).astype(np.int32), "tsd": ts, "tss": np.sort(ts),
             "tsm": np.sort(ts) if i == 2 else ts,
             "d": (rng.integers(0, 5, n) * 3 + 1).astype(np.int32), "x": rng.integers(-10 ** 6, 10 ** 6, n).astype(np.int32),
             "dbl": rng.normal(0, 1e3, n), "u": rng.integers(0, 50, n).astype(np.int32)}
        raw, dic = {"dictionary": False}, {"detect_sorted": False}
        mixed = [raw, dic, {}, raw][i]
        bufs = S.build_segment(f"tb{i}", {
            "ts": (a["ts"], S.LONG, raw), "tsi": (a["tsi"], S.INT, raw), "tsd": (a["tsd"], S.LONG, dic),
            "tss": (a["tss"], S.LONG, {}), "tsm": (a["tsm"], S.LONG, mixed), "d": (a["d"], S.INT, dic),
            "x": (a["x"], S.INT, raw), "dbl": (a["dbl"], S.DOUBLE, raw), "u": (a["u"], S.INT, dic)})
        assert bufs.columns["tss"].encoding == "SORTED" and bufs.columns["tsd"].encoding == "FIXED_BIT"
        assert bufs.columns["tsm"].encoding == ["RAW", "FIXED_BIT", "SORTED", "RAW"][i]
        arrays.append(a)
        segs.append(engine.ImmutableSegment(bufs))
    return arrays, segs


def materialised(arrays, col, kt, extra=()):
    """The oracle's segments: k = the restated transform of `col` as a raw LONG column, plus the plain columns."""
    out = []
    for i, a in enumerate(arrays):
        cols = {"k": (R.evaluate(kt, a[col]) if len(a[col]) else np.zeros(0, np.int64), S.LONG, {"dictionary": False})}
        for c in ("d", "x", "dbl", "u") + tuple(extra):
            t = S.DOUBLE if c == "dbl" else S.INT
            cols[c] = (a[c], t, {"dictionary": False} if c in ("x", "dbl") else {"detect_sorted": False})
        out.append(S.build_segment(f"ok{i}", cols))
    return out


# Every dateTrunc unit, one with another output unit, timeConvert across three unit pairs (down, down, up) and
# dateTimeConvert with sizes != 1 and with a granularity of size 1, over column {c} whose values are in unit {U}
EXPRS = [f"dateTrunc('{u}', {{c}}, '{{U}}')" for u in TRUNC_UNITS] + [
    "DATETRUNC('day', {c}, '{U}', 'UTC', 'HOURS')",
    "timeConvert({c}, '{U}', 'HOURS')", "timeConvert({c}, '{U}', 'DAYS')", "timeConvert({c}, '{U}', 'MICROSECONDS')",
    "dateTimeConvert({c}, '1:{U}:EPOCH', '1:MINUTES:EPOCH', '15:MINUTES')",
    "DATETIMECONVERT({c}, '3:{U}:EPOCH', '2:HOURS:EPOCH', '4:HOURS')",
    "dateTimeConvert({c}, '1:{U}:EPOCH', '1:{U}:EPOCH', '1:DAYS')"]
# the source encodings: raw LONG, raw INT, dictionary, sorted, and raw / dictionary / sorted mixed in one batch
SOURCES = [("ts", "MILLISECONDS"), ("tsi", "SECONDS"), ("tsd", "MILLISECONDS"), ("tss", "MILLISECONDS"),
           ("tsm", "MILLISECONDS")]


PARITY = ("SELECT {k}, d, COUNT(*), SUM(x), MIN(x), MAX(x), AVG(x), SUM(dbl) FROM t "
          "WHERE x BETWEEN -600000 AND 700000 GROUP BY {k}, d LIMIT 100000")


def check_parity(engine, arrays, segs, which, col, expr):
    kt = key_transform(expr)
    q = PARITY.format(k=expr)
    res = engine.ServerQueryExecutor().execute(q, [segs[i] for i in which])
    nm, og = oracle.execute(PARITY.format(k="k"), materialised([arrays[i] for i in which], col, kt))
    assert res.num_docs_matched() == nm, expr
    got = res.groups()
    assert all(type(k[0]) is int for k in got), expr   # the key is a LONG
    assert_same_groups(got, og, {5})
    res.destroy()


# ------------------------------------------------------------------------------- 1. Pinot's expected values
def test_pinot_expected_values_on_the_device(engine):
    """A raw LONG column holds every input of the golden tuples, input j repeated j + 1 times; each golden
    (function, arguments) groups the docs holding its inputs: the keys and counts are the expected values'."""
    cases = EXPECTED["datetrunc"] + EXPECTED["datetimeconvert"]
    inputs = sorted({c["input"] for c in cases})
    g = np.concatenate([np.full(j + 1, v, dtype=np.int64) for j, v in enumerate(inputs)])
    np.random.default_rng(3).shuffle(g)
    seg = engine.ImmutableSegment(S.build_segment("golden", {"ts": (g, S.LONG, {"dictionary": False})}))
    by_text = collections.OrderedDict()
    for c in cases:
        by_text.setdefault(key_transform(c["expr"]).text, []).append(c)
    assert len(by_text) >= 30
    for text, cs in by_text.items():
        want = collections.Counter()
        for v in {c["input"] for c in cs}:
            (e,) = {c["expected"] for c in cs if c["input"] == v}
            want[e] += inputs.index(v) + 1
        ins = ", ".join(str(v) for v in sorted({c["input"] for c in cs}))
        res = engine.ServerQueryExecutor().execute(
            f"SELECT {cs[0]['expr']}, COUNT(*) FROM t WHERE ts IN ({ins}) GROUP BY {text} LIMIT 100", [seg])
        assert {k[0]: v[0] for k, v in res.groups().items()} == dict(want), text
        res.destroy()


# ------------------------------------------------------------------------------- 2. parity with the oracle
@pytest.mark.parametrize("expr", EXPRS, ids=[e.split(",")[0].replace("{c}", "").replace("'", "").replace("(", "-")
                                            + f"-{i}" for i, e in enumerate(EXPRS)])
def test_parity_with_oracle_over_materialised_column(engine, data, expr):
    """One transform over every source encoding (each query shape compiles its scan once: about a second)."""
    arrays, segs = data
    for col, unit in SOURCES:
        check_parity(engine, arrays, segs, range(len(SIZES)), col, expr.format(c=col, U=unit))


@pytest.mark.parametrize("which", [[0], [3], [0, 3], [1]], ids=["one_doc", "empty", "one_doc_and_empty", "4099_docs"])
def test_parity_small_batches(engine, data, which):
    """A 1-doc segment, an empty one and a doc count that is no multiple of 4 or 1024, each on its own, through
    every encoding's route."""
    arrays, segs = data
    for col in ("ts", "tsd", "tss"):
        check_parity(engine, arrays, segs, which, col, f"dateTrunc('hour', {col})")
    check_parity(engine, arrays, segs, which, "tsi", "dateTimeConvert(tsi, '1:SECONDS:EPOCH', '1:HOURS:EPOCH', '2:HOURS')")


# ------------------------------------------------------------------------------- 3. composition
def test_order_by_key_desc_limit_through_the_server_table(engine, data):
    arrays, segs = data
    q = ("SET minServerGroupTrimSize = 4; SELECT {k}, COUNT(*), SUM(x) FROM t WHERE d < 10 GROUP BY {k} "
         "ORDER BY {k} DESC LIMIT 5")
    for expr, col in (("dateTrunc('hour', ts)", "ts"), ("timeConvert(tsd, 'MILLISECONDS', 'DAYS')", "tsd")):
        qc = parse_sql(q.format(k=expr))
        assert qc.safe_trim()
        got = engine.ServerQueryExecutor(server_trim=True).execute(qc, segs).groups()
        qk = q.format(k="k")
        _, full = oracle.execute(qk, materialised(arrays, col, key_transform(expr)))
        exp = server_table(oracle.parse_sql(qk), full)
        assert len(exp) == 5 < len(full)
        assert_same_groups(got, exp)
        assert list(got) == list(exp)
    # unsafe trim: ordered by an aggregation, the key second
    q2 = ("SET minServerGroupTrimSize = 8; SELECT {k}, d, MAX(x) FROM t GROUP BY d, {k} ORDER BY MAX(x) DESC, {k} LIMIT 3")
    expr = "dateTrunc('month', tss)"
    got = engine.ServerQueryExecutor(server_trim=True).execute(q2.format(k=expr), segs).groups()
    _, full = oracle.execute(q2.format(k="k"), materialised(arrays, "tss", key_transform(expr)))
    exp = server_table(oracle.parse_sql(q2.format(k="k")), full)
    assert len(got) == len(exp) == 15
    assert_same_groups(got, exp)
    assert list(got) == list(exp)


@pytest.mark.parametrize("plan", ["auto", "hash"])
def test_num_groups_limit_below_the_bucket_count(engine, data, monkeypatch, plan):
    if plan == "hash":
        monkeypatch.setenv("PINOT_AMD_GROUP_PLAN", "hash")
    arrays, segs = data
    expr = "dateTrunc('hour', ts)"
    q = "SET numGroupsLimit = 40; SELECT {k}, COUNT(*), SUM(x) FROM t GROUP BY {k} LIMIT 100000"
    res = engine.ServerQueryExecutor().execute(q.format(k=expr), segs)
    stats = {}
    nm, og = oracle.execute(q.format(k="k"), materialised(arrays, "ts", key_transform(expr)), stats=stats)
    assert stats["num_groups_limit_reached"] and res.num_groups_limit_reached()
    assert len(np.unique(R.date_trunc("hour", arrays[1]["ts"]))) > 40
    assert_same_groups(res.groups(), og)


@pytest.mark.parametrize("col", ["ts", "tsm"])
def test_value_set_aggregations_with_a_transformed_key(engine, data, col):
    arrays, segs = data
    expr = f"dateTrunc('day', {col})"
    q = "SELECT {k}, DISTINCTCOUNT(u), PERCENTILE50(x), DISTINCTSUM(u), COUNT(*) FROM t WHERE d < 10 GROUP BY {k} LIMIT 100000"
    kt = key_transform(expr)
    np_segs = [dict(a, k=R.evaluate(kt, a[col]) if len(a[col]) else np.zeros(0, np.int64)) for a in arrays]
    qk = parse_sql(q.format(k="k"))
    exp = vref.reference_rows(qk, np_segs, lambda s: s["d"] < 10)
    for ex in (engine.ServerQueryExecutor(distinct_count="native"), engine.ServerQueryExecutor()):
        res = ex.execute(q.format(k=expr), segs)
        got = {canonical_key(r[:1]): list(r[1:]) for r in res.rows()}
        assert set(got) == set(exp) and len(got) > 8
        for k, e in exp.items():
            for a, gv, ev in zip(qk.aggregations, got[k], e):
                assert vref.same(gv, ev, a.func, False), (expr, k, a.func, gv, ev)
        res.destroy()


# ------------------------------------------------------------------------------- 4. the hot path is the narrow twin
def test_hot_path_is_the_narrow_twin(engine, data):
    """The same query over segments whose buckets are an ordinary dictionary-encoded LONG column: the same plan, the
    same bytes."""
    arrays, segs = data
    expr = "dateTrunc('hour', ts)"
    kt = key_transform(expr)
    staged = []
    for i, a in enumerate(arrays):
        k = R.evaluate(kt, a["ts"]) if len(a["ts"]) else np.zeros(0, np.int64)
        staged.append(engine.ImmutableSegment(S.build_segment(f"kd{i}", {
            "kd": (k, S.LONG, {"detect_sorted": False}), "d": (a["d"], S.INT, {"detect_sorted": False}),
            "x": (a["x"], S.INT, {"dictionary": False})})))
    q = "SELECT {k}, COUNT(*), SUM(x), MAX(x) FROM t WHERE d < 10 GROUP BY {k} LIMIT 100000"
    twin = engine.ServerQueryExecutor().execute(q.format(k=expr), segs)
    plain = engine.ServerQueryExecutor().execute(q.format(k="kd"), staged)
    assert twin.groups() == plain.groups() and len(plain.groups()) > 100
    assert twin.kernel_info() == plain.kernel_info()
    assert twin.algorithmic_bytes() == plain.algorithmic_bytes()
    # 8-bit-or-so dictIds instead of the 8-byte timestamps
    raw = engine.ServerQueryExecutor().execute("SELECT COUNT(*), SUM(x), MAX(ts) FROM t WHERE d < 10", segs)
    assert twin.algorithmic_bytes() < raw.algorithmic_bytes()


# ------------------------------------------------------------------------------- 5. identity and reuse
def counts_by(arrays, col, kt):
    c = collections.Counter()
    for a in arrays:
        if len(a[col]):
            c.update(R.evaluate(kt, a[col]).tolist())
    return dict(c)


def test_queries_differing_only_in_the_unit_share_no_plan(engine, data):
    arrays, segs = data
    qs = {u: f"SELECT dateTrunc('{u}', tsd), COUNT(*) FROM t GROUP BY dateTrunc('{u}', tsd) LIMIT 100000"
          for u in ("hour", "day")}
    exp = {u: counts_by(arrays, "tsd", key_transform(f"dateTrunc('{u}', tsd)")) for u in qs}
    assert exp["hour"] != exp["day"]
    for _ in range(3):   # executed, destroyed (the plan goes back to the prepared plans) and re-executed alternately
        for u, q in qs.items():
            res = engine.ServerQueryExecutor().execute(q, segs)
            assert {k[0]: v[0] for k, v in res.groups().items()} == exp[u], u
            res.destroy()


def test_twins_are_built_once_per_column_and_spec(engine, data):
    arrays, segs = data
    q = "SELECT {k}, COUNT(*) FROM t GROUP BY {k} LIMIT 100000"
    gran = "dateTimeConvert(tss, '1:MILLISECONDS:EPOCH', '1:MILLISECONDS:EPOCH', '{g}')"
    before = [s.device_bytes() for s in segs]
    first = engine.ServerQueryExecutor().execute(q.format(k=gran.format(g="6:HOURS")), segs)
    assert "raw_keys" in first.plan_timing()
    built = [s.device_bytes() for s in segs]
    assert all(b > a for a, b in zip(before, built))   # the twins count (the empty segment's too: its padding)
    again = engine.ServerQueryExecutor().execute(q.format(k=gran.format(g="6:HOURS")), segs)
    assert again.groups() == first.groups()
    assert [s.device_bytes() for s in segs] == built
    # the same bucket written another way names the same twin; a new granularity builds another
    same = engine.ServerQueryExecutor().execute(q.format(k=gran.format(g="360:MINUTES")), segs)
    assert same.groups() == first.groups()
    assert [s.device_bytes() for s in segs] == built
    other = engine.ServerQueryExecutor().execute(q.format(k=gran.format(g="7:HOURS")), segs)
    assert other.groups() != first.groups()
    assert all(b > a for a, b in zip(built, [s.device_bytes() for s in segs]))


# ------------------------------------------------------------------------------- 6. refusals
def spec_of(engine, expr):
    return engine.key_transform_spec(key_transform(expr))


def test_refusals_leave_no_twin_behind(engine):
    from pinot_amd._lib import PinotAmdError, lib
    rng = np.random.default_rng(9)
    n = 300
    ts = draw_ts(rng, n)
    seg = engine.ImmutableSegment(S.build_segment("refuse", {
        "ts": (ts, S.LONG, {"dictionary": False}), "s": (np.array([f"v{i % 7}" for i in range(n)], dtype=object), S.STRING, {}),
        "sr": (np.array([f"w{i % 5}" for i in range(n)], dtype=object), S.STRING, {"dictionary": False}),
        "f": (rng.normal(0, 1, n), S.DOUBLE, {"dictionary": False}), "fd": (rng.integers(0, 9, n) * 0.5, S.DOUBLE, {})}))
    before = seg.device_bytes()
    q = "SELECT COUNT(*) FROM t GROUP BY dateTrunc('hour', {c})"
    ex = engine.ServerQueryExecutor()
    for c in ("s", "sr"):
        with pytest.raises(PinotAmdError, match=r"\(-1\)"):      # STRING source: EINVAL
            ex.execute(q.format(c=c), [seg])
    for c in ("f", "fd"):
        with pytest.raises(PinotAmdError, match=r"\(-2\)"):      # FLOAT / DOUBLE source: EUNSUPPORTED
            ex.execute(q.format(c=c), [seg])
    with pytest.raises(PinotAmdError, match=r"\(-1\)"):          # no such column
        ex.execute(q.format(c="nope"), [seg])
    with pytest.raises(PinotAmdError, match="key_space"):
        ex.execute(q.format(c="ts"), [seg], key_space={})
    # at add: bad enums, sizes <= 0, a granularity below a millisecond, NULL arguments
    L = lib()
    qh = C.c_void_p()
    assert L.pinot_amd_query_create(C.byref(qh)) == 0
    good = spec_of(engine, "dateTimeConvert(ts, '1:MILLISECONDS:EPOCH', '1:HOURS:EPOCH', '15:MINUTES')")
    for field, bad in (("kind", 3), ("kind", -1), ("in_unit", 7), ("out_unit", -1), ("gran_unit", 9), ("in_size", 0),
                       ("out_size", -2), ("gran_size", 0)):
        sp = type(good).from_buffer_copy(good)
        setattr(sp, field, bad)
        assert L.pinot_amd_query_add_group_by_transform(qh, b"ts", C.byref(sp)) == EINVAL, field
    sp = spec_of(engine, "dateTrunc('hour', ts)")
    sp.trunc_unit = 9
    assert L.pinot_amd_query_add_group_by_transform(qh, b"ts", C.byref(sp)) == EINVAL
    sp = type(good).from_buffer_copy(good)
    sp.gran_unit, sp.gran_size = 1, 999   # 999 microseconds
    assert L.pinot_amd_query_add_group_by_transform(qh, b"ts", C.byref(sp)) == EINVAL
    assert L.pinot_amd_query_add_group_by_transform(qh, None, C.byref(good)) == EINVAL
    assert L.pinot_amd_query_add_group_by_transform(qh, b"ts", None) == EINVAL
    # set_group_key_values on a transformed key
    assert L.pinot_amd_query_add_group_by_transform(qh, b"ts", C.byref(good)) == 0
    vals = (C.c_int64 * 2)(0, 1)
    assert L.pinot_amd_query_set_group_key_values(qh, b"ts", 1, 2, vals, None, None) == EUNSUPPORTED
    L.pinot_amd_query_destroy(qh)
    assert seg.device_bytes() == before                           # nothing was staged by any refusal
    res = ex.execute("SELECT dateTrunc('hour', ts), COUNT(*) FROM t GROUP BY dateTrunc('hour', ts) LIMIT 100000", [seg])
    assert {k[0]: v[0] for k, v in res.groups().items()} == counts_by([{"ts": ts}], "ts", key_transform("dateTrunc('hour', ts)"))
    assert seg.device_bytes() > before
