"""Arithmetic expressions on the device (pinot_amd_query_define_expression): the expression twin's values bit for bit
against the numpy restatement (expr_ref.py), and every use of an expression -- filters, FILTER lanes, aggregations,
value-set aggregations, GROUP BY keys, the server table, selection -- against the same query over a raw DOUBLE column
`k` the test materialised from the restatement on the same docs (the oracle cannot evaluate expressions; the
value-set aggregations and selections compare with their own numpy references, as their suites do).

Double sums compare within the project's 1e-12 relative rule (assert_same_groups); everything else exactly."""
import collections

import numpy as np
import pytest

import expr_ref as R
import oracle
import selection_ref
import value_aggs_ref as vref
from oracle_reduce import server_table
from pinot_amd import segment as S
from pinot_amd.query import canonical_key, expr_text, parse_expression, parse_sql

pytestmark = pytest.mark.gpu

from test_gpu_parity import assert_same_groups  # noqa: E402

SIZES = [1, 4099, 5000, 0]      # the 1024-doc tile and the 4-docs-per-lane boundary, a single doc, no doc
NAN, INF = float("nan"), float("inf")
PAD = 4 * 1024 * 8 + 256        # the staging padding of every column (pinot_amd_required_padding)


@pytest.fixture(scope="module")
def engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from pinot_amd import engine as E
    return E


def tree(text):
    return parse_expression(text)


def text_of(sql_expr):
    return expr_text(tree(sql_expr))


def restate(sql_expr, a):
    n = len(next(iter(a.values())))
    return R.evaluate(tree(sql_expr), a, n) if n else np.zeros(0, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ data
@pytest.fixture(scope="module")
def data(engine):
    """(per-segment column arrays, staged segments). ri / rl / rf / rd: raw INT / LONG / FLOAT / DOUBLE; dn: a 6-bit
    dictionary INT; dl: a dictionary LONG; so: a sorted INT; mx: a LONG that is raw / dictionary / sorted / raw by
    segment; d: a dictionary key; x, dbl: plain values."""
    rng = np.random.default_rng(1307)
    arrays, segs = [], []
    for i, n in enumerate(SIZES):
        mx = rng.integers(-50, 50, n).astype(np.int64)
        a = {"ri": rng.integers(-1000, 1000, n).astype(np.int32),
             "rl": rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64),
             "rf": rng.normal(0, 50, n).astype(np.float32),
             "rd": np.round(rng.normal(0, 200, n), 1),
             "dn": (rng.integers(0, 37, n) - 9).astype(np.int32),
             "dl": (rng.integers(0, 3000, n) * 1_000_003).astype(np.int64),
             "so": np.sort(rng.integers(0, 40, n)).astype(np.int32),
             "mx": np.sort(mx) if i == 2 else mx,
             "d": (rng.integers(0, 5, n) * 3 + 1).astype(np.int32),
             "x": rng.integers(-10 ** 6, 10 ** 6, n).astype(np.int32),
             "dbl": rng.normal(0, 1e3, n)}
        raw, dic = {"dictionary": False}, {"detect_sorted": False}
        bufs = S.build_segment(f"xp{i}", {
            "ri": (a["ri"], S.INT, raw), "rl": (a["rl"], S.LONG, raw), "rf": (a["rf"], S.FLOAT, raw),
            "rd": (a["rd"], S.DOUBLE, raw), "dn": (a["dn"], S.INT, dic), "dl": (a["dl"], S.LONG, dic),
            "so": (a["so"], S.INT, {}), "mx": (a["mx"], S.LONG, [raw, dic, {}, raw][i]), "d": (a["d"], S.INT, dic),
            "x": (a["x"], S.INT, raw), "dbl": (a["dbl"], S.DOUBLE, raw)})
        assert bufs.columns["so"].encoding == "SORTED" and bufs.columns["dn"].encoding == "FIXED_BIT"
        assert bufs.columns["mx"].encoding == ["RAW", "FIXED_BIT", "SORTED", "RAW"][i]
        if n > 1:
            assert bufs.columns["dn"].bits_per_element <= 15
        arrays.append(a)
        segs.append(engine.ImmutableSegment(bufs))
    return arrays, segs


EDGE = [0.0, -0.0, NAN, INF, -INF, 5e-324, -5e-324, 2.2250738585072014e-308, 1.0, -1.0, 0.5, -0.5, 3.0, -3.0, 1e308,
        -1e308, 1.5, 2.5, 134217729.0, 0.1, 7.0, 1e-300, 4.0]
EDGE_LONG = [(1 << 53) + 1, -(1 << 53) - 1, (1 << 63) - 1, -(1 << 63), 0, 1, -1, (1 << 53) + 3, 1 << 62, 12345678901]


@pytest.fixture(scope="module")
def edges(engine):
    """Every pair (p, q) of the edge doubles -- +-0, NaN, +-inf, denormals, the ends of the range -- with a LONG l
    that is past 2^53 and an INT i; 529 docs, raw."""
    p = np.repeat(np.array(EDGE), len(EDGE))
    q = np.tile(np.array(EDGE), len(EDGE))
    n = len(p)
    with np.errstate(over="ignore"):   # (1e308 as a FLOAT is +inf, on purpose)
        f = np.array([EDGE[(j * 5) % len(EDGE)] for j in range(n)]).astype(np.float32)
    a = {"p": p, "q": q, "l": np.array([EDGE_LONG[j % len(EDGE_LONG)] for j in range(n)], dtype=np.int64),
         "i": np.array([(j * 7919) % 2001 - 1000 for j in range(n)], dtype=np.int32), "f": f}
    raw = {"dictionary": False}
    seg = engine.ImmutableSegment(S.build_segment("xedge", {
        "p": (a["p"], S.DOUBLE, raw), "q": (a["q"], S.DOUBLE, raw), "l": (a["l"], S.LONG, raw), "i": (a["i"], S.INT, raw),
        "f": (a["f"], S.FLOAT, raw)}))
    return a, seg


def twin_values(engine, exprs, segs, n_total):
    """The twins' values per doc, fetched through a selection without ORDER BY (the docs in (segment, docId) order)."""
    res = engine.ServerQueryExecutor().execute(f"SELECT {', '.join(exprs)} FROM t LIMIT {n_total + 1}", segs)
    rows, origins = res.rows(), res.origins()
    res.destroy()
    assert len(rows) == n_total and origins == sorted(origins)
    return [np.array([r[j] for r in rows], dtype=np.float64) for j in range(len(exprs))]


def assert_bits(got, want, what):
    g, w = R.canonical_bits(got), R.canonical_bits(want)
    bad = np.nonzero(g != w)[0]
    assert len(bad) == 0, (what, len(bad), [(int(j), float(got[j]), float(want[j])) for j in bad[:5]])


# ------------------------------------------------------------------------------------------------ 1. bit-exactness
OPERATORS = [
    ["p + q", "p - q", "p * q", "p / q", "p % q", "add(p, q, 2.5, -1e308)", "mult(p, 3, q, 1e-300)"],
    ["abs(p)", "ceil(p)", "floor(p)", "sqrt(p)", "sign(p)", "least(p, q)", "greatest(p, q)", "least(p, q, -0.0)",
     "greatest(p, 0, q)"],
    ["l + 0", "l - i", "l * f", "f / i", "i % 7", "sqrt(abs(l)) / (i + 0.5)", "floor(l / 3) + ceil(f)", "p - l"],
]


@pytest.mark.parametrize("group", range(len(OPERATORS)), ids=["arith", "functions", "typed"])
def test_every_operator_is_bit_exact_on_the_edge_values(engine, edges, group):
    a, seg = edges
    got = twin_values(engine, OPERATORS[group], [seg], len(a["p"]))
    for e, g in zip(OPERATORS[group], got):
        assert_bits(g, restate(e, a), e)


def test_multiply_add_is_not_fused(engine):
    """a * b + c with a = b = 2^27 + 1 (INT) and c = -(2^54 + 2^28) (LONG): 0.0 with two roundings, 1.0 fused."""
    n = 1030
    a = {"a": np.full(n, 134217729, dtype=np.int32), "b": np.full(n, 134217729, dtype=np.int32),
         "c": np.full(n, -((1 << 54) + (1 << 28)), dtype=np.int64)}
    raw = {"dictionary": False}
    seg = engine.ImmutableSegment(S.build_segment("xfma", {k: (v, S.LONG if k == "c" else S.INT, raw) for k, v in a.items()}))
    (got,) = twin_values(engine, ["a * b + c"], [seg], n)
    assert np.all(got == 0.0) and restate("a * b + c", a)[0] == 0.0
    res = engine.ServerQueryExecutor().execute("SELECT SUM(a * b + c), MAX(a * b + c) FROM t", [seg])
    assert res.groups()[()] == [0.0, 0.0]


SOURCE_EXPRS = ["ri + rl * rf - rd", "dn * 2.5 + dl", "so / 3", "mx % 7 - dn", "greatest(ri, dn, so) - floor(rd / 7)"]


def test_every_source_encoding_is_bit_exact(engine, data):
    """Raw INT / LONG / FLOAT / DOUBLE, a narrow and a LONG dictionary, a sorted column and the column whose encoding
    differs by segment, over the 1-doc, 4099-doc, 5000-doc and empty segments in one batch."""
    arrays, segs = data
    got = twin_values(engine, SOURCE_EXPRS, segs, sum(SIZES))
    for e, g in zip(SOURCE_EXPRS, got):
        assert_bits(g, np.concatenate([restate(e, a) for a in arrays]), e)


def test_a_dictionary_wider_than_15_bits(engine):
    n = 40_000
    rng = np.random.default_rng(5)
    a = {"w": rng.permutation(n).astype(np.int64) * 3 - 7, "v": rng.integers(-9, 9, n).astype(np.int32)}
    bufs = S.build_segment("xwide", {"w": (a["w"], S.LONG, {"detect_sorted": False}), "v": (a["v"], S.INT, {"detect_sorted": False})})
    assert bufs.columns["w"].bits_per_element == 16 and bufs.columns["v"].bits_per_element == 5
    seg = engine.ImmutableSegment(bufs)
    (got,) = twin_values(engine, ["w * v - 1"], [seg], n)
    assert_bits(got, restate("w * v - 1", a), "w * v - 1")


# ------------------------------------------------------------------------------------------------ 2. each use
def materialised(arrays, sql_expr, extra=()):
    """The oracle's segments: k = the restated expression as a raw DOUBLE column, plus the plain columns."""
    out = []
    for i, a in enumerate(arrays):
        cols = {"k": (restate(sql_expr, a), S.DOUBLE, {"dictionary": False})}
        for c in ("d", "x", "dbl") + tuple(extra):
            t = S.DOUBLE if c == "dbl" else S.INT
            cols[c] = (a[c], t, {"dictionary": False} if c in ("x", "dbl") else {"detect_sorted": False})
        out.append(S.build_segment(f"ok{i}", cols))
    return out


AGGS = ("SELECT d, COUNT(*), SUM({k}), MIN({k}), MAX({k}), AVG({k}), MINMAXRANGE({k}) FROM t "
        "WHERE x BETWEEN -600000 AND 700000 GROUP BY d LIMIT 100000")


@pytest.mark.parametrize("expr", ["rd * ri * 1.07", "(rl - dl) / rl", "mx % 7 - dn", "abs(rf) + so"])
def test_aggregations_against_the_oracle(engine, data, expr):
    arrays, segs = data
    res = engine.ServerQueryExecutor().execute(AGGS.format(k=expr), segs)
    nm, og = oracle.execute(AGGS.format(k="k"), materialised(arrays, expr))
    assert res.num_docs_matched() == nm
    assert_same_groups(res.groups(), og, {1, 4})
    res.destroy()


@pytest.mark.parametrize("which", [[0], [3], [0, 3], [1]], ids=["one_doc", "empty", "one_doc_and_empty", "4099_docs"])
def test_small_batches(engine, data, which):
    arrays, segs = data
    expr = "ri - dn * so + mx"
    res = engine.ServerQueryExecutor().execute(AGGS.format(k=expr), [segs[i] for i in which])
    nm, og = oracle.execute(AGGS.format(k="k"), materialised([arrays[i] for i in which], expr))
    assert res.num_docs_matched() == nm
    assert_same_groups(res.groups(), og, {1, 4})


PRED_EXPR = "ri % 7 - dn"   # integral doubles in -33..33
PREDICATES = ["{k} = 3", "{k} <> 3", "{k} IN (-2, 0, 5.0, 99)", "{k} NOT IN (-2, 0, 5)", "{k} > 4.5", "{k} <= -3",
              "{k} BETWEEN -1 AND 6", "NOT {k} BETWEEN -1 AND 6", "NOT {k} = 3", "NOT ({k} IN (1, 2) OR {k} < -5)",
              "{k} > 2 AND d < 10 OR {k} = -7"]


@pytest.mark.parametrize("pred", PREDICATES)
def test_predicates_in_the_filter_and_in_a_lane(engine, data, pred):
    arrays, segs = data
    oseg = materialised(arrays, PRED_EXPR)
    q = "SELECT d, COUNT(*), SUM(x) FROM t WHERE {p} GROUP BY d LIMIT 100000"
    res = engine.ServerQueryExecutor().execute(q.format(p=pred.format(k=PRED_EXPR)), segs)
    nm, og = oracle.execute(q.format(p=pred.format(k="k")), oseg)
    assert res.num_docs_matched() == nm and nm > 0
    assert_same_groups(res.groups(), og)
    # the same predicate as a FILTER lane beside the main filter: the lane's count and sum are the oracle's over
    # (main filter AND predicate); the unfiltered COUNT(*) the main filter's
    lane = ("SELECT COUNT(*), COUNT(*) FILTER (WHERE {p}), SUM(x) FILTER (WHERE {p}) FROM t WHERE x > -500000")
    got = engine.ServerQueryExecutor().execute(lane.format(p=pred.format(k=PRED_EXPR)), segs).groups()[()]
    _, main = oracle.execute("SELECT COUNT(*) FROM t WHERE x > -500000", oseg)
    _, both = oracle.execute("SELECT COUNT(*), SUM(x) FROM t WHERE x > -500000 AND ({p})".format(p=pred.format(k="k")), oseg)
    assert got == [main[()][0], both[()][0], both[()][1]]


@pytest.mark.parametrize("expr", ["mx % 7 - dn", "floor(rd / 40) * 0.5"])
def test_value_set_aggregations(engine, data, expr):
    arrays, segs = data
    q = ("SELECT d, DISTINCTCOUNT({k}), PERCENTILE({k}, 95), PERCENTILE50({k}), DISTINCTSUM({k}), DISTINCTAVG({k}), "
         "COUNT(*) FROM t WHERE x > -700000 GROUP BY d LIMIT 100000")
    np_segs = [dict(a, k=restate(expr, a)) for a in arrays]
    qk = parse_sql(q.format(k="k"))
    exp = vref.reference_rows(qk, np_segs, lambda s: s["x"] > -700000)
    for ex in (engine.ServerQueryExecutor(distinct_count="native"), engine.ServerQueryExecutor()):
        res = ex.execute(q.format(k=expr), segs)
        got = {canonical_key(r[:1]): list(r[1:]) for r in res.rows()}
        assert set(got) == set(exp) and len(got) == 5
        for key, e in exp.items():
            for a, gv, ev in zip(qk.aggregations, got[key], e):
                assert vref.same(gv, ev, a.func, True), (expr, key, a.func, gv, ev)
        res.destroy()


def test_group_by_an_expression_keeps_java_double_identity(engine, edges):
    """The key is a double: -0.0 and 0.0 are two groups, every NaN one."""
    a, seg = edges
    expr = "p * q"
    k = restate(expr, a)
    oseg = [S.build_segment("okedge", {"k": (k, S.DOUBLE, {"dictionary": False}), "i": (a["i"], S.INT, {"dictionary": False})})]
    q = "SELECT {k}, COUNT(*), MAX(i) FROM t GROUP BY {k} LIMIT 100000"
    res = engine.ServerQueryExecutor().execute(q.format(k=expr), [seg])
    _, og = oracle.execute(q.format(k="k"), oseg)
    got = res.groups()
    keys = {canonical_key(g) for g in got}
    assert len(keys) == len(got) == len(og)
    assert canonical_key((0.0,)) in keys and canonical_key((-0.0,)) in keys and canonical_key((NAN,)) in keys
    assert {canonical_key(g): v for g, v in got.items()} == {canonical_key(g): v for g, v in og.items()}


@pytest.mark.parametrize("keys", ["{k}", "d, {k}"], ids=["alone", "beside_a_dictionary_key"])
def test_group_by_against_the_oracle(engine, data, keys):
    arrays, segs = data
    expr = "floor(rd / 40) + so"
    q = "SELECT {g}, COUNT(*), SUM(x), MAX(dbl) FROM t WHERE x > -800000 GROUP BY {g} LIMIT 100000"
    res = engine.ServerQueryExecutor().execute(q.format(g=keys.format(k=expr)), segs)
    nm, og = oracle.execute(q.format(g=keys.format(k="k")), materialised(arrays, expr))
    assert res.num_docs_matched() == nm and len(og) > 30
    assert_same_groups(res.groups(), og)


def test_num_groups_limit(engine, data):
    arrays, segs = data
    expr = "floor(rd / 10)"
    q = "SET numGroupsLimit = 40; SELECT {k}, COUNT(*), SUM(x) FROM t GROUP BY {k} LIMIT 100000"
    res = engine.ServerQueryExecutor().execute(q.format(k=expr), segs)
    stats = {}
    _, og = oracle.execute(q.format(k="k"), materialised(arrays, expr), stats=stats)
    assert stats["num_groups_limit_reached"] and res.num_groups_limit_reached()
    assert len(np.unique(restate(expr, arrays[1]))) > 40
    assert_same_groups(res.groups(), og)


def test_server_table_ordered_by_an_expression(engine, data):
    arrays, segs = data
    expr = "floor(rd / 40) + so"
    q = "SET minServerGroupTrimSize = 4; SELECT {k}, COUNT(*), SUM(x) FROM t WHERE d < 10 GROUP BY {k} ORDER BY {k} DESC LIMIT 5"
    qc = parse_sql(q.format(k=expr))
    assert qc.safe_trim()
    got = engine.ServerQueryExecutor(server_trim=True).execute(qc, segs).groups()
    _, full = oracle.execute(q.format(k="k"), materialised(arrays, expr))
    exp = server_table(oracle.parse_sql(q.format(k="k")), full)
    assert len(exp) == 5 < len(full)
    assert_same_groups(got, exp)
    assert list(got) == list(exp)
    # by an aggregated expression (an unsafe trim), the dictionary key second
    agg = "ri * 2 - mx"
    q2 = "SET minServerGroupTrimSize = 2; SELECT d, MAX({k}), COUNT(*) FROM t GROUP BY d ORDER BY MAX({k}) DESC, d LIMIT 1"
    got = engine.ServerQueryExecutor(server_trim=True).execute(q2.format(k=agg), segs).groups()
    _, full = oracle.execute(q2.format(k="k"), materialised(arrays, agg))
    exp = server_table(oracle.parse_sql(q2.format(k="k")), full)
    assert len(got) == len(exp) == 5 and len(full) == 5     # max(5 * LIMIT, minServerGroupTrimSize)
    assert_same_groups(got, exp)
    assert list(got) == list(exp)


@pytest.mark.parametrize("desc", [False, True])
def test_selection_ordered_by_an_expression(engine, data, desc):
    arrays, segs = data
    expr = "ri - dn * 2.5"
    text = text_of(expr)
    tables = [dict(a, **{text: restate(expr, a)}) for a in arrays]
    masks = [a["x"] > 0 for a in arrays]
    for k in (7, 1500):
        sql = f"SELECT {expr}, x, d FROM t WHERE x > 0 ORDER BY {expr}{' DESC' if desc else ''}, x LIMIT {k}"
        res = engine.ServerQueryExecutor().execute(sql, segs)
        exp_rows, exp_origins, exp_matched = selection_ref.select(tables, masks, [text, "x", "d"],
                                                                  [(text, not desc), ("x", True)], k)
        assert res.columns == [text, "x", "d"]
        assert res.origins() == exp_origins
        assert selection_ref.same_rows(res.rows(), exp_rows)
        assert res.num_docs_matched() == exp_matched
        res.destroy()


# ------------------------------------------------------------------------------------------------ 3. plans
def test_the_plan_is_a_raw_double_columns(engine, data):
    """The same query over segments that hold the expression's values as an ordinary raw DOUBLE column: the same
    kernels, the same bytes, the same groups."""
    arrays, segs = data
    expr = "rd * ri * 1.07"
    staged = [engine.ImmutableSegment(S.build_segment(f"kd{i}", {
        "kd": (restate(expr, a), S.DOUBLE, {"dictionary": False}), "d": (a["d"], S.INT, {"detect_sorted": False}),
        "x": (a["x"], S.INT, {"dictionary": False})})) for i, a in enumerate(arrays)]
    q = "SELECT d, SUM({k}), MAX({k}), COUNT(*) FROM t WHERE x > 0 GROUP BY d LIMIT 100000"
    twin = engine.ServerQueryExecutor().execute(q.format(k=expr), segs)
    plain = engine.ServerQueryExecutor().execute(q.format(k="kd"), staged)
    assert_same_groups(twin.groups(), plain.groups(), {0})     # (the double sum: two executions' atomic orders)
    assert len(plain.groups()) == 5
    assert twin.kernel_info() == plain.kernel_info()
    assert twin.algorithmic_bytes() == plain.algorithmic_bytes()


def test_equal_trees_build_one_twin(engine, data):
    arrays, segs = data
    q = "SELECT SUM({k}), COUNT(*) FROM t"
    before = [s.device_bytes() for s in segs]
    first = engine.ServerQueryExecutor().execute(q.format(k="rf * 2 + dn"), segs)
    assert "raw_keys" in first.plan_timing()
    built = [s.device_bytes() for s in segs]
    assert [b - a for a, b in zip(before, built)] == [n * 8 + PAD for n in SIZES]   # the empty segment's: its padding
    want = first.groups()
    first.destroy()
    # 2 and 2.0 are one number; the twin outlives the result that built it and is read again
    for k in ("rf * 2.0 + dn", "rf * 2 + dn", "add(mult(2, rf), dn)"):
        res = engine.ServerQueryExecutor().execute(q.format(k=k), segs)
        assert res.groups() == want
        assert [s.device_bytes() for s in segs] == built, k
        res.destroy()
    other = engine.ServerQueryExecutor().execute(q.format(k="rf * 3 + dn"), segs)
    assert other.groups() != want
    assert all(b > a for a, b in zip(built, [s.device_bytes() for s in segs]))


def test_queries_differing_only_in_a_literal_share_no_plan(engine, data):
    arrays, segs = data
    qs = {lit: f"SELECT d, COUNT(*) FROM t WHERE ri - so - {lit} > 0 GROUP BY d LIMIT 100000" for lit in (3, 4)}
    exp = {}
    for lit in qs:
        c = collections.Counter()
        for a in arrays:
            c.update(a["d"][restate(f"ri - so - {lit}", a) > 0].tolist())
        exp[lit] = dict(c)
    assert exp[3] != exp[4]
    for _ in range(3):   # executed, destroyed (the plan goes back to the prepared plans) and re-executed alternately
        for lit, q in qs.items():
            res = engine.ServerQueryExecutor().execute(q, segs)
            assert {k[0]: v[0] for k, v in res.groups().items()} == exp[lit], lit
            res.destroy()


def test_the_two_column_sum_keeps_its_plan(engine, data):
    """SUM(a * b) of two plain columns stays the scan's own expression: no twin is staged and INT operands sum
    exactly in int64; SUM(a * b * 1) is a double sum over a twin."""
    arrays, segs = data
    before = [s.device_bytes() for s in segs]
    two = engine.ServerQueryExecutor().execute("SELECT SUM(ri * x), SUM(ri) FROM t", segs)
    assert [s.device_bytes() for s in segs] == before
    exact = sum(int(v) for a in arrays for v in a["ri"].astype(np.int64) * a["x"].astype(np.int64))
    assert two.groups()[()][0] == float(exact)
    plain = engine.ServerQueryExecutor().execute("SELECT SUM(x), SUM(ri) FROM t", segs)
    assert two.kernel_info() == plain.kernel_info()
    twin = engine.ServerQueryExecutor().execute("SELECT SUM(ri * x * 1), SUM(ri) FROM t", segs)
    assert all(b > a for a, b in zip(before, [s.device_bytes() for s in segs]))
    want = float(np.sum(np.concatenate([restate("ri * x * 1", a) for a in arrays])))
    assert abs(twin.groups()[()][0] - want) <= 1e-12 * abs(want) + 1e-9


def test_eviction_under_a_small_budget(engine, monkeypatch):
    """PINOT_AMD_EXPR_TWIN_BYTES between two and three twins: a third expression drops the least recently used twin
    no live result reads; a live result's twin stays, its plan re-executes; the dropped expression rebuilds and
    answers correctly; with nothing droppable the budget is exceeded and the query still runs."""
    n = 3000
    rng = np.random.default_rng(77)
    a = {"u": rng.integers(-99, 99, n).astype(np.int32), "v": rng.integers(1, 50, n).astype(np.int32)}
    seg = engine.ImmutableSegment(S.build_segment("xevict", {k: (v, S.INT, {"dictionary": False}) for k, v in a.items()}))
    twin = n * 8 + PAD
    monkeypatch.setenv("PINOT_AMD_EXPR_TWIN_BYTES", str(2 * twin + twin // 2))
    base = seg.device_bytes()
    ex = engine.ServerQueryExecutor()
    q = "SELECT SUM({k}), MIN({k}) FROM t WHERE v > 3"

    def want(k):
        v = restate(k, a)[a["v"] > 3]
        return [float(np.sum(v)), float(np.min(v))]
    live = ex.execute(q.format(k="u * 2 - v"), [seg])           # A: stays live
    assert live.groups()[()] == want("u * 2 - v") and seg.device_bytes() == base + twin
    b = ex.execute(q.format(k="u * 3 - v"), [seg])               # B: idle once destroyed
    assert b.groups()[()] == want("u * 3 - v") and seg.device_bytes() == base + 2 * twin
    b.destroy()
    c = ex.execute(q.format(k="u * 4 - v"), [seg])               # C: over the budget -- A is older but live, B goes
    assert c.groups()[()] == want("u * 4 - v") and seg.device_bytes() == base + 2 * twin
    live.execute_again()
    assert live.groups()[()] == want("u * 2 - v")
    d = ex.execute(q.format(k="u * 5 - v"), [seg])               # A and C live: nothing droppable, over the budget
    assert d.groups()[()] == want("u * 5 - v") and seg.device_bytes() == base + 3 * twin
    c.destroy()
    d.destroy()
    again = ex.execute(q.format(k="u * 3 - v"), [seg])           # B rebuilds (C, the oldest idle twin, goes; then D)
    assert again.groups()[()] == want("u * 3 - v")
    assert seg.device_bytes() <= base + 2 * twin
    live.execute_again()
    assert live.groups()[()] == want("u * 2 - v")
    for r in (again, live):
        r.destroy()


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_stage_nothing(engine):
    from pinot_amd._lib import PinotAmdError
    n = 300
    rng = np.random.default_rng(9)
    a = rng.integers(0, 9, n).astype(np.int32)
    seg = engine.ImmutableSegment(S.build_segment("xrefuse", {
        "a": (a, S.INT, {"dictionary": False}),
        "s": (np.array([f"v{i % 7}" for i in range(n)], dtype=object), S.STRING, {}),
        "m": ([rng.integers(0, 9, 1 + i % 3).astype(np.int32) for i in range(n)], S.INT, {"multi_value": True})}))
    before = seg.device_bytes()
    ex = engine.ServerQueryExecutor()
    refused = [
        ("SELECT SUM(a + s + 1) FROM t", PinotAmdError, r"\(-1\).*STRING column s in an expression"),   # EINVAL
        ("SELECT COUNT(*) FROM t WHERE a * m > 3", PinotAmdError, r"\(-2\).*multi-value"),   # an MV source: EUNSUPPORTED
        ("SELECT SUM(a + nope + 1) FROM t", PinotAmdError, r"\(-1\).*no column nope"),           # the library's batch check
        ("SELECT COUNT(*) FROM t WHERE a + nope > 1", PinotAmdError, "unknown column 'nope'"),  # (looked up here)
        # one good and one refused expression in a query: the good one's twin is not staged either
        ("SELECT SUM(a * 2), SUM(abs(s)) FROM t", PinotAmdError, r"\(-1\).*STRING column s in an expression"),
    ]
    for sql, exc, what in refused:
        with pytest.raises(exc, match=what):
            ex.execute(sql, [seg])
        assert seg.device_bytes() == before, sql                     # nothing was staged by the refusal
    with pytest.raises(ValueError, match="key_space"):
        ex.execute("SELECT COUNT(*) FROM t GROUP BY a * 2", [seg], key_space={})
    assert seg.device_bytes() == before
    res = ex.execute("SELECT SUM(a * 2) FROM t", [seg])
    assert res.groups()[()] == [float(2 * int(a.sum()))]
    assert seg.device_bytes() == before + n * 8 + PAD
