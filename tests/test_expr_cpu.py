"""Arithmetic expressions without a device: the numpy restatement (expr_ref) pinned to hand-computed values, the
parser's precedence and canonical texts, every refusal, and pinot_amd_query_define_expression's argument checks.

(The reference's query tests over tests/golden's data assert no literal result of an arithmetic expression --
InnerSegment* / InterSegmentAggregationSingleValueQueriesTest hold none -- so there is no golden file for them.)"""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import expr_ref as R
from pinot_amd import query as Q
from pinot_amd.query import parse_expression as expression, parse_sql

NAN = float("nan")
INF = float("inf")


def bits(x) -> int:
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def ev(text, **cols):
    n = len(next(iter(cols.values())))
    return R.evaluate(expression(text), {k: np.asarray(v) for k, v in cols.items()}, n)


def same(got, want):
    assert [hex(b) for b in R.canonical_bits(got)] == [hex(b) for b in R.canonical_bits(np.asarray(want, dtype=np.float64))]


# ------------------------------------------------------------------------------------------ the restatement
def test_plus_of_negative_zeros_is_positive_zero():
    # acc = 0.0 at init; 0.0 + -0.0 = 0.0, 0.0 + -0.0 = 0.0
    same(ev("plus(x,y)", x=[-0.0], y=[-0.0]), [0.0])
    assert bits(ev("plus(x,y)", x=[-0.0], y=[-0.0])[0]) == 0
    # minus has no accumulator: -0.0 - 0.0 = -0.0
    assert bits(ev("minus(x,y)", x=[-0.0], y=[0.0])[0]) == 1 << 63
    # times starts from 1.0: 1.0 * -0.0 * 5 = -0.0
    assert bits(ev("times(x,y)", x=[-0.0], y=[5.0])[0]) == 1 << 63


def test_literals_are_hoisted_in_order():
    # add(x, 1e16, 1, -1e16): literals first, in order: ((0.0 + 1e16) + 1.0) + -1e16 = 0.0 (1e16 + 1 rounds to 1e16),
    # then + x. Left to right over all arguments it would be ((x + 1e16) + 1) - 1e16.
    assert R.fold_literals("add", expression("add(x,1e16,1,-1e16)")[2]) == 0.0
    same(ev("add(x,1e16,1,-1e16)", x=[3.0]), [3.0])
    same(ev("add(1e16,x,-1e16)", x=[1.0]), [1.0])          # (0 + 1e16 - 1e16) + 1 = 1, not (1e16 + 1) - 1e16 = 0
    # mult(x, 1e200, 1e200, 1e-200): the literal product overflows to inf before x is seen
    assert R.fold_literals("mult", expression("mult(x,1e200,1e200,1e-200)")[2]) == INF
    same(ev("mult(x,1e200,1e200,1e-200)", x=[0.0]), [NAN])  # inf * 0
    # SQL a + b + c nests: plus(plus(a,b),c) -- the inner sum is no literal, nothing is hoisted across it
    same(ev("x + 1e16 + 1 + -1e16", x=[3.0]), [0.0 + (0.0 + (0.0 + 1e16 + 3.0) + 1.0) - 1e16])


def test_mod_is_fmod():
    same(ev("mod(x,y)", x=[5, -5, 5.5, -5.5, 5, 0], y=[-3, 3, 2, 2, 0, 0]), [2.0, -2.0, 1.5, -1.5, NAN, NAN])
    assert bits(ev("mod(x,y)", x=[-4.0], y=[2.0])[0]) == 1 << 63   # -0.0: the dividend's sign


def test_division_by_zero():
    same(ev("divide(x,y)", x=[1, -1, 0, -0.0, INF], y=[0, 0, 0, 0, INF]), [INF, -INF, NAN, NAN, NAN])
    same(ev("divide(x,y)", x=[1.0], y=[-0.0]), [-INF])


def test_single_parameter_functions():
    assert ev("floor(x)", x=[-0.5])[0] == -1.0
    assert bits(ev("ceil(x)", x=[-0.5])[0]) == 1 << 63        # -0.0
    same(ev("sign(x)", x=[NAN, -0.0, 0.0, -3.5, 1e-320, INF, -INF]), [NAN, -0.0, 0.0, -1.0, 1.0, 1.0, -1.0])
    assert bits(ev("sign(x)", x=[-0.0])[0]) == 1 << 63
    same(ev("abs(x)", x=[-0.0, -INF, NAN, -5e-324]), [0.0, INF, NAN, 5e-324])
    same(ev("sqrt(x)", x=[-1.0, -0.0, 4.0, 2.0, INF]), [NAN, -0.0, 2.0, math.sqrt(2.0), INF])
    assert bits(ev("sqrt(x)", x=[-0.0])[0]) == 1 << 63


def test_least_greatest_are_java_min_max():
    same(ev("least(x,y)", x=[NAN, 1.0, 0.0, -0.0, 2.0], y=[1.0, NAN, -0.0, 0.0, 1.0]), [NAN, NAN, -0.0, -0.0, 1.0])
    same(ev("greatest(x,y)", x=[NAN, 1.0, 0.0, -0.0, 2.0], y=[1.0, NAN, -0.0, 0.0, 1.0]), [NAN, NAN, 0.0, 0.0, 2.0])
    same(ev("least(x,y,-2.5)", x=[1.0, -3.0], y=[2.0, 5.0]), [-2.5, -3.0])
    same(ev("greatest(x,0,y)", x=[-1.0], y=[-0.0]), [0.0])


def test_long_rounds_above_2_53():
    x = np.array([2**53 + 1, 2**53 + 3, -(2**53) - 1, 2**63 - 1], dtype=np.int64)
    same(ev("plus(x,0)", x=x), [2.0**53, 2.0**53 + 4, -(2.0**53), 2.0**63])      # ties to even
    same(ev("minus(x,y)", x=x, y=np.array([2**53] * 4, dtype=np.int64)), [0.0, 4.0, -(2.0**54), 2.0**63 - 2.0**53])


def test_int_and_float_widen():
    same(ev("times(x,y)", x=np.array([134217729], dtype=np.int32), y=np.array([134217729], dtype=np.int32)),
         [float(134217729) * float(134217729)])
    same(ev("plus(x,0)", x=np.array([0.1], dtype=np.float32)), [float(np.float32(0.1))])


def test_unfused_multiply_add():
    """a * b + c with a = b = 2^27 + 1 and c = -(2^54 + 2^28): the product 2^54 + 2^28 + 1 rounds to 2^54 + 2^28, so the
    sum is 0.0; a fused multiply-add keeps the 1."""
    a = np.array([134217729], dtype=np.int32)
    c = np.array([-(2**54 + 2**28)], dtype=np.int64)
    same(ev("a * b + c", a=a, b=a, c=c), [0.0])
    assert math.fma(134217729.0, 134217729.0, float(c[0])) == 1.0 if hasattr(math, "fma") else True


# ------------------------------------------------------------------------------------------ the parser
@pytest.mark.parametrize("sql,text", [
    ("a + b * c", "plus(a,times(b,c))"),
    ("(a + b) * c", "times(plus(a,b),c)"),
    ("a - b - c", "minus(minus(a,b),c)"),
    ("a / b % c * d", "times(mod(divide(a,b),c),d)"),
    ("a + b + c", "plus(plus(a,b),c)"),
    ("add(a, b, c)", "add(a,b,c)"),
    ("ADD(a,b)", "add(a,b)"),
    ("price * qty * 1.07", "times(times(price,qty),'1.07')"),
    ("(rev - cost) / rev", "divide(minus(rev,cost),rev)"),
    ("floor(x / 100)", "floor(divide(x,'100'))"),
    ("a * -2", "times(a,'-2')"),
    ("a -1", "minus(a,'1')"),
    ("a - -1", "minus(a,'-1')"),
    ("a-1*b", "minus(a,times('1',b))"),
    ("a * 2.0", "times(a,'2.0')"),
    ("a * 1e10", "times(a,'1.0E10')"),
    ("a + 0.00001", "plus(a,'1.0E-5')"),
    ("least(a, b, -2.5)", "least(a,b,'-2.5')"),
    ("GREATEST(abs(a), Ceiling(b), SQRT(c), sign(d))", "greatest(abs(a),ceiling(b),sqrt(c),sign(d))"),
    ("mod(a, 3)", "mod(a,'3')"),
])
def test_precedence_and_canonical_texts(sql, text):
    qc = parse_sql(f"SELECT {sql} FROM t LIMIT 1")
    assert qc.select_columns == [text]
    assert Q.expr_text(expression(text)) == text          # the canonical text parses back to itself


def test_two_and_two_point_zero_are_one_number():
    a, b = Q.expr_postfix(expression("a * 2")), Q.expr_postfix(expression("a * 2.0"))
    assert a == b and a[1] == (Q.X_LITERAL, 0, None, 2.0)


def test_expressions_everywhere():
    qc = parse_sql("SELECT d, SUM(price * qty * 1.07), PERCENTILE(a + b + 0, 95), SUM(x) FILTER (WHERE a - b > 0), "
                   "AVG((rev - cost) / rev) FROM t WHERE price * qty > 1000 AND (a - b) * 2 BETWEEN 1 AND 5 "
                   "AND (c = 1 OR a % 2 IN (0, 1)) GROUP BY d, floor(x / 100) "
                   "ORDER BY floor(x / 100), SUM(price * qty * 1.07) DESC LIMIT 7")
    assert [a.text for a in qc.aggregations] == [
        "sum(times(times(price,qty),'1.07'))", "percentile95(plus(plus(a,b),'0'))", "sum(x) FILTER(WHERE minus(a,b) > '0')",
        "avg(divide(minus(rev,cost),rev))"]
    assert all(a.expr is None for a in qc.aggregations)
    assert qc.group_by == ["d", "floor(divide(x,'100'))"]
    assert qc.order_by == [("floor(divide(x,'100'))", True), ("sum(times(times(price,qty),'1.07'))", False)]
    assert qc.order_by_targets() == [(0, 1, True), (1, 0, False)]
    cols = [p.column for clause in qc.cnf for p, _ in clause]
    assert cols == ["times(price,qty)", "times(minus(a,b),'2')", "c", "mod(a,'2')"]
    assert qc.expressions() == ["times(price,qty)", "times(minus(a,b),'2')", "mod(a,'2')",
                                "times(times(price,qty),'1.07')", "plus(plus(a,b),'0')", "minus(a,b)",
                                "divide(minus(rev,cost),rev)", "floor(divide(x,'100'))"]
    assert qc.aggregations[0].columns == ("price", "qty")
    sel = parse_sql("SELECT a - b, c FROM t WHERE a > 1 ORDER BY a - b DESC, c LIMIT 5")
    assert sel.is_selection() and sel.select_columns == ["minus(a,b)", "c"]
    assert sel.order_by == [("minus(a,b)", False), ("c", True)]
    assert sel.selection_columns() == ["minus(a,b)", "c"]


def test_two_column_sum_keeps_its_form():
    """times | minus | plus of two plain columns stays the two-column form of pinot_amd_query_add_aggregation_expr
    (exact for INT operands) under every function, as before; anything else is an expression."""
    qc = parse_sql("SELECT SUM(a * b), MIN(a - b), AVG(CAST(a AS DOUBLE) + b), SUM(a * b * 1), SUM(a / b), "
                   "PERCENTILE(a + b, 50), PERCENTILE(a + b + 0, 50), SUM(a * 2) FROM t")
    assert [a.expr for a in qc.aggregations] == [("MUL", "a", "b"), ("SUB", "a", "b"), ("ADD", "a", "b"), None, None,
                                                  ("ADD", "a", "b"), None, None]
    assert [a.column for a in qc.aggregations] == ["times(a,b)", "minus(a,b)", "plus(a,b)", "times(times(a,b),'1')",
                                                    "divide(a,b)", "plus(a,b)", "plus(plus(a,b),'0')", "times(a,'2')"]
    assert qc.expressions() == ["times(times(a,b),'1')", "divide(a,b)", "plus(plus(a,b),'0')", "times(a,'2')"]


def test_mirror_split_groups_by_the_expression_text():
    """A value-set aggregation over an expression: its sub query groups by the expression's text. times / minus / plus
    of two plain columns stays the two-column form, which the value-set functions keep refusing."""
    from pinot_amd.query import split_distinct_count
    qc = parse_sql("SELECT g, PERCENTILE(a + b + c, 95), DISTINCTSUM(a / b), DISTINCTCOUNT(a / b) FROM t GROUP BY g")
    _, subs = split_distinct_count(qc)
    assert [(i, s.group_by) for i, s in subs] == [(0, ["g", "plus(plus(a,b),c)"]), (1, ["g", "divide(a,b)"])]
    for sql in ("SELECT PERCENTILE(a + b, 95) FROM t", "SELECT DISTINCTAVG(a - b) FROM t"):
        qc = parse_sql(sql)
        assert qc.aggregations[0].expr is not None and qc.expressions() == []
        with pytest.raises(ValueError, match="one column"):
            split_distinct_count(qc)


@pytest.mark.parametrize("sql,what", [
    ("SELECT exp(a) FROM t", "exp"),
    ("SELECT SUM(ln(a)) FROM t", "ln"),
    ("SELECT a FROM t WHERE log2(a) > 1", "log2"),
    ("SELECT COUNT(*) FROM t GROUP BY log10(a)", "log10"),
    ("SELECT SUM(power(a, 2)) FROM t", "power"),
    ("SELECT round(a, 2) FROM t", "round"),
    ("SELECT roundDecimal(a, 2) FROM t", "roundDecimal"),
    ("SELECT truncate(a, 2) FROM t", "truncate"),
    ("SELECT sin(a) FROM t", "sin"),
    ("SELECT SUM(cos(a) * b) FROM t", "cos"),
    ("SELECT CASE WHEN a > 1 THEN 1 ELSE 0 END FROM t", "CASE"),
    ("SELECT SUM(CAST(a AS DOUBLE) * b * 2) FROM t", "CAST"),
    ("SELECT foo(a) FROM t", "foo"),
    ("SELECT a FROM t WHERE abs(2) > 1", "abs of a literal"),
    ("SELECT sqrt(4) + a FROM t", "sqrt of a literal"),
    ("SELECT -a FROM t", "unary minus"),
    ("SELECT sub(a, b, c) FROM t", "exactly two"),
    ("SELECT add(a) FROM t", "two or more"),
    ("SELECT abs(a, b) FROM t", "exactly one"),
    ("SELECT a + 'x' FROM t", "string literal"),
    ("SELECT COUNT(*) FROM t GROUP BY dateTrunc('hour', a + b)", "datetrunc of an expression"),
    ("SELECT COUNT(*) FROM t GROUP BY timeConvert(abs(a), 'SECONDS', 'HOURS')", "timeconvert of an expression"),
    ("SELECT SUM(dateTrunc('hour', ts) + 1) FROM t", "key transform"),
    ("SELECT SUM(a + MAX(b)) FROM t", "aggregation"),
    ("SELECT 1 + 2 FROM t", "needs a column"),
    ("SELECT " + " + ".join(f"c{i}" for i in range(9)) + " FROM t", "8 distinct columns"),
    ("SELECT " + " + ".join(["a"] * 17) + " FROM t", "32 nodes"),
])
def test_refusals_name_the_form(sql, what):
    with pytest.raises(ValueError, match=what):
        parse_sql(sql)


def test_multi_gpu_path_and_key_space_refuse_expressions():
    from pinot_amd import dist, engine
    for sql in ("SELECT SUM(a * b * 2) FROM t GROUP BY d", "SELECT COUNT(*) FROM t GROUP BY floor(a / 10)",
                "SELECT COUNT(*) FROM t WHERE a - b > 0 GROUP BY d"):
        qc = parse_sql(sql)
        with pytest.raises(ValueError, match="arithmetic expressions"):
            dist.key_columns(qc)
        with pytest.raises(ValueError, match="arithmetic expressions"):
            engine.ServerQueryExecutor().execute(qc, [object()], key_space={"d": [1]})
    # the two-column form is no expression of this kind: it merges as before
    assert dist.key_columns(parse_sql("SELECT SUM(a * b) FROM t GROUP BY d")) == ["d"]


# ------------------------------------------------------------------------------------------ the C entry point
def _define(L, qh, rows):
    from pinot_amd._lib import XNode
    nodes = (XNode * max(len(rows), 1))()
    for n, (kind, nargs, col, lit) in zip(nodes, rows):
        n.kind, n.num_args, n.column, n.literal = kind, nargs, (col.encode() if col is not None else None), lit
    out = C.c_char_p()
    rc = L.pinot_amd_query_define_expression(qh, nodes, len(rows), C.byref(out))
    return rc, (out.value.decode() if rc == 0 else L.pinot_amd_last_error().decode())


def test_define_expression_validates_its_arguments():
    """No device: the postfix is checked and canonicalised at the call."""
    from pinot_amd._lib import lib
    L = lib()
    qh = C.c_void_p()
    assert L.pinot_amd_query_create(C.byref(qh)) == 0
    col = lambda c: (Q.X_COLUMN, 0, c, 0.0)
    lit = lambda v: (Q.X_LITERAL, 0, None, v)
    op = lambda k, n: (k, n, None, 0.0)
    rc, name = _define(L, qh, [col("a"), col("b"), op(Q.X_MULT, 2)])
    assert rc == 0 and "$" in name
    # equal trees, one name: 2 and 2.0; literals hoisted wherever they stand; the same tree twice
    rc, n1 = _define(L, qh, Q.expr_postfix(expression("a * 2")))
    rc2, n2 = _define(L, qh, Q.expr_postfix(expression("a * 2.0")))
    rc3, n3 = _define(L, qh, Q.expr_postfix(expression("mult(2, a)")))
    assert (rc, rc2, rc3) == (0, 0, 0) and n1 == n2 == n3
    assert _define(L, qh, Q.expr_postfix(expression("a * 3")))[1] != n1                # another literal, another name
    assert _define(L, qh, Q.expr_postfix(expression("a - 2")))[1] != _define(L, qh, Q.expr_postfix(expression("2 - a")))[1]
    assert _define(L, qh, Q.expr_postfix(expression("add(a,1,2)")))[1] == _define(L, qh, Q.expr_postfix(expression("add(3,a)")))[1]
    # 0.0 + -0.0 = 0.0: after the folding the two sums hold one literal; a difference folds nothing
    assert _define(L, qh, Q.expr_postfix(expression("a + -0.0")))[1] == _define(L, qh, Q.expr_postfix(expression("a + 0.0")))[1]
    assert _define(L, qh, Q.expr_postfix(expression("a - -0.0")))[1] != _define(L, qh, Q.expr_postfix(expression("a - 0.0")))[1]
    assert _define(L, qh, [col("a"), lit(NAN), op(Q.X_SUB, 2)])[1] == \
        _define(L, qh, [col("a"), lit(struct.unpack("<d", struct.pack("<Q", 0x7FF0000000000001))[0]), op(Q.X_SUB, 2)])[1]
    EINVAL, EUNSUPPORTED = -1, -2
    bad = [
        ([], "no nodes"),
        ([col("a"), col("b")], "two values left"),
        ([col("a"), op(Q.X_ADD, 2)], "pops more than there is"),
        ([col("a"), col("b"), op(Q.X_ADD, 1)], "add of one"),
        ([col("a"), col("b"), col("c"), op(Q.X_SUB, 3)], "sub of three"),
        ([col("a"), col("b"), op(Q.X_DIV, 1)], "div of one"),
        ([col("a"), col("b"), op(Q.X_ABS, 2)], "abs of two"),
        ([col("a"), op(Q.X_LEAST, 1)], "least of one"),
        ([lit(2.0), op(Q.X_SQRT, 1)], "sqrt of a literal"),
        ([lit(2.0), op(Q.X_SIGN, 1), col("a"), op(Q.X_ADD, 2)], "sign of a literal inside"),
        ([lit(1.0), lit(2.0), op(Q.X_ADD, 2)], "no column"),
        ([(Q.X_COLUMN, 0, None, 0.0)], "column without a name"),
        ([(Q.X_COLUMN, 0, "", 0.0)], "empty column name"),
        ([col("a")] + [x for _ in range(16) for x in (col("a"), op(Q.X_ADD, 2))], "33 nodes"),
        ([col(f"c{i}") for i in range(9)] + [op(Q.X_ADD, 9)], "9 columns"),
    ]
    for rows, why in bad:
        rc, msg = _define(L, qh, rows)
        assert rc == EINVAL, (why, rc, msg)
        assert "define_expression" in msg, (why, msg)
    for kind in (14, 99, -1):
        rc, msg = _define(L, qh, [col("a"), op(kind, 1)])
        assert rc == EUNSUPPORTED and "not supported" in msg, (kind, rc, msg)
    from pinot_amd._lib import XNode
    out = C.c_char_p()
    assert L.pinot_amd_query_define_expression(qh, None, 1, C.byref(out)) == EINVAL
    assert L.pinot_amd_query_define_expression(None, (XNode * 1)(), 1, C.byref(out)) == EINVAL
    assert L.pinot_amd_query_define_expression(qh, (XNode * 1)(), 1, None) == EINVAL
    # 32 nodes and 8 columns are taken
    assert _define(L, qh, [col("a")] + [x for _ in range(15) for x in (col("a"), op(Q.X_ADD, 2))] + [op(Q.X_ABS, 1)])[0] == 0
    assert _define(L, qh, [col(f"c{i}") for i in range(8)] + [op(Q.X_GREATEST, 8)])[0] == 0
    # the name where a column's is taken; a key transform or an installed key space of it: EUNSUPPORTED
    name = n1.encode()
    assert L.pinot_amd_query_add_group_by(qh, name) == 0
    assert L.pinot_amd_query_add_aggregation(qh, 1, name, None) == 0
    assert L.pinot_amd_query_add_aggregation_param(qh, 8, name, 95.0, None) == 0
    from pinot_amd import engine as E
    spec = E.key_transform_spec(Q.key_transform("dateTrunc('hour', ts)"))
    assert L.pinot_amd_query_add_group_by_transform(qh, name, C.byref(spec)) == EUNSUPPORTED
    vals = (C.c_double * 2)(0.0, 1.0)
    assert L.pinot_amd_query_set_group_key_values(qh, name, 3, 2, None, vals, None) == EUNSUPPORTED
    L.pinot_amd_query_destroy(qh)
