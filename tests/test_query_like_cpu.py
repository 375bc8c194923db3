"""LIKE / REGEXP_LIKE in the SQL front end: the parser forms, RegexpLikePredicate.toString in predicate_text /
filter_text (WHERE and FILTER lanes), the CNF with negation, and the errors."""
import pytest

from pinot_amd.query import (FilterContext, Predicate, filter_text, like_to_regexp, parse_sql, predicate_text,
                             regexp_case_insensitive, to_cnf)


def where(sql_filter: str) -> FilterContext:
    return parse_sql("SELECT COUNT(*) FROM t WHERE " + sql_filter, pattern_predicates=True).filter


def test_pattern_predicates_are_opt_in():
    # parse_sql's default keeps rejecting them (its QueryContexts also go to consumers without pattern support)
    for f in ("a LIKE 'x'", "a NOT LIKE 'x%'", "REGEXP_LIKE(a, 'x')", "NOT REGEXP_LIKE(a, 'x', 'i')"):
        with pytest.raises(ValueError, match="pattern predicates"):
            parse_sql("SELECT COUNT(*) FROM t WHERE " + f)
        with pytest.raises(ValueError, match="pattern predicates"):
            parse_sql(f"SELECT SUM(n) FILTER (WHERE {f}) FROM t")
        assert where(f) is not None
    # the two modes do not share parsed queries
    sql = "SELECT COUNT(*) FROM t WHERE a LIKE 'y'"
    assert parse_sql(sql, pattern_predicates=True).filter.predicate.type == "REGEXP_LIKE"
    with pytest.raises(ValueError):
        parse_sql(sql)


def test_like_is_case_insensitive_regexp_like():
    f = where("url LIKE '%checkout%'")
    assert f.type == "PREDICATE"
    assert f.predicate == Predicate("REGEXP_LIKE", "url", ("checkout",), case_insensitive=True)
    assert where("url LIKE 'https://a%'").predicate.values == ("^https:\\/\\/a",)
    assert like_to_regexp("https://a%") == "^https:\\/\\/a"
    assert where("c LIKE ''").predicate.values == ("^$",)
    assert where("c LIKE '%'").predicate.values == ("",)
    assert where("c LIKE 'it''s_%'").predicate.values == ("^it's.",)


def test_not_like_and_not_regexp_like_are_negated_leaves():
    f = where("c NOT LIKE 'a%'")
    assert f.type == "NOT" and f.children[0].predicate == Predicate("REGEXP_LIKE", "c", ("^a",), case_insensitive=True)
    g = where("NOT REGEXP_LIKE(c, 'a|b')")
    assert g.type == "NOT" and g.children[0].predicate == Predicate("REGEXP_LIKE", "c", ("a|b",))
    (leaf,), = to_cnf(f)
    assert leaf == (f.children[0].predicate, True)
    with pytest.raises(NotImplementedError):
        f.children[0].predicate.negated()


def test_regexp_like_forms():
    assert where("REGEXP_LIKE(c, '^a.*b$')").predicate == Predicate("REGEXP_LIKE", "c", ("^a.*b$",))
    assert where("regexp_like(c, 'x', 'i')").predicate == Predicate("REGEXP_LIKE", "c", ("x",), case_insensitive=True)
    assert where("REGEXP_LIKE(c, 'x', 'I')").predicate.case_insensitive is True
    assert where("REGEXP_LIKE(c, 'x', 'c')").predicate.case_insensitive is False
    assert where("REGEXP_LIKE(c, 'x', 'C')").predicate.case_insensitive is False
    assert where("REGEXP_LIKE(c, 'x', '')").predicate.case_insensitive is False
    assert regexp_case_insensitive("i") and not regexp_case_insensitive("c") and not regexp_case_insensitive("")


def test_text():
    assert predicate_text(where("REGEXP_LIKE(c, 'a|b')").predicate) == "regexp_like(c,'a|b')"
    assert predicate_text(where("REGEXP_LIKE(c, 'a|b', 'i')").predicate) == "regexp_like(c,'a|b','i')"
    assert predicate_text(where("c LIKE 'C+%'").predicate) == "regexp_like(c,'^C\\+','i')"
    f = where("c LIKE '%x' AND (n > 3 OR NOT REGEXP_LIKE(d, '^y'))")
    assert filter_text(f) == "(regexp_like(c,'x$','i') AND (n > '3' OR (NOT regexp_like(d,'^y'))))"
    assert filter_text(where("c NOT LIKE 'a_'")) == "(NOT regexp_like(c,'^a.$','i'))"


def test_filter_lanes():
    qc = parse_sql("SELECT COUNT(*), SUM(n) FILTER (WHERE url LIKE '%cart%'), "
                   "MAX(n) FILTER (WHERE NOT REGEXP_LIKE(url, '^http:') AND n < 5) FROM t WHERE n >= 0",
                   pattern_predicates=True)
    a = qc.aggregations
    assert a[0].filter is None
    assert filter_text(a[1].filter) == "regexp_like(url,'cart','i')"
    assert a[1].text == "sum(n) FILTER(WHERE regexp_like(url,'cart','i'))"
    assert filter_text(a[2].filter) == "((NOT regexp_like(url,'^http:')) AND n < '5')"
    assert a[2].cnf == [[(Predicate("REGEXP_LIKE", "url", ("^http:",)), True)],
                          [(Predicate("RANGE", "n", upper=5, upper_inclusive=False), False)]]


def test_cnf_with_negation():
    f = where("NOT (a LIKE 'x%' AND REGEXP_LIKE(b, 'y')) OR n = 1")
    pa = Predicate("REGEXP_LIKE", "a", ("^x",), case_insensitive=True)
    pb = Predicate("REGEXP_LIKE", "b", ("y",))
    assert to_cnf(f) == [[(pa, True), (pb, True), (Predicate("EQ", "n", (1,)), False)]]
    g = where("a LIKE 'x' OR (b LIKE 'y' AND n IN (1, 2))")
    px = Predicate("REGEXP_LIKE", "a", ("^x$",), case_insensitive=True)
    py = Predicate("REGEXP_LIKE", "b", ("^y$",), case_insensitive=True)
    assert to_cnf(g) == [[(px, False), (py, False)], [(px, False), (Predicate("IN", "n", (1, 2)), False)]]
    # two patterns on one column stay two leaves
    assert len(to_cnf(where("a LIKE 'x%' AND a LIKE '%y'"))) == 2


def test_other_clauses_keep_working():
    qc = parse_sql("SELECT c, COUNT(*) FROM t WHERE c LIKE 'a%' GROUP BY c ORDER BY c LIMIT 5", pattern_predicates=True)
    assert qc.group_by == ["c"] and qc.limit == 5
    qs = parse_sql("SELECT c, n FROM t WHERE REGEXP_LIKE(c, 'a') ORDER BY n DESC LIMIT 3", pattern_predicates=True)
    assert qs.is_selection()


@pytest.mark.parametrize("sql, word", [
    ("REGEXP_LIKE(c, 'x', 'g')", "match parameter"),
    ("REGEXP_LIKE(c, 'x', 'ii')", "one character"),
    ("REGEXP_LIKE(c, 5)", "string literal"),
    ("REGEXP_LIKE(c)", "','"),
    ("REGEXP_LIKE(c, 'x', 1)", "string literal"),
    ("REGEXP_LIKE(c, 'x', 'i', 'y')", "')'"),
    ("REGEXP_LIKE('x', c)", "identifier"),
    ("c LIKE 5", "string literal"),
    ("c LIKE", "string literal"),
    ("c NOT LIKE n", "string literal"),
    ("(a - b) LIKE 'x'", "LIKE"),
])
def test_errors(sql, word):
    with pytest.raises(ValueError) as e:
        where(sql)
    assert word in str(e.value), str(e.value)
