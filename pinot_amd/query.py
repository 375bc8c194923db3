"""QueryContext for the segment-execution path: a small SQL front end and the filter's CNF form.

Mirrors the pieces of pinot-core's request context that the hot path consumes
(pinot-common/.../request/context/predicate/*Predicate.java, FilterContext.java,
pinot-core/.../query/request/context/QueryContext.java): aggregation functions, GROUP BY
expressions, the filter tree, ORDER BY / LIMIT / OFFSET for the final reduce, and the numGroupsLimit
query option. A query with neither aggregations nor GROUP BY is a selection query (SelectionPlanNode). Only the SQL this path executes is accepted (identifiers, numeric/string
literals, comparisons, BETWEEN, [NOT] IN, AND/OR/NOT); anything else raises ValueError.
"""
from __future__ import annotations

import collections
import dataclasses
import functools
import math
import re
import struct
from typing import List, Optional, Sequence, Tuple

import numpy as np

AGG_FUNCS = ("COUNT", "SUM", "MIN", "MAX", "AVG", "SUMLONG", "MINMAXRANGE", "DISTINCTCOUNT", "PERCENTILE",
             "DISTINCTSUM", "DISTINCTAVG", "COUNTMV", "SUMMV", "MINMV", "MAXMV", "AVGMV", "MINMAXRANGEMV",
             "DISTINCTCOUNTHLL")
# the aggregations over a multi-value column: every value of a matching doc counts (CountMV / SumMV / MinMV / MaxMV /
# AvgMV / MinMaxRangeMVAggregationFunction); partials as their SV parents': AVGMV (sum, count of values),
# MINMAXRANGEMV (min, max)
MV_FUNCS = ("COUNTMV", "SUMMV", "MINMV", "MAXMV", "AVGMV", "MINMAXRANGEMV")
# the aggregations answered from a (group-by columns..., column) COUNT(*) query: each group's histogram over the
# column's distinct values (split_distinct_count)
VALUE_SET_FUNCS = ("DISTINCTCOUNT", "PERCENTILE", "DISTINCTSUM", "DISTINCTAVG", "DISTINCTCOUNTHLL")
# DistinctCountHLLAggregationFunction: log2m of DISTINCTCOUNTHLL(c) (CommonConstants.Helix.DEFAULT_HYPERLOGLOG_LOG2M)
# and the range the engine takes
HLL_DEFAULT_LOG2M, HLL_MIN_LOG2M, HLL_MAX_LOG2M = 8, 4, 16
# the sketch functions the engine refuses by name (canonical: upper case, no underscores)
HLL_REFUSED_FUNCS = ("DISTINCTCOUNTRAWHLL", "DISTINCTCOUNTHLLPLUS", "DISTINCTCOUNTRAWHLLPLUS", "DISTINCTCOUNTSMARTHLL",
                     "DISTINCTCOUNTHLLMV", "DISTINCTCOUNTRAWHLLMV", "DISTINCTCOUNTHLLPLUSMV")
DEFAULT_GROUP_BY_LIMIT = 10          # Pinot's default LIMIT for group-by results
DEFAULT_NUM_GROUPS_LIMIT = 100_000   # InstancePlanMakerImplV2.DEFAULT_NUM_GROUPS_LIMIT


@dataclasses.dataclass(frozen=True)
class Predicate:
    """EQ / NOT_EQ / IN / NOT_IN / RANGE / REGEXP_LIKE on one column (RangePredicate: None bound = UNBOUNDED;
    RegexpLikePredicate: values = (pattern,), case_insensitive = match parameter 'i'; a LIKE is the REGEXP_LIKE of
    like_to_regexp's pattern with 'i')."""
    type: str
    column: str
    values: Tuple = ()
    lower: object = None
    upper: object = None
    lower_inclusive: bool = True
    upper_inclusive: bool = True
    case_insensitive: bool = False

    def negated(self) -> "Predicate":
        flip = {"EQ": "NOT_EQ", "NOT_EQ": "EQ", "IN": "NOT_IN", "NOT_IN": "IN"}
        if self.type in flip:
            return dataclasses.replace(self, type=flip[self.type])
        raise NotImplementedError  # RANGE / REGEXP_LIKE negation is represented with a negate flag


@dataclasses.dataclass
class FilterContext:
    type: str  # AND | OR | NOT | PREDICATE
    children: List["FilterContext"] = dataclasses.field(default_factory=list)
    predicate: Optional[Predicate] = None

    @staticmethod
    def pred(p: Predicate) -> "FilterContext":
        return FilterContext("PREDICATE", predicate=p)

    @staticmethod
    def and_(*c) -> "FilterContext":
        return FilterContext("AND", list(c))

    @staticmethod
    def or_(*c) -> "FilterContext":
        return FilterContext("OR", list(c))

    @staticmethod
    def not_(c) -> "FilterContext":
        return FilterContext("NOT", [c])


Leaf = Tuple[Predicate, bool]  # (predicate, negate)


def to_cnf(f: Optional[FilterContext]) -> List[List[Leaf]]:
    """AND of OR-clauses of (predicate, negate) leaves; NOT is pushed to the leaves (De Morgan)."""
    if f is None:
        return []

    def nnf(node: FilterContext, neg: bool):
        if node.type == "PREDICATE":
            return ("LEAF", (node.predicate, neg))
        if node.type == "NOT":
            return nnf(node.children[0], not neg)
        op = node.type
        if neg:
            op = "OR" if op == "AND" else "AND"
        return (op, [nnf(c, neg) for c in node.children])

    def cnf(n) -> List[List[Leaf]]:
        if n[0] == "LEAF":
            return [[n[1]]]
        parts = [cnf(c) for c in n[1]]
        if n[0] == "AND":
            out = []
            for p in parts:
                out.extend(p)
            return out
        # OR: distribute
        acc = [[]]
        for p in parts:
            acc = [a + b for a in acc for b in p]
        return acc

    return cnf(nnf(f, False))


def _literal_text(v) -> str:
    """A predicate literal as the reference's predicates hold it (a string): 9999 -> 9999, 1.5 -> 1.5."""
    return v if isinstance(v, str) else repr(v)


REGEXP_METACHARACTERS = "^$.{}[]()*+?|<>-&/"


def like_to_regexp(like: str) -> str:
    """RegexpPatternConverterUtils.likeToRegexpLike: the REGEXP_LIKE pattern of a LIKE pattern."""
    start, end, prefix, suffix = 0, len(like), "^", "$"
    if not like:
        return "^$"
    if len(like) == 1:
        if like == "%":
            return ""
    else:
        if like[0] == "%":
            start = next((i for i, ch in enumerate(like) if ch != "%"), -1)
            if start == -1:
                return ""
            prefix = ""
        if like[-1] == "%":
            end = max(i for i, ch in enumerate(like) if ch != "%") + 1
            suffix = ""
    out, prev_backslash = [prefix], False
    for ch in like[start:end]:
        if ch == "_":
            out.append(ch if prev_backslash else ".")
        elif ch == "%":
            out.append(ch if prev_backslash else ".*")
        else:
            # a metacharacter, or a backslash that escaped no wildcard: escaped in the output
            if ch in REGEXP_METACHARACTERS or prev_backslash:
                out.append("\\")
            out.append(ch)
        prev_backslash = ch == "\\"
    if prev_backslash:
        out.append("\\")
    return "".join(out) + suffix


def regexp_case_insensitive(match_parameter: str) -> bool:
    """RegexpPatternConverterUtils.isCaseInsensitive: '' / 'c' / 'C' -> False, 'i' / 'I' -> True."""
    if not match_parameter:
        return False
    if len(match_parameter) != 1:
        raise ValueError(f"REGEXP_LIKE: match parameter must be exactly one character, got {match_parameter!r}")
    if match_parameter.lower() == "i":
        return True
    if match_parameter.lower() == "c":
        return False
    raise ValueError(f"REGEXP_LIKE: unsupported match parameter {match_parameter!r} (only 'i' and 'c')")


def predicate_text(p: Predicate) -> str:
    """EqPredicate / NotEqPredicate / InPredicate / NotInPredicate / RangePredicate / RegexpLikePredicate.toString."""
    if p.type == "REGEXP_LIKE":
        return f"regexp_like({p.column},'{p.values[0]}'" + (",'i')" if p.case_insensitive else ")")
    if p.type in ("EQ", "NOT_EQ"):
        return f"{p.column} {'=' if p.type == 'EQ' else '!='} '{_literal_text(p.values[0])}'"
    if p.type in ("IN", "NOT_IN"):
        vals = ",".join(f"'{_literal_text(v)}'" for v in p.values)
        return f"{p.column} {'IN' if p.type == 'IN' else 'NOT IN'} ({vals})"
    lo = None if p.lower is None else f"{p.column} {'>=' if p.lower_inclusive else '>'} '{_literal_text(p.lower)}'"
    hi = None if p.upper is None else f"{p.column} {'<=' if p.upper_inclusive else '<'} '{_literal_text(p.upper)}'"
    if lo is None or hi is None:
        return hi if lo is None else lo
    if p.lower_inclusive and p.upper_inclusive:
        return f"{p.column} BETWEEN '{_literal_text(p.lower)}' AND '{_literal_text(p.upper)}'"
    return f"({lo} AND {hi})"


def filter_text(f: FilterContext) -> str:
    """FilterContext.toString: what getResultColumnName prints after FILTER(WHERE."""
    if f.type == "PREDICATE":
        return predicate_text(f.predicate)
    if f.type == "NOT":
        return f"(NOT {filter_text(f.children[0])})"
    return "(" + f" {f.type} ".join(filter_text(c) for c in f.children) + ")"


EXPR_OPS = {"*": "MUL", "-": "SUB", "+": "ADD"}
EXPR_FUNC = {"MUL": "times", "SUB": "minus", "ADD": "plus"}


def agg_text(func: str, column: str, param=None) -> str:
    """percentile50(c) for PERCENTILE50(c), PERCENTILE(c, 50) and PERCENTILE(c, '50') alike; percentile(c,99.9)."""
    if func == "PERCENTILE":
        p = float(param)
        return f"percentile{int(p)}({column})" if p.is_integer() else f"percentile({column},{p!r})"
    return f"{func.lower()}({column})"


_PERCENTILE_N = re.compile(r"^PERCENTILE(\d{1,3})$")


def check_percentile(p) -> float:
    """AggregationFunctionFactory.java:534-536: 0 <= percentile <= 100."""
    p = float(p)
    if not 0.0 <= p <= 100.0:  # NaN fails both comparisons
        raise ValueError(f"percentile {p!r} not in [0, 100]")
    return p


def check_log2m(v) -> int:
    """DISTINCTCOUNTHLL's second argument: an integer, 4 <= log2m <= 16 here."""
    if isinstance(v, str) and v.strip().lstrip("+").isdigit():
        v = int(v)
    if isinstance(v, bool) or not isinstance(v, int) or not HLL_MIN_LOG2M <= v <= HLL_MAX_LOG2M:
        raise ValueError(f"DISTINCTCOUNTHLL: log2m {v!r} is not an integer in [{HLL_MIN_LOG2M}, {HLL_MAX_LOG2M}]")
    return v


def agg_head(word: str):
    """(function, percentile or None) when `word` names an aggregation function -- PERCENTILE with up to three
    digits after the name carries its percentile (AggregationFunctionFactory.java:143,191) -- else None."""
    w = word.upper()
    if w in AGG_FUNCS:
        return w, None
    if w.replace("_", "") in MV_FUNCS:  # Pinot canonicalises function names: SUM_MV is SUMMV
        return w.replace("_", ""), None
    if w.replace("_", "") == "DISTINCTCOUNTHLL":  # distinct_count_hll
        return "DISTINCTCOUNTHLL", None
    if w.replace("_", "") in HLL_REFUSED_FUNCS:
        raise ValueError(f"{word} is not supported: of the sketch functions only DISTINCTCOUNTHLL over a single-value "
                         "column (raw / HLL++ / smart sketches and multi-value columns are not)")
    m = _PERCENTILE_N.match(w)
    if m:
        return "PERCENTILE", check_percentile(m.group(1))
    return None


@dataclasses.dataclass
class Aggregation:
    """AggregationFunction over a column or a binary arithmetic transform of two columns.

    column: "*" for COUNT(*), the column name, or the expression's canonical text
    (``times(a,b)``, Pinot's FunctionContext names) for an expression argument.
    expr: None for a plain column, else (op, column_a, column_b) with op MUL / SUB / ADD
    (MultiplicationTransformFunction / SubtractionTransformFunction / AdditionTransformFunction;
    CAST(x AS DOUBLE) operands are accepted: every transform already computes in double)."""
    func: str          # COUNT SUM MIN MAX AVG SUMLONG MINMAXRANGE DISTINCTCOUNT PERCENTILE DISTINCTSUM DISTINCTAVG
                       # COUNTMV SUMMV MINMV MAXMV AVGMV MINMAXRANGEMV
    column: str
    alias: Optional[str] = None
    expr: Optional[Tuple[str, str, str]] = None
    param: Optional[float] = None   # PERCENTILE: the percentile, 0 <= param <= 100
    # AGG(...) FILTER (WHERE filter): the aggregation takes the docs matching the query's filter AND this one
    # (AggregationFunctionUtils.buildFilteredAggregationInfos); None: the query's filter alone
    filter: Optional[FilterContext] = None

    @property
    def text(self) -> str:
        """The function's canonical text (what ORDER BY names when there is no alias); a filtered aggregation's is
        AggregationFunctionUtils.getResultColumnName: ``sum(x) FILTER(WHERE x > '9999')``."""
        t = agg_text(self.func, self.column, self.param)
        return t if self.filter is None else f"{t} FILTER(WHERE {filter_text(self.filter)})"

    @property
    def cnf(self) -> List[List[Leaf]]:
        """The aggregation filter in conjunctive normal form ([] without one)."""
        return to_cnf(self.filter)

    @property
    def name(self) -> str:
        return self.alias or self.text

    @property
    def columns(self) -> Tuple[str, ...]:
        if self.column == "*":
            return ()
        if self.expr:
            return (self.expr[1], self.expr[2])
        e = expression(self.column)
        return tuple(expr_columns(e)) if e is not None else (self.column,)


TIME_UNITS = ("NANOSECONDS", "MICROSECONDS", "MILLISECONDS", "SECONDS", "MINUTES", "HOURS", "DAYS")  # TimeUnit
TRUNC_UNITS = ("millisecond", "second", "minute", "hour", "day", "week", "month", "quarter", "year")
KEY_TRANSFORMS = ("datetrunc", "timeconvert", "datetimeconvert")  # canonical names: lower case, no underscores


@dataclasses.dataclass(frozen=True)
class KeyTransform:
    """A GROUP BY key that is a time-bucket function of one INT / LONG column (pinot_amd_key_transform_spec):
    dateTrunc(unit, col [, inputUnit [, tz [, outputUnit]]]), timeConvert(col, inputUnit, outputUnit) or
    dateTimeConvert(col, 'a:U:EPOCH', 'b:W:EPOCH', 'g:G'). Units are TimeUnit names; the key is a LONG."""
    kind: str                 # datetrunc | timeconvert | datetimeconvert
    column: str
    in_unit: str = "MILLISECONDS"
    out_unit: str = "MILLISECONDS"
    trunc_unit: Optional[str] = None   # datetrunc
    in_size: int = 1                   # datetimeconvert
    out_size: int = 1
    gran_unit: Optional[str] = None
    gran_size: int = 1

    @property
    def text(self) -> str:
        """The canonical text: what QueryContext.group_by holds and SELECT / ORDER BY items are matched by."""
        if self.kind == "datetrunc":
            return f"datetrunc('{self.trunc_unit}',{self.column},'{self.in_unit}','UTC','{self.out_unit}')"
        if self.kind == "timeconvert":
            return f"timeconvert({self.column},'{self.in_unit}','{self.out_unit}')"
        return (f"datetimeconvert({self.column},'{self.in_size}:{self.in_unit}:EPOCH',"
                f"'{self.out_size}:{self.out_unit}:EPOCH','{self.gran_size}:{self.gran_unit}')")


def _time_unit(s, what: str, func: str) -> str:
    u = str(s).upper()
    if u in ("WEEKS", "MONTHS", "YEARS"):  # CustomTimeUnitTransformer / DateTimeFormatUnitSpec's custom units
        raise ValueError(f"{func}: {what} {u} is not supported (only TimeUnit NANOSECONDS .. DAYS)")
    if u not in TIME_UNITS:
        raise ValueError(f"{func}: bad {what} {s!r}")
    return u


def _epoch_format(s, what: str) -> Tuple[int, str]:
    """'size:UNIT:EPOCH' (DateTimeFormatSpec's colon form) -> (size, unit)."""
    parts = str(s).split(":")
    fmt = parts[2].upper() if len(parts) >= 3 else ""
    if "|" in str(s) or fmt in ("SIMPLE_DATE_FORMAT", "TIMESTAMP") or len(parts) > 3:
        raise ValueError(f"dateTimeConvert: {what} {s!r} is not supported (only 'size:UNIT:EPOCH')")
    if len(parts) != 3 or fmt != "EPOCH":
        raise ValueError(f"dateTimeConvert: bad {what} {s!r}")
    return _positive_size(parts[0], what), _time_unit(parts[1], what + " unit", "dateTimeConvert")


def _positive_size(s, what: str) -> int:
    try:
        n = int(s)
    except ValueError:
        raise ValueError(f"dateTimeConvert: bad {what} size {s!r}") from None
    if n <= 0:
        raise ValueError(f"dateTimeConvert: {what} size must be positive, not {n}")
    return n


def make_key_transform(func: str, args: Sequence[Tuple[str, object]]) -> KeyTransform:
    """The KeyTransform of a call: func is the canonical name, args are ('id' | 'str' | 'num', value) tokens.
    Optional arguments take Pinot's defaults; unsupported forms raise ValueError naming the form."""
    def strs(items, what):
        for k, v in items:
            if k != "str":
                raise ValueError(f"{what}: expected a string literal, not {v!r}")
        return [v for _, v in items]

    if func == "datetrunc":   # DateTruncTransformFunction.init
        if not 2 <= len(args) <= 5:
            raise ValueError("dateTrunc takes two to five arguments")
        if args[0][0] not in ("str", "id") or args[1][0] != "id":
            raise ValueError("dateTrunc(unit, column, ...): the unit is a literal, the value a column")
        unit = str(args[0][1]).lower()
        if unit not in TRUNC_UNITS:
            raise ValueError(f"dateTrunc: bad unit {args[0][1]!r}")
        rest = strs(args[2:], "dateTrunc")
        in_unit = _time_unit(rest[0], "input unit", "dateTrunc") if rest else "MILLISECONDS"
        if len(rest) >= 2 and rest[1].upper() != "UTC":
            raise ValueError(f"dateTrunc: time zone {rest[1]!r} is not supported (only UTC)")
        out_unit = _time_unit(rest[2], "output unit", "dateTrunc") if len(rest) >= 3 else in_unit
        return KeyTransform("datetrunc", args[1][1], in_unit, out_unit, trunc_unit=unit)
    if func == "timeconvert":  # TimeConversionTransformFunction.init
        if len(args) != 3 or args[0][0] != "id":
            raise ValueError("timeConvert(column, inputUnit, outputUnit) takes a column and two units")
        rest = strs(args[1:], "timeConvert")
        return KeyTransform("timeconvert", args[0][1], _time_unit(rest[0], "input unit", "timeConvert"),
                            _time_unit(rest[1], "output unit", "timeConvert"))
    if func == "datetimeconvert":  # DateTimeConversionTransformFunction.init
        if len(args) == 5:
            raise ValueError("dateTimeConvert: a bucketing time zone argument is not supported")
        if len(args) != 4 or args[0][0] != "id":
            raise ValueError("dateTimeConvert(column, inputFormat, outputFormat, granularity) takes four arguments")
        rest = strs(args[1:], "dateTimeConvert")
        in_size, in_unit = _epoch_format(rest[0], "input format")
        out_size, out_unit = _epoch_format(rest[1], "output format")
        g = rest[2].split(":")
        if len(g) != 2:
            raise ValueError(f"dateTimeConvert: bad granularity {rest[2]!r}")
        gran_unit = _time_unit(g[1], "granularity unit", "dateTimeConvert")
        return KeyTransform("datetimeconvert", args[0][1], in_unit, out_unit, in_size=in_size, out_size=out_size,
                            gran_unit=gran_unit, gran_size=_positive_size(g[0], "granularity"))
    raise ValueError(f"unknown key transform {func}")


def key_transform(text: str) -> Optional[KeyTransform]:
    """The parsed transform of a GROUP BY item's text (canonical or as written), None for a plain column."""
    return _key_transform(text) if "(" in text else None


@functools.lru_cache(maxsize=256)
def _key_transform(text: str) -> Optional[KeyTransform]:
    p = _Parser(text)
    if not p.transform_ahead():
        return None
    kt = p.transform_call()
    if p.peek()[0] != "eof":
        raise ValueError(f"unexpected trailing token {p.peek()}")
    return kt


# ------------------------------------------------------------------------------ arithmetic expressions
# pinot_amd_xnode_kind, and the reference's function names (TransformFunctionType: ADD("add", "plus"), ... -- a call
# keeps the name it was written with, lower case and without underscores; an operator is plus / minus / times /
# divide / mod, CalciteSqlParser's canonical SqlKind names)
X_COLUMN, X_LITERAL, X_ADD, X_SUB, X_MULT, X_DIV, X_MOD, X_ABS, X_CEIL, X_FLOOR, X_SQRT, X_SIGN, X_LEAST, X_GREATEST = range(14)
ARITH_FUNCS = {"add": X_ADD, "plus": X_ADD, "sub": X_SUB, "minus": X_SUB, "mult": X_MULT, "times": X_MULT,
               "div": X_DIV, "divide": X_DIV, "mod": X_MOD, "abs": X_ABS, "ceil": X_CEIL, "ceiling": X_CEIL,
               "floor": X_FLOOR, "sqrt": X_SQRT, "sign": X_SIGN, "least": X_LEAST, "greatest": X_GREATEST}
ARITH_OPS = {"+": "plus", "-": "minus", "*": "times", "/": "divide", "%": "mod"}
# functions whose libm / BigDecimal results are not bit-reproducible on the device: refused by name
UNSUPPORTED_FUNCS = ("exp", "ln", "log", "log2", "log10", "power", "pow", "round", "rounddecimal", "truncate", "sin",
                     "cos", "tan", "asin", "acos", "atan", "atan2", "sinh", "cosh", "tanh", "cot", "degrees", "radians",
                     "cbrt", "case", "cast")


def java_double_text(x: float) -> str:
    """Double.toString: decimal for 1e-3 <= |x| < 1e7, else computerised scientific notation (1.0E10)."""
    x = float(x)
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "Infinity" if x > 0 else "-Infinity"
    if x == 0.0 or 1e-3 <= abs(x) < 1e7:
        return repr(x)
    mant, exp = f"{x!r}".lower().split("e") if "e" in repr(x).lower() else (None, None)
    if mant is None:  # repr printed it in positional notation: normalise the digits
        digits, e10 = f"{x:.17e}".split("e")
        for prec in range(0, 18):  # the shortest digits that read back as x
            cand = f"{x:.{prec}e}"
            if float(cand) == x:
                digits, e10 = cand.split("e")
                break
        mant, exp = digits, e10
    if "." not in mant:
        mant += ".0"
    return f"{mant}E{int(exp)}"


def literal_text(v) -> str:
    """LiteralContext.toString without its quotes: an integral literal as an int / long, anything else as a double."""
    return str(v) if isinstance(v, int) else java_double_text(v)


def expr_text(e) -> str:
    """ExpressionContext.toString of an expression tree: ('col', name) | ('lit', int or float) |
    ('fn', name, [args]) -> times(times(a,b),'1.07')."""
    if e[0] == "col":
        return e[1]
    if e[0] == "lit":
        return f"'{literal_text(e[1])}'"
    if e[0] == "cast":
        raise ValueError("CAST in an expression is not supported")
    return f"{e[1]}({','.join(expr_text(a) for a in e[2])})"


def expr_columns(e) -> List[str]:
    """The distinct columns of an expression tree, in first-use order."""
    out: List[str] = []

    def walk(n):
        if n[0] == "col":
            if n[1] not in out:
                out.append(n[1])
        elif n[0] == "fn":
            for a in n[2]:
                walk(a)
    walk(e)
    return out


def expr_postfix(e) -> List[Tuple[int, int, Optional[str], float]]:
    """pinot_amd_xnode rows (kind, num_args, column, literal) of an expression tree, in postfix."""
    out = []

    def walk(n):
        if n[0] == "col":
            out.append((X_COLUMN, 0, n[1], 0.0))
        elif n[0] == "lit":
            out.append((X_LITERAL, 0, None, float(n[1])))
        elif n[0] == "fn":
            for a in n[2]:
                walk(a)
            out.append((ARITH_FUNCS[n[1]], len(n[2]), None, 0.0))
        else:
            raise ValueError("CAST in an expression is not supported")
    walk(e)
    return out


def check_expr(e) -> None:
    """The arities of the reference's transform functions and the library's limits (32 nodes, 8 columns)."""
    def walk(n):
        if n[0] != "fn":
            return 1
        kind, k = ARITH_FUNCS[n[1]], len(n[2])
        if kind in (X_ADD, X_MULT, X_LEAST, X_GREATEST):
            if k < 2:
                raise ValueError(f"{n[1]} takes two or more arguments")
        elif kind in (X_SUB, X_DIV, X_MOD):
            if k != 2:
                raise ValueError(f"{n[1]} takes exactly two arguments")
        else:
            if k != 1:
                raise ValueError(f"{n[1]} takes exactly one argument")
            if n[2][0][0] == "lit":
                raise ValueError(f"{n[1]} of a literal is not supported (the reference requires a non-literal argument)")
        return 1 + sum(walk(a) for a in n[2])
    if walk(e) > 32:
        raise ValueError("an expression takes at most 32 nodes")
    if len(expr_columns(e)) > 8:
        raise ValueError("an expression takes at most 8 distinct columns")
    if not expr_columns(e):
        raise ValueError("an expression needs a column")


def expression(text: str):
    """The parsed tree of an expression's text (canonical or as written); None for a plain column, a key transform
    and COUNT's `*`."""
    return _expression(text) if "(" in text else None


@functools.lru_cache(maxsize=512)
def _expression(text: str):
    p = _Parser(text)
    if p.transform_ahead():
        return None
    e = p.value_expr()
    if p.peek()[0] != "eof":
        raise ValueError(f"unexpected trailing token {p.peek()}")
    return None if e[0] == "col" else e


def parse_expression(text: str):
    """The tree of an arithmetic expression as written (`a * b + 2`) or in canonical text; a plain column is
    ('col', name)."""
    p = _Parser(text)
    e = p.value_expr()
    if p.peek()[0] != "eof":
        raise ValueError(f"unexpected trailing token {p.peek()}")
    return e


@dataclasses.dataclass
class QueryContext:
    table: str
    aggregations: List[Aggregation]
    group_by: List[str]
    filter: Optional[FilterContext]
    order_by: List[Tuple[str, bool]]   # (expression or alias, ascending)
    limit: int
    select_columns: List[str]           # plain columns in the SELECT list (group-by outputs)
    num_groups_limit: int = DEFAULT_NUM_GROUPS_LIMIT
    # the server combine table's trim options (QueryOptionsUtils: minServerGroupTrimSize, groupTrimThreshold)
    min_server_group_trim_size: int = 5000
    min_segment_group_trim_size: int = -1  # QueryOptions minSegmentGroupTrimSize (CommonConstants.java:1436)
    group_trim_threshold: int = 1_000_000
    # serverReturnFinalResult, sortAggregateLimitThreshold (CommonConstants: default 10000)
    server_return_final_result: bool = False
    sort_aggregate_limit_threshold: int = 10_000
    offset: int = 0                     # LIMIT n OFFSET m / LIMIT m, n (the broker applies it; a server keeps offset + limit)
    # filteredAggregationsSkipEmptyGroups: with only filtered aggregations, a group exists iff some lane has a doc
    filtered_aggregations_skip_empty_groups: bool = False
    # SELECT DISTINCT a, b ... (DistinctPlanNode): the distinct columns are group_by (= select_columns), in list order
    distinct: bool = False

    def is_distinct(self) -> bool:
        """SELECT DISTINCT columns [WHERE] [ORDER BY] [LIMIT]: the distinct rows of the columns (DistinctPlanNode)."""
        return self.distinct

    def has_filtered_aggregations(self) -> bool:
        return any(a.filter is not None for a in self.aggregations)

    def expressions(self) -> List[str]:
        """The texts of the query's arithmetic expressions (in filters, aggregation arguments and filters, GROUP BY,
        SELECT and ORDER BY items), each once; not the two-column form SUM / MIN / MAX / AVG keep (Aggregation.expr)."""
        out: List[str] = []

        def note(text):
            if text != "*" and text not in out and expression(text) is not None:
                out.append(text)
        for clause in self.cnf:
            for p, _ in clause:
                note(p.column)
        for a in self.aggregations:
            if a.expr is None:
                note(a.column)
            for clause in a.cnf:
                for p, _ in clause:
                    note(p.column)
        for g in list(self.group_by) + list(self.select_columns):
            note(g)
        if self.is_selection():
            for c, _ in self.order_by:
                note(c)
        return out

    def is_selection(self) -> bool:
        """SELECT columns [ORDER BY ...] LIMIT n: neither aggregations nor GROUP BY (SelectionPlanNode)."""
        return not self.aggregations and not self.group_by

    def select_list(self, segment=None) -> List[str]:
        """The selected columns in select-list order, `*` expanded to every column of `segment` (an object with a
        `columns` mapping) in String order (SelectionOperatorUtils.java:100-115), duplicates kept once."""
        out = []
        for c in self.select_columns:
            if c == "*":
                if segment is None:
                    raise ValueError("SELECT * needs a segment to expand")
                names = sorted(segment.columns, key=lambda n: n.encode("utf-16-be"))
            else:
                names = [c]
            for n in names:
                if n not in out:
                    out.append(n)
        return out

    def selection_columns(self, segment=None) -> List[str]:
        """The server's selection schema (SelectionOperatorUtils.extractExpressions, java:83-125): the ORDER BY
        columns, deduplicated and in ORDER BY order, then the selected columns not among them in select-list order.
        With LIMIT 0 the ORDER BY is ignored."""
        out = []
        if self.limit + self.offset > 0:
            for c, _ in self.order_by:
                if c not in out:
                    out.append(c)
        for c in self.select_list(segment):
            if c not in out:
                out.append(c)
        return out

    def safe_trim(self) -> bool:
        """QueryContext._isUnsafeTrim is false: the ORDER BY expressions, as a set, are the GROUP BY ones (no
        HAVING in this subset) -- QueryContext.java:746-747, isSameOrderAndGroupByColumns."""
        if not self.group_by or not self.order_by:
            return False
        t = self.order_by_targets()
        return all(k == 0 for k, _, _ in t) and {i for _, i, _ in t} == set(range(len(self.group_by)))

    def order_by_targets(self) -> List[Tuple[int, int, bool]]:
        """ORDER BY as (kind, index, ascending): kind 0 = group-by column index, 1 = aggregation index
        (matched by alias or the function text, as the broker's select list does)."""
        out = []
        for expr, asc in self.order_by:
            e = expr.lower().replace(" ", "")
            hit = None
            for j, g in enumerate(self.group_by):
                if e == g.lower():
                    hit = (0, j)
            for i, a in enumerate(self.aggregations):
                if e in (a.name.lower().replace(" ", ""), a.text.lower().replace(" ", "")):
                    hit = (1, i)
            if hit is None:
                raise ValueError(f"ORDER BY {expr} not in select list")
            out.append((hit[0], hit[1], asc))
        return out

    @property
    def cnf(self) -> List[List[Leaf]]:
        return to_cnf(self.filter)


# ---------------------------------------------------------------------------------------- parser
_TOKEN = re.compile(r"\s*(?:(?P<num>-?\d+\.\d*(?:[eE][-+]?\d+)?|-?\d+(?:[eE][-+]?\d+)?)|(?P<str>'(?:[^']|'')*')"
                    r"|(?P<op><>|!=|<=|>=|=|<|>|\(|\)|,|\*|\+|-|/|%)|(?P<id>[A-Za-z_][A-Za-z0-9_.$]*))")


def _tokenize(sql: str):
    pos, out = 0, []
    sql = sql.strip().rstrip(";")
    while pos < len(sql):
        m = _TOKEN.match(sql, pos)
        if not m or m.end() == pos:
            if sql[pos:].strip() == "":
                break
            raise ValueError(f"cannot tokenize at: {sql[pos:pos + 20]!r}")
        pos = m.end()
        if m.group("num") is not None:
            t = m.group("num")
            out.append(("num", float(t) if any(ch in t for ch in ".eE") else int(t)))
        elif m.group("str") is not None:
            out.append(("str", m.group("str")[1:-1].replace("''", "'")))
        elif m.group("op") is not None:
            out.append(("op", m.group("op")))
        else:
            out.append(("id", m.group("id")))
    return out


class _Parser:
    def __init__(self, sql: str, pattern_predicates: bool = False):
        self.t = _tokenize(sql)
        self.i = 0
        self.pattern_predicates = pattern_predicates

    def need_pattern_predicates(self, what: str) -> None:
        if not self.pattern_predicates:
            raise ValueError(f"{what}: pattern predicates are not enabled for this parse "
                             "(parse_sql(sql, pattern_predicates=True); ServerQueryExecutor enables them for SQL text)")

    def peek(self, k=0):
        return self.t[self.i + k] if self.i + k < len(self.t) else ("eof", None)

    def kw(self, *words) -> bool:
        for k, w in enumerate(words):
            tok = self.peek(k)
            if tok[0] != "id" or tok[1].upper() != w:
                return False
        return True

    def eat_kw(self, *words):
        if not self.kw(*words):
            raise ValueError(f"expected {' '.join(words)} at token {self.peek()}")
        self.i += len(words)

    def eat_op(self, op):
        tok = self.peek()
        if tok != ("op", op):
            raise ValueError(f"expected {op!r} at token {tok}")
        self.i += 1

    def ident(self) -> str:
        tok = self.peek()
        if tok[0] != "id":
            raise ValueError(f"expected identifier at {tok}")
        self.i += 1
        return tok[1]

    def literal(self):
        tok = self.peek()
        if tok[0] not in ("num", "str"):
            raise ValueError(f"expected literal at {tok}")
        self.i += 1
        return tok[1]

    def transform_ahead(self) -> bool:
        """At dateTrunc( / timeConvert( / dateTimeConvert( in any letter case, underscores ignored (Pinot
        canonicalises function names the same way)."""
        tok = self.peek()
        return (tok[0] == "id" and tok[1].replace("_", "").lower() in KEY_TRANSFORMS
                and self.peek(1) == ("op", "("))

    def transform_call(self) -> KeyTransform:
        func = self.ident().replace("_", "").lower()
        self.eat_op("(")
        args = []
        while True:
            tok = self.peek()
            if tok[0] not in ("id", "str", "num"):
                raise ValueError(f"{func}: expected a column or a literal at {tok}")
            self.i += 1
            args.append(tok)
            nxt = self.peek()
            if nxt[0] == "num" or (nxt[0] == "op" and nxt[1] in ("+", "-", "*", "/", "%", "(")):
                raise ValueError(f"{func} of an expression is not supported (a key transform takes an INT / LONG column)")
            if nxt != ("op", ","):
                break
            self.i += 1
        self.eat_op(")")
        return make_key_transform(func, args)

    def key_item(self) -> str:
        """A GROUP BY / SELECT / ORDER BY item that is not an aggregation: a column, or a key transform as its
        canonical text."""
        if self.transform_ahead():
            return self.transform_call().text
        e = self.value_expr()
        if e[0] == "col":
            return e[1]
        check_expr(e)
        return expr_text(e)

    # -- arithmetic expressions: unary minus on literals, * / %, + -, parentheses, the function calls --
    def value_expr(self):
        node = self.value_term()
        while True:
            tok = self.peek()
            if tok[0] == "op" and tok[1] in ("+", "-"):
                self.i += 1
                node = ("fn", ARITH_OPS[tok[1]], [node, self.value_term()])
            elif tok[0] == "num" and _is_negative(tok[1]):  # `a -1`: the tokenizer glued the operator to the literal
                node = ("fn", "minus", [node, self.value_term(strip_minus=True)])
            else:
                return node

    def value_term(self, strip_minus=False):
        node = self.value_unary(strip_minus)
        while self.peek()[0] == "op" and self.peek()[1] in ("*", "/", "%"):
            op = self.peek()[1]
            self.i += 1
            node = ("fn", ARITH_OPS[op], [node, self.value_unary()])
        return node

    def value_unary(self, strip_minus=False):
        tok = self.peek()
        if tok[0] == "num":
            self.i += 1
            return ("lit", -tok[1] if strip_minus else tok[1])
        if tok[0] == "str":  # a quoted number, as the canonical text prints its literals
            self.i += 1
            try:
                return ("lit", int(tok[1]))
            except ValueError:
                try:
                    return ("lit", float(tok[1]))
                except ValueError:
                    raise ValueError(f"string literal {tok[1]!r} in an arithmetic expression") from None
        if tok == ("op", "-"):
            if self.peek(1)[0] != "num":
                raise ValueError("unary minus is supported on literals only")
            self.i += 2
            return ("lit", -self.peek(-1)[1])
        if tok == ("op", "("):
            self.i += 1
            e = self.value_expr()
            self.eat_op(")")
            return e
        if tok[0] != "id":
            raise ValueError(f"expected a column, a literal or a function call at {tok}")
        if self.kw("CAST") and self.peek(1) == ("op", "("):
            return ("cast", self.operand())
        if tok[1].upper() == "CASE":
            raise ValueError("CASE is not supported in an expression")
        if self.peek(1) != ("op", "("):
            return ("col", self.ident())
        name = tok[1].replace("_", "").lower()
        if name in KEY_TRANSFORMS:
            raise ValueError(f"the key transform {tok[1]} inside an expression is not supported (only as a GROUP BY key)")
        if agg_head(tok[1]):
            raise ValueError(f"the aggregation {tok[1]} inside an expression is not supported")
        if name not in ARITH_FUNCS:
            why = " (its result is not bit-reproducible on the device)" if name in UNSUPPORTED_FUNCS else ""
            raise ValueError(f"function {tok[1]} is not supported in an expression{why}: only "
                             "add sub mult div mod abs ceil floor sqrt sign least greatest")
        self.i += 2
        args = [self.value_expr()]
        while self.peek() == ("op", ","):
            self.i += 1
            args.append(self.value_expr())
        self.eat_op(")")
        return ("fn", name, args)

    def agg_arg(self, func: str):
        """An aggregation's argument: (column or canonical expression text, two-column (op, a, b) or None). times |
        minus | plus of two plain columns (CAST(column AS numeric type) counts as the column) keeps the two-column
        form of pinot_amd_query_add_aggregation_expr under every function, as before: SUM / MIN / MAX / AVG /
        MINMAXRANGE take it, with the exact int64 sum of INT operands, and the value-set functions keep refusing it
        ("takes one column"; PERCENTILE(a + b + 0, 95) is an expression). Every other expression is a virtual column
        named by its text."""
        e = self.value_expr()
        if e[0] == "col":
            return e[1], None
        if e[0] == "cast":
            return e[1], None
        if (e[0] == "fn" and e[1] in ("times", "minus", "plus") and len(e[2]) == 2
                and all(a[0] in ("col", "cast") for a in e[2])):
            a, b = e[2][0][1], e[2][1][1]
            op = {"times": "MUL", "minus": "SUB", "plus": "ADD"}[e[1]]
            return f"{EXPR_FUNC[op]}({a},{b})", (op, a, b)
        check_expr(e)
        return expr_text(e), None

    # -- grammar --
    def query(self) -> QueryContext:
        self.eat_kw("SELECT")
        # SELECT DISTINCT a, b: the keyword, unless what follows makes it a column named "distinct"
        distinct = self.kw("DISTINCT") and self.peek(1) not in (("op", ","), ("op", "(")) and \
            not (self.peek(1)[0] == "id" and self.peek(1)[1].upper() == "FROM") and self.peek(1)[0] != "eof"
        if distinct:
            self.i += 1
        aggs, cols = [], []
        while True:
            tok = self.peek()
            if tok[0] == "id" and agg_head(tok[1]) and self.peek(1) == ("op", "("):
                func, param = agg_head(tok[1])
                self.i += 2
                expr = None
                if self.peek() == ("op", "*"):
                    self.i += 1
                    col = "*"
                else:
                    col, expr = self.agg_arg(func)
                param = self.percentile_arg(func, param)
                if func == "DISTINCTCOUNTHLL" and (col == "*" or expr is not None or expression(col) is not None):
                    raise ValueError(f"DISTINCTCOUNTHLL({col}) is not supported: it takes one column, not an expression")
                self.eat_op(")")
                agg_filter = self.agg_filter()
                alias = None
                if self.kw("AS"):
                    self.i += 1
                    alias = self.ident()
                elif self.peek()[0] == "id" and self.peek()[1].upper() not in ("FROM",):
                    alias = self.ident()   # implicit alias: sum(x) revenue
                aggs.append(Aggregation(func, col, alias, expr, param, agg_filter))
            elif tok == ("op", "*"):
                self.i += 1
                cols.append("*")
            else:
                cols.append(self.key_item())
            if self.peek() == ("op", ","):
                self.i += 1
                continue
            break
        self.eat_kw("FROM")
        table = self.ident()
        flt = None
        if self.kw("WHERE"):
            self.i += 1
            flt = self.expr()
        group_by = []
        if self.kw("GROUP", "BY"):
            self.i += 2
            group_by.append(self.key_item())
            while self.peek() == ("op", ","):
                self.i += 1
                group_by.append(self.key_item())
        order = []
        if self.kw("ORDER", "BY"):
            self.i += 2
            while True:
                order.append(self.order_item())
                if self.peek() != ("op", ","):
                    break
                self.i += 1
        limit, offset = DEFAULT_GROUP_BY_LIMIT, 0
        if self.kw("LIMIT"):
            self.i += 1
            limit = self.count("LIMIT")
            if self.peek() == ("op", ","):  # LIMIT offset, limit
                self.i += 1
                offset, limit = limit, self.count("LIMIT")
            elif self.kw("OFFSET"):
                self.i += 1
                offset = self.count("OFFSET")
        if self.peek()[0] != "eof":
            raise ValueError(f"unexpected trailing token {self.peek()}")
        if distinct:
            if aggs:
                raise ValueError(f"SELECT DISTINCT takes columns, not an aggregation ({aggs[0].text})")
            if group_by:
                raise ValueError("SELECT DISTINCT takes no GROUP BY")
            if "*" in cols:
                raise ValueError("SELECT DISTINCT * is not supported: name the columns")
            if offset:
                raise ValueError(f"SELECT DISTINCT with OFFSET {offset} is not supported")
            group_by = list(dict.fromkeys(cols))  # (a column listed twice is one distinct column)
            cols = list(group_by)
            for e, _ in order:
                if e not in group_by:  # (both are key_item's canonical text; column names are case-sensitive)
                    raise ValueError(f"ORDER BY {e} is not in the SELECT DISTINCT list")
        if "*" in cols and (aggs or group_by):
            raise ValueError("SELECT * takes no aggregation and no GROUP BY")
        for c in cols + [e for e, _ in order]:
            if "(" in c and key_transform(c) is not None and c not in group_by:
                if not aggs and not group_by:
                    raise ValueError("a key transform in a selection query is not supported (only as a GROUP BY key)")
                raise ValueError(f"{c} is not a GROUP BY key of the query")
        return QueryContext(table, aggs, group_by, flt, order, limit, cols, offset=offset, distinct=bool(distinct))

    def agg_filter(self) -> Optional[FilterContext]:
        """FILTER (WHERE <expr>) behind an aggregation call, or None."""
        if not (self.kw("FILTER") and self.peek(1) == ("op", "(")):
            return None
        self.i += 2
        self.eat_kw("WHERE")
        if self.peek() == ("op", ")"):
            raise ValueError("FILTER (WHERE ...) needs an expression")
        depth, k = 1, 0
        while depth and self.peek(k)[0] != "eof":  # the clause's tokens: a key transform is no filter column
            tok = self.peek(k)
            if tok[0] == "id" and tok[1].replace("_", "").lower() in KEY_TRANSFORMS and self.peek(k + 1) == ("op", "("):
                raise ValueError(f"FILTER (WHERE ...) on the key transform {tok[1]} is not supported")
            depth += (tok == ("op", "(")) - (tok == ("op", ")"))
            k += 1
        f = self.expr()
        self.eat_op(")")
        return f

    def count(self, what: str) -> int:
        v = self.literal()
        if not isinstance(v, int) or v < 0:
            raise ValueError(f"{what} takes a non-negative integer, not {v!r}")
        return v

    def percentile_arg(self, func, param):
        """PERCENTILE(c, 50) / PERCENTILE(c, 99.9) / PERCENTILE(c, '50'): the second argument, unless the
        function's name carried the percentile."""
        if func == "DISTINCTCOUNTHLL":  # DISTINCTCOUNTHLL(c [, log2m]): an integer literal
            log2m = HLL_DEFAULT_LOG2M
            if self.peek() == ("op", ","):
                self.i += 1
                log2m = self.literal()
            return check_log2m(log2m)
        if func != "PERCENTILE":
            return None
        if self.peek() == ("op", ","):
            if param is not None:
                raise ValueError("PERCENTILE<n>(column) takes one argument")
            self.i += 1
            lit = self.literal()
            try:
                param = check_percentile(lit)
            except (TypeError, ValueError):
                raise ValueError(f"bad percentile {lit!r}") from None
        if param is None:
            raise ValueError("PERCENTILE needs its percentile: PERCENTILE50(c) or PERCENTILE(c, 50)")
        return param

    def operand(self) -> str:
        """A column, optionally as CAST(column AS type) (the cast does not change the value the
        arithmetic transforms compute: they read every argument as double)."""
        if self.kw("CAST") and self.peek(1) == ("op", "("):
            self.i += 2
            col = self.ident()
            self.eat_kw("AS")
            t = self.ident().upper()
            if t not in ("DOUBLE", "FLOAT", "LONG", "INT", "BIGINT", "INTEGER"):
                raise ValueError(f"unsupported CAST type {t}")
            self.eat_op(")")
            return col
        return self.ident()

    def order_item(self):
        tok = self.peek()
        if tok[0] == "id" and agg_head(tok[1]) and self.peek(1) == ("op", "("):
            func, param = agg_head(tok[1])
            self.i += 2
            if self.peek() == ("op", "*"):
                col = "*"
                self.i += 1
            else:
                col, _ = self.agg_arg(func)
            param = self.percentile_arg(func, param)
            self.eat_op(")")
            expr = agg_text(func, col, param)
            f = self.agg_filter()
            if f is not None:  # a filtered aggregation named by its result column text
                expr += f" FILTER(WHERE {filter_text(f)})"
        else:
            expr = self.key_item()
        asc = True
        if self.kw("DESC"):
            self.i += 1
            asc = False
        elif self.kw("ASC"):
            self.i += 1
        return (expr, asc)

    def expr(self) -> FilterContext:
        node = self.and_expr()
        children = [node]
        while self.kw("OR"):
            self.i += 1
            children.append(self.and_expr())
        return children[0] if len(children) == 1 else FilterContext.or_(*children)

    def and_expr(self) -> FilterContext:
        children = [self.not_expr()]
        while self.kw("AND"):
            self.i += 1
            children.append(self.not_expr())
        return children[0] if len(children) == 1 else FilterContext.and_(*children)

    def not_expr(self) -> FilterContext:
        if self.kw("NOT"):
            self.i += 1
            return FilterContext.not_(self.not_expr())
        if self.peek() == ("op", "("):
            # a parenthesised filter -- or the parenthesis opens an arithmetic expression: `(a - b) * 2 > 5`
            start = self.i
            try:
                self.i += 1
                e = self.expr()
                self.eat_op(")")
                nxt = self.peek()
                if not ((nxt[0] == "op" and nxt[1] not in (")", ",")) or nxt[0] == "num"
                        or self.kw("IN") or self.kw("NOT", "IN") or self.kw("BETWEEN") or self.kw("NOT", "BETWEEN")):
                    return e
            except ValueError:
                pass
            self.i = start
        return self.comparison()

    def regexp_like(self) -> FilterContext:
        """REGEXP_LIKE(col, 'pattern'[, 'match parameter'])."""
        self.i += 1
        self.eat_op("(")
        col = self.ident()
        self.eat_op(",")
        pat = self.peek()
        if pat[0] != "str":
            raise ValueError(f"REGEXP_LIKE: the pattern must be a string literal, got {pat}")
        self.i += 1
        ci = False
        if self.peek() == ("op", ","):
            self.i += 1
            par = self.peek()
            if par[0] != "str":
                raise ValueError(f"REGEXP_LIKE: the match parameter must be a string literal, got {par}")
            self.i += 1
            ci = regexp_case_insensitive(par[1])
        self.eat_op(")")
        return FilterContext.pred(Predicate("REGEXP_LIKE", col, (pat[1],), case_insensitive=ci))

    def comparison(self) -> FilterContext:
        if self.kw("REGEXP_LIKE") and self.peek(1) == ("op", "("):
            self.need_pattern_predicates("REGEXP_LIKE")
            return self.regexp_like()
        lhs = self.value_expr()
        if lhs[0] == "col":
            col = lhs[1]
        else:
            check_expr(lhs)
            col = expr_text(lhs)
        if self.kw("NOT", "IN") or self.kw("IN"):
            neg = self.kw("NOT")
            self.i += 2 if neg else 1
            self.eat_op("(")
            vals = [self.literal()]
            while self.peek() == ("op", ","):
                self.i += 1
                vals.append(self.literal())
            self.eat_op(")")
            return FilterContext.pred(Predicate("NOT_IN" if neg else "IN", col, tuple(vals)))
        if self.kw("NOT", "LIKE") or self.kw("LIKE"):
            # RequestContextUtils: LIKE is rewritten to REGEXP_LIKE(col, likeToRegexpLike(pattern), 'i')
            self.need_pattern_predicates("LIKE")
            neg = self.kw("NOT")
            self.i += 2 if neg else 1
            pat = self.peek()
            if pat[0] != "str":
                raise ValueError(f"LIKE: the pattern must be a string literal, got {pat}")
            if lhs[0] != "col":
                raise ValueError(f"LIKE on the expression {col}: a STRING column is needed")
            self.i += 1
            p = FilterContext.pred(Predicate("REGEXP_LIKE", col, (like_to_regexp(pat[1]),), case_insensitive=True))
            return FilterContext.not_(p) if neg else p
        if self.kw("NOT", "BETWEEN") or self.kw("BETWEEN"):
            neg = self.kw("NOT")
            self.i += 2 if neg else 1
            lo = self.literal()
            self.eat_kw("AND")
            hi = self.literal()
            p = FilterContext.pred(Predicate("RANGE", col, lower=lo, upper=hi))
            return FilterContext.not_(p) if neg else p
        tok = self.peek()
        if tok[0] != "op":
            raise ValueError(f"expected comparison operator at {tok}")
        self.i += 1
        v = self.literal()
        op = tok[1]
        if op == "=":
            return FilterContext.pred(Predicate("EQ", col, (v,)))
        if op in ("<>", "!="):
            return FilterContext.pred(Predicate("NOT_EQ", col, (v,)))
        if op == "<":
            return FilterContext.pred(Predicate("RANGE", col, upper=v, upper_inclusive=False))
        if op == "<=":
            return FilterContext.pred(Predicate("RANGE", col, upper=v, upper_inclusive=True))
        if op == ">":
            return FilterContext.pred(Predicate("RANGE", col, lower=v, lower_inclusive=False))
        if op == ">=":
            return FilterContext.pred(Predicate("RANGE", col, lower=v, lower_inclusive=True))
        raise ValueError(f"unsupported operator {op}")


def _is_negative(v) -> bool:
    return v < 0 or (isinstance(v, float) and v == 0 and math.copysign(1.0, v) < 0)


_SET_OPTION = re.compile(r"^\s*SET\s+([A-Za-z_][A-Za-z0-9_]*)\s*=\s*'?([^;']*)'?\s*;", re.IGNORECASE)
_OPTION_CLAUSE = re.compile(r"\bOPTION\s*\(([^)]*)\)\s*;?\s*$", re.IGNORECASE)


def _query_options(sql: str):
    """Query options from ``SET key = value;`` prefixes (multi-stage style, CalciteSqlParser) and a
    trailing legacy ``OPTION(key=value, ...)`` clause; returns (remaining SQL, options)."""
    opts = {}
    while True:
        m = _SET_OPTION.match(sql)
        if not m:
            break
        opts[m.group(1)] = m.group(2).strip()
        sql = sql[m.end():]
    m = _OPTION_CLAUSE.search(sql)
    if m:
        for kv in m.group(1).split(","):
            if kv.strip():
                k, _, v = kv.partition("=")
                opts[k.strip()] = v.strip().strip("'")
        sql = sql[:m.start()]
    return sql, opts


_PARSED: "collections.OrderedDict[tuple, QueryContext]" = collections.OrderedDict()


def parse_sql(sql: str, pattern_predicates: bool = False) -> QueryContext:
    """Compile a Pinot SQL query of the supported subset into a QueryContext. The numGroupsLimit,
    minServerGroupTrimSize, groupTrimThreshold, serverReturnFinalResult, sortAggregateLimitThreshold and
    minSegmentGroupTrimSize query options (QueryOptionsUtils) are honoured; other options are ignored.
    A re-issued query text returns the QueryContext compiled the first time (256 most recent texts; the contexts
    are never mutated after parsing -- derived queries are dataclasses.replace copies): a configs[2] IN list of
    18K literals took 30-80 ms to parse, longer than its device step.
    pattern_predicates: accept [NOT] LIKE and [NOT] REGEXP_LIKE(col, 'p'[, 'i']) as REGEXP_LIKE predicates. Off by
    default: a QueryContext also goes to consumers that know the five earlier predicate types only (the CPU oracle,
    host-side mirrors), and for them such a query stays the ValueError it always was; ServerQueryExecutor, which
    executes the predicates, turns it on for the SQL text it is given."""
    key = (sql, bool(pattern_predicates))
    qc = _PARSED.get(key)
    if qc is not None:
        _PARSED.move_to_end(key)
        return qc
    qc = _parse_sql(sql, pattern_predicates)
    _PARSED[key] = qc
    if len(_PARSED) > 256:
        _PARSED.popitem(last=False)
    return qc


def _parse_sql(sql: str, pattern_predicates: bool = False) -> QueryContext:
    sql, opts = _query_options(sql)
    qc = _Parser(sql, pattern_predicates).query()
    for k, v in opts.items():
        if k.lower() == "numgroupslimit":
            qc.num_groups_limit = int(v)
        elif k.lower() == "minservergrouptrimsize":
            qc.min_server_group_trim_size = int(v)
        elif k.lower() == "grouptrimthreshold":
            qc.group_trim_threshold = int(v)
        elif k.lower() == "serverreturnfinalresult":
            qc.server_return_final_result = v.strip().lower() == "true"
        elif k.lower() == "sortaggregatelimitthreshold":
            qc.sort_aggregate_limit_threshold = int(v)
        elif k.lower() == "minsegmentgrouptrimsize":
            qc.min_segment_group_trim_size = int(v)
        elif k.lower() == "filteredaggregationsskipemptygroups":
            qc.filtered_aggregations_skip_empty_groups = v.strip().lower() == "true"
    return qc


# ---------------------------------------------------------------------------------------- reduce
def final_value(func: str, partial, param=None):
    """AggregationFunction.extractFinalResult: AVG -> sum / count, MINMAXRANGE -> max - min
    (MinMaxRangeAggregationFunction: MinMaxRangePair(+inf, -inf) when no doc matched), DISTINCTCOUNT -> the set's
    size, PERCENTILE (param: the percentile) -> percentile_select over the histogram, DISTINCTSUM / DISTINCTAVG ->
    the set's sum (/ its size), others unchanged."""
    if func in ("AVG", "AVGMV"):
        s, c = partial
        return s / c if c else float("-inf")
    if func in ("MINMAXRANGE", "MINMAXRANGEMV"):
        mn, mx = partial
        return mx - mn
    if func == "DISTINCTCOUNT":
        return len(partial)
    if func == "DISTINCTCOUNTHLL":  # partial: (log2m, registers), or the library's estimate
        return int(partial.v) if isinstance(partial, FinalValue) else hll_cardinality(partial[1])
    if func not in _HISTOGRAM_FINALS:  # (one look-up on the path of the plain aggregations)
        return partial
    if isinstance(partial, FinalValue):
        return partial.v
    if func == "PERCENTILE":
        return percentile_select(partial, param)
    if func == "DISTINCTSUM":
        return distinct_sum(partial)
    # DistinctAvgAggregationFunction.java:83-95: 0.0 / 0 = NaN for the empty set
    return distinct_sum(partial) / len(partial) if len(partial) else float("nan")


_HISTOGRAM_FINALS = frozenset(("PERCENTILE", "DISTINCTSUM", "DISTINCTAVG"))


def merge_partial(func: str, a, b):
    """AggregationFunction.merge (used by the combine and broker reduce)."""
    if func in ("COUNT", "SUM", "SUMLONG", "COUNTMV", "SUMMV"):
        return a + b
    if func in ("MIN", "MINMV"):
        return min(a, b)
    if func in ("MAX", "MAXMV"):
        return max(a, b)
    if func in ("AVG", "AVGMV"):
        return (a[0] + b[0], a[1] + b[1])
    if func in ("MINMAXRANGE", "MINMAXRANGEMV"):
        return (min(a[0], b[0]), max(a[1], b[1]))
    if func in ("DISTINCTCOUNT", "DISTINCTSUM", "DISTINCTAVG"):
        return a | b
    if func == "DISTINCTCOUNTHLL":
        return hll_merge(a, b)
    if func == "PERCENTILE":  # histograms (distinct_value -> matching docs) add
        out = dict(a)
        for v, c in b.items():
            out[v] = out.get(v, 0) + c
        return out
    raise ValueError(func)


# ------------------------------------------------------------------------------- DISTINCTCOUNT
def split_distinct_count(qc: QueryContext):
    """DistinctCountAggregationFunction keeps, per group, the set of distinct values of its column
    among the matching docs (intermediate = the set, merge = union, final = its size). Planned as
    device queries: the query without its DISTINCTCOUNTs (or COUNT(*) if nothing else is left), and
    per DISTINCTCOUNT(c) the same filter grouped by (group-by columns..., c) — each distinct c of a
    group is one group of that query. PERCENTILE, DISTINCTSUM and DISTINCTAVG read the same query (its COUNT is
    the number of docs holding the value: the group's histogram), so every such aggregation on one column shares
    one sub query, listed under the first of them. Returns (base query, [(aggregation index, sub query)])."""
    if qc.has_filtered_aggregations():
        raise ValueError("FILTER (WHERE ...) in a query with DISTINCTCOUNT / PERCENTILE / DISTINCTSUM / DISTINCTAVG is "
                         "not supported: the value-set queries do not take the lanes' predicates")
    rest = [a for a in qc.aggregations if a.func not in VALUE_SET_FUNCS]
    base = dataclasses.replace(qc, aggregations=rest or [Aggregation("COUNT", "*")], order_by=[])
    subs = []
    seen = set()
    for i, a in enumerate(qc.aggregations):
        if a.func in VALUE_SET_FUNCS:
            if a.expr is not None or a.column == "*":
                raise ValueError(f"{a.func} takes one column")
            if a.column in seen:  # PERCENTILE / DISTINCTSUM / DISTINCTAVG / DISTINCTCOUNT of one column share
                continue           # its query: the sub query of the first of them (fold_distinct_count)
            seen.add(a.column)
            subs.append((i, dataclasses.replace(qc, aggregations=[Aggregation("COUNT", "*")], order_by=[],
                                                group_by=list(qc.group_by) + [a.column],
                                                num_groups_limit=max(qc.num_groups_limit, 1 << 30))))
    return base, subs


_NAN_BITS = 0x7FF8000000000000


def distinct_value(v):
    """The identity of a value in DISTINCTCOUNT's set and in a group key: FLOAT/DOUBLE values compare
    by Double.doubleToLongBits (every NaN one value, -0.0 != 0.0: the fastutil Double/Float open hash
    sets of DistinctCountAggregationFunction), so floats become their canonical 64-bit pattern; other
    values are themselves."""
    if isinstance(v, (float, np.floating)):
        f = float(v)
        return ("f", _NAN_BITS if math.isnan(f) else struct.unpack("<q", struct.pack("<d", f))[0])
    return v


class JavaDouble(float):
    """A FLOAT/DOUBLE group-key value with Java's key identity (Double.equals / doubleToLongBits, as the
    group-key maps use): every NaN equals every NaN and -0.0 != 0.0, so dicts keyed by group tuples
    keep the groups Pinot keeps apart. Arithmetic and ordering are a float's."""
    __slots__ = ()

    def __eq__(self, other):
        if isinstance(other, float):
            return distinct_value(float(self)) == distinct_value(float(other))
        return float.__eq__(self, other)

    def __ne__(self, other):
        r = self.__eq__(other)
        return r if r is NotImplemented else not r

    def __hash__(self):  # consistent with float's hash where the identities agree
        return hash(_NAN_BITS) if math.isnan(self) else float.__hash__(self)

    def __repr__(self):
        return float.__repr__(self)


def canonical_key(key) -> tuple:
    return tuple(distinct_value(v) for v in key)


def fold_distinct_count(qc: QueryContext, base_groups: dict, sub_groups: Sequence[Tuple[int, dict]],
                        column_types: Optional[Dict[str, str]] = None) -> dict:
    """Groups of the original query from split_distinct_count's results (same group keys as the
    base query: a group exists iff a doc matched, in every one of the queries alike). Keys and set
    elements are matched by distinct_value (bit patterns for floats), never by Python float equality.
    column_types: column -> stored type, which DISTINCTCOUNTHLL's hash depends on (without it: LONG for Python ints,
    DOUBLE for floats, STRING for strings); its partial is (log2m, registers) hashed here from the distinct values."""
    # per sub query: group -> value set, or -- when a PERCENTILE reads the column -- group -> histogram
    # (distinct_value -> matching docs: the sub query's COUNT(*))
    by_column = {qc.aggregations[i].column: i for i, _ in sub_groups}
    counted = {by_column[a.column] for a in qc.aggregations if a.func == "PERCENTILE"}
    hists = {i: {} for i, _ in sub_groups}
    for i, g in sub_groups:
        if i in counted:
            for key, parts in g.items():
                h = hists[i].setdefault(canonical_key(key[:-1]), {})
                v = distinct_value(key[-1])
                h[v] = h.get(v, 0) + int(parts[0])
        else:
            for key in g:
                hists[i].setdefault(canonical_key(key[:-1]), set()).add(distinct_value(key[-1]))
    rest_idx = [j for j, a in enumerate(qc.aggregations) if a.func not in VALUE_SET_FUNCS]
    out = {}
    for key, parts in base_groups.items():
        full = [None] * len(qc.aggregations)
        for j, p in zip(rest_idx, parts):
            full[j] = p
        ck = canonical_key(key)
        for j, a in enumerate(qc.aggregations):
            if a.func in VALUE_SET_FUNCS:
                h = hists[by_column[a.column]].get(ck, {})
                if a.func == "DISTINCTCOUNTHLL":
                    t = (column_types or {}).get(a.column)
                    full[j] = (int(a.param), hll_registers(h, t, int(a.param)))
                else:
                    full[j] = dict(h) if a.func == "PERCENTILE" else frozenset(h)
        out[key] = full
    return out


# ----------------------------------------------------------------------------- DISTINCTCOUNTHLL
# DistinctCountHLLAggregationFunction over stream-lib's HyperLogLog and MurmurHash, restated (the library's
# restatement is csrc/hll.h). All hash arithmetic is Java int: 32 bits, wrapping, >>> logical.
_M32 = 0xFFFFFFFF
_MURMUR_M = 0x5BD1E995


def _hash_long(d: int) -> int:
    """MurmurHash.hashLong(long)."""
    m = _MURMUR_M
    k = ((d & _M32) * m) & _M32
    k ^= k >> 24
    h = (k * m) & _M32
    k = (((d >> 32) & _M32) * m) & _M32
    k ^= k >> 24
    h = (h * m) & _M32
    h ^= (k * m) & _M32
    h ^= h >> 13
    h = (h * m) & _M32
    h ^= h >> 15
    return h


def _hash_bytes(data: bytes, seed: int = -1) -> int:
    """MurmurHash.hash(byte[], length, seed): MurmurHash2 with its tail bytes sign-extended (Java bytes)."""
    m = _MURMUR_M
    n = len(data)
    h = (seed ^ n) & _M32
    for i in range(0, n - (n & 3), 4):
        k = int.from_bytes(data[i:i + 4], "little")
        k = (k * m) & _M32
        k ^= k >> 24
        k = (k * m) & _M32
        h = (h * m) & _M32
        h ^= k
    left = n & 3
    if left:
        sb = [b - 256 if b >= 128 else b for b in data[n - left:]]
        if left >= 3:
            h ^= (sb[-3] << 16) & _M32
        if left >= 2:
            h ^= (sb[-2] << 8) & _M32
        h ^= sb[-1] & _M32
        h = (h * m) & _M32
    h ^= h >> 13
    h = (h * m) & _M32
    h ^= h >> 15
    return h


def hll_hash(value, stored_type: Optional[str] = None) -> int:
    """MurmurHash.hash(Object) of a column value boxed as its stored type, as an unsigned 32-bit int: INT / LONG
    hashLong(v); FLOAT hashLong((long) floatToRawIntBits); DOUBLE hashLong(doubleToRawLongBits); STRING the UTF-8
    bytes up to the first NUL with seed -1. `value` may be a distinct_value identity (("f", bits) for floats)."""
    if isinstance(value, tuple):  # distinct_value of a float: the double's bits
        value = struct.unpack("<d", struct.pack("<q", value[1]))[0]
    if stored_type is None:
        stored_type = "STRING" if isinstance(value, str) else "DOUBLE" if isinstance(value, (float, np.floating)) else "LONG"
    if stored_type == "STRING":
        return _hash_bytes(str(value).encode("utf-8").split(b"\0", 1)[0])
    if stored_type == "FLOAT":
        return _hash_long(struct.unpack("<i", struct.pack("<f", float(value)))[0])
    if stored_type == "DOUBLE":
        return _hash_long(struct.unpack("<q", struct.pack("<d", float(value)))[0])
    return _hash_long(int(value))


def hll_registers(values, stored_type: Optional[str], log2m: int) -> bytes:
    """The RegisterSet of a HyperLogLog(log2m) offered `values` (HyperLogLog.offerHashed), one byte per register."""
    log2m = check_log2m(log2m)
    regs = bytearray(1 << log2m)
    tail = (1 << (log2m - 1)) + 1
    for v in values:
        x = hll_hash(v, stored_type)
        j = x >> (32 - log2m)
        w = ((x << log2m) & _M32) | tail
        r = 32 - w.bit_length() + 1  # Integer.numberOfLeadingZeros(w) + 1
        if r > regs[j]:
            regs[j] = r
    return bytes(regs)


def hll_merge(a, b):
    """HyperLogLog.addAll: the element-wise maximum of two (log2m, registers) partials of equal log2m."""
    if a[0] != b[0] or len(a[1]) != len(b[1]):
        raise ValueError(f"cannot merge HyperLogLogs of log2m {a[0]} and {b[0]}")
    return (a[0], bytes(map(max, a[1], b[1])))


JAVA_LONG_MAX = (1 << 63) - 1


def hll_cardinality(registers) -> int:
    """HyperLogLog.cardinality() of a register array (2^log2m bytes): the one estimator both Python paths use.
    Math.round(+inf) = Long.MAX_VALUE when the small-range correction meets no zero register."""
    regs = bytes(registers)
    m = len(regs)
    log2m = m.bit_length() - 1
    if m != 1 << log2m or not HLL_MIN_LOG2M <= log2m <= HLL_MAX_LOG2M:
        raise ValueError(f"{m} registers are not a HyperLogLog of log2m {HLL_MIN_LOG2M}..{HLL_MAX_LOG2M}")
    s = sum(1 << (32 - r) for r in regs) / 4294967296.0  # exact: every term a multiple of 2^-25, the total <= 2^16
    zeros = regs.count(0)
    alpha_mm = {4: 0.673, 5: 0.697, 6: 0.709}.get(log2m, 0.7213 / (1 + 1.079 / m)) * m * m
    estimate = alpha_mm * (1 / s)
    if estimate <= 2.5 * m:
        if zeros == 0:
            return JAVA_LONG_MAX
        return int(math.floor(m * math.log(m / float(zeros)) + 0.5))
    return int(math.floor(estimate + 0.5))


def _value_as_double(v) -> float:
    """The double a set element / histogram key (distinct_value) stands for."""
    if isinstance(v, tuple):
        return struct.unpack("<d", struct.pack("<q", v[1]))[0]
    return float(v)


def percentile_select(hist, p) -> float:
    """PercentileAggregationFunction.java:207-252 over a histogram (distinct_value -> matching docs) instead of
    the DoubleArrayList it stands for: the values sorted as Arrays.sort(double[]) sorts them (-0.0 < 0.0, NaN
    greatest and one value); n docs: the last value for p = 100, else the one at index
    (int) ((double) n * p / 100.0) -- one double multiply, one double divide, truncated; no doc: -inf
    (DEFAULT_FINAL_RESULT). The native path and the mirror path both end here or in the kernel that restates it."""
    n = sum(hist.values())
    if n == 0:
        return float("-inf")
    idx = n - 1 if p == 100 else min(int(float(n) * float(p) / 100.0), n - 1)
    cum = 0
    last = None
    for v, c in sorted(((_value_as_double(k), c) for k, c in hist.items()), key=lambda t: _double_order(t[0])):
        cum += c
        last = v
        if cum > idx:
            break
    return last


def distinct_sum(values) -> float:
    """DistinctSumAggregationFunction.java:83-95 over DISTINCTCOUNT's set: the sum of the represented values as a
    double (0.0 for the empty set). Integers sum exactly and round once; floats go through math.fsum (Pinot sums in
    hash-set order: its result is only defined up to that order)."""
    if all(not isinstance(v, tuple) for v in values):
        return float(sum(int(v) for v in values))
    return 0.0 + math.fsum(_value_as_double(v) for v in values)


class FinalValue:
    """A partial known only by its final value (QueryResult.rows() of a natively executed PERCENTILE / DISTINCTSUM /
    DISTINCTAVG reads the value the library computed, not the histogram): final_value returns it."""
    __slots__ = ("v",)

    def __init__(self, v):
        self.v = v


def hists_from_csr(offsets, values, counts, stored_type: str) -> List[dict]:
    """The per-group PERCENTILE partials from the library's CSR (pinot_amd_result_fetch_value_counts): group g's
    entries of `values` (fetch's key encoding) and `counts`. One dict distinct_value -> matching docs per group."""
    off = np.asarray(offsets, dtype=np.int64)
    vals = np.ascontiguousarray(np.asarray(values, dtype=np.int64))
    cnts = np.asarray(counts, dtype=np.int64).tolist()
    if off.size == 0:
        return []
    if off[0] != 0 or np.any(np.diff(off) < 0) or off[-1] > vals.size or off[-1] > len(cnts):
        raise ValueError("malformed CSR offsets")
    if stored_type == "STRING":
        raise ValueError("a histogram of STRING values has no percentile")
    if stored_type in ("FLOAT", "DOUBLE"):
        items = [distinct_value(f) for f in vals.view(np.float64).tolist()]
    else:
        items = vals.tolist()
    o = off.tolist()
    return [dict(zip(items[o[g]:o[g + 1]], cnts[o[g]:o[g + 1]])) for g in range(len(o) - 1)]


def sets_from_csr(offsets, values, stored_type: str, strings=None) -> List[frozenset]:
    """The per-group DISTINCTCOUNT partials from the library's CSR (pinot_amd_result_fetch_distinct_values):
    offsets[g] .. offsets[g + 1] delimit group g's entries of `values`, each an int64 in fetch's key encoding
    (the value for INT / LONG, the double's bits for FLOAT / DOUBLE, an index into `strings` for STRING). Returns
    one frozenset of distinct_value(v) per group -- what fold_distinct_count builds from the (group, value)
    pairs -- and [] for no groups. A pure function of its arguments (no device)."""
    off = np.asarray(offsets, dtype=np.int64)
    vals = np.ascontiguousarray(np.asarray(values, dtype=np.int64))
    if off.size == 0:
        return []
    if off[0] != 0 or np.any(np.diff(off) < 0) or off[-1] > vals.size:
        raise ValueError("malformed CSR offsets")
    if stored_type == "STRING":
        if strings is None:
            raise ValueError("STRING values need their dictionary")
        items = [strings[i] for i in vals.tolist()]
    elif stored_type in ("FLOAT", "DOUBLE"):
        items = [distinct_value(f) for f in vals.view(np.float64).tolist()]
    else:
        items = vals.tolist()
    o = off.tolist()
    return [frozenset(items[o[g]:o[g + 1]]) for g in range(len(o) - 1)]


class DistinctSize:
    """A DISTINCTCOUNT partial known only by its size (QueryResult.rows() of a natively executed query reads the
    counts, not the sets): final_value takes its len()."""
    __slots__ = ("n",)

    def __init__(self, n: int):
        self.n = int(n)

    def __len__(self):
        return self.n


def _dict_order(v):
    """A group-by value's position key in its (merged) dictionary's order: numbers ascending with
    Double.compare semantics for floats (-0.0 before 0.0, NaN last), strings by UTF-16 code units."""
    if isinstance(v, str):
        return (0, v.encode("utf-16-be"))
    if isinstance(v, float):
        return (1, (1, 0.0, 0) if math.isnan(v) else (0, v, int(math.copysign(1.0, v) > 0)))
    return (1, (0, v, 0))


def _double_order(x):
    x = float(x)
    return (1, 0.0, 0) if math.isnan(x) else (0, x, int(math.copysign(1.0, x) > 0))


class _Reverse:
    __slots__ = ("k",)

    def __init__(self, k):
        self.k = k

    def __lt__(self, o):
        return o.k < self.k

    def __eq__(self, o):
        return self.k == o.k


def server_table(qc: QueryContext, groups: dict) -> dict:
    """The server's combine table over combined groups, as the library applies it at compaction
    (pinot_amd_query_set_result_limit / set_server_options; GroupByUtils.java:104-149, IndexedTable.finish):
    no ORDER BY -> the first LIMIT groups in ascending key order (last group-by column compared first);
    ORDER BY -> sorted by it (ties in ascending key order) and cut to LIMIT under a safe trim below
    sortAggregateLimitThreshold or with serverReturnFinalResult, else to trimSize = max(5 * LIMIT,
    minServerGroupTrimSize) (no cut when that option is <= 0)."""
    keys = sorted(groups, key=lambda k: tuple(_dict_order(v) for v in reversed(k)))
    if not qc.order_by:
        return {k: groups[k] for k in keys[:qc.limit]}
    rank = {k: i for i, k in enumerate(keys)}
    targets = qc.order_by_targets()

    def sort_key(k):
        out = []
        for kind, idx, asc in targets:
            o = _dict_order(k[idx]) if kind == 0 else _double_order(final_value(qc.aggregations[idx].func, groups[k][idx], qc.aggregations[idx].param))
            out.append(o if asc else _Reverse(o))
        return tuple(out) + (rank[k],)
    ordered = sorted(keys, key=sort_key)
    if (qc.safe_trim() and qc.limit < qc.sort_aggregate_limit_threshold) or qc.server_return_final_result:
        keep = qc.limit
    elif qc.min_server_group_trim_size > 0:
        keep = max(5 * qc.limit, qc.min_server_group_trim_size)
    else:
        keep = len(ordered)
    return {k: groups[k] for k in ordered[:keep]}


def reduce_rows(qc: QueryContext, groups: dict) -> List[tuple]:
    """Broker reduce for group-by: final results, ORDER BY, LIMIT (default 10).

    groups: key tuple -> list of per-aggregation partials. Returns rows of
    (group values..., final aggregation values...).
    """
    rows = []
    for key, parts in groups.items():
        rows.append(tuple(key) + tuple(final_value(a.func, p, a.param) for a, p in zip(qc.aggregations, parts)))
    names = list(qc.group_by) + [a.name for a in qc.aggregations]
    exprs = list(qc.group_by) + [a.text for a in qc.aggregations]
    for expr, asc in reversed(qc.order_by):
        e = expr.lower()
        idx = None
        for i, (n, x) in enumerate(zip(names, exprs)):
            if e in (n.lower(), x.lower()):
                idx = i
        if idx is None:
            raise ValueError(f"ORDER BY {expr} not in select list")
        rows.sort(key=lambda r: r[idx], reverse=not asc)
    return rows[: qc.limit]
