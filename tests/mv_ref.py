"""Multi-value columns restated in numpy, independent of the library, and the single-value segments the CPU oracle
can read instead.

Semantics (BaseDictionaryBasedPredicateEvaluator.applyMV, PredicateType.isExclusive; the aggregateMV bodies of
Count / Sum / Min / Max / Avg / MinMaxRange):

* EQ / IN / RANGE match a doc iff any of its values matches; NOT_EQ / NOT_IN iff no value is in the excluded set;
* COUNTMV counts values, SUMMV adds them as doubles, MINMV / MAXMV compare with < / > from +inf / -inf (NaN never
  enters), AVGMV is (sum of values, count of values), MINMAXRANGEMV (min, max).

A query template marks every predicate on an MV column with braces: ``WHERE {tags = 5} AND x > 3``. `rewrite` turns
it into the MV query (braces dropped) and the oracle's query: leaf k becomes ``f_k = 1`` over an INT column f_k in
{0, 1} this module evaluates per doc, and COUNTMV(c) / SUMMV(c) / MINMV(c) / MAXMV(c) become SUM(c_cnt) / SUM(c_sum) /
MIN(c_min) / MAX(c_max) over the per-doc reductions (AVGMV and MINMAXRANGEMV take two of them; `fold` puts the
oracle's columns back together as the MV query's partials)."""
import math
import re

import numpy as np

from pinot_amd import segment as S
from pinot_amd.query import parse_sql


# ----------------------------------------------------------------------------------------- per doc
def _as_number(v, sample):
    if isinstance(sample, str):
        return str(v)
    return float(v) if isinstance(sample, float) else int(v)


def match_value(v, p) -> bool:
    """One value against the inclusive form of predicate p (EQ / IN / RANGE; NOT_EQ / NOT_IN as EQ / IN)."""
    if p.type in ("EQ", "NOT_EQ", "IN", "NOT_IN"):
        return any(v == _as_number(x, v) for x in p.values)
    if p.lower is not None:
        lo = _as_number(p.lower, v)
        if v < lo or (v == lo and not p.lower_inclusive):
            return False
    if p.upper is not None:
        hi = _as_number(p.upper, v)
        if v > hi or (v == hi and not p.upper_inclusive):
            return False
    return True


def match(values, p) -> bool:
    """A doc's values against predicate p: ANY for the inclusive types, NONE for NOT_EQ / NOT_IN."""
    hit = any(match_value(v, p) for v in values)
    return (not hit) if p.type in ("NOT_EQ", "NOT_IN") else hit


def match_filter(doc, f) -> bool:
    """A FilterContext tree over a doc given as {column: list of values (an SV column: one value)}."""
    if f.type == "PREDICATE":
        return match(doc[f.predicate.column], f.predicate)
    if f.type == "NOT":
        return not match_filter(doc, f.children[0])
    r = [match_filter(doc, c) for c in f.children]
    return all(r) if f.type == "AND" else any(r)


def doc_count(values) -> int:
    return len(values)


def doc_sum_exact(values) -> int:
    return sum(int(v) for v in values)


def doc_sum_double(values) -> float:
    s = 0.0
    for v in values:  # in value order
        s += float(v)
    return s


def doc_min(values):
    m = math.inf
    for v in values:
        if v < m:
            m = v
    return m


def doc_max(values):
    m = -math.inf
    for v in values:
        if v > m:
            m = v
    return m


# ----------------------------------------------------------------------------------------- queries
_LEAF = re.compile(r"\{([^{}]*)\}")
_MV_CALL = re.compile(r"\b(COUNTMV|SUMMV|MINMV|MAXMV|AVGMV|MINMAXRANGEMV)\((\w+)\)", re.I)
_SV_OF = {"COUNTMV": ["SUM({c}_cnt)"], "SUMMV": ["SUM({c}_sum)"], "MINMV": ["MIN({c}_min)"], "MAXMV": ["MAX({c}_max)"],
          "AVGMV": ["SUM({c}_sum)", "SUM({c}_cnt)"], "MINMAXRANGEMV": ["MIN({c}_min)", "MAX({c}_max)"]}


def rewrite(template: str):
    """(the MV query, the oracle's SV query, the MV leaves as FilterContexts, fold). fold(values) turns a group's
    values of the SV query into the MV query's partials."""
    leaves = [parse_sql("SELECT COUNT(*) FROM t WHERE " + m.group(1)).filter for m in _LEAF.finditer(template)]
    mv_sql = _LEAF.sub(lambda m: m.group(1), template)
    k = iter(range(len(leaves)))
    sv_sql = _LEAF.sub(lambda m: f"f_{next(k)} = 1", template)
    head, sep, tail = sv_sql.partition(" FROM ")
    shape = []  # per select item of the MV query that is an aggregation: how many oracle columns it takes

    def sv_call(m):
        cols = _SV_OF[m.group(1).upper()]
        return ", ".join(c.format(c=m.group(2)) for c in cols)
    sv_sql = _MV_CALL.sub(sv_call, head) + sep + tail
    for a in parse_sql(mv_sql).aggregations:
        shape.append(len(_SV_OF.get(a.func, [None])))

    def fold(values):
        out, i = [], 0
        for n in shape:
            if n == 1:
                out.append(values[i])
            else:
                out.append((values[i], values[i + 1]))  # AvgPair (sum, count) / MinMaxRangePair (min, max)
            i += n
        assert i == len(values)
        return out
    return mv_sql, sv_sql, leaves, fold


# ----------------------------------------------------------------------------------------- oracle segments
def _np_type(stored):
    return {S.INT: np.int32, S.LONG: np.int64, S.FLOAT: np.float32, S.DOUBLE: np.float64}[stored]


def reductions(docs, stored: str, exact_sum: bool):
    """The per-doc (count INT, sum LONG | DOUBLE, min, max) arrays of an MV column's docs; min / max of a FLOAT /
    DOUBLE column as DOUBLE (never NaN)."""
    fl = stored in (S.FLOAT, S.DOUBLE)
    cnt = np.array([doc_count(d) for d in docs], dtype=np.int32)
    if exact_sum:
        sm = np.array([doc_sum_exact(d) for d in docs], dtype=np.int64)
    else:
        sm = np.array([doc_sum_double(d) for d in docs], dtype=np.float64)
    mt = np.float64 if fl else _np_type(stored)
    mn = np.array([doc_min(list(d)) for d in docs], dtype=mt)
    mx = np.array([doc_max(list(d)) for d in docs], dtype=mt)
    return cnt, sm, mn, mx


def oracle_segment(name, sv_columns, mv_columns, leaves, reduced, cache=None):
    """A SegmentBuffers of single-value columns: sv_columns {name: (values, type, kwargs)} as they are; f_k per MV
    leaf; <c>_cnt / _sum / _min / _max for every column of `reduced` {name: (count, sum, min, max) from
    reductions()}. mv_columns {name: list of per-doc value lists} feeds the leaves. cache: a dict keeping each leaf's
    column per (segment name, leaf)."""
    n = len(next(iter(mv_columns.values()))) if mv_columns else len(next(iter(sv_columns.values()))[0])
    cols = dict(sv_columns)
    raw = {"dictionary": False}
    for k, f in enumerate(leaves):
        key = (name, repr(f))
        bits = None if cache is None else cache.get(key)
        if bits is None:
            bits = np.zeros(n, dtype=np.int32)
            for d in range(n):
                doc = {c: v[d] for c, v in mv_columns.items()}
                doc.update({c: [spec[0][d]] for c, spec in sv_columns.items()})
                bits[d] = 1 if match_filter(doc, f) else 0
            if cache is not None:
                cache[key] = bits
        cols[f"f_{k}"] = (bits, S.INT, {"detect_sorted": False})
    for c, (cnt, sm, mn, mx) in reduced.items():
        cols[c + "_cnt"] = (cnt, S.INT, raw)
        cols[c + "_sum"] = (sm, S.LONG if sm.dtype == np.int64 else S.DOUBLE, raw)
        mt = {np.dtype(np.int32): S.INT, np.dtype(np.int64): S.LONG, np.dtype(np.float64): S.DOUBLE}[mn.dtype]
        cols[c + "_min"] = (mn, mt, raw)
        cols[c + "_max"] = (mx, mt, raw)
    return S.build_segment(name, cols)


def doc_bitset(mv_columns, sv_columns, filt, n) -> np.ndarray:
    """The dense docId bitset (uint64 words, bit d of word d / 64) of filter `filt` over n docs."""
    words = np.zeros((n + 63) // 64, dtype=np.uint64)
    for d in range(n):
        doc = {c: v[d] for c, v in mv_columns.items()}
        doc.update({c: [spec[0][d]] for c, spec in sv_columns.items()})
        if match_filter(doc, filt):
            words[d >> 6] |= np.uint64(1) << np.uint64(d & 63)
    return words
