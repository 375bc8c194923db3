"""Per-doc numpy restatement of filtered aggregations, AGG(x) FILTER (WHERE f), shared by test_filtered_aggs_cpu.py
and test_gpu_filtered_aggs.py. It imports nothing from the planner and builds no lanes: per group it gathers each
aggregation's values over the docs matching `main AND that aggregation's filter` and applies the function.

  doc selection   AggregationFunctionUtils.buildFilteredAggregationInfos (java:416-420): main AND f; no FILTER: main
  groups          the main filter's (java:462-474), also when every aggregation is filtered; with
                  filteredAggregationsSkipEmptyGroups and no unfiltered aggregation: the docs of main AND (f1 OR ... OR fn)
  empty values    COUNT 0, SUM 0.0, SUMLONG 0, MIN +inf, MAX -inf, AVG -inf (AvgPair(0, 0)), MINMAXRANGE -inf
  NaN             GROUP BY MIN / MAX compare with < / > (NaN never enters); aggregation-only MIN / MAX are Math.min /
                  Math.max (NaN propagates); MINMAXRANGE's pair compares with < / > everywhere

A segment is a dict column -> numpy array (one entry per doc); the main filter and each aggregation's filter are
functions of that dict returning a boolean mask (None: every doc)."""
import math

import numpy as np

from pinot_amd.query import canonical_key

NAN_BITS = 0x7FF8000000000000
INF = float("inf")


def _values(a, cols, idx):
    """The values aggregation `a` reads at docs idx: the column's, or the transform's (exact Python ints for two
    integer INT operands, else doubles as the transform functions compute)."""
    if a.expr is None:
        return cols[a.column][idx]
    op, ca, cb = a.expr
    x, y = cols[ca][idx], cols[cb][idx]
    if x.dtype.kind != "f" and y.dtype.kind != "f" and x.dtype.itemsize <= 4 and y.dtype.itemsize <= 4:
        x, y = x.astype(np.int64), y.astype(np.int64)
    else:
        x, y = x.astype(np.float64), y.astype(np.float64)
    return x * y if op == "MUL" else x - y if op == "SUB" else x + y


def _sum(v) -> float:
    if v.dtype.kind == "f":
        return 0.0 + math.fsum(v.astype(np.float64).tolist())
    return float(sum(int(x) for x in v))  # the exact integer sum, rounded once


def final(a, v, grouped: bool):
    """Final value of query.Aggregation `a` over its gathered values v (a numpy array; the doc indices for COUNT(*))."""
    n = len(v)
    if a.func == "COUNT":
        return n
    if a.func == "SUM":
        return _sum(v)
    if a.func == "SUMLONG":
        s = sum(int(x) for x in v) & ((1 << 64) - 1)
        return s - (1 << 64) if s >> 63 else s
    if a.func == "AVG":
        return _sum(v) / n if n else -INF
    d = v.astype(np.float64)
    nan = bool(np.isnan(d).any())
    d = d[~np.isnan(d)]
    if a.func == "MINMAXRANGE":
        return (float(d.max()) if len(d) else -INF) - (float(d.min()) if len(d) else INF)
    if a.func == "MIN":
        return float("nan") if nan and not grouped else float(d.min()) if len(d) else INF
    if a.func == "MAX":
        return float("nan") if nan and not grouped else float(d.max()) if len(d) else -INF
    raise ValueError(a.func)


def reference(qc, segments, main=None, lanes=None, skip_empty=False):
    """(canonical group key -> [final value per aggregation of qc], num_docs_matched). lanes: per aggregation of qc
    its filter's mask function or None. Without GROUP BY the one group () always exists."""
    lanes = list(lanes) if lanes is not None else [None] * len(qc.aggregations)
    assert len(lanes) == len(qc.aggregations)
    names = sorted({c for a in qc.aggregations for c in a.columns} | set(qc.group_by))
    cols = {c: np.concatenate([np.asarray(s[c]) for s in segments]) for c in names}
    ndocs = [len(next(iter(s.values()))) for s in segments]

    def mask(f):
        if f is None:
            return np.ones(sum(ndocs), dtype=bool)
        return np.concatenate([np.asarray(f(s), dtype=bool).reshape(-1) for s in segments])

    m = mask(main)
    lane_masks = [None if f is None else m & mask(f) for f in lanes]
    if skip_empty and all(x is not None for x in lane_masks) and lane_masks:
        m = np.logical_or.reduce(lane_masks)
    take = [m if x is None else x & m for x in lane_masks]
    grouped = bool(qc.group_by)
    out = {}
    if not grouped:
        out[()] = [final(a, _values(a, cols, np.flatnonzero(t)) if a.column != "*" else np.flatnonzero(t), False)
                   for a, t in zip(qc.aggregations, take)]
        return out, int(m.sum())
    docs = np.flatnonzero(m)
    if len(docs) == 0:
        return out, 0
    codes = []
    for g in qc.group_by:
        a = cols[g][docs]
        if a.dtype.kind == "f":
            bits = a.astype(np.float64).view(np.int64).copy()
            bits[np.isnan(a)] = NAN_BITS
            a = bits
        codes.append(np.unique(a, return_inverse=True)[1].reshape(-1))
    _, first, inv = np.unique(np.stack(codes, axis=1), axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=len(first)))])
    for j in range(len(first)):
        idx = docs[order[bounds[j]:bounds[j + 1]]]
        key = canonical_key(tuple(cols[g][docs[first[j]]].item() for g in qc.group_by))
        vals = []
        for a, t in zip(qc.aggregations, take):
            sub = idx[t[idx]]
            vals.append(final(a, _values(a, cols, sub) if a.column != "*" else sub, True))
        out[key] = vals
    return out, int(m.sum())


def same(got, exp, a, float_sum: bool) -> bool:
    """Integers compare exactly; a double sum (SUM / AVG over FLOAT / DOUBLE values) within the project's 1e-12
    relative rule; NaN by isnan; MIN / MAX / MINMAXRANGE and the infinities exactly."""
    if isinstance(exp, float) and math.isnan(exp):
        return isinstance(got, float) and math.isnan(got)
    if float_sum and a.func in ("SUM", "AVG") and math.isfinite(exp):
        return abs(got - exp) <= 1e-12 * abs(exp)
    return got == exp


def reads_floats(a, segment) -> bool:
    return any(np.asarray(segment[c]).dtype.kind == "f" for c in a.columns)
