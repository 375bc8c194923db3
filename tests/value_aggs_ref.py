"""Per-doc numpy restatement of PERCENTILE, DISTINCTSUM and DISTINCTAVG (and the few plain aggregations the value-
aggregation tests mix in), shared by test_value_aggs_cpu.py and test_gpu_value_aggs.py. It never builds a histogram:
per group it gathers the column's value of every matching doc over every segment, then

  PERCENTILE   PercentileAggregationFunction.java:79-131,207-252 -- the values as doubles, sorted as
               Arrays.sort(double[]) sorts (-0.0 < 0.0, NaN last); the last for p = 100, else the element at
               (int) ((double) n * p / 100.0); -inf without a doc
  DISTINCTSUM  DistinctSumAggregationFunction.java:83-95 -- the distinct values (Java identity: doubleToLongBits,
               one NaN) summed: Python ints for INT / LONG, math.fsum for FLOAT / DOUBLE; 0.0 for none
  DISTINCTAVG  DistinctAvgAggregationFunction.java:83-95 -- that sum over the number of distinct values; NaN for none

A segment is a dict column -> numpy array (one entry per doc); a filter is a function of that dict returning a
boolean mask."""
import math

import numpy as np

from pinot_amd.query import canonical_key, distinct_value

NAN_BITS = 0x7FF8000000000000


def java_sorted(values) -> np.ndarray:
    """float64 values in Arrays.sort(double[]) order."""
    v = np.asarray(values, dtype=np.float64)
    return v[np.lexsort((~np.signbit(v), v))]


def percentile(values, p) -> float:
    v = java_sorted(values)
    n = len(v)
    if n == 0:
        return float("-inf")
    return float(v[n - 1] if p == 100 else v[int(float(n) * float(p) / 100.0)])


def distinct(values) -> list:
    """The distinct values by Java identity, as Python ints (integer arrays) or floats."""
    a = np.asarray(values)
    if a.dtype.kind == "f":
        bits = a.astype(np.float64).view(np.int64).copy()
        bits[np.isnan(a)] = NAN_BITS
        return np.unique(bits).view(np.float64).tolist()
    return [int(x) for x in np.unique(a)]


def distinct_sum(values) -> float:
    d = distinct(values)
    if np.asarray(values).dtype.kind == "f":
        return 0.0 + math.fsum(d)
    return float(sum(d))


def distinct_avg(values) -> float:
    d = distinct(values)
    return distinct_sum(values) / len(d) if d else float("nan")


def final(a, values):
    """Final value of query.Aggregation `a` over one group's gathered values (None for COUNT(*))."""
    if a.func == "COUNT":
        return len(values)
    if a.func == "PERCENTILE":
        return percentile(values, a.param)
    if a.func == "DISTINCTSUM":
        return distinct_sum(values)
    if a.func == "DISTINCTAVG":
        return distinct_avg(values)
    if a.func == "DISTINCTCOUNT":
        return len(distinct(values))
    if a.func == "SUM":
        v = np.asarray(values)
        return float(sum(int(x) for x in v)) if v.dtype.kind != "f" else math.fsum(v.astype(np.float64).tolist())
    raise ValueError(a.func)


def reference_rows(qc, segments, flt=None) -> dict:
    """canonical group key -> [final value per aggregation of qc], over every matching doc of every segment
    (groups exist iff a doc matched; without GROUP BY the one group () always exists)."""
    cols = sorted({c for a in qc.aggregations for c in a.columns} | set(qc.group_by))
    picked = {c: [] for c in cols}
    for seg in segments:
        m = np.ones(len(next(iter(seg.values()))), dtype=bool) if flt is None else np.asarray(flt(seg), dtype=bool)
        for c in cols:
            picked[c].append(np.asarray(seg[c])[m])
    picked = {c: np.concatenate(v) for c, v in picked.items()}
    ndocs = len(next(iter(picked.values()))) if picked else 0
    if not qc.group_by:
        index = {(): np.arange(ndocs)}
    elif ndocs == 0:
        index = {}
    else:
        codes = []   # per GROUP BY column: one integer per Java-distinct value
        for g in qc.group_by:
            a = picked[g]
            if a.dtype.kind == "f":
                bits = a.astype(np.float64).view(np.int64).copy()
                bits[np.isnan(a)] = NAN_BITS
                a = bits
            codes.append(np.unique(a, return_inverse=True)[1].reshape(-1))
        _, first, inv = np.unique(np.stack(codes, axis=1), axis=0, return_index=True, return_inverse=True)
        inv = inv.reshape(-1)
        order = np.argsort(inv, kind="stable")
        bounds = np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=len(first)))])
        index = {canonical_key(tuple(picked[g][first[j]].item() for g in qc.group_by)): order[bounds[j]:bounds[j + 1]]
                 for j in range(len(first))}
    out = {}
    for k, idx in index.items():
        out[k] = [final(a, picked[a.column][idx] if a.column != "*" else idx) for a in qc.aggregations]
    return out


def same(got, exp, func, is_float_column) -> bool:
    """The issue's comparison rules: PERCENTILE bit-equal doubles (NaN by isnan); DISTINCTSUM / DISTINCTAVG equal for
    integer columns, within 1e-12 relative of the math.fsum restatement for FLOAT / DOUBLE; the rest equal."""
    if isinstance(exp, float) and math.isnan(exp):
        return isinstance(got, float) and math.isnan(got)
    if func == "PERCENTILE":
        return distinct_value(float(got)) == distinct_value(float(exp))
    if func in ("DISTINCTSUM", "DISTINCTAVG") and is_float_column:
        return abs(got - exp) <= 1e-12 * abs(exp)
    return got == exp
