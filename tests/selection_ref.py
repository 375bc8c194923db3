"""Per-doc numpy restatement of a selection query (SELECT columns [ORDER BY ...] LIMIT n [OFFSET m]) over a batch of
segments, sharing nothing with the library: boolean filter masks, then one np.lexsort over (docId, segment, keys...).

Semantics restated (reference paths relative to the Pinot checkout, pinot-core/src/main/java/org/apache/pinot/core):
  * the server keeps offset + limit rows (operator/query/SelectionOrderByOperator.java:112); the broker applies the
    offset, so it is not applied here;
  * ORDER BY compares by value: INT / LONG numerically, FLOAT / DOUBLE as Float.compare / Double.compare (-0.0 < 0.0,
    every NaN one value above +inf), STRING as String.compareTo (UTF-16 code units); DESC reverses the order;
  * ties, which Pinot leaves unspecified (query/selection/SelectionOperatorUtils.java:630-637), come in ascending
    (segment index in the batch, docId);
  * without ORDER BY: the first offset + limit matching docs in (segment index, docId) order, and numDocsScanned is
    the number of rows returned; with ORDER BY it is every matching doc;
  * LIMIT 0 ignores the ORDER BY and returns no row.
"""
import math
import struct

import numpy as np


def _order_ranks(values):
    """Dense ranks of `values` (one column over the batch's matching docs) in the column's value order."""
    v = np.asarray(values)
    if v.dtype.kind in "iu":
        return np.unique(v.astype(np.int64), return_inverse=True)[1]
    if v.dtype.kind == "f":
        # Double.compare order as unsigned integers: the canonical NaN above +inf, negative values reversed
        d = v.astype(np.float64)
        bits = d.view(np.uint64).copy()
        bits[np.isnan(d)] = np.uint64(0x7FF8000000000000)
        neg = (bits >> np.uint64(63)) != 0
        bits = np.where(neg, ~bits, bits | np.uint64(1 << 63))
        return np.unique(bits, return_inverse=True)[1]
    # strings: String.compareTo = UTF-16 code unit order
    strs = [str(x) for x in v.tolist()]
    order = {s: i for i, s in enumerate(sorted(set(strs), key=lambda s: s.encode("utf-16-be")))}
    return np.asarray([order[s] for s in strs], dtype=np.int64)


def select(tables, masks, columns, order_by=(), limit=10, offset=0):
    """tables: one dict column -> per-doc numpy array per segment; masks: one boolean array per segment (None: every
    doc); columns: the selected columns; order_by: (column, ascending) pairs.
    Returns (rows as tuples of Python values in `columns` order, origins as (segment, docId) pairs, numDocsScanned)."""
    k = limit + offset
    seg_ids, doc_ids = [], []
    for si, t in enumerate(tables):
        n = len(next(iter(t.values()))) if t else 0
        m = np.ones(n, dtype=bool) if masks is None or masks[si] is None else np.asarray(masks[si], dtype=bool)
        d = np.nonzero(m)[0]
        seg_ids.append(np.full(len(d), si, dtype=np.int64))
        doc_ids.append(d.astype(np.int64))
    seg = np.concatenate(seg_ids) if seg_ids else np.zeros(0, dtype=np.int64)
    doc = np.concatenate(doc_ids) if doc_ids else np.zeros(0, dtype=np.int64)
    matched = len(seg)
    if k == 0:
        return [], [], 0
    keys = [doc, seg]  # np.lexsort: the last key is the primary one
    for col, asc in reversed(list(order_by)):
        vals = np.concatenate([np.asarray(tables[si][col])[doc_ids[si]] for si in range(len(tables))]) \
            if matched else np.zeros(0)
        r = _order_ranks(vals) if matched else np.zeros(0, dtype=np.int64)
        keys.append(r if asc else -r)
    idx = np.lexsort(tuple(keys))[:k]
    rows = []
    for i in idx.tolist():
        t = tables[int(seg[i])]
        rows.append(tuple(_py(t[c][int(doc[i])]) for c in columns))
    origins = [(int(seg[i]), int(doc[i])) for i in idx.tolist()]
    return rows, origins, (matched if order_by else len(rows))


def _py(v):
    if isinstance(v, (np.floating, float)):
        return float(v)
    if isinstance(v, (np.integer, int)):
        return int(v)
    return str(v)


def same_value(a, b) -> bool:
    """Equality by bits for floats (NaN equals NaN, -0.0 differs from 0.0), plain equality otherwise."""
    if isinstance(a, float) or isinstance(b, float):
        a, b = float(a), float(b)
        if math.isnan(a) or math.isnan(b):
            return math.isnan(a) and math.isnan(b)
        return struct.pack("<d", a) == struct.pack("<d", b)
    return a == b


def same_rows(a, b) -> bool:
    return len(a) == len(b) and all(len(x) == len(y) and all(same_value(p, q) for p, q in zip(x, y))
                                    for x, y in zip(a, b))
