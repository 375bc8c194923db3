"""DISTINCTCOUNTHLL restated per doc (DistinctCountHLLAggregationFunction over stream-lib's HyperLogLog and
MurmurHash), independent of pinot_amd.query: every matching doc's value is offered, not the distinct set. numpy for
the fixed-width types (Java int arithmetic as wrapping uint32), plain Python for strings and the estimator."""
import math

import numpy as np

M = np.uint32(0x5BD1E995)
LONG_MAX = (1 << 63) - 1


def hash_long(d):
    """MurmurHash.hashLong over an int64 array -> uint32 array."""
    d = np.asarray(d, dtype=np.int64).view(np.uint64)
    with np.errstate(over="ignore"):
        k = (d & np.uint64(0xFFFFFFFF)).astype(np.uint32) * M
        k ^= k >> np.uint32(24)
        h = k * M
        k = (d >> np.uint64(32)).astype(np.uint32) * M
        k ^= k >> np.uint32(24)
        h = h * M
        h ^= k * M
        h ^= h >> np.uint32(13)
        h = h * M
        h ^= h >> np.uint32(15)
    return h


def hash_bytes(b: bytes, seed: int = -1) -> int:
    """MurmurHash.hash(byte[], len, seed): tail bytes sign-extended."""
    m, mask = 0x5BD1E995, 0xFFFFFFFF
    n = len(b)
    h = (seed ^ n) & mask
    for i in range(n >> 2):
        k = b[4 * i] | (b[4 * i + 1] << 8) | (b[4 * i + 2] << 16) | (b[4 * i + 3] << 24)
        k = (k * m) & mask
        k ^= k >> 24
        k = (k * m) & mask
        h = ((h * m) & mask) ^ k
    left = n & 3
    if left:
        def sx(x):
            return x - 256 if x > 127 else x
        if left >= 3:
            h ^= (sx(b[n - 3]) << 16) & mask
        if left >= 2:
            h ^= (sx(b[n - 2]) << 8) & mask
        h ^= sx(b[n - 1]) & mask
        h = (h * m) & mask
    h ^= h >> 13
    h = (h * m) & mask
    h ^= h >> 15
    return h


def hashes(values, stored_type: str):
    """uint32 hash per value: MurmurHash.hash(Object) of the value boxed as its stored type."""
    if stored_type == "STRING":
        return np.array([hash_bytes(str(v).encode("utf-8").split(b"\0", 1)[0]) for v in values], dtype=np.uint32)
    if stored_type in ("INT", "LONG"):
        return hash_long(np.asarray(values).astype(np.int64))
    if stored_type == "FLOAT":  # (long) Float.floatToRawIntBits: the int sign-extended
        return hash_long(np.asarray(values, dtype=np.float32).view(np.int32).astype(np.int64))
    if stored_type == "DOUBLE":
        return hash_long(np.asarray(values, dtype=np.float64).view(np.int64))
    raise ValueError(stored_type)


def index_rank(x, log2m: int):
    """HyperLogLog.offerHashed: (register, rank) per uint32 hash."""
    x = np.asarray(x, dtype=np.uint32)
    idx = (x >> np.uint32(32 - log2m)).astype(np.int64)
    with np.errstate(over="ignore"):
        w = (x << np.uint32(log2m)) | np.uint32((1 << (log2m - 1)) + 1)
    # numberOfLeadingZeros(w) + 1; w != 0
    nlz = 31 - np.floor(np.log2(w.astype(np.float64))).astype(np.int64)
    return idx, nlz + 1


def registers(values, stored_type: str, log2m: int) -> bytes:
    regs = np.zeros(1 << log2m, dtype=np.uint8)
    if len(values):
        idx, rank = index_rank(hashes(values, stored_type), log2m)
        np.maximum.at(regs, idx, rank.astype(np.uint8))
    return regs.tobytes()


def cardinality(regs: bytes) -> int:
    m = len(regs)
    log2m = m.bit_length() - 1
    assert m == 1 << log2m
    total = 0.0
    for r in regs:
        total += 1.0 / (1 << r)
    zeros = sum(1 for r in regs if r == 0)
    if log2m == 4:
        alpha_mm = 0.673 * m * m
    elif log2m == 5:
        alpha_mm = 0.697 * m * m
    elif log2m == 6:
        alpha_mm = 0.709 * m * m
    else:
        alpha_mm = (0.7213 / (1 + 1.079 / m)) * m * m
    estimate = alpha_mm * (1 / total)
    if estimate <= 2.5 * m:
        if zeros == 0:
            return LONG_MAX  # Math.round(+inf)
        return int(math.floor(m * math.log(m / float(zeros)) + 0.5))
    return int(math.floor(estimate + 0.5))


def grouped(values, stored_type: str, log2m: int, keys=None, mask=None):
    """{group key tuple: registers} over the docs `mask` keeps; keys: list of per-doc key arrays (None: one group (),
    present even when no doc matches)."""
    n = len(values)
    mask = np.ones(n, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    sel = np.flatnonzero(mask)
    vals = [values[i] for i in sel] if stored_type == "STRING" else np.asarray(values)[sel]
    if not keys:
        return {(): registers(vals, stored_type, log2m)}
    m = 1 << log2m
    out = {}
    if len(sel) == 0:
        return out
    idx, rank = index_rank(hashes(vals, stored_type), log2m)
    kcols = [np.asarray(k)[sel] for k in keys]
    order = np.lexsort(kcols[::-1])
    ks = [k[order] for k in kcols]
    change = np.ones(len(sel), dtype=bool)
    change[1:] = np.any([k[1:] != k[:-1] for k in ks], axis=0)
    starts = np.flatnonzero(change)
    gid = np.cumsum(change) - 1
    regs = np.zeros((len(starts), m), dtype=np.uint8)
    np.maximum.at(regs, (gid, idx[order]), rank[order].astype(np.uint8))
    for g, s in enumerate(starts):
        out[tuple(k[s].item() for k in ks)] = regs[g].tobytes()
    return out
