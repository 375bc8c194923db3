"""A numpy restatement (float64 throughout) of Pinot's arithmetic transform functions, over the expression trees
pinot_amd.query parses: ('col', name) | ('lit', int or float) | ('fn', name, [args]).

Every node is a Java double. Columns are read as transformToDoubleValuesSV reads them (INT and FLOAT widen, LONG is
(double) v, rounding to nearest-even above 2^53); literals are getDoubleLiteral(). The evaluation order is the
reference's (pinot-core/.../operator/transform/function/):

  add / plus (n >= 2)    acc = 0.0 + (the literal arguments, in order), then acc += each other argument in order
                         (AdditionTransformFunction.java:89-105): plus(x, y) of two -0.0 is 0.0
  mult / times (n >= 2)  acc = 1.0 * literals, then acc *= each other argument (MultiplicationTransformFunction)
  sub / minus, div / divide, mod   first - second, first / second (IEEE), Java % = C fmod
  abs ceil floor sqrt sign         Math.abs / ceil / floor / sqrt / signum
  least / greatest                 a left fold of Math.min / Math.max (NaN propagates, -0.0 < 0.0)

Math.min, Math.max and Math.signum are written out below, not taken from np.minimum / np.maximum / np.sign.
"""
import numpy as np

ADD = ("add", "plus")
MULT = ("mult", "times")
NEG_ZERO_BITS = np.uint64(0x8000000000000000)


def to_double(values) -> np.ndarray:
    """transformToDoubleValuesSV: int32 / float32 widen exactly, int64 rounds to the nearest double (ties to even)."""
    return np.asarray(values).astype(np.float64)


def _bits(x: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def java_min(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Math.min(double, double): a if a is NaN; b if both are zeros and b is -0.0; else a <= b ? a : b (so a NaN b wins
    the comparison that fails)."""
    with np.errstate(invalid="ignore"):
        out = np.where(a <= b, a, b)
    both_zero = (a == 0.0) & (b == 0.0)
    out = np.where(both_zero & (_bits(b) == NEG_ZERO_BITS), b, out)
    return np.where(a != a, a, out)


def java_max(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Math.max(double, double): a if a is NaN; b if both are zeros and a is -0.0; else a >= b ? a : b."""
    with np.errstate(invalid="ignore"):
        out = np.where(a >= b, a, b)
    both_zero = (a == 0.0) & (b == 0.0)
    out = np.where(both_zero & (_bits(a) == NEG_ZERO_BITS), b, out)
    return np.where(a != a, a, out)


def java_signum(a: np.ndarray) -> np.ndarray:
    """Math.signum: 1.0 / -1.0 for positive / negative values, the argument itself for +-0.0 and NaN."""
    out = a.copy()
    out[a > 0.0] = 1.0
    out[a < 0.0] = -1.0
    return out


def fold_literals(name: str, args) -> float:
    """The value AdditionTransformFunction / MultiplicationTransformFunction hold after init: 0.0 + (or 1.0 *) the
    literal arguments in order, one double operation each."""
    acc = 0.0 if name in ADD else 1.0
    for a in args:
        if a[0] == "lit":
            acc = acc + float(a[1]) if name in ADD else acc * float(a[1])
    return acc


def evaluate(e, cols: dict, n: int) -> np.ndarray:
    """The expression's value per doc: `cols` maps a column to its values (any numeric dtype), n is the doc count."""
    if e[0] == "col":
        return to_double(cols[e[1]])
    if e[0] == "lit":
        return np.full(n, float(e[1]), dtype=np.float64)
    name, args = e[1], e[2]
    with np.errstate(all="ignore"):
        if name in ADD or name in MULT:
            acc = np.full(n, fold_literals(name, args), dtype=np.float64)
            for a in args:
                if a[0] != "lit":
                    v = evaluate(a, cols, n)
                    acc = acc + v if name in ADD else acc * v
            return acc
        v = [evaluate(a, cols, n) for a in args]
        if name in ("sub", "minus"):
            return v[0] - v[1]
        if name in ("div", "divide"):
            return v[0] / v[1]
        if name == "mod":
            return np.fmod(v[0], v[1])
        if name == "abs":
            return np.abs(v[0])
        if name in ("ceil", "ceiling"):
            return np.ceil(v[0])
        if name == "floor":
            return np.floor(v[0])
        if name == "sqrt":
            return np.sqrt(v[0])
        if name == "sign":
            return java_signum(v[0])
        if name in ("least", "greatest"):
            f = java_min if name == "least" else java_max
            acc = v[0]
            for x in v[1:]:
                acc = f(acc, x)
            return acc
    raise ValueError(f"unknown function {name}")


def canonical_bits(x) -> np.ndarray:
    """The doubles' bit patterns with every NaN as one value (Double.doubleToLongBits)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    b = x.view(np.uint64).copy()
    b[x != x] = np.uint64(0x7FF8000000000000)
    return b
