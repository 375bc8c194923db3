"""Numpy restatement of the three GROUP BY key transforms, in Java long arithmetic (int64 arrays, wrapping where Java
wraps), shared by test_time_transforms_cpu.py and test_gpu_time_groupby.py. It shares no code with the library.

  TimeUnit.convert   the JDK's: scaling down divides truncating toward zero, scaling up multiplies and saturates at
                     Long.MIN_VALUE / Long.MAX_VALUE
  dateTrunc          DateTruncTransformFunction.java:132-142, DateTimeUtils.getTimestampField (UTC):
                     out = outputUnit.convert(roundFloor_unit(MILLISECONDS.convert(v, inputUnit)), MILLISECONDS);
                     roundFloor is Joda's true floor; week = Monday 00:00; month / quarter / year = the first instant
                     of the civil month / quarter / year of the proleptic Gregorian calendar
  timeConvert        JavaTimeUnitTransformer.java:37-41: out = outputUnit.convert(v, inputUnit)
  dateTimeConvert    EpochToEpochTransformer.java:44-46, BaseDateTimeTransformer.java:208-243 (EPOCH -> EPOCH, no
                     bucketing zone): ms = U.toMillis(v * a) (the product wraps); q = (ms / G) * G truncating toward
                     zero, G = G.toMillis(g); out = W.convert(q, MILLISECONDS) / b

`evaluate(kt, values)` applies a pinot_amd.query.KeyTransform to an integer array."""
import numpy as np

UNITS = ("NANOSECONDS", "MICROSECONDS", "MILLISECONDS", "SECONDS", "MINUTES", "HOURS", "DAYS")
NANOS = dict(zip(UNITS, (1, 10 ** 3, 10 ** 6, 10 ** 9, 60 * 10 ** 9, 3600 * 10 ** 9, 86400 * 10 ** 9)))
I64 = np.iinfo(np.int64)
DAY_MS = 86_400_000
FIXED_MS = {"millisecond": 1, "second": 1000, "minute": 60_000, "hour": 3_600_000, "day": DAY_MS}


def _i64(v) -> np.ndarray:
    return np.atleast_1d(np.asarray(v, dtype=np.int64)).copy()


def trunc_div(a: np.ndarray, d: int) -> np.ndarray:
    """Java's a / d for d > 0: toward zero."""
    q = a // np.int64(d)
    return q + ((a % np.int64(d) != 0) & (a < 0))


def convert(v, to_unit: str, from_unit: str) -> np.ndarray:
    """to_unit.convert(v, from_unit)."""
    a = _i64(v)
    f, t = NANOS[from_unit], NANOS[to_unit]
    if f == t:
        return a
    if f < t:
        return trunc_div(a, t // f)
    r = f // t
    lim = I64.max // r
    with np.errstate(over="ignore"):
        out = a * np.int64(r)
    out[a > lim] = I64.max
    out[a < -lim] = I64.min
    return out


def floor_to(a: np.ndarray, d: int) -> np.ndarray:
    with np.errstate(over="ignore"):
        return (a // np.int64(d)) * np.int64(d)


def days_from_civil(y: np.ndarray, m: np.ndarray) -> np.ndarray:
    """Days since 1970-01-01 of the first day of month m of year y (proleptic Gregorian)."""
    y = y - (m <= 2)
    era = y // 400
    yoe = y - era * 400
    doy = (153 * np.where(m > 2, m - 3, m + 9) + 2) // 5
    return era * 146097 + yoe * 365 + yoe // 4 - yoe // 100 + doy - 719468


def civil_from_days(z: np.ndarray):
    z = z + 719468
    era = z // 146097
    doe = z - era * 146097
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)
    mp = (5 * doy + 2) // 153
    m = np.where(mp < 10, mp + 3, mp - 9)
    return yoe + era * 400 + (m <= 2), m


def round_floor(ms, unit: str) -> np.ndarray:
    ms = _i64(ms)
    if unit in FIXED_MS:
        return floor_to(ms, FIXED_MS[unit])
    if unit == "week":
        with np.errstate(over="ignore"):
            return floor_to(ms + np.int64(3 * DAY_MS), 7 * DAY_MS) - np.int64(3 * DAY_MS)
    y, m = civil_from_days(ms // np.int64(DAY_MS))
    if unit == "year":
        m = np.ones_like(m)
    elif unit == "quarter":
        m = (m - 1) // 3 * 3 + 1
    elif unit != "month":
        raise ValueError(unit)
    with np.errstate(over="ignore"):
        return days_from_civil(y, m) * np.int64(DAY_MS)


def date_trunc(unit: str, v, in_unit="MILLISECONDS", out_unit=None) -> np.ndarray:
    return convert(round_floor(convert(v, "MILLISECONDS", in_unit), unit.lower()), out_unit or in_unit, "MILLISECONDS")


def time_convert(v, in_unit: str, out_unit: str) -> np.ndarray:
    return convert(v, out_unit, in_unit)


def date_time_convert(v, in_size: int, in_unit: str, out_size: int, out_unit: str, gran_size: int, gran_unit: str):
    with np.errstate(over="ignore"):
        ms = convert(_i64(v) * np.int64(in_size), "MILLISECONDS", in_unit)
    g = int(convert([gran_size], "MILLISECONDS", gran_unit)[0])
    with np.errstate(over="ignore"):
        q = trunc_div(ms, g) * np.int64(g)
    return trunc_div(convert(q, out_unit, "MILLISECONDS"), out_size)


def evaluate(kt, values) -> np.ndarray:
    """The LONG key values of pinot_amd.query.KeyTransform `kt` over `values`."""
    if kt.kind == "datetrunc":
        return date_trunc(kt.trunc_unit, values, kt.in_unit, kt.out_unit)
    if kt.kind == "timeconvert":
        return time_convert(values, kt.in_unit, kt.out_unit)
    return date_time_convert(values, kt.in_size, kt.in_unit, kt.out_size, kt.out_unit, kt.gran_size, kt.gran_unit)
