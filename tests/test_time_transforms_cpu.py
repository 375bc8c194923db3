"""GROUP BY time buckets without a device: the numpy restatement of dateTrunc / timeConvert / dateTimeConvert
(time_transform_ref.py) against the values Pinot's own tests assert (tests/golden/time_transforms_expected.json),
against hand-computed edge cases and against Python's datetime for the civil units; and the SQL front end: spellings,
defaults, the canonical text, SELECT / ORDER BY matching and the refusal of every unsupported form."""
import datetime as dt
import json
import os

import numpy as np
import pytest

import time_transform_ref as R
from helpers import GOLDEN
from pinot_amd.query import KeyTransform, key_transform, parse_sql, split_distinct_count

I64 = np.iinfo(np.int64)
with open(os.path.join(GOLDEN, "time_transforms_expected.json")) as f:
    EXPECTED = json.load(f)
CASES = [(k, c) for k in ("datetrunc", "datetimeconvert") for c in EXPECTED[k]]


@pytest.mark.parametrize("kind,case", CASES, ids=[f"{k}-{c['source'].split(':')[1]}" for k, c in CASES])
def test_restatement_reproduces_pinot_expected(kind, case):
    kt = key_transform(case["expr"])
    assert kt is not None and kt.kind == kind and kt.column == "ts"
    assert R.evaluate(kt, [case["input"]]).tolist() == [case["expected"]]


@pytest.mark.parametrize("case", EXPECTED["datetimeconvert_utc_zone"])
def test_bucketing_zone_is_refused(case):
    with pytest.raises(ValueError, match="time zone"):
        key_transform(case["expr"])


def test_negative_instants():
    assert R.date_trunc("hour", [-1]).tolist() == [-3_600_000]                 # a true floor
    assert R.date_trunc("day", [-1, -86_400_000, -86_400_001]).tolist() == [-86_400_000, -86_400_000, -172_800_000]
    assert R.date_trunc("week", [-1]).tolist() == [-259_200_000]               # Monday 1969-12-29
    assert R.date_trunc("week", [-259_200_000, -259_200_001]).tolist() == [-259_200_000, -864_000_000]
    assert R.date_trunc("month", [-1]).tolist() == [-31 * 86_400_000]          # 1969-12-01
    assert R.date_trunc("year", [-1]).tolist() == [-365 * 86_400_000]          # 1969-01-01
    # dateTimeConvert divides toward zero: the hour of -1 ms is 0, not -3600000
    assert R.date_time_convert([-1], 1, "MILLISECONDS", 1, "MILLISECONDS", 1, "HOURS").tolist() == [0]
    assert R.date_time_convert([-3_600_001], 1, "MILLISECONDS", 1, "HOURS", 1, "HOURS").tolist() == [-1]
    assert R.time_convert([-1, -1000, -1001], "MILLISECONDS", "SECONDS").tolist() == [0, -1, -1]


def test_saturation():
    big = 1 << 40
    ms = R.convert([big, -big], "MILLISECONDS", "DAYS")
    assert ms.tolist() == [I64.max, I64.min]
    # dateTrunc of a DAYS input that saturates: floor of Long.MAX_VALUE to the hour, back to days
    assert R.date_trunc("hour", [big], "DAYS").tolist() == [(I64.max - I64.max % 3_600_000) // 86_400_000]
    assert R.time_convert([big], "DAYS", "NANOSECONDS").tolist() == [I64.max]
    assert R.time_convert([-big], "DAYS", "NANOSECONDS").tolist() == [I64.min]
    lim = I64.max // 1000
    assert R.time_convert([lim, lim + 1, -lim, -lim - 1], "SECONDS", "MILLISECONDS").tolist() == \
        [lim * 1000, I64.max, -lim * 1000, I64.min]
    # dateTimeConvert: v * size wraps (Java long), toMillis saturates
    v = (1 << 62) + 5
    wrapped = (v * 4 + (1 << 63)) % (1 << 64) - (1 << 63)
    assert R.date_time_convert([v], 4, "MILLISECONDS", 1, "MILLISECONDS", 1, "MILLISECONDS").tolist() == [wrapped]
    assert R.date_time_convert([big], 1, "DAYS", 1, "DAYS", 1, "DAYS").tolist() == [I64.max // 86_400_000]


def _ms(d: dt.datetime) -> int:
    delta = d - dt.datetime(1970, 1, 1)
    return (delta.days * 86_400 + delta.seconds) * 1000 + delta.microseconds // 1000


def test_civil_units_against_datetime():
    rng = np.random.default_rng(5)
    lo, hi = _ms(dt.datetime(1, 1, 1)), _ms(dt.datetime(9999, 12, 31, 23, 59, 59, 999000))
    fixed = [dt.datetime(y, m, d, 23, 59, 59, 999000) for y in (1900, 2000, 2100, 2024, 1600, 4)
             for m, d in ((2, 28), (3, 1), (12, 31), (1, 1))]
    fixed += [dt.datetime(2000, 2, 29), dt.datetime(2024, 2, 29, 12), dt.datetime(1600, 2, 29), dt.datetime(1969, 12, 31),
              dt.datetime(1, 1, 1), dt.datetime(9999, 12, 31)]
    inst = np.concatenate([rng.integers(lo, hi, 4000, endpoint=True), np.array([_ms(d) for d in fixed], dtype=np.int64),
                           np.array([lo, hi], dtype=np.int64)])
    when = [dt.datetime(1970, 1, 1) + dt.timedelta(milliseconds=int(x)) for x in inst]
    exp = {
        "year": [_ms(d.replace(month=1, day=1, hour=0, minute=0, second=0, microsecond=0)) for d in when],
        "quarter": [_ms(d.replace(month=(d.month - 1) // 3 * 3 + 1, day=1, hour=0, minute=0, second=0, microsecond=0))
                    for d in when],
        "month": [_ms(d.replace(day=1, hour=0, minute=0, second=0, microsecond=0)) for d in when],
        "week": [_ms((d - dt.timedelta(days=d.weekday())).replace(hour=0, minute=0, second=0, microsecond=0))
                 for d in when if d >= dt.datetime(1, 1, 8)],
        "day": [_ms(d.replace(hour=0, minute=0, second=0, microsecond=0)) for d in when],
    }
    for unit in ("year", "quarter", "month", "day"):
        assert R.date_trunc(unit, inst).tolist() == exp[unit], unit
    late = np.array([x for x, d in zip(inst.tolist(), when) if d >= dt.datetime(1, 1, 8)], dtype=np.int64)
    assert R.date_trunc("week", late).tolist() == exp["week"]
    # through another input / output unit: seconds in, days out
    secs = inst // 1000
    assert R.date_trunc("month", secs, "SECONDS", "DAYS").tolist() == [e // 86_400_000 for e in exp["month"]]


HOUR = "datetrunc('hour',ts,'MILLISECONDS','UTC','MILLISECONDS')"


@pytest.mark.parametrize("spelling", ["dateTrunc('hour', ts)", "DATETRUNC('HOUR', ts)", "datetrunc('hour',ts,'milliseconds')",
                                      "date_trunc('Hour', ts, 'MILLISECONDS', 'UTC')",
                                      "DATE_TRUNC(hour, ts, 'MILLISECONDS', 'utc', 'milliseconds')"])
def test_datetrunc_spellings_and_defaults(spelling):
    qc = parse_sql(f"SELECT {spelling}, SUM(clicks) FROM t WHERE ts > 5 GROUP BY {spelling} ORDER BY {spelling} LIMIT 1000")
    assert qc.group_by == [HOUR] and qc.select_columns == [HOUR]
    assert qc.order_by == [(HOUR, True)] and qc.order_by_targets() == [(0, 0, True)]
    assert qc.safe_trim() and not qc.is_selection()
    assert key_transform(HOUR) == KeyTransform("datetrunc", "ts", "MILLISECONDS", "MILLISECONDS", trunc_unit="hour")


def test_canonical_texts():
    qc = parse_sql("SELECT COUNT(*) FROM t GROUP BY dateTrunc('week', ts, 'seconds'), "
                   "timeConvert(ts, 'milliseconds', 'DAYS'), TIMECONVERT(ts,'SECONDS','hours'), "
                   "DATETIMECONVERT(ts, '1:milliseconds:epoch', '1:HOURS:EPOCH', '15:minutes'), "
                   "dateTimeConvert(t2, '5:MINUTES:EPOCH', '2:DAYS:EPOCH', '1:DAYS'), plain")
    assert qc.group_by == [
        "datetrunc('week',ts,'SECONDS','UTC','SECONDS')",
        "timeconvert(ts,'MILLISECONDS','DAYS')",
        "timeconvert(ts,'SECONDS','HOURS')",
        "datetimeconvert(ts,'1:MILLISECONDS:EPOCH','1:HOURS:EPOCH','15:MINUTES')",
        "datetimeconvert(t2,'5:MINUTES:EPOCH','2:DAYS:EPOCH','1:DAYS')",
        "plain"]
    for g in qc.group_by[:-1]:   # the canonical text parses to the same transform
        assert key_transform(g).text == g
    assert key_transform("plain") is None and key_transform("count(*)") is None
    kt = key_transform(qc.group_by[3])
    assert (kt.in_size, kt.in_unit, kt.out_size, kt.out_unit, kt.gran_size, kt.gran_unit) == \
        (1, "MILLISECONDS", 1, "HOURS", 15, "MINUTES")
    assert key_transform("dateTrunc('day', ts, 'SECONDS', 'UTC', 'HOURS')").out_unit == "HOURS"


def test_select_and_order_by_match_by_canonical_text():
    qc = parse_sql("SELECT d, DATETIMECONVERT(ts,'1:MILLISECONDS:EPOCH','1:HOURS:EPOCH','1:HOURS'), COUNT(*) FROM t "
                   "GROUP BY d, dateTimeConvert(ts, '1:MILLISECONDS:EPOCH', '1:HOURS:EPOCH', '1:HOURS') "
                   "ORDER BY datetimeconvert(ts, '1:milliseconds:EPOCH', '1:hours:EPOCH', '1:hours') DESC, count(*) LIMIT 7")
    text = "datetimeconvert(ts,'1:MILLISECONDS:EPOCH','1:HOURS:EPOCH','1:HOURS')"
    assert qc.group_by == ["d", text] and qc.select_columns == ["d", text]
    assert qc.order_by_targets() == [(0, 1, False), (1, 0, True)]
    assert not qc.safe_trim()
    # hour and day buckets are different keys
    with pytest.raises(ValueError, match="not a GROUP BY key"):
        parse_sql("SELECT dateTrunc('day', ts), COUNT(*) FROM t GROUP BY dateTrunc('hour', ts)")
    with pytest.raises(ValueError, match="not a GROUP BY key"):
        parse_sql("SELECT COUNT(*) FROM t GROUP BY dateTrunc('hour', ts) ORDER BY dateTrunc('hour', ts, 'SECONDS')")


def test_value_set_sub_queries_keep_the_key():
    qc = parse_sql("SELECT dateTrunc('hour', ts), DISTINCTCOUNT(u), PERCENTILE50(x) FROM t GROUP BY dateTrunc('hour', ts)")
    base, subs = split_distinct_count(qc)
    assert base.group_by == [HOUR]
    assert [sq.group_by for _, sq in subs] == [[HOUR, "u"], [HOUR, "x"]]


@pytest.mark.parametrize("sql,what", [
    ("dateTrunc('hour', ts, 'MILLISECONDS', 'Europe/Berlin')", "time zone"),
    ("dateTrunc('hour', ts, 'MILLISECONDS', 'CET', 'SECONDS')", "time zone"),
    ("dateTrunc('decade', ts)", "bad unit"),
    ("dateTrunc('hour', ts, 'FORTNIGHTS')", "bad input unit"),
    ("dateTrunc('hour')", "two to five"),
    ("dateTrunc('hour', 5)", "column"),
    ("timeConvert(ts, 'MILLISECONDS', 'WEEKS')", "WEEKS"),
    ("timeConvert(ts, 'MILLISECONDS', 'months')", "MONTHS"),
    ("timeConvert(ts, 'MILLISECONDS', 'YEARS')", "YEARS"),
    ("timeConvert(ts, 'MILLISECONDS')", "two units"),
    ("dateTimeConvert(ts, '1:MILLISECONDS:EPOCH', '1:DAYS:SIMPLE_DATE_FORMAT:yyyyMMdd', '1:DAYS')", "not supported"),
    ("dateTimeConvert(ts, '1:DAYS:SIMPLE_DATE_FORMAT:yyyyMMdd', '1:MILLISECONDS:EPOCH', '1:DAYS')", "not supported"),
    ("dateTimeConvert(ts, '1:MILLISECONDS:TIMESTAMP', '1:MILLISECONDS:EPOCH', '1:DAYS')", "not supported"),
    ("dateTimeConvert(ts, 'EPOCH|MILLISECONDS|1', '1:MILLISECONDS:EPOCH', '1:DAYS')", "not supported"),
    ("dateTimeConvert(ts, '1:MILLISECONDS:EPOCH', '1:WEEKS:EPOCH', '1:DAYS')", "WEEKS"),
    ("dateTimeConvert(ts, '1:MILLISECONDS:EPOCH', '1:MILLISECONDS:EPOCH', '1:MONTHS')", "MONTHS"),
    ("dateTimeConvert(ts, '1:MILLISECONDS:EPOCH', '1:MILLISECONDS:EPOCH', '1:HOURS', 'CET')", "time zone"),
    ("dateTimeConvert(ts, '0:MILLISECONDS:EPOCH', '1:MILLISECONDS:EPOCH', '1:HOURS')", "positive"),
    ("dateTimeConvert(ts, '1:MILLISECONDS:EPOCH', '1:MILLISECONDS:EPOCH', '-4:HOURS')", "positive"),
    ("dateTimeConvert(ts, '1:MILLISECONDS:EPOCH', '1:MILLISECONDS:EPOCH')", "four arguments"),
])
def test_unsupported_forms_raise(sql, what):
    with pytest.raises(ValueError, match=what):
        parse_sql(f"SELECT COUNT(*) FROM t GROUP BY {sql}")


def test_transform_in_a_selection_query_is_refused():
    with pytest.raises(ValueError, match="selection"):
        parse_sql("SELECT dateTrunc('hour', ts) FROM t LIMIT 5")
    with pytest.raises(ValueError, match="selection"):
        parse_sql("SELECT ts FROM t ORDER BY dateTrunc('hour', ts) LIMIT 5")


def test_add_group_by_transform_validates_its_spec():
    """The C entry point without a device: bad enums, sizes <= 0 and NULL arguments are EINVAL at add; a transformed
    key takes no installed key space (EUNSUPPORTED); a plain GROUP BY on the same column still does."""
    import ctypes as C
    from pinot_amd import engine as E
    from pinot_amd._lib import lib
    L = lib()
    qh = C.c_void_p()
    assert L.pinot_amd_query_create(C.byref(qh)) == 0
    good = E.key_transform_spec(key_transform("dateTimeConvert(ts, '5:MINUTES:EPOCH', '1:HOURS:EPOCH', '4:HOURS')"))
    assert (good.kind, good.in_unit, good.in_size, good.out_unit, good.out_size, good.gran_unit, good.gran_size) == \
        (2, 4, 5, 5, 1, 5, 4)
    trunc = E.key_transform_spec(key_transform("dateTrunc('quarter', ts, 'SECONDS')"))
    assert (trunc.kind, trunc.trunc_unit, trunc.in_unit, trunc.out_unit) == (0, 7, 3, 3)
    for field, bad in (("kind", 3), ("kind", -1), ("in_unit", 7), ("out_unit", -1), ("gran_unit", 7), ("in_size", 0),
                       ("out_size", -1), ("gran_size", 0)):
        sp = type(good).from_buffer_copy(good)
        setattr(sp, field, bad)
        assert L.pinot_amd_query_add_group_by_transform(qh, b"ts", C.byref(sp)) == -1, field
    sp = type(trunc).from_buffer_copy(trunc)
    sp.trunc_unit = 9
    assert L.pinot_amd_query_add_group_by_transform(qh, b"ts", C.byref(sp)) == -1
    assert L.pinot_amd_query_add_group_by_transform(qh, None, C.byref(good)) == -1
    assert L.pinot_amd_query_add_group_by_transform(qh, b"ts", None) == -1
    vals = (C.c_int64 * 2)(0, 1)
    assert L.pinot_amd_query_set_group_key_values(qh, b"ts", 1, 2, vals, None, None) == 0   # no transformed key yet
    assert L.pinot_amd_query_add_group_by(qh, b"d") == 0
    assert L.pinot_amd_query_add_group_by_transform(qh, b"ts", C.byref(trunc)) == 0
    assert L.pinot_amd_query_add_group_by_transform(qh, b"ts", C.byref(good)) == 0
    assert L.pinot_amd_query_add_order_by(qh, 0, 2, 0) == 0      # the third key, by position
    assert L.pinot_amd_query_add_order_by(qh, 0, 3, 0) == -1
    assert L.pinot_amd_query_set_group_key_values(qh, b"ts", 1, 2, vals, None, None) == -2
    assert L.pinot_amd_query_set_group_key_values(qh, b"d", 0, 2, vals, None, None) == 0
    L.pinot_amd_query_destroy(qh)


def test_multi_gpu_path_refuses_transformed_keys():
    from pinot_amd import dist
    qc = parse_sql("SELECT COUNT(*) FROM t GROUP BY d, dateTrunc('hour', ts)")
    with pytest.raises(ValueError, match="transformed key"):
        dist.key_columns(qc)
    with pytest.raises(ValueError, match="transformed key"):
        dist.global_key_space([], qc.group_by)
    assert dist.key_columns(parse_sql("SELECT COUNT(*) FROM t GROUP BY d")) == ["d"]
