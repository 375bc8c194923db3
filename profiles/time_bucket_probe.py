"""Time-bucket GROUP BY keys on bench-sized segments.

    python profiles/time_bucket_probe.py [--segments 4] [--rows 10000000] [--steps 30] [--out FILE]

Each segment is a bench segment (datagen.ad_segment: 10M rows) spanning one day, plus `ts` (raw LONG epoch
milliseconds), `tsd` (the same instants at one-second resolution, dictionary-encoded: 86400 values, 17 bits) and `hourd`
(their 24 hourly buckets as an ordinary dictionary-encoded LONG column, 5 bits: what the twin of
dateTrunc('hour', ts) must equal). Prints one JSON line:

* twin build time per segment for the raw LONG and the dictionary source: the `raw_keys` phase of the first
  query's plan_timing over the segments;
* the re-issued time (execute_again, device events: last_kernel_ms) of the bench-shaped query grouped by
  dateTrunc('hour', ts), by dateTrunc('hour', tsd) and -- the baseline -- by hourd, alternating the three, median
  and min..max over the steps, with each plan's kernel_info and algorithmic bytes.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DAY0 = 17000 * 86_400_000  # the day's first millisecond
QUERY = ("SELECT {k}, COUNT(*), SUM(clicks), SUM(impressions), SUM(cost), MAX(cost) FROM t "
         "WHERE clicks > 100 GROUP BY {k} LIMIT 1000")


def segment(name, n, seed):
    import torch
    from pinot_amd import datagen, segment as S
    bufs = datagen.ad_segment(name, n, seed)
    g = torch.Generator(device="cuda")
    g.manual_seed(seed + 7)
    sec = torch.randint(0, 86400, (n,), generator=g, device="cuda", dtype=torch.int32)
    sec[:86400] = torch.arange(86400, device="cuda", dtype=torch.int32)   # every second present: dictId = second
    ms = DAY0 + sec.to(torch.int64) * 1000 + torch.randint(0, 1000, (n,), generator=g, device="cuda", dtype=torch.int64)
    bufs.columns["ts"] = S.ColumnBuffers("ts", S.LONG, n, False, fwd=S.raw_fwd_header(n, S.LONG) + datagen._be_bytes(ms, 8))
    dsec = DAY0 + np.arange(86400, dtype=np.int64) * 1000
    bufs.columns["tsd"] = S.ColumnBuffers("tsd", S.LONG, n, True, False, 86400, 17, datagen._fixed_bit(sec, 17),
                                          S.dictionary_bytes(dsec, S.LONG), None, dsec)
    hour = torch.div(sec, 3600, rounding_mode="floor").to(torch.int32)
    dhour = DAY0 + np.arange(24, dtype=np.int64) * 3_600_000
    bufs.columns["hourd"] = S.ColumnBuffers("hourd", S.LONG, n, True, False, 24, 5, datagen._fixed_bit(hour, 5),
                                            S.dictionary_bytes(dhour, S.LONG), None, dhour)
    torch.cuda.synchronize()
    return bufs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    from pinot_amd import engine as E
    segs = [E.ImmutableSegment(segment(f"tb{i}", args.rows, 100 + i)) for i in range(args.segments)]
    ex = E.ServerQueryExecutor()
    keys = {"twin_raw_long": "dateTrunc('hour', ts)", "twin_dictionary": "dateTrunc('hour', tsd)", "staged_dictionary": "hourd"}
    out = {"segments": args.segments, "rows_per_segment": args.rows, "steps": args.steps}
    res = {}
    for name, k in keys.items():
        before = sum(s.device_bytes() for s in segs)
        r = ex.execute(QUERY.format(k=k), segs)
        res[name] = r
        out[name] = {"key": k, "kernel_info": r.kernel_info(), "algorithmic_bytes": r.algorithmic_bytes(),
                     "first_execute_raw_keys_ms": r.plan_timing().get("raw_keys"),
                     "twin_bytes_per_segment": (sum(s.device_bytes() for s in segs) - before) / args.segments}
        if name != "staged_dictionary":
            out[name]["twin_build_ms_per_segment"] = out[name]["first_execute_raw_keys_ms"] / args.segments
    groups = {n: r.groups() for n, r in res.items()}

    def same(a, b):  # keys and integer results exactly; SUM(cost), a double sum in atomic order, within 1e-12 relative
        return set(a) == set(b) and all(
            x[:3] == y[:3] and x[4] == y[4] and abs(x[3] - y[3]) <= 1e-12 * abs(y[3]) for x, y in ((a[k], b[k]) for k in b))

    out["results_equal"] = (same(groups["twin_raw_long"], groups["staged_dictionary"])
                            and same(groups["twin_dictionary"], groups["staged_dictionary"]))
    out["groups"] = len(groups["staged_dictionary"])
    for r in res.values():   # warm up every plan
        for _ in range(3):
            r.execute_again()
    ms = {n: [] for n in res}
    for _ in range(args.steps):  # alternating, so drift hits all three alike
        for n, r in res.items():
            r.execute_again()
            ms[n].append(r.last_kernel_ms())
    for n, v in ms.items():
        out[n]["reissued_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    base = out["staged_dictionary"]["reissued_ms"]["median"]
    for n in ("twin_raw_long", "twin_dictionary"):
        out[n]["reissued_vs_staged"] = out[n]["reissued_ms"]["median"] / base
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
