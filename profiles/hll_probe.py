"""DISTINCTCOUNTHLL on bench-sized segments.

    python profiles/hll_probe.py [--segments 2] [--rows 10000000] [--steps 15] [--out FILE]

Bench segments (datagen.ad_segment): `impressions` is a raw LONG column of ~rows distinct values per segment,
`daysSinceEpoch` a dictionary-encoded one. Prints one JSON line:

* the first execute of DISTINCTCOUNTHLL over segments 1.. after segment 0 took the hipRTC compiles, on the host's clock,
  per segment -- it holds the twin build (hll_hash_kernel, the dictId remap, the packing and the staging copies) and
  the planning of the base and register queries -- for the raw LONG source and for the dictionary source, with the
  twins' device bytes per segment;
* the re-issued time (execute_again, device events: last_kernel_ms, base plus child scans) of DISTINCTCOUNTHLL(impressions)
  and of the baseline the parent commit runs, native DISTINCTCOUNT(impressions) of the same query, alternating, median
  and min..max over the steps: without GROUP BY and grouped by country; each plan's kernel_info and algorithmic bytes
  (the register query reads log2m + 5 bits per doc for the column), and the device memory each first execute took
  (the plans' tables and work buffers; the twins apart).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"no_group_by": "SELECT {agg} FROM t WHERE clicks > 100",
          "group_by_country": "SELECT country, {agg} FROM t WHERE clicks > 100 GROUP BY country LIMIT 1000"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=2)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    from pinot_amd import datagen, engine as E
    segs = [E.ImmutableSegment(datagen.ad_segment(f"hp{i}", args.rows, 300 + i)) for i in range(args.segments)]
    ex = E.ServerQueryExecutor(distinct_count="native")
    out = {"segments": args.segments, "rows_per_segment": args.rows, "steps": args.steps, "log2m": 8}

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    # ---- twin build: segment 0 warms the compiles, segments 1.. are timed
    built = max(args.segments - 1, 1)
    for tag, col in (("raw_long_source", "impressions"), ("dictionary_source", "daysSinceEpoch")):
        q = f"SELECT DISTINCTCOUNTHLL({col}) FROM t"
        ex.execute(q, segs[:1]).rows()
        rest = segs[1:] or segs[:1]
        before = sum(s.device_bytes() for s in rest)
        t0 = time.perf_counter()
        r = ex.execute(q, rest)
        rows = r.rows()
        t1 = time.perf_counter()
        twins = sum(s.device_bytes() for s in rest) - before
        r2 = ex.execute(q, rest)
        r2.rows()
        t2 = time.perf_counter()
        out[tag] = {"column": col, "first_execute_ms_per_segment": (t1 - t0) * 1e3 / built,
                    "second_execute_ms_per_segment": (t2 - t1) * 1e3 / built, "twin_bytes_per_segment": twins / built,
                    "estimate": rows[0][0], "kernel_info": r.kernel_info()}
    # ---- re-issued: DISTINCTCOUNTHLL against native DISTINCTCOUNT
    plans = {}
    for shape, text in SHAPES.items():
        o = {}
        for tag, agg in (("hll", "DISTINCTCOUNTHLL(impressions)"), ("distinctcount", "DISTINCTCOUNT(impressions)")):
            f0 = free_bytes()
            try:
                r = ex.execute(text.format(agg=agg), segs)
                rows = r.rows()
            except Exception as e:  # the baseline may not fit: recorded, not hidden
                o[tag] = {"error": str(e)[:300]}
                continue
            o[tag] = {"kernel_info": r.kernel_info(), "algorithmic_bytes": r.algorithmic_bytes(),
                      "first_execute_device_bytes": f0 - free_bytes(), "groups": len(rows),
                      "first_row": [int(x) for x in rows[0]] if rows else None}
            plans[(shape, tag)] = r
        out[shape] = o
    for r in plans.values():
        for _ in range(2):
            r.execute_again()
            r.rows()
    for shape in SHAPES:
        tags = [t for t in ("hll", "distinctcount") if (shape, t) in plans]
        ms = {t: [] for t in tags}
        for _ in range(args.steps):  # alternating, so drift hits both alike
            for t in tags:
                r = plans[(shape, t)]
                r.execute_again()
                ms[t].append(r.last_kernel_ms())
        for t, v in ms.items():
            out[shape][t]["reissued_scan_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        # the fold runs when the groups are first read after an execution: execute_again + rows() on the host's clock
        for t in tags:
            r = plans[(shape, t)]
            v = []
            for _ in range(max(args.steps // 3, 3)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r.execute_again()
                r.rows()
                v.append((time.perf_counter() - t0) * 1e3)
            out[shape][t]["reissued_with_fold_wall_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
