"""Mirror against native for one value-set query: bench.py's AdAnalytics table, the query re-issued
alternately through ServerQueryExecutor(distinct_count="mirror") and ("native") in one process; median and min-max of
--reps re-issues after --warmup rounds of execute_again + rows(), of rows() alone and of the scan kernels alone
(last_kernel_ms). --shape value-aggs: PERCENTILE50 / PERCENTILE99 / DISTINCTAVG; --shape distinctcount: the round-7
DISTINCTCOUNT shape (runs on a tree without the newer functions too: the fold's regression guard).

    python scripts/measure_value_aggs.py --shape value-aggs --segments 40 --rows 10000000 --reps 15
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

QUERIES = {
    "value-aggs": "SELECT country, PERCENTILE50(clicks), PERCENTILE99(clicks), DISTINCTAVG(clicks), COUNT(*) "
                  "FROM adAnalytics GROUP BY country LIMIT 1000",
    "distinctcount": "SELECT country, DISTINCTCOUNT(clicks), COUNT(*) FROM adAnalytics GROUP BY country LIMIT 1000",
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(QUERIES), default="value-aggs")
    ap.add_argument("--segments", type=int, default=40)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="mirror,native")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import torch
    from pinot_amd import datagen, engine
    torch.cuda.set_device(0)
    q = QUERIES[args.shape]
    segs = [engine.ImmutableSegment(datagen.ad_segment(f"ad_{i}", args.rows, seed=i)) for i in range(args.segments)]
    modes = args.modes.split(",")
    res, cold = {}, {}
    for m in modes:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res[m] = engine.ServerQueryExecutor(distinct_count=m).execute(q, segs)
        rows = res[m].rows()
        torch.cuda.synchronize()
        cold[m] = (time.perf_counter() - t0) * 1e3
        if m == modes[0]:
            first = rows
        else:
            assert rows == first, "the modes disagree"
    t = {m: {"all": [], "rows": [], "scan": []} for m in modes}
    for rep in range(args.warmup + args.reps):
        for m in modes:
            r = res[m]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.execute_again()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            r.rows()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if rep >= args.warmup:
                t[m]["all"].append((t2 - t0) * 1e3)
                t[m]["rows"].append((t2 - t1) * 1e3)
                t[m]["scan"].append(r.last_kernel_ms())
    print(f"{args.label}query: {q}")
    print(f"table: bench.py's AdAnalytics table (datagen.ad_segment), {args.segments} segments x {args.rows} rows; "
          f"{len(first)} groups")
    if "native" in res:
        print(f"native kernel_info: {res['native'].kernel_info()}")
    print(f"{args.reps} re-issues per mode after {args.warmup} warm-up rounds, interleaved {'/'.join(modes)}, host clock "
          "around execute_again + rows() ending in a device synchronise")
    names = {"all": "execute_again + rows()", "rows": "rows() alone (fetch + fold)", "scan": "scan kernels (last_kernel_ms)"}
    for m in modes:
        for k in ("all", "rows", "scan"):
            v = t[m][k]
            print(f"{m} {names[k]:<32} median {statistics.median(v):9.3f} ms  min {min(v):9.3f}  max {max(v):9.3f}")
    print("cold (first execute + rows()): " + ", ".join(f"{m} {cold[m]:.1f} ms" for m in modes))
    for r in res.values():
        r.destroy()


if __name__ == "__main__":
    main()
