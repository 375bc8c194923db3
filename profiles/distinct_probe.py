# SELECT DISTINCT against its imitation -- GROUP BY cols + COUNT(*) through the server table -- on the bench tables:
#   bench-key   the bench table's key (daysSinceEpoch, 365 keys) under the bench filter, ORDER BY the key
#   highcard    configs[3]'s two 1000-value dimensions (1M keys): the imitation takes the partitioned plan
#   wide        the wide-key table's five columns (key space 4e18): the hash plan on both sides
#   limit10     LIMIT 10 without ORDER BY over every segment of the bench table (the staged scan stops early)
# Kernel ms are device events around a warm re-issue (execute_again of the prepared plan); medians over --reps, with
# the spread of the repeats. The roofline fraction is the plan's algorithmic bytes over the median at the HBM peak.
#   PYTHONPATH=. python profiles/distinct_probe.py --mode distinct|groupby [--segments 100] [--rows 10000000]
#                                                  [--reps 15] [--shapes bench-key,highcard,wide,limit10] --out FILE
# --mode groupby issues no DISTINCT, so the same file measures a checkout from before the feature (the comparison is
# run alternating the two modes in one session on one device).
import argparse
import json
import statistics

import torch

from pinot_amd import datagen
from pinot_amd import engine as E

HBM_PEAK_GBS = 8000.0  # MI355X spec, as bench.py

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=["distinct", "groupby"], required=True)
ap.add_argument("--segments", type=int, default=100)
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--shapes", default="bench-key,highcard,wide,limit10")
ap.add_argument("--out", required=True)
ap.add_argument("--commit", default="")
args = ap.parse_args()

BENCH_FILTER = f"daysSinceEpoch BETWEEN {datagen.DAYS_BASE + 100} AND {datagen.DAYS_BASE + 300} AND clicks > 100"
WIDE = "w1, w2, w3, w4, w5"
# shape -> (segment generator, keys, WHERE, ORDER BY or "", LIMIT, SET prefix of the imitation)
SHAPES = {
    "bench-key": (datagen.ad_segment, "daysSinceEpoch", BENCH_FILTER, "daysSinceEpoch", 1000, ""),
    "highcard": (datagen.highcard_segment, "dimA, dimB", "metInt < 900", "dimA, dimB", 1000, "SET numGroupsLimit = 2000000; "),
    "wide": (datagen.widekeys_segment, WIDE, "metInt < 900", "w1, w2", 1000, "SET numGroupsLimit = 2000000000; "),
    "limit10": (datagen.ad_segment, "country", "clicks > 100", "", 10, ""),
}


def sql_of(shape):
    _, keys, where, order, limit, prefix = SHAPES[shape]
    tail = (f" ORDER BY {order}" if order else "") + f" LIMIT {limit}"
    if args.mode == "distinct":
        return f"SELECT DISTINCT {keys} FROM t WHERE {where}{tail}"
    return f"{prefix}SELECT {keys}, COUNT(*) FROM t WHERE {where} GROUP BY {keys}{tail}"


assert torch.cuda.is_available(), "this probe measures on the GPU"
out = {"mode": args.mode, "commit": args.commit, "segments": args.segments, "rows_per_segment": args.rows,
       "reps": args.reps, "queries": {}}
ex = E.ServerQueryExecutor(server_trim=True)  # the imitation's LIMIT rows come from the server table
held = (None, [])
for shape in args.shapes.split(","):
    gen = SHAPES[shape][0]
    if held[0] is not gen:  # one table in HBM at a time
        for s in held[1]:
            s.destroy()
        held = (gen, [E.ImmutableSegment(gen(f"{shape}{i}", args.rows, seed=i)) for i in range(args.segments)])
    sql = sql_of(shape)
    r = ex.execute(sql, held[1])   # cold: plans and compiles
    rows = r.rows()
    for _ in range(3):
        r.execute_again()
    torch.cuda.synchronize()
    kms = []
    for _ in range(args.reps):
        r.execute_again()
        torch.cuda.synchronize()
        kms.append(r.last_kernel_ms())
    med = statistics.median(kms)
    gb = r.algorithmic_bytes() / 1e9
    out["queries"][shape] = {"sql": sql, "kernel_info": r.kernel_info(), "kernel_ms_median": med,
                             "kernel_ms_min": min(kms), "kernel_ms_max": max(kms), "algorithmic_gb": gb,
                             "roofline_fraction": (gb / HBM_PEAK_GBS * 1e3) / med if med > 0 else None,
                             "docs_matched": r.num_docs_matched(), "rows": len(rows),
                             "first_keys": repr([tuple(x[:len(SHAPES[shape][1].split(','))]) for x in rows[:2]])}
    q = out["queries"][shape]
    print(shape, q["kernel_info"], f"{med:.3f} ms ({min(kms):.3f}..{max(kms):.3f})", f"{gb:.3f} GB",
          f"roofline {q['roofline_fraction']:.3f}" if q["roofline_fraction"] else "", flush=True)
    r.destroy()
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
