# Filtered aggregations on the bench table (datagen.ad_segment, 100 x 10M rows): the fused query -- COUNT(*) plus two
# filter lanes under the bench query's main filter, one scan on the LDS-table plan -- against the three plain queries
# that answer the same question (WHERE main, WHERE main AND f1, WHERE main AND f2). Kernel ms are device events around
# a warm re-issue (execute_again of the prepared plan); medians over --reps.
#   PYTHONPATH=. python profiles/filtered_probe.py --mode fused|plain [--segments 100] [--rows 10000000] [--reps 15] --out FILE
# --mode plain issues no FILTER clause, so the same file measures a checkout from before the feature (the comparison
# is run there, alternating with --mode fused here, in one session on one device).
import argparse
import json
import statistics

import torch

from pinot_amd import datagen
from pinot_amd import engine as E

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=["fused", "plain"], required=True)
ap.add_argument("--segments", type=int, default=100)
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--out", required=True)
ap.add_argument("--commit", default="")
args = ap.parse_args()

MAIN = f"daysSinceEpoch BETWEEN {datagen.DAYS_BASE + 100} AND {datagen.DAYS_BASE + 300} AND clicks > 100"
F1 = "country IN (7, 42, 123)"            # a lane on dictionary data (an accept-mask / dictId-set leaf)
F2 = f"impressions < {1 << 39}"           # a lane on a raw LONG range
FUSED = ("SELECT daysSinceEpoch, COUNT(*), "
         f"SUM(clicks) FILTER (WHERE {F1}), SUM(impressions) FILTER (WHERE {F1}), "
         f"SUM(cost) FILTER (WHERE {F2}), MAX(cost) FILTER (WHERE {F2}) "
         f"FROM adAnalytics WHERE {MAIN} GROUP BY daysSinceEpoch LIMIT 1000")
PLAIN = [
    ("main", f"SELECT daysSinceEpoch, COUNT(*) FROM adAnalytics WHERE {MAIN} GROUP BY daysSinceEpoch LIMIT 1000"),
    ("main_and_f1", f"SELECT daysSinceEpoch, SUM(clicks), SUM(impressions) FROM adAnalytics WHERE {MAIN} AND {F1} "
                    "GROUP BY daysSinceEpoch LIMIT 1000"),
    ("main_and_f2", f"SELECT daysSinceEpoch, SUM(cost), MAX(cost) FROM adAnalytics WHERE {MAIN} AND {F2} "
                    "GROUP BY daysSinceEpoch LIMIT 1000"),
]

assert torch.cuda.is_available(), "this probe measures on the GPU"
segs = [E.ImmutableSegment(datagen.ad_segment(f"ad{i}", args.rows, seed=i)) for i in range(args.segments)]
ex = E.ServerQueryExecutor()
out = {"mode": args.mode, "commit": args.commit, "segments": args.segments, "rows_per_segment": args.rows,
       "reps": args.reps, "queries": {}}
for name, sql in ([("fused", FUSED)] if args.mode == "fused" else PLAIN):
    r = ex.execute(sql, segs)   # cold: plans and compiles
    rows = r.rows()
    for _ in range(3):
        r.execute_again()
    torch.cuda.synchronize()
    kms = []
    for _ in range(args.reps):
        r.execute_again()
        torch.cuda.synchronize()
        kms.append(r.last_kernel_ms())
    out["queries"][name] = {"sql": sql, "kernel_info": r.kernel_info(), "kernel_ms_median": statistics.median(kms),
                            "kernel_ms_min": min(kms), "kernel_ms_max": max(kms),
                            "algorithmic_gb": r.algorithmic_bytes() / 1e9, "groups": len(rows),
                            "checksum": repr(sorted(rows)[:2])}
    print(name, out["queries"][name]["kernel_info"], f"{statistics.median(kms):.3f} ms", flush=True)
    r.destroy()
out["kernel_ms_sum_of_medians"] = sum(q["kernel_ms_median"] for q in out["queries"].values())
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
