# Selection queries on the bench table (datagen.ad_segment, 100 x 10M rows): kernel ms (device events around the
# passes) and end-to-end ms (host clock around a re-issued execute that ends in a device synchronise), against the
# fused scan of SELECT MAX(impressions) with the same filter, which streams the same columns.
#   PYTHONPATH=. python profiles/selection_probe.py [--segments 100] [--rows 10000000] [--reps 15] [--out FILE]
import argparse
import statistics
import sys
import time

import torch

from pinot_amd import datagen
from pinot_amd import engine as E

ap = argparse.ArgumentParser()
ap.add_argument("--segments", type=int, default=100)
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--out", default="profiles/r09/selection.txt")
ap.add_argument("--commit", default="")
args = ap.parse_args()

FILTER = f" WHERE daysSinceEpoch BETWEEN {datagen.DAYS_BASE + 100} AND {datagen.DAYS_BASE + 300} AND clicks > 100"
COLS = "daysSinceEpoch, clicks, impressions"
QUERIES = [
    ("max_nofilter (yardstick)", "SELECT MAX(impressions) FROM adAnalytics", None),
    ("max_filter (yardstick)", "SELECT MAX(impressions) FROM adAnalytics" + FILTER, None),
    ("orderby_limit10", f"SELECT {COLS} FROM adAnalytics ORDER BY impressions DESC LIMIT 10", "max_nofilter (yardstick)"),
    ("orderby_filter_limit10", f"SELECT {COLS} FROM adAnalytics{FILTER} ORDER BY impressions DESC LIMIT 10",
     "max_filter (yardstick)"),
    ("orderby_filter_limit1000", f"SELECT {COLS} FROM adAnalytics{FILTER} ORDER BY impressions DESC LIMIT 1000",
     "max_filter (yardstick)"),
    ("noorder_filter_limit10", f"SELECT {COLS} FROM adAnalytics{FILTER} LIMIT 10", "max_filter (yardstick)"),
]

assert torch.cuda.is_available(), "this probe measures on the GPU"
segs = [E.ImmutableSegment(datagen.ad_segment(f"ad{i}", args.rows, seed=i)) for i in range(args.segments)]
ex = E.ServerQueryExecutor()
lines = [f"# selection_probe: {args.segments} segments x {args.rows} rows, {args.reps} repeats after warm-up, medians"
         f" (min..max); commit {args.commit or 'working tree'}",
         "# kernel ms: device events around the passes (scan, candidate sort, cut, gather); e2e ms: host clock around "
         "a re-issued execute (prepared plan) + rows() / groups(), ending in a device synchronise"]
kernel = {}
for name, sql, ref in QUERIES:
    def fetch(r):
        return r.rows() if hasattr(r, "origins") else r.groups()

    r = ex.execute(sql, segs)          # cold: plans and compiles
    fetch(r)
    for _ in range(3):                 # warm-up of every shape the timed window uses
        r.execute_again()
        fetch(r)
    kms, ems = [], []
    for _ in range(args.reps):
        r.execute_again()
        torch.cuda.synchronize()
        kms.append(r.last_kernel_ms())
    info, nbytes = r.kernel_info(), r.algorithmic_bytes()
    r.destroy()
    for _ in range(args.reps):         # re-issued: the prepared plan, end to end
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = ex.execute(sql, segs)
        fetch(r)
        torch.cuda.synchronize()
        ems.append((time.perf_counter() - t) * 1e3)
        r.destroy()
    k = statistics.median(kms)
    kernel[name] = k
    line = (f"{name:28s} {info:16s} kernel ms {k:8.3f} ({min(kms):.3f}..{max(kms):.3f})  e2e ms "
            f"{statistics.median(ems):8.3f} ({min(ems):.3f}..{max(ems):.3f})  algorithmic GB {nbytes / 1e9:7.3f}  "
            f"GB/s {nbytes / 1e6 / k:8.1f}")
    if ref:
        line += f"  kernel ratio vs {ref.split()[0]} {k / kernel[ref]:.3f}"
    print(line, flush=True)
    lines.append(line)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote", args.out, file=sys.stderr)
