# Multi-value columns on one segment of --rows docs x ~3 values at 6 bits (card 64), beside a 6-bit single-value column:
#   mv_filter   COUNT(*) WHERE tags = v   mv_match_kernel (dictId stream + start bits -> docId bitset) and the scan
#               that reads the bitset; its algorithmic bytes are total_values * (bits + 1) / 8 + the bitset twice
#   sv_filter   COUNT(*) WHERE sv = v     the fused scan over the 6-bit forward index: the same question on an SV column
#   twins       the first SELECT COUNTMV, SUMMV, MINMV, MAXMV: the one-time cost of the four per-doc twins
#               (plan_timing's raw_keys: mv_reduce_kernel, the copy to the host and the raw-column staging)
#   copy        a device-to-device copy of 1 GiB (torch): the rate the filters' bytes are set against
# Kernel ms are device events around a warm re-issue (execute_again of the prepared plan); medians over --reps.
# mv_filter's time covers the match kernel, the bitset's memset and the scan, so bytes / time is a lower bound of
# the match kernel's own rate.
#   PYTHONPATH=. python profiles/mv_probe.py [--rows 10000000] [--reps 15] --out profiles/r12/mv.json
import argparse
import json
import statistics
import time

import numpy as np
import torch

from pinot_amd import engine as E
from pinot_amd import segment as S

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--out", required=True)
ap.add_argument("--commit", default="")
args = ap.parse_args()

assert torch.cuda.is_available(), "this probe measures on the GPU"
rng = np.random.default_rng(12)
n = args.rows
lens = rng.integers(1, 6, n)                       # 1..5 values, 3 on average
total = int(lens.sum())
ids = rng.integers(0, 64, total).astype(np.int32)  # dictIds of a 64-value dictionary: 6 bits
ids[:64] = np.arange(64)                           # (every value present)
dvals = np.arange(64, dtype=np.int32) * 3
tags = S.ColumnBuffers("tags", S.INT, n, True, False, 64, 6, S.mv_fwd_bytes_flat(ids, lens, 6),
                       S.dictionary_bytes(dvals, S.INT), None, dvals, True, total, int(lens.max()))
sv = S.build_column("sv", dvals[rng.integers(0, 64, n)], S.INT, detect_sorted=False)
seg = E.ImmutableSegment(S.SegmentBuffers("mvprobe", n, {"tags": tags, "sv": sv}))
ex = E.ServerQueryExecutor()
out = {"commit": args.commit, "rows": n, "total_values": total, "bits": 6, "reps": args.reps, "queries": {}}


def timed(name, sql):
    r = ex.execute(sql, [seg])   # cold: plans and compiles
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
    q = {"sql": sql, "kernel_info": r.kernel_info(), "kernel_ms_median": med, "kernel_ms_min": min(kms),
         "kernel_ms_max": max(kms), "algorithmic_gb": r.algorithmic_bytes() / 1e9,
         "gb_per_s": r.algorithmic_bytes() / 1e9 / (med / 1e3), "rows": repr(rows[:1])}
    out["queries"][name] = q
    print(name, q["kernel_info"], f"{med:.3f} ms", f"{q['gb_per_s']:.0f} GB/s", flush=True)
    r.destroy()


timed("mv_filter", "SELECT COUNT(*) FROM t WHERE tags = 21")
timed("sv_filter", "SELECT COUNT(*) FROM t WHERE sv = 21")

b0 = seg.device_bytes()
t0 = time.perf_counter()
r = ex.execute("SELECT COUNTMV(tags), SUMMV(tags), MINMV(tags), MAXMV(tags) FROM t", [seg])
rows = r.rows()
out["twins"] = {"first_query_ms": (time.perf_counter() - t0) * 1e3, "raw_keys_ms": r.plan_timing()["raw_keys"],
                "twin_bytes": seg.device_bytes() - b0, "rows": repr(rows)}
r.destroy()
print("twins", out["twins"], flush=True)
timed("mv_aggs", "SELECT COUNTMV(tags), SUMMV(tags), MINMV(tags), MAXMV(tags) FROM t")

src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
dst = torch.empty_like(src)
for _ in range(3):
    dst.copy_(src)
ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
cms = []
for _ in range(args.reps):
    ev0.record()
    dst.copy_(src)
    ev1.record()
    torch.cuda.synchronize()
    cms.append(ev0.elapsed_time(ev1))
copy_gbs = 2 * (1 << 30) / 1e9 / (statistics.median(cms) / 1e3)  # read + written
out["copy"] = {"bytes": 1 << 30, "ms_median": statistics.median(cms), "gb_per_s_read_plus_write": copy_gbs}
out["mv_filter_share_of_copy_rate"] = out["queries"]["mv_filter"]["gb_per_s"] / copy_gbs
print("copy", f"{copy_gbs:.0f} GB/s", "mv_filter share", f"{out['mv_filter_share_of_copy_rate']:.3f}", flush=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
