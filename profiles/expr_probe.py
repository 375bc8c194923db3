"""Arithmetic expressions on bench-sized segments.

    python profiles/expr_probe.py [--segments 4] [--rows 10000000] [--steps 30] [--out FILE]

Each segment is a bench segment (datagen.ad_segment: 10M rows) plus two raw DOUBLE columns holding, per doc, the
values of the two probed expressions computed in numpy -- `clicks * cost * 1` (2 columns; the same values as
`clicks * cost`, which alone inside SUM is the scan's two-column form and builds no twin) and
`(impressions - clicks) / cost * 1.07` (3 columns, 7 nodes) -- the baseline a query over the expression must equal.
Prints one JSON line:

* the twin build per 10M-row segment: the evaluator's time (plan_timing's expr_kernel: launch to completion on the host's
  clock, so it includes the launch latency) and the whole `raw_keys` phase (allocation, zeroing, the kernel, the staging fingerprint) of the first
  query over segments 1.., after segment 0 took the hipRTC compile; the evaluator's achieved bytes/s (sources read +
  8 B written per row) beside the 6.29 TB/s a float4 copy reaches on this part (MI355X_MICROARCH);
* the re-issued time (execute_again, device events: last_kernel_ms) of the bench-shaped query
  GROUP BY daysSinceEpoch, SUM(expr) over the twin and -- the baseline, a shape the parent commit runs -- over the
  staged raw DOUBLE column, alternating, median and min..max over the steps, with each plan's kernel_info and
  algorithmic bytes.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUERY = ("SELECT daysSinceEpoch, COUNT(*), SUM(clicks), SUM({k}), MAX({k}) FROM t WHERE clicks > 100 "
         "GROUP BY daysSinceEpoch LIMIT 1000")
# (`clicks * cost` alone inside SUM / MAX is the scan's two-column form, no twin: the trailing `* 1` makes it an expression
# with the same values)
EXPRS = {"two_columns": ("clicks * cost * 1", "k2", 4 + 8), "three_columns_seven_nodes": ("(impressions - clicks) / cost * 1.07", "k3", 8 + 4 + 8)}
COPY_CEILING = 6.29e12


def raw_values(cb, n, dtype):
    hdr = len(cb.fwd) - n * np.dtype(dtype).itemsize
    return np.frombuffer(cb.fwd, dtype=dtype, count=n, offset=hdr)


def segment(name, n, seed):
    from pinot_amd import datagen, segment as S
    bufs = datagen.ad_segment(name, n, seed)
    clicks = raw_values(bufs.columns["clicks"], n, ">i4").astype(np.float64)
    imp = raw_values(bufs.columns["impressions"], n, ">i8").astype(np.float64)
    cost = raw_values(bufs.columns["cost"], n, ">f8").astype(np.float64)
    with np.errstate(all="ignore"):
        vals = {"k2": clicks * cost, "k3": ((imp - clicks) / cost) * 1.07}
    for c, v in vals.items():
        bufs.columns[c] = S.ColumnBuffers(c, S.DOUBLE, n, False, fwd=S.raw_fwd_header(n, S.DOUBLE) + v.astype(">f8").tobytes())
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
    segs = [E.ImmutableSegment(segment(f"xp{i}", args.rows, 100 + i)) for i in range(args.segments)]
    ex = E.ServerQueryExecutor()
    out = {"segments": args.segments, "rows_per_segment": args.rows, "steps": args.steps, "copy_ceiling_bytes_per_s": COPY_CEILING}
    res = {}
    for name, (expr, staged, src_bytes) in EXPRS.items():
        warm = ex.execute(f"SELECT SUM({expr}) FROM t", segs[:1])            # segment 0: the hipRTC compile
        t0 = warm.plan_timing()
        before = sum(s.device_bytes() for s in segs)
        first = ex.execute(QUERY.format(k=expr), segs)                       # segments 1..: built here
        t = first.plan_timing()
        built = args.segments - 1
        bytes_moved = (src_bytes + 8) * args.rows * built
        o = {"expression": expr, "first_segment_raw_keys_ms_with_compile": t0.get("raw_keys"),
             "raw_keys_ms_per_segment": t["raw_keys"] / built, "expr_kernel_ms_per_segment": t["expr_kernel"] / built,
             "evaluator_bytes_per_row": src_bytes + 8,
             "evaluator_bytes_per_s": bytes_moved / (t["expr_kernel"] * 1e-3),
             "twin_bytes_per_segment": (sum(s.device_bytes() for s in segs) - before) / built}
        o["evaluator_vs_copy_ceiling"] = o["evaluator_bytes_per_s"] / COPY_CEILING
        plain = ex.execute(QUERY.format(k=staged), segs)
        for tag, r in (("twin", first), ("staged", plain)):
            o[tag] = {"kernel_info": r.kernel_info(), "algorithmic_bytes": r.algorithmic_bytes()}
        ga, gb = first.groups(), plain.groups()
        o["results_equal"] = set(ga) == set(gb) and all(
            x[0] == y[0] and x[1] == y[1] and x[3] == y[3] and abs(x[2] - y[2]) <= 1e-12 * abs(y[2])
            for x, y in ((ga[k], gb[k]) for k in gb))
        o["groups"] = len(gb)
        res[name] = (first, plain)
        out[name] = o
        warm.destroy()
    for pair in res.values():   # warm up every plan
        for r in pair:
            for _ in range(3):
                r.execute_again()
    for name, (first, plain) in res.items():
        ms = {"twin": [], "staged": []}
        for _ in range(args.steps):  # alternating, so drift hits both alike
            for tag, r in (("twin", first), ("staged", plain)):
                r.execute_again()
                ms[tag].append(r.last_kernel_ms())
        for tag, v in ms.items():
            out[name][tag]["reissued_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        out[name]["reissued_twin_vs_staged"] = out[name]["twin"]["reissued_ms"]["median"] / out[name]["staged"]["reissued_ms"]["median"]
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
