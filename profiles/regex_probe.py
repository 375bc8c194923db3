# LIKE / REGEXP_LIKE over STRING dictionaries: the two runners of one DFA table, per dictionary size.
#   resolve     pinot_amd_segment_regexp_match_dictionary on one segment whose dictionary holds --cards URL-like values
#               of about 40 bytes: PINOT_AMD_REGEX_DEVICE=never (the host runner, one thread, as planning runs) against
#               =always (the DFA upload, dict_regex_match_kernel, the mask copy and the synchronisation: wall time of the
#               call, so bytes / time is a LOWER bound of the kernel's own rate). The first device call also builds the
#               dictionary's device copy (stage_ms, once per segment and column). Medians over --reps.
#   query       at --query-card values and --query-docs docs: the first execution of COUNT(*) WHERE url LIKE
#               '%checkout%' (it resolves the leaf), the re-issued query (the prepared plan) and the same scan with an IN
#               of the matching values: the last two run the same generated kernel over the same dictId set.
#   copy        a device-to-device copy of 1 GiB (torch): the HBM rate the kernel's dictionary bytes / s stand beside.
# The auto cutoff of PINOT_AMD_REGEX_DEVICE is the smallest measured size at which the device call is faster for every
# pattern, rounded up to a power of two.
#   PYTHONPATH=. python profiles/regex_probe.py --out profiles/r14/regex_probe.json
import argparse
import ctypes as C
import dataclasses
import json
import os
import statistics
import time

import numpy as np
import torch

from pinot_amd import engine as E
from pinot_amd import segment as S
from pinot_amd._lib import check, lib
from pinot_amd.query import FilterContext, Predicate, like_to_regexp, parse_sql

ap = argparse.ArgumentParser()
ap.add_argument("--cards", default="1000,10000,100000,1000000,10000000")
ap.add_argument("--query-card", type=int, default=1_000_000)
ap.add_argument("--query-docs", type=int, default=100_000_000)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", required=True)
ap.add_argument("--commit", default="")
args = ap.parse_args()
assert torch.cuda.is_available(), "this probe measures on the GPU"

WORDS = np.array(["cart", "pay", "home", "search", "item", "checkout", "login", "help", "order", "track", "offer", "blog",
                  "about", "terms", "news", "faq"])
PATTERNS = [("like_contains", like_to_regexp("%checkout%"), True), ("like_prefix", like_to_regexp("https://a%"), True),
            ("alternation_class", "/(cart|pay)[0-9]+$", False)]


def url_values(card):
    """card sorted distinct values "https://<host>.example.com/<10 digits>/<word><2 digits>": the host letter grows
    with the index (an eighth of the values under each of a..h), the word is a hash of it."""
    i = np.arange(card, dtype=np.int64)
    host = np.array(list("abcdefgh"))[np.minimum(i * 8 // max(card, 1), 7)]
    h = (i * 2654435761) % (1 << 32)
    word = WORDS[(h >> 8) % len(WORDS)]
    tail = np.char.zfill(((h >> 16) % 100).astype(str), 2)
    num = np.char.zfill(i.astype(str), 10)
    v = np.char.add(np.char.add(np.char.add("https://", host), ".example.com/"), num)
    return np.char.add(np.char.add(np.char.add(v, "/"), word), tail)


def string_column(name, values, dict_ids, num_docs):
    card = len(values)
    bits = max(1, int(card - 1).bit_length())
    enc = np.char.encode(values, "ascii")
    return S.ColumnBuffers(name, S.STRING, num_docs, True, False, card, bits, S.pack_fixed_bit(dict_ids, bits),
                           enc.astype(f"S{enc.dtype.itemsize}").tobytes(), None, None)


def resolve(seg, pattern, ci):
    n = C.c_int64()
    t0 = time.perf_counter()
    check(lib().pinot_amd_segment_regexp_match_dictionary(seg.handle, b"url", pattern.encode(), 1 if ci else 0, None, 0,
                                                          C.byref(n)), "regexp_match_dictionary")
    return (time.perf_counter() - t0) * 1e3, n.value


out = {"commit": args.commit, "reps": args.reps, "value_bytes_mean": None, "resolve": [], "query": None}
for card in [int(c) for c in args.cards.split(",")]:
    vals = url_values(card)
    nbytes = int(np.char.str_len(vals).sum())
    seg = E.ImmutableSegment(S.SegmentBuffers(f"rxp{card}", card, {
        "url": string_column("url", vals, np.arange(card, dtype=np.int64), card)}))
    row = {"card": card, "dictionary_bytes": nbytes, "patterns": {}}
    os.environ["PINOT_AMD_REGEX_DEVICE"] = "always"
    b0 = seg.device_bytes()
    row["stage_ms"], _ = resolve(seg, "x", False)  # builds the device copy
    row["device_copy_bytes"] = seg.device_bytes() - b0
    for name, pat, ci in PATTERNS:
        res = {}
        for runner in ("never", "always"):
            os.environ["PINOT_AMD_REGEX_DEVICE"] = runner
            resolve(seg, pat, ci)
            ms = []
            for _ in range(args.reps if card < 10_000_000 or runner == "always" else 3):
                t, n = resolve(seg, pat, ci)
                ms.append(t)
            res[runner] = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "matching": n}
        assert res["never"]["matching"] == res["always"]["matching"]
        res["device_gb_per_s_lower_bound"] = nbytes / 1e9 / (res["always"]["ms_median"] / 1e3)
        res["host_gb_per_s"] = nbytes / 1e9 / (res["never"]["ms_median"] / 1e3)
        row["patterns"][name] = res
        print(card, name, f"host {res['never']['ms_median']:.3f} ms", f"device {res['always']['ms_median']:.3f} ms",
              f"{res['device_gb_per_s_lower_bound']:.1f} GB/s", "matching", n, flush=True)
    out["resolve"].append(row)
    seg.destroy()
    del vals
faster = [r["card"] for r in out["resolve"]
          if all(p["always"]["ms_median"] < p["never"]["ms_median"] for p in r["patterns"].values())]
out["break_even"] = {"smallest_card_device_faster_for_every_pattern": min(faster) if faster else None,
                     "rounded_up_to_power_of_two": (1 << (min(faster) - 1).bit_length()) if faster else None}
print("break-even", out["break_even"], flush=True)

# ---- the query: first execution, re-issue, and the same scan with an IN of the same dictIds
card, docs = args.query_card, args.query_docs
vals = url_values(card)
rng = np.random.default_rng(14)
ids = rng.integers(0, card, docs).astype(np.int64)
seg = E.ImmutableSegment(S.SegmentBuffers("rxq", docs, {"url": string_column("url", vals, ids, docs)}))
del ids
os.environ["PINOT_AMD_REGEX_DEVICE"] = "always"
ex = E.ServerQueryExecutor()
like_sql = "SELECT COUNT(*) FROM t WHERE url LIKE '%checkout%'"
in_values = tuple(str(v) for v in vals[np.char.find(vals, "checkout") >= 0])
in_qc = dataclasses.replace(parse_sql("SELECT COUNT(*) FROM t WHERE url IN ('x')"),
                            filter=FilterContext.pred(Predicate("IN", "url", in_values)))


def issue(q):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = ex.execute(q, [seg])
    m = r.num_docs_matched()
    wall = (time.perf_counter() - t0) * 1e3
    info = {"wall_ms": wall, "kernel_ms": r.last_kernel_ms(), "matched": m, "plan_cache": "plan_cache" in r.plan_timing(),
            "kernel_info": r.kernel_info()}
    r.destroy()
    return info


first = issue(like_sql)
again = [issue(like_sql) for _ in range(args.reps)]
in_first = issue(in_qc)
in_again = [issue(in_qc) for _ in range(args.reps)]
assert first["matched"] == in_first["matched"] and all(a["plan_cache"] for a in again)


def med(rows, k):
    return statistics.median(r[k] for r in rows)


out["query"] = {"card": card, "docs": docs, "in_values": len(in_values), "first": first,
                "reissue": {"wall_ms_median": med(again, "wall_ms"), "kernel_ms_median": med(again, "kernel_ms"),
                            "kernel_ms_min": min(a["kernel_ms"] for a in again),
                            "kernel_ms_max": max(a["kernel_ms"] for a in again)},
                "in_first": in_first,
                "in_reissue": {"wall_ms_median": med(in_again, "wall_ms"), "kernel_ms_median": med(in_again, "kernel_ms"),
                               "kernel_ms_min": min(a["kernel_ms"] for a in in_again),
                               "kernel_ms_max": max(a["kernel_ms"] for a in in_again)}}
print("query", json.dumps(out["query"]), flush=True)
seg.destroy()

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
out["copy"] = {"bytes": 1 << 30, "ms_median": statistics.median(cms),
               "gb_per_s_read_plus_write": 2 * (1 << 30) / 1e9 / (statistics.median(cms) / 1e3)}
print("copy", out["copy"], flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
