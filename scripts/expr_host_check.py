"""Host-side check of the expression code under AddressSanitizer + UBSan, without a GPU and without Python loading it:

    python scripts/expr_host_check.py [--cxx g++] [--workdir DIR]

1. builds scripts/expr_host_check.cpp (pinot_amd/csrc/expr.h: validation, canonicalisation, source generation) with
   -fsanitize=address,undefined as a stand-alone program;
2. feeds it well-formed and malformed postfix trees: the verdicts must be the expected ones, equal trees must get one
   name, and no sanitizer report may appear;
3. lets it print the generated value functions as a host C++ program, builds that under the same sanitizers and
   compares its results, bit for bit (every NaN one value), with tests/expr_ref.py over the cross product of the edge
   doubles (+-0, NaN, +-inf, denormals, the ends of the range, LONGs past 2^53 as doubles).
"""
import argparse
import itertools
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import expr_ref as R  # noqa: E402
from pinot_amd.query import expr_postfix, parse_expression  # noqa: E402

SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off"]
EDGE = [0.0, -0.0, float("nan"), float("inf"), float("-inf"), 5e-324, -5e-324, 2.2250738585072014e-308, 1.0, -1.0, 0.5,
        -0.5, 3.0, -3.0, 1e308, -1e308, 1.5, 2.5, 134217729.0, 0.1, 7.0, 1e-300, 4.0, float(2 ** 53 + 2), -float(2 ** 63),
        -18014398777917440.0]
EXPRS = ["p + q", "p - q", "p * q", "p / q", "p % q", "add(p, q, 2.5, -1e308)", "mult(p, 3, q, 1e-300)", "abs(p) - q",
         "ceil(p) + floor(q)", "sqrt(p) * sign(q)", "least(p, q)", "greatest(p, q)", "least(p, q, -0.0)",
         "greatest(p, 0, q)", "p * q + r", "(p - q) / p * 1.07", "floor(p / 100) % 7",
         "greatest(abs(p - q) / r, floor(sqrt(p * q + r)) % 7, least(p, q, r)) + sign(r)"]


def hexbits(x: float) -> str:
    return "7ff8000000000000" if x != x else struct.pack(">d", x).hex()


def spec(rows) -> str:
    out = []
    for kind, nargs, col, lit in rows:
        out.append(f"c:{col}" if kind == 0 else f"l:{struct.pack('>d', lit).hex()}" if kind == 1 else f"{kind}:{nargs}")
    return " ".join(out)


def run(cmd, **kw):
    return subprocess.run(cmd, check=True, text=True, capture_output=True, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default="g++")
    ap.add_argument("--workdir", default=None)
    args = ap.parse_args()
    work = args.workdir or tempfile.mkdtemp(prefix="expr_host_check_")
    os.makedirs(work, exist_ok=True)
    chk = os.path.join(work, "expr_host_check")
    run([args.cxx, *SAN, os.path.join(ROOT, "scripts", "expr_host_check.cpp"), "-o", chk])
    # -- verdicts and names
    good = [spec(expr_postfix(parse_expression(e))) for e in EXPRS]
    same = [("a * 2", "a * 2.0"), ("mult(2, a)", "a * 2"), ("add(a,1,2)", "add(3,a)"), ("a + -0.0", "a + 0.0")]
    differ = [("a * 2", "a * 3"), ("a - 2", "2 - a"), ("a - -0.0", "a - 0.0"), ("least(a,b)", "least(b,a)")]
    bad = {"c:a c:b": 1, "c:a 2:2": 1, "c:a c:b 2:1": 1, "c:a c:b c:c 3:3": 1, "c:a c:b 7:2": 1, "l:4000000000000000 10:1": 1,
           "l:3ff0000000000000 l:4000000000000000 2:2": 1, "c:a 14:1": 2, "c:a -1:1": 2, "c:a 99:1": 2,
           " ".join(f"c:c{i}" for i in range(9)) + " 2:9": 1, "c:a " + " ".join(["c:a 2:2"] * 16): 1, "c:a 12:1": 1}
    pairs = [spec(expr_postfix(parse_expression(e))) for pr in same + differ for e in pr]
    lines = good + list(bad) + pairs
    out = run([chk, "names"], input="\n".join(lines) + "\n").stdout.splitlines()
    assert len(out) == len(lines), (len(out), len(lines))
    for ln in out[:len(good)]:
        assert ln.startswith("ok $x("), ln
    for (sp, want), ln in zip(bad.items(), out[len(good):len(good) + len(bad)]):
        assert ln.startswith(f"refused {want} "), (sp, want, ln)
    names = out[len(good) + len(bad):]
    for k, pr in enumerate(same + differ):
        a, b = names[2 * k], names[2 * k + 1]
        assert (a == b) == (k < len(same)), (pr, a, b)
    # -- the generated value functions as host C++
    src = os.path.join(work, "expr_values.cpp")
    with open(src, "w") as f:
        f.write(run([chk, "host"], input="\n".join(good) + "\n").stdout)
    val = os.path.join(work, "expr_values")
    run([args.cxx, *SAN, src, "-o", val])
    total = 0
    for i, e in enumerate(EXPRS):
        tree = parse_expression(e)
        cols = [r[2] for r in expr_postfix(tree) if r[0] == 0]
        cols = list(dict.fromkeys(cols))       # first-use order: the value function's parameters
        grid = list(itertools.product(EDGE, repeat=len(cols)))
        if len(grid) > 6000:
            grid = grid[::3]
        arrs = {c: np.array([g[j] for g in grid]) for j, c in enumerate(cols)}
        want = R.canonical_bits(R.evaluate(tree, arrs, len(grid)))
        inp = "\n".join(f"{i} " + " ".join(hexbits(v) for v in g) for g in grid) + "\n"
        got = run([val], input=inp).stdout.split()
        assert len(got) == len(grid), (e, len(got))
        for g, w, row in zip(got, want, grid):
            assert int(g, 16) == int(w), (e, row, g, hex(int(w)))
        total += len(grid)
    print(f"expr_host_check ok: {len(lines)} trees through the validator, {len(EXPRS)} generated value functions x "
          f"{total} argument tuples bit-identical to the restatement, no sanitizer report ({work})")


if __name__ == "__main__":
    main()
