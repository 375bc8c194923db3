"""DISTINCTCOUNTHLL without a GPU: the per-doc reference (tests/hll_ref.py) and pinot_amd.query's restatement against
the eight values Pinot's testDistinctCountHLL asserts; the estimator's edges; hash vectors; the parser; the mirror
fold; the C ABI's argument checks; and pinot_amd/csrc/hll.h through a stand-alone driver (tests/hll_main.cpp) built
with the host compiler under -fsanitize=address,undefined and run as a program of its own."""
import ctypes as C
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import hll_ref as H
from helpers import GOLDEN
from pinot_amd import _lib
from pinot_amd import query as Q
from pinot_amd.query import parse_sql

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EINVAL, EUNSUPPORTED = -1, -2
LONG_MAX = (1 << 63) - 1


@pytest.fixture(scope="module")
def sv():
    return np.load(os.path.join(GOLDEN, "test_data_sv.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def pins():
    with open(os.path.join(GOLDEN, "sv_hll_expected.json")) as f:
        return json.load(f)


def sv_filter_mask(d):
    """helpers.SV_FILTER (InterSegment...QueriesTest.FILTER) over the columns."""
    c11 = d["column11"]
    return ((d["column1"] > 100000000) & (d["column3"] >= 20000000) & (d["column3"] <= 1000000000)
            & (d["column5"] == "gFuH") & ((d["column6"] < 500000000) | ~np.isin(c11, ["t", "P"]))
            & (d["daysSinceEpoch"] == 126164076))


def top_row(g1, g3, card):
    """GROUP BY column9 ORDER BY v1 DESC, v2 DESC LIMIT 1"""
    return max((card(g1[k]), card(g3[k])) for k in g1)


# --------------------------------------------------------------------------------------------------- the pins
def test_pins_reference_and_query(sv, pins):
    assert len(pins["cases"]) == 4
    for case in pins["cases"]:
        mask = sv_filter_mask(sv) if case["filter"] else np.ones(len(sv["column1"]), dtype=bool)
        keys = [sv["column9"]] if case["group_by"] else None
        g1 = H.grouped(sv["column1"], "INT", 8, keys, mask)
        g3 = H.grouped(sv["column3"], "INT", 8, keys, mask)
        if case["group_by"]:
            got = top_row(g1, g3, H.cardinality)
            got_q = top_row(g1, g3, Q.hll_cardinality)
        else:
            got = (H.cardinality(g1[()]), H.cardinality(g3[()]))
            # query.py's own path to the registers: the distinct values, hashed once each
            r1 = Q.hll_registers(set(sv["column1"][mask].tolist()), "INT", 8)
            r3 = Q.hll_registers(set(sv["column3"][mask].tolist()), "INT", 8)
            assert r1 == g1[()] and r3 == g3[()], case
            # "inter": four copies of the segment merge to the same registers
            assert Q.hll_merge(Q.hll_merge((8, r1), (8, r1)), Q.hll_merge((8, r1), (8, r1))) == (8, r1)
            got_q = (Q.hll_cardinality(r1), Q.hll_cardinality(r3))
        assert list(got) == case["expected"], case
        assert list(got_q) == case["expected"], case


# ------------------------------------------------------------------------------------------------ the estimator
def _registers_with(log2m, zeros, value=1):
    m = 1 << log2m
    return bytes([0] * zeros + [value] * (m - zeros))


@pytest.mark.parametrize("card", [H.cardinality, Q.hll_cardinality])
def test_estimator_edges(card):
    for log2m in (4, 5, 6, 8, 12, 16):
        assert card(bytes(1 << log2m)) == 0
    # every register 1 at log2m 8: estimate = alphaMM / (m / 2) ~ 1.437 m <= 2.5 m, zeros == 0 -> Math.round(+inf)
    assert card(bytes([1] * 256)) == LONG_MAX
    # the alphaMM cases: all registers 3 -> sum = m / 8, estimate = alpha * m * 8 > 2.5 m
    assert card(bytes([3] * 16)) == round(0.673 * 16 * 8)
    assert card(bytes([3] * 32)) == round(0.697 * 32 * 8)
    assert card(bytes([3] * 64)) == round(0.709 * 64 * 8)
    assert card(bytes([3] * 128)) == int(np.floor((0.7213 / (1 + 1.079 / 128)) * 128 * 128 * (1 / 16.0) + 0.5))
    # either side of the 2.5 m switch at log2m 8, registers in {0, 2}: z zeros give sum = z + (256 - z) / 4
    m = 256
    alpha_mm = (0.7213 / (1 + 1.079 / m)) * m * m
    below = next(z for z in range(m, 0, -1) if alpha_mm / (z + (m - z) / 4.0) > 2.5 * m)  # the first z past the switch
    above = below + 1
    assert alpha_mm * (1 / (above + (m - above) / 4.0)) <= 2.5 * m < alpha_mm * (1 / (below + (m - below) / 4.0))
    assert card(_registers_with(8, above, 2)) == int(np.floor(m * np.log(m / float(above)) + 0.5))
    assert card(_registers_with(8, below, 2)) == int(np.floor(alpha_mm * (1 / (below + (m - below) / 4.0)) + 0.5))


# ------------------------------------------------------------------------------------------------ hash vectors
def test_hash_vectors():
    for log2m in (4, 8, 12, 16):
        regs = Q.hll_registers([0], "INT", log2m)
        assert regs[0] == 33 - log2m and regs.count(0) == (1 << log2m) - 1   # 0 hashes to 0: the maximum rank
        assert regs == H.registers(np.array([0], dtype=np.int32), "INT", log2m)
    assert Q.hll_hash(0, "INT") == 0 and Q.hll_hash(0, "LONG") == 0
    assert Q.hll_hash(2735739, "INT") == 0x23000000 == int(H.hashes([2735739], "INT")[0])
    assert Q.hll_hash(-7, "INT") == Q.hll_hash(-7, "LONG") == int(H.hashes([-7], "LONG")[0])   # (long) v sign-extends
    assert Q.hll_hash(-0.0, "DOUBLE") != Q.hll_hash(0.0, "DOUBLE")
    assert Q.hll_hash(-0.0, "FLOAT") != Q.hll_hash(0.0, "FLOAT")
    assert Q.hll_hash(1.5, "FLOAT") != Q.hll_hash(1.5, "DOUBLE")
    for t in ("FLOAT", "DOUBLE"):
        for v in (1.5, -0.0, 0.0, float("inf"), 3.0e38):
            assert Q.hll_hash(v, t) == int(H.hashes([v], t)[0]), (t, v)
    strings = ["", "a", "ab", "abc", "abcd", "abcde", "abcdef", "abcdefg", "abcdefgh", "abcdefghi", "é", "aé", "éa",
               "abÿ", "€", "abc\U0001F600"]
    for s in strings:
        assert Q.hll_hash(s, "STRING") == H.hash_bytes(s.encode("utf-8")), s
    assert Q.hll_hash("ab\0cd", "STRING") == Q.hll_hash("ab", "STRING")      # the value ends at its first NUL
    assert H.hashes(["ab\0cd"], "STRING")[0] == H.hashes(["ab"], "STRING")[0]
    # the tail is sign-extended: "é" = c3 a9 hashes unlike the masked variant
    h = (0xFFFFFFFF ^ 2)
    h ^= ((0xC3 - 256) << 8) & 0xFFFFFFFF
    h ^= (0xA9 - 256) & 0xFFFFFFFF
    h = (h * 0x5BD1E995) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0x5BD1E995) & 0xFFFFFFFF
    h ^= h >> 15
    assert Q.hll_hash("é", "STRING") == h


def test_merge_and_registers_agree():
    rng = np.random.default_rng(3)
    a = rng.integers(-(1 << 62), 1 << 62, 3000)
    b = rng.integers(-5, 5, 100)
    for log2m in (4, 8, 12, 16):
        ra, rb = H.registers(a, "LONG", log2m), H.registers(b, "LONG", log2m)
        assert Q.hll_registers(a.tolist(), "LONG", log2m) == ra
        merged = Q.hll_merge((log2m, ra), (log2m, rb))
        assert merged == (log2m, H.registers(np.concatenate([a, b]), "LONG", log2m))
        assert Q.hll_cardinality(merged[1]) == H.cardinality(merged[1])
    with pytest.raises(ValueError):
        Q.hll_merge((4, bytes(16)), (5, bytes(32)))
    assert Q.merge_partial("DISTINCTCOUNTHLL", (4, bytes([1] * 16)), (4, bytes([0, 2] * 8))) == (4, bytes([1, 2] * 8))
    assert Q.final_value("DISTINCTCOUNTHLL", (8, bytes(256))) == 0


# --------------------------------------------------------------------------------------------------- the parser
def test_parser_spellings():
    for text, log2m in [("DISTINCTCOUNTHLL(c)", 8), ("distinctcounthll(c)", 8), ("distinct_count_hll(c)", 8),
                        ("DistinctCountHLL(c, 12)", 12), ("DISTINCTCOUNTHLL(c, 4)", 4), ("DISTINCTCOUNTHLL(c, 16)", 16),
                        ("DISTINCTCOUNTHLL(c, '10')", 10)]:
        qc = parse_sql(f"SELECT {text} FROM t")
        a = qc.aggregations[0]
        assert (a.func, a.column, a.param) == ("DISTINCTCOUNTHLL", "c", log2m), text
        assert a.name == "distinctcounthll(c)"
    qc = parse_sql("SELECT g, DISTINCTCOUNTHLL(c) AS v FROM t GROUP BY g ORDER BY v DESC, distinctcounthll(c) LIMIT 3")
    assert qc.order_by_targets()[0][:2] == (1, 0)
    for bad in ["DISTINCTCOUNTHLL(c, 3)", "DISTINCTCOUNTHLL(c, 17)", "DISTINCTCOUNTHLL(c, 8.5)", "DISTINCTCOUNTHLL(c, 'x')",
                "DISTINCTCOUNTHLL(*)", "DISTINCTCOUNTHLL(a + b)", "DISTINCTCOUNTHLL(a * b)",
                "DISTINCTCOUNTHLL(dateTrunc('DAY', c))", "DISTINCTCOUNTRAWHLL(c)", "DISTINCTCOUNTHLLPLUS(c)",
                "DISTINCTCOUNTSMARTHLL(c)", "DISTINCTCOUNTHLLMV(c)", "distinct_count_hll_mv(c)"]:
        with pytest.raises(ValueError):
            parse_sql(f"SELECT {bad} FROM t")


# ------------------------------------------------------------------------------------------------ the mirror fold
def test_mirror_fold():
    qc = parse_sql("SELECT g, DISTINCTCOUNTHLL(c), DISTINCTCOUNTHLL(c, 4), DISTINCTCOUNT(c), SUM(x) FROM t GROUP BY g")
    base, subs = Q.split_distinct_count(qc)
    assert [a.func for a in base.aggregations] == ["SUM"] and len(subs) == 1       # one (g, c) query serves all three
    assert subs[0][1].group_by == ["g", "c"]
    base_groups = {(1,): [10.0], (2,): [5.0], (3,): [0.0]}
    sub_groups = {(1, 7): [3], (1, 0): [1], (1, -9): [1], (2, 2735739): [4]}
    out = Q.fold_distinct_count(qc, base_groups, [(subs[0][0], sub_groups)], {"c": "INT"})
    assert out[(1,)][0] == (8, H.registers(np.array([7, 0, -9]), "INT", 8))
    assert out[(1,)][1] == (4, H.registers(np.array([7, 0, -9]), "INT", 4))
    assert out[(1,)][2] == frozenset({7, 0, -9}) and out[(1,)][3] == 10.0
    assert out[(2,)][0][1][0x23] == 25 and Q.final_value("DISTINCTCOUNTHLL", out[(2,)][0]) == 1
    assert out[(3,)][0] == (8, bytes(256))                                          # a base group without a value row
    rows = Q.reduce_rows(qc, out)
    assert sorted(rows)[0][:4] == (1, 3, 3, 3)
    # FLOAT columns hash the float's bits, DOUBLE the double's
    qf = parse_sql("SELECT DISTINCTCOUNTHLL(f) FROM t")
    b, s = Q.split_distinct_count(qf)
    vals = [1.5, -0.0, 0.0, float("nan")]
    sg = {(Q.JavaDouble(v),): [1] for v in vals}   # (the engine's float keys: -0.0 and 0.0 are two)
    of = Q.fold_distinct_count(qf, {(): [4]}, [(s[0][0], sg)], {"f": "FLOAT"})
    od = Q.fold_distinct_count(qf, {(): [4]}, [(s[0][0], sg)], {"f": "DOUBLE"})
    assert of[()][0] == (8, H.registers(np.array(vals, dtype=np.float32), "FLOAT", 8))
    assert od[()][0] == (8, H.registers(np.array(vals, dtype=np.float64), "DOUBLE", 8))
    assert of != od
    with pytest.raises(ValueError):
        Q.split_distinct_count(parse_sql("SELECT DISTINCTCOUNTHLL(c) FILTER (WHERE x > 1) FROM t"))


# ------------------------------------------------------------------------------------------------------ the ABI
def test_abi_symbols_and_refusals():
    assert "pinot_amd_query_add_aggregation_hll" in _lib.SIGNATURES
    assert "pinot_amd_result_fetch_hll" in _lib.SIGNATURES
    from pinot_amd.engine import AGG_CODE
    assert AGG_CODE["DISTINCTCOUNTHLL"] == 17
    L = _lib.lib()
    qh = C.c_void_p()
    assert L.pinot_amd_query_create(C.byref(qh)) == 0
    try:
        idx = C.c_int32(-1)
        assert L.pinot_amd_query_add_aggregation_hll(qh, b"c", 8, C.byref(idx)) == 0 and idx.value == 0
        for log2m in (4, 16):
            assert L.pinot_amd_query_add_aggregation_hll(qh, b"c", log2m, C.byref(idx)) == 0
        assert idx.value == 2
        assert L.pinot_amd_query_add_aggregation_hll(qh, b"c", 12, None) == 0
        for log2m in (-1, 0, 3, 17, 32, 1 << 20):
            assert L.pinot_amd_query_add_aggregation_hll(qh, b"c", log2m, C.byref(idx)) == EINVAL, log2m
        assert L.pinot_amd_query_add_aggregation_hll(qh, b"*", 8, C.byref(idx)) == EINVAL
        assert L.pinot_amd_query_add_aggregation_hll(qh, b"", 8, C.byref(idx)) == EINVAL
        assert L.pinot_amd_query_add_aggregation_hll(qh, None, 8, C.byref(idx)) == EINVAL
        assert L.pinot_amd_query_add_aggregation_hll(None, b"c", 8, C.byref(idx)) == EINVAL
        # the other entry points keep refusing the type
        assert L.pinot_amd_query_add_aggregation(qh, 17, b"c", C.byref(idx)) == EINVAL
        assert L.pinot_amd_query_add_aggregation_param(qh, 17, b"c", 8.0, C.byref(idx)) == EINVAL
        assert L.pinot_amd_query_add_aggregation_mv(qh, 17, b"c", C.byref(idx)) == EINVAL
    finally:
        L.pinot_amd_query_destroy(qh)
    log2m, ng = C.c_int32(), C.c_int64()
    assert L.pinot_amd_result_fetch_hll(None, 0, 0, None, C.byref(log2m), C.byref(ng)) == EINVAL


# ------------------------------------------------------------------------------- hll.h under the sanitizers
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("hll") / "hll_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "hll_main.cpp"), "-o", exe], check=True)

    def run(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-4000:]
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
        out = p.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


KIND = {"INT": 0, "LONG": 1, "FLOAT": 2, "DOUBLE": 3}


def _bits(v, t):
    if t == "INT":
        return struct.unpack("<I", struct.pack("<i", int(v)))[0]
    if t == "LONG":
        return struct.unpack("<Q", struct.pack("<q", int(v)))[0]
    if t == "FLOAT":
        return struct.unpack("<I", np.float32(v).tobytes())[0]
    return struct.unpack("<Q", np.float64(v).tobytes())[0]


def test_header_against_reference(driver):
    rng = np.random.default_rng(17)
    values = {
        "INT": np.concatenate([rng.integers(-(1 << 31), 1 << 31, 200), [0, 1, -1, 2735739, -(1 << 31), (1 << 31) - 1]]
                              ).astype(np.int32),
        "LONG": np.concatenate([rng.integers(-(1 << 63), (1 << 63) - 1, 200),
                                [0, -1, 1 << 62, -(1 << 62), -(1 << 63), (1 << 63) - 1, 1 << 32, (1 << 32) - 1]]
                               ).astype(np.int64),
        "FLOAT": np.concatenate([rng.normal(0, 1e6, 200), [0.0, -0.0, np.inf, -np.inf, np.nan, 1.5]]).astype(np.float32),
        "DOUBLE": np.concatenate([rng.normal(0, 1e12, 200), [0.0, -0.0, np.inf, -np.inf, np.nan, 1.5]]),
    }
    strings = ["", "a", "ab", "abc", "abcd", "abcde", "abcdef", "abcdefg", "abcdefgh", "abcdefghi", "é", "aé", "éa",
               "€", "abÿ", "abc\U0001F600", "x" * 257]
    strings += ["".join(chr(int(c)) for c in rng.integers(32, 0x2000, int(n))) for n in rng.integers(0, 40, 60)]
    for log2m in (4, 8, 12, 16):
        lines, exp = [], []
        for t, vals in values.items():
            hs = H.hashes(vals, t)
            idx, rank = H.index_rank(hs, log2m)
            for v, h, j, r in zip(vals, hs, idx, rank):
                lines.append(f"V {KIND[t]} {log2m} {_bits(v, t):x}")
                exp.append(f"{int(h)} {int(j)} {int(r)}")
        for s in strings:
            b = s.encode("utf-8")
            h = H.hash_bytes(b)
            j, r = H.index_rank([h], log2m)
            lines.append(f"S {log2m} {b.hex() or '-'}")
            exp.append(f"{h} {int(j[0])} {int(r[0])}")
        got = driver(lines)
        bad = [(l, g, e) for l, g, e in zip(lines, got, exp) if g != e]
        assert not bad, bad[:10]
        assert all(1 <= int(g.split()[2]) <= 33 - log2m for g in got)
        # the estimator over sketches of growing size, sparse to saturated, and the edge cases
        m = 1 << log2m
        sketches = [bytes(m), bytes([1] * m), bytes([33 - log2m] * m), bytes([0] * (m - 1) + [1])]
        for n in (1, 3, m // 4, m, 3 * m, 40 * m):
            sketches.append(H.registers(rng.integers(-(1 << 62), 1 << 62, n), "LONG", log2m))
        got = driver([f"E {log2m} {s.hex()}" for s in sketches])
        assert [int(g) for g in got] == [H.cardinality(s) for s in sketches]
    for log2m in (5, 6):
        s = H.registers(rng.integers(0, 1 << 40, 500), "LONG", log2m)
        assert int(driver([f"E {log2m} {s.hex()}"])[0]) == H.cardinality(s) == Q.hll_cardinality(s)
