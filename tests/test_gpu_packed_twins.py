"""Packed twins of raw INT / LONG columns (frame-of-reference bit packing built at staging, read by the streaming
scan kernels in place of the raw bytes): every plane-width combination, bases at the ends of the value types,
ragged tile counts, the shape grouping of multi-segment launches, every plan kind that streams columns, and the
accessors and byte accounting. Each result is compared with the CPU oracle (integers exactly, SUM of doubles as
assert_same_groups does) and with a PINOT_AMD_PACKED=0 plan over the same staged segments, which reads the raw bytes."""
import numpy as np
import pytest

import oracle
from pinot_amd import segment as S
from pinot_amd.query import parse_sql

pytestmark = pytest.mark.gpu

from test_gpu_parity import assert_same_groups  # noqa: E402

I32, I64 = np.iinfo(np.int32), np.iinfo(np.int64)
PAD = 4 * 1024 * 8 + 256  # pinot_amd_required_padding


@pytest.fixture(scope="module")
def engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from pinot_amd import engine as E
    return E


def planes(values, stored_bits):
    """The twin's (low plane bits, high plane bits) for a column's values, or None: bit_length(max - min) split
    into a 0 / 16 / 32-bit low plane and a high plane rounded up the ladder 0, 1, 2, 4, 8, 10, 12, 16; built only
    at <= 3/4 of the stored width."""
    b = (int(values.max()) - int(values.min())).bit_length()
    if b > 48:
        return None
    lo = 0 if b <= 16 else 16 if b <= 32 else 32
    hi = next(w for w in (0, 1, 2, 4, 8, 10, 12, 16) if b - lo <= w)
    return (lo, hi) if 4 * (lo + hi) <= 3 * stored_bits else None


def ranged(rng, n, base, b, dtype):
    """n values of base + [0, 2^b), both ends present when n >= 2 (so the range has exactly b bits)."""
    span = (1 << b) - 1
    off = rng.integers(0, span, n, dtype=np.uint64, endpoint=True) if b else np.zeros(n, np.uint64)
    if n >= 2:
        off[0], off[1] = 0, span
    return (np.uint64(base % (1 << 64)) + off).astype(np.uint64).view(np.int64).astype(dtype)


# column -> (base, bits of range); INT then LONG
INT_COLS = {"i_b0": (7, 0), "i_b1": (0, 1), "i_b7": (-50, 7), "i_b8": (0, 8), "i_b9": (-300, 9), "i_b10": (0, 10),
            "i_b15": (1_000_000, 15), "i_b16": (I32.min, 16), "i_b17": (-70_000, 17), "i_b24": (I32.max - (1 << 24) + 1, 24),
            "i_b25": (-(1 << 24), 25)}
LONG_COLS = {"l_b0": (-5, 0), "l_b8": (1 << 40, 8), "l_b16": (0, 16), "l_b17": (I64.min + 3, 17), "l_b24": (-(1 << 23), 24),
             "l_b32": (-(1 << 31), 32), "l_b33": (1_700_000_000_000, 33), "l_b40": (0, 40), "l_b48": (I64.max - (1 << 48) + 1, 48),
             "l_b49": (-(1 << 48), 49)}


def sweep_segment(rng, n, name="sweep"):
    cols = {"d": ((rng.integers(0, 365, n) * 3 + 1).astype(np.int32), S.INT, {})}  # 365 values: 9-bit dictIds
    for c, (base, b) in INT_COLS.items():
        cols[c] = (ranged(rng, n, base, b, np.int32), S.INT, {"dictionary": False})
    for c, (base, b) in LONG_COLS.items():
        cols[c] = (ranged(rng, n, base, b, np.int64), S.LONG, {"dictionary": False})
    full = rng.integers(I64.min, I64.max, n, dtype=np.int64, endpoint=True)
    full[:2] = [I64.min, I64.max][:min(n, 2)]  # max - min = 2^64 - 1: needs the unsigned difference
    cols["l_full"] = (full, S.LONG, {"dictionary": False})
    cols["dbl"] = (rng.normal(0, 1e3, n), S.DOUBLE, {"dictionary": False})
    return S.build_segment(name, cols)


SWEEP_QUERIES = [
    "SELECT d, COUNT(*), SUM(i_b0), SUM(i_b1), SUM(i_b7), MIN(i_b8), MAX(i_b9), SUM(dbl) FROM t "
    "WHERE i_b10 BETWEEN 100 AND 900 GROUP BY d",
    "SELECT COUNT(*), SUM(i_b10), SUM(i_b15), MIN(i_b16), MAX(i_b16), SUM(i_b17), SUM(i_b17 + i_b10) FROM t "
    "WHERE i_b7 IN (-50, -49, -3, 0, 11, 77)",
    "SELECT d, SUM(i_b24), SUM(i_b25), MAX(i_b24), SUM(i_b10 * i_b9), MIN(i_b16 - i_b15) FROM t "
    "WHERE NOT (i_b8 > 100 AND i_b9 < 0) GROUP BY d",
    "SELECT d, COUNT(*), SUM(l_b0), SUM(l_b8), SUM(l_b16), MIN(l_b17), MAX(l_b17), SUM(l_b24) FROM t "
    "WHERE l_b40 BETWEEN 1000 AND 800000000000 GROUP BY d",
    "SELECT COUNT(*), SUM(l_b32), SUM(l_b33), SUM(l_b40), MIN(l_b48), MAX(l_b48), SUM(l_b17) FROM t "
    "WHERE l_b16 NOT IN (0, 1, 2, 3, 65535) AND l_b24 > -8000000",
    "SELECT d, SUM(l_b49), MIN(l_full), MAX(l_full), SUM(l_b48), SUM(dbl) FROM t WHERE l_b32 < 1000000000 GROUP BY d",
]


def packed_sets(res):
    """packed_info as one set of 'column:lo+hi' per shape launch."""
    return [set(x.split(",")) - {""} for x in res.packed_info().split(";")]


def run_both_ways(engine, monkeypatch, q, bufs, segs, expect_packed=True):
    """Executes q with twins and with PINOT_AMD_PACKED=0 over the same staged segments; both against the oracle,
    exact fields identical between the two. Returns the packed run's result."""
    qc = parse_sql(q)
    fsum = {i for i, a in enumerate(qc.aggregations) if a.func in ("SUM", "AVG") and a.column == "dbl"}
    nm, og = oracle.execute(q, bufs)
    if not qc.group_by and nm == 0:
        og = {(): og[()]}
    monkeypatch.delenv("PINOT_AMD_PACKED", raising=False)
    res = engine.ServerQueryExecutor().execute(qc, segs)
    if expect_packed:
        assert res.packed_info() != "", (q, res.kernel_info())
    monkeypatch.setenv("PINOT_AMD_PACKED", "0")
    raw = engine.ServerQueryExecutor().execute(qc, segs)
    monkeypatch.delenv("PINOT_AMD_PACKED")
    assert raw.packed_info() == "", q
    assert res.num_docs_matched() == nm == raw.num_docs_matched(), q
    got, got_raw = res.groups(), raw.groups()
    assert_same_groups(got, og, fsum)
    assert_same_groups(got_raw, og, fsum)
    for k in got:
        for i, (a, b) in enumerate(zip(got[k], got_raw[k])):
            if i not in fsum:
                assert a == b, (q, k, i, a, b)
    raw.destroy()
    return res


@pytest.fixture(scope="module")
def sweep_data(engine):
    out = {}
    for n in (1, 1023, 1025, 4101, 250_007):
        bufs = sweep_segment(np.random.default_rng(1000 + n), n, f"sweep{n}")
        out[n] = (bufs, engine.ImmutableSegment(bufs))
    return out


@pytest.mark.parametrize("cols", ["int", "long"])
@pytest.mark.parametrize("n", [1, 1023, 1025, 4101, 250_007])
def test_width_sweep(engine, monkeypatch, sweep_data, n, cols):
    bufs, seg = sweep_data[n]
    for q in SWEEP_QUERIES[:3] if cols == "int" else SWEEP_QUERIES[3:]:  # (each shape compiles once per process)
        run_both_ways(engine, monkeypatch, q, [bufs], [seg]).destroy()


def test_packed_info_planes_and_base(engine, sweep_data):
    bufs, seg = sweep_data[250_007]
    want = {"i_b0": (0, 0), "i_b1": (0, 1), "i_b7": (0, 8), "i_b8": (0, 8), "i_b9": (0, 10), "i_b10": (0, 10),
            "i_b15": (0, 16), "i_b16": (0, 16), "i_b17": (16, 1), "i_b24": (16, 8), "i_b25": None,
            "l_b0": (0, 0), "l_b8": (0, 8), "l_b16": (0, 16), "l_b17": (16, 1), "l_b24": (16, 8), "l_b32": (16, 16),
            "l_b33": (32, 1), "l_b40": (32, 8), "l_b48": (32, 16), "l_b49": None, "l_full": None}
    n = 250_007
    for c, w in want.items():
        info = seg.packed_info(c)
        if w is None:
            assert info is None, (c, info)
            continue
        base = (INT_COLS.get(c) or LONG_COLS.get(c))[0]
        assert info is not None and (info["lo_bits"], info["hi_bits"], info["base"]) == (w[0], w[1], base), (c, info)
        nbytes = (n * w[0] // 8 + PAD if w[0] else 0) + ((n * w[1] + 7) // 8 + PAD if w[1] else 0)
        assert info["bytes"] == nbytes, (c, info)
    for c in ("d", "dbl"):  # dictionary-encoded and floating-point columns have no twin
        assert seg.packed_info(c) is None
    # one-doc segments: every range is 0 bits, a twin without planes
    assert sweep_data[1][1].packed_info("l_full") == {"lo_bits": 0, "hi_bits": 0, "base": I64.min, "bytes": 0}


@pytest.fixture
def fused(monkeypatch):
    monkeypatch.setenv("PINOT_AMD_SELECT", "never")  # the fused scan, whatever the cost model makes of the filter


def _simple_segment(rng, n, name, click_range=1000, imp_bits=40, keys=365):
    return S.build_segment(name, {
        "d": ((rng.integers(0, keys, n) * 3 + 1).astype(np.int32), S.INT, {}),
        "clicks": (np.concatenate([[0, click_range - 1], rng.integers(0, click_range, n - 2)]).astype(np.int32),
                   S.INT, {"dictionary": False}),
        "imp": (ranged(rng, n, 5, imp_bits, np.int64), S.LONG, {"dictionary": False}),
        "dbl": (rng.random(n) * 100.0, S.DOUBLE, {"dictionary": False}),
    })


def test_device_bytes_and_knob_off(engine, monkeypatch, fused):
    """device_bytes grows by exactly the twins' bytes; PINOT_AMD_PACKED=0 at staging builds none."""
    bufs = _simple_segment(np.random.default_rng(2), 4096, "acct")
    seg = engine.ImmutableSegment(bufs)
    twins = sum(seg.packed_info(c)["bytes"] for c in ("clicks", "imp"))
    assert twins == (4096 * 10 // 8 + PAD) + (4096 * 4 + PAD) + (4096 * 8 // 8 + PAD)
    monkeypatch.setenv("PINOT_AMD_PACKED", "0")
    bare = engine.ImmutableSegment(bufs)
    assert bare.packed_info("clicks") is None and bare.packed_info("imp") is None
    assert seg.device_bytes() - bare.device_bytes() == twins
    q = "SELECT d, COUNT(*), SUM(clicks), SUM(imp) FROM t WHERE clicks > 100 GROUP BY d"
    exp = oracle.execute(q, [bufs])[1]
    monkeypatch.delenv("PINOT_AMD_PACKED")
    r = engine.ServerQueryExecutor().execute(q, [bare])  # knob on at plan time, no twin staged: raw bytes
    assert r.packed_info() == "" and r.groups() == exp


def test_algorithmic_bytes_and_plan_identity(engine, monkeypatch, fused):
    """The bytes the plan reads, both ways, for 4096 docs; the knob is part of a prepared plan's identity."""
    n = 4096
    bufs = _simple_segment(np.random.default_rng(3), n, "alg")
    seg = engine.ImmutableSegment(bufs)
    q = "SELECT d, COUNT(*), SUM(clicks), SUM(imp), SUM(dbl) FROM t WHERE clicks > 100 GROUP BY d"
    exp = oracle.execute(q, [bufs])[1]
    ex = engine.ServerQueryExecutor()
    r = ex.execute(q, [seg])
    assert packed_sets(r) == [{"clicks:0+10", "imp:32+8"}], r.packed_info()
    assert r.algorithmic_bytes() == n * (9 + 10 + 40 + 64) / 8
    assert_same_groups(r.groups(), exp, {3})
    r.destroy()
    monkeypatch.setenv("PINOT_AMD_PACKED", "0")
    r0 = ex.execute(q, [seg])
    assert "plan_cache" not in r0.plan_timing()  # not the packed plan just released
    assert r0.packed_info() == ""
    assert r0.algorithmic_bytes() == n * (9 + 32 + 64 + 64) / 8
    assert_same_groups(r0.groups(), exp, {3})
    r0.destroy()
    monkeypatch.delenv("PINOT_AMD_PACKED")
    r = ex.execute(q, [seg])
    assert "plan_cache" in r.plan_timing() and packed_sets(r) == [{"clicks:0+10", "imp:32+8"}]
    assert_same_groups(r.groups(), exp, {3})


MS_Q = "SELECT d, COUNT(*), SUM(clicks), MAX(clicks), SUM(imp), SUM(dbl) FROM t WHERE clicks >= 7 GROUP BY d"


def _multi(engine, ranges, imp_bits=None, sizes=None):
    rng = np.random.default_rng(sum(ranges))
    sizes = sizes or [5000 + 1111 * i for i in range(len(ranges))]
    bufs = [_simple_segment(rng, n, f"ms{i}", click_range=r, imp_bits=(imp_bits or [40] * len(ranges))[i])
            for i, (n, r) in enumerate(zip(sizes, ranges))]
    return bufs, [engine.ImmutableSegment(b) for b in bufs]


def test_close_ranges_share_one_launch(engine, monkeypatch, fused):
    bufs, segs = _multi(engine, [900, 1000, 1023])
    r = run_both_ways(engine, monkeypatch, MS_Q, bufs, segs)
    assert " x" not in r.kernel_info(), r.kernel_info()
    assert packed_sets(r) == [{"clicks:0+10", "imp:32+8"}]


@pytest.mark.parametrize("ranges", [[200, 1000], [200, 1000, 60000, 250]], ids=["two_widths", "three_widths"])
def test_few_widths_run_as_separate_shapes(engine, monkeypatch, fused, ranges):
    bufs, segs = _multi(engine, ranges)
    r = run_both_ways(engine, monkeypatch, MS_Q, bufs, segs)
    shapes = len({planes(np.array([0, x - 1]), 32) for x in ranges})
    assert r.kernel_info().endswith(f" x{shapes}"), r.kernel_info()
    assert len(packed_sets(r)) == shapes and all("imp:32+8" in x and len(x) == 2 for x in packed_sets(r))


def test_many_widths_fall_back_to_raw_bytes(engine, monkeypatch, fused):
    """5 widths of one column: it reads its raw bytes, the launch stays whole, the other column keeps its twin."""
    bufs, segs = _multi(engine, [2, 12, 200, 1000, 60000])
    r = run_both_ways(engine, monkeypatch, MS_Q, bufs, segs)
    assert " x" not in r.kernel_info(), r.kernel_info()
    assert packed_sets(r) == [{"imp:32+8"}]


def test_unpackable_segment_among_packable(engine, monkeypatch, fused):
    """One segment's LONG column has no twin (49 bits): the launch reads that column's raw bytes everywhere."""
    bufs, segs = _multi(engine, [1000, 1000, 1000], imp_bits=[40, 49, 40], sizes=[4101, 3000, 70_001])
    assert segs[1].packed_info("imp") is None and segs[0].packed_info("imp") is not None
    r = run_both_ways(engine, monkeypatch, MS_Q, bufs, segs)
    assert packed_sets(r) == [{"clicks:0+10"}], r.packed_info()


FORCED_Q = "SELECT a, b, COUNT(*), SUM(clicks), MIN(imp), MAX(imp), SUM(clicks * w), SUM(dbl) FROM t WHERE clicks > 500 AND w < 40000 GROUP BY a, b"


@pytest.fixture(scope="module")
def forced_data(engine):
    n = 250_007
    rng = np.random.default_rng(9)
    bufs = S.build_segment("forced", {
        "a": ((rng.integers(0, 1000, n) * 3 + 1).astype(np.int32), S.INT, {}),
        "b": ((rng.integers(0, 1000, n) * 5 - 7).astype(np.int32), S.INT, {}),
        "c": (rng.integers(0, 2000, n).astype(np.int32), S.INT, {}),
        "clicks": (ranged(rng, n, 0, 10, np.int32), S.INT, {"dictionary": False}),
        "w": (ranged(rng, n, -20_000, 17, np.int32), S.INT, {"dictionary": False}),
        "imp": (ranged(rng, n, -(1 << 39), 40, np.int64), S.LONG, {"dictionary": False}),
        "dbl": (rng.random(n) * 100.0, S.DOUBLE, {"dictionary": False}),
    })
    return bufs, engine.ImmutableSegment(bufs)


@pytest.mark.parametrize("plan", ["partitioned", "hash", "select", "fgate", "wide_lds"])
def test_forced_plans(engine, monkeypatch, forced_data, plan):
    bufs, seg = forced_data
    q = "SET numGroupsLimit = 2000000; " + FORCED_Q
    if plan == "partitioned":
        monkeypatch.setenv("PINOT_AMD_PARTITIONED", "1")
        monkeypatch.setenv("PINOT_AMD_ATOMIC_HANDOVER", "0")
        monkeypatch.setenv("PINOT_AMD_SELECT", "never")
    elif plan == "hash":
        monkeypatch.setenv("PINOT_AMD_GROUP_PLAN", "hash")
        monkeypatch.setenv("PINOT_AMD_SELECT", "never")
    elif plan == "select":
        monkeypatch.setenv("PINOT_AMD_SELECT", "always")
        monkeypatch.setenv("PINOT_AMD_PARTITIONED", "0")
    elif plan == "fgate":
        monkeypatch.setenv("PINOT_AMD_FILTER_GATE", "1")
        monkeypatch.setenv("PINOT_AMD_SELECT", "never")
        q = FORCED_Q.replace("a, b", "c")  # a dense plan: the gate is a fused scan's
    else:  # 2000 keys x 6 to 8 arrays x 8 B = 96 to 128 KB: above the 40 KB per-block table, the CU-wide one
        monkeypatch.setenv("PINOT_AMD_SELECT", "never")
        q = FORCED_Q.replace("a, b", "c")
    r = run_both_ways(engine, monkeypatch, q, [bufs], [seg])
    info = r.kernel_info()
    want = {"partitioned": "jit-partitioned", "hash": "jit-hash", "select": "-select", "fgate": "+fgate", "wide_lds": "jit"}
    assert want[plan] in info, info
    # the select pass streams only its filter columns (the gather reads raw bytes); every other plan streams all
    # three raw integer columns
    cols = {"clicks:0+10", "w:16+1"} | (set() if plan == "select" else {"imp:32+8"})
    assert packed_sets(r) == [cols], r.packed_info()
