"""Multi-value columns on the device: staging and validation of FixedBitMVForwardIndexWriter's bytes
(pinot_amd_segment_add_mv_column), getDictIdMV for a whole column (pinot_amd_fwd_read_dict_ids_mv), ANY-match filters
(mv_match_kernel -> docId bitsets) and the *MV aggregations over the per-doc twins (mv_reduce_kernel).

The oracle cannot read MV columns: expected results are its answers to the query rewritten over single-value columns
that tests/mv_ref.py materialises from an independent numpy restatement (a {0, 1} column per MV leaf, per-doc count /
sum / min / max columns per MV column). Integers compare exactly, double sums within the project's 1e-12 relative rule
(assert_same_groups)."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

import mv_ref as R
import oracle
from pinot_amd import segment as S
from pinot_amd.query import FilterContext, Predicate, parse_sql

pytestmark = pytest.mark.gpu

from test_gpu_parity import assert_same_groups  # noqa: E402

EINVAL, EUNSUPPORTED = -1, -2
SIZES = [1, 4099, 5000, 0, 70_000]
PINNED_DOCS = [[1, 2], [3], [2, 2, 5], [7], [1, 7]]
PINNED_FWD = bytes.fromhex("00000000B3000512E080")
MV_TYPES = {"tags": S.INT, "w": S.LONG, "d": S.DOUBLE, "s": S.STRING, "one": S.INT, "wide": S.INT}
EXACT_SUM = {"tags": True, "w": False, "d": False, "one": True}  # w: 8 values near 2^62 overflow int64


@pytest.fixture(scope="module")
def engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from pinot_amd import engine as E
    return E


def draw_segment(rng, n, big):
    """{column: per-doc value lists} (MV) and {column: array} (SV) of one segment."""
    lens = rng.integers(1, 6 if big else 9, n)
    total = int(lens.sum())
    cut = np.r_[0, np.cumsum(lens)]

    def split(flat):
        return [flat[cut[i]:cut[i + 1]].tolist() for i in range(n)]
    tags = rng.integers(0, 37, total) * 3 - 20                     # card 37, duplicates inside a doc
    sign = np.where(rng.random(total) < 0.9, 1, -1)
    w = sign * ((1 << 62) - rng.integers(0, 1 << 40, total))       # near +-2^62: the per-doc sum is a DOUBLE
    d = np.round(rng.random(total) * 1000.0, 3)                    # >= 0
    if n > 10:
        d[cut[7]] = np.nan                                          # one doc holds NaN beside other values
        assert lens[7] >= 1
    s = np.array([f"s{v:02d}" for v in rng.integers(0, 50, total)], dtype=object)
    wide = rng.permutation(70_000)[:total] if total <= 70_000 else np.r_[rng.permutation(70_000),
                                                                       rng.integers(0, 70_000, total - 70_000)]
    mv = {"tags": split(tags.astype(np.int32)), "w": split(w.astype(np.int64)), "d": split(d), "s": split(s),
          "one": [[int(v)] for v in rng.integers(0, 1000, n)], "wide": split(wide.astype(np.int32))}
    if n > 10 and len(mv["d"][7]) == 1:
        mv["d"][7] = [float("nan"), 1.5]
    sv = {"g": np.array([f"g{v}" for v in rng.integers(0, 7, n)], dtype=object),
          "x": rng.integers(-1000, 1000, n).astype(np.int32)}
    return mv, sv


@pytest.fixture(scope="module")
def data(engine):
    """Per segment: the MV value lists, the SV arrays, the SegmentBuffers and the staged segment."""
    rng = np.random.default_rng(1212)
    out = []
    for i, n in enumerate(SIZES):
        mv, sv = draw_segment(rng, n, n > 10_000)
        cols = {c: (mv[c], MV_TYPES[c], {"multi_value": True}) for c in mv}
        cols["g"] = (sv["g"], S.STRING, {"detect_sorted": False, "inverted": True})
        cols["x"] = (sv["x"], S.INT, {"dictionary": False})
        bufs = S.build_segment(f"mv{i}", cols)
        out.append({"mv": mv, "sv": sv, "bufs": bufs, "seg": engine.ImmutableSegment(bufs), "n": n})
    big = out[-1]["bufs"].columns
    assert big["wide"].bits_per_element == 17 and big["wide"].cardinality == 70_000
    assert big["tags"].total_values > 50 * 4096 and big["tags"].cardinality == 37
    return out


_REDUCED = {}
_LEAF_BITS = {}  # (segment, leaf) -> the leaf's {0, 1} column, evaluated once


def reduced(data, i, col):
    """The per-doc reductions of segment i's column, computed once."""
    if (i, col) not in _REDUCED:
        _REDUCED[(i, col)] = R.reductions(data[i]["mv"][col], MV_TYPES[col], EXACT_SUM[col])
    return _REDUCED[(i, col)]


def sv_specs(seg):
    return {"g": (seg["sv"]["g"], S.STRING, {"detect_sorted": False, "inverted": True}),
            "x": (seg["sv"]["x"], S.INT, {"dictionary": False})}


def expected(data, which, template, agg_cols=()):
    """(the MV query, matched docs and groups the oracle gives the rewritten SV query over materialised segments)."""
    mv_sql, sv_sql, leaves, fold = R.rewrite(template)
    segs = []
    for i in which:
        red = {c: reduced(data, i, c) for c in agg_cols}
        lcols = {p.column for f in leaves for p in _preds(f) if p.column in MV_TYPES}
        segs.append(R.oracle_segment(f"o{i}", sv_specs(data[i]), {c: data[i]["mv"][c] for c in lcols}, leaves, red,
                                     cache=_LEAF_BITS))
    nm, og = oracle.execute(sv_sql, segs)
    return mv_sql, nm, {k: fold(v) for k, v in og.items()}


def _preds(f):
    if f.type == "PREDICATE":
        return [f.predicate]
    return [p for c in f.children for p in _preds(c)]


def run(engine, data, which, template, agg_cols=(), float_sums=(), executor=None):
    mv_sql, nm, exp = expected(data, which, template, agg_cols)
    ex = executor or engine.ServerQueryExecutor()
    res = ex.execute(mv_sql, [data[i]["seg"] for i in which])
    assert res.num_docs_matched() == nm, mv_sql
    got = res.groups()
    assert_same_groups(got, exp, set(float_sums))
    return res, got, exp


# ------------------------------------------------------------------------------- low level
def test_read_dict_ids_mv_every_segment(engine, data):
    import torch
    from pinot_amd._lib import check, lib
    for seg in data:
        for c, cb in seg["bufs"].columns.items():
            if not cb.multi_value:
                continue
            assert seg["seg"].mv_info(c) == (cb.total_values, cb.max_values)
            off = torch.full((seg["n"] + 1,), -1, dtype=torch.int32, device="cuda")
            ids = torch.full((max(cb.total_values, 1),), -1, dtype=torch.int32, device="cuda")
            check(lib().pinot_amd_fwd_read_dict_ids_mv(seg["seg"].column_fwd_ptr(c), seg["n"], cb.total_values,
                                                       cb.bits_per_element, off.data_ptr(), ids.data_ptr(), None))
            torch.cuda.synchronize()
            eo, ei = S.unpack_mv_fwd(cb.fwd, cb.bits_per_element, seg["n"], cb.total_values)
            assert np.array_equal(off.cpu().numpy(), eo), (seg["n"], c)
            assert np.array_equal(ids.cpu().numpy()[:cb.total_values], ei), (seg["n"], c)
        assert seg["seg"].mv_info("g") is None


def test_read_dict_ids_mv_pinned_bytes(engine):
    import torch
    from pinot_amd._lib import check, lib
    pad = lib().pinot_amd_required_padding()
    d = torch.zeros(len(PINNED_FWD) + pad, dtype=torch.uint8, device="cuda")
    d[:len(PINNED_FWD)] = torch.frombuffer(bytearray(PINNED_FWD), dtype=torch.uint8).cuda()
    off = torch.zeros(6, dtype=torch.int32, device="cuda")
    ids = torch.zeros(9, dtype=torch.int32, device="cuda")
    check(lib().pinot_amd_fwd_read_dict_ids_mv(d.data_ptr(), 5, 9, 3, off.data_ptr(), ids.data_ptr(), None))
    torch.cuda.synchronize()
    o, v = off.cpu().numpy(), np.array([1, 2, 3, 5, 7])[ids.cpu().numpy()]
    assert [v[o[k]:o[k + 1]].tolist() for k in range(5)] == PINNED_DOCS
    # either output may be NULL
    check(lib().pinot_amd_fwd_read_dict_ids_mv(d.data_ptr(), 5, 9, 3, None, ids.data_ptr(), None))
    check(lib().pinot_amd_fwd_read_dict_ids_mv(d.data_ptr(), 5, 9, 3, off.data_ptr(), None, None))
    assert lib().pinot_amd_fwd_read_dict_ids_mv(d.data_ptr(), 5, 4, 3, off.data_ptr(), None, None) == EINVAL


# ------------------------------------------------------------------------------- staging refusals
def _stage(engine, cb, num_docs=5):
    return engine.ImmutableSegment(S.SegmentBuffers("bad", num_docs, {cb.name: cb}))


def test_staging_refusals(engine):
    from pinot_amd._lib import PinotAmdError, lib
    good = S.build_column("c", PINNED_DOCS, S.INT, multi_value=True)
    _stage(engine, good).destroy()
    cleared = bytearray(PINNED_FWD)
    cleared[4] &= 0xDF  # value 2 no longer starts a doc: 4 start bits for 5 docs
    moved = bytearray(PINNED_FWD)
    moved[4] = 0x73     # value 0 starts no doc, value 1 does: still 5 start bits
    header = bytearray(PINNED_FWD)
    header[3] = 1       # chunk 0 said to start at value 1
    bad = {"a cleared start bit": dataclasses.replace(good, fwd=bytes(cleared)),
           "bit 0 unset": dataclasses.replace(good, fwd=bytes(moved)),
           "a wrong total_num_values": dataclasses.replace(good, total_values=17),
           "a wrong header entry": dataclasses.replace(good, fwd=bytes(header)),
           "a doc longer than max_num_values_per_doc": dataclasses.replace(good, max_values=2)}
    for what, cb in bad.items():
        with pytest.raises(PinotAmdError, match=r"\(-1\)"):
            _stage(engine, cb)
        assert b"column c" in lib().pinot_amd_last_error(), what
    # an inverted index on an MV column: EUNSUPPORTED; FIXED_BIT_MV through the SV call: EINVAL, naming the MV call
    with pytest.raises(PinotAmdError, match=r"\(-2\)"):
        _stage(engine, dataclasses.replace(good, inverted=b"\0\0\0\4"))
    seg = _stage(engine, good)
    spec = engine.ColumnSpec()
    spec.name, spec.stored_type, spec.encoding, spec.cardinality, spec.bits_per_element = b"c2", 0, 3, 5, 3
    spec.h_fwd, spec.fwd_size = C.cast(C.c_char_p(good.fwd), C.c_void_p), len(good.fwd)
    spec.h_dictionary, spec.dictionary_size = C.cast(C.c_char_p(good.dictionary), C.c_void_p), len(good.dictionary)
    assert lib().pinot_amd_segment_add_column(seg.handle, C.byref(spec)) == EINVAL
    assert b"pinot_amd_segment_add_mv_column" in lib().pinot_amd_last_error()
    seg.destroy()


# ------------------------------------------------------------------------------- the pinned table
@pytest.fixture(scope="module")
def pinned(engine):
    bufs = S.build_segment("pinned", {"c": (PINNED_DOCS, S.INT, {"multi_value": True}),
                                      "g": (np.array(list("aabba"), dtype=object), S.STRING, {"detect_sorted": False})})
    assert bufs.columns["c"].fwd == PINNED_FWD
    return engine.ImmutableSegment(bufs)


@pytest.mark.parametrize("where,docs", [("c = 2", 2), ("c != 2", 3), ("c IN (1,3)", 3), ("c NOT IN (1,3)", 2),
                                        ("c > 5 AND c < 2", 1), ("c BETWEEN 3 AND 5", 2)])
def test_pinned_filters(engine, pinned, where, docs):
    res = engine.ServerQueryExecutor().execute(parse_sql(f"SELECT COUNT(*) FROM t WHERE {where}"), [pinned])
    assert res.groups()[()] == [docs] and res.num_docs_matched() == docs
    res.destroy()


def test_pinned_aggregations(engine, pinned):
    q = "SELECT COUNTMV(c), SUMMV(c), MINMV(c), MAXMV(c), AVGMV(c), MINMAXRANGEMV(c) FROM t"
    res = engine.ServerQueryExecutor().execute(parse_sql(q), [pinned])
    assert res.groups()[()] == [9, 30.0, 1.0, 7.0, (30.0, 9), (1.0, 7.0)]
    assert type(res.groups()[()][0]) is int
    assert res.rows() == [(9, 30.0, 1.0, 7.0, 30.0 / 9, 6.0)]
    res.destroy()
    q = "SELECT g, COUNT_MV(c), sum_mv(c), MINMV(c), MAXMV(c), AVGMV(c) FROM t GROUP BY g"
    res = engine.ServerQueryExecutor().execute(parse_sql(q), [pinned])
    assert res.groups() == {("a",): [5, 14.0, 1.0, 7.0, (14.0, 5)], ("b",): [4, 16.0, 2.0, 7.0, (16.0, 4)]}
    assert sorted(res.rows()) == [("a", 5, 14.0, 1.0, 7.0, 2.8), ("b", 4, 16.0, 2.0, 7.0, 4.0)]
    res.destroy()
    # no matching doc: the SV functions' empty values
    res = engine.ServerQueryExecutor().execute(q.replace("g, ", "").replace(" GROUP BY g", " WHERE c = 4")
                                               .replace("AVGMV(c)", "AVGMV(c), MINMAXRANGEMV(c)"), [pinned])
    assert res.rows() == [(0, 0.0, math.inf, -math.inf, -math.inf, -math.inf)]
    res.destroy()


# ------------------------------------------------------------------------------- filters over the batch
ALL = list(range(len(SIZES)))
FILTERS = [
    "{tags = 1}", "{tags != 1}", "{tags IN (-20, 1, 88)}", "{tags NOT IN (-20, 1, 88)}",
    "NOT {tags BETWEEN -5 AND 40}",                      # negate = 1 on a RANGE leaf
    "{tags BETWEEN -5 AND 40}", "{tags > 40}",           # a sorted dictId range
    "{tags > 70} AND {tags < -10}",                      # independent leaves, a > b
    "{wide IN (5, 77, 4000, 31000, 69999, 123456)}",     # a dictId bitmap of > 64 words, staged in LDS
    "{s IN ('s03', 's17', 's49', 'nope')}", "{s != 's03'}",
    "{one = 1234}", "{one != 1234}",                     # absent from every dictionary: alwaysFalse / alwaysTrue
    "{tags = 1} OR x > 900",                             # an MV leaf and an SV leaf in one clause
    "{tags IN (1, 4)} AND g = 'g3'",
]


@pytest.mark.parametrize("template", FILTERS)
def test_filters(engine, data, template):
    res, got, exp = run(engine, data, ALL, f"SELECT COUNT(*), SUM(x) FROM t WHERE {template}")
    if "{one " not in template:  # (those leaves are constants in every segment: no bitset is left to expand)
        assert "fwselect" not in res.kernel_info()
    res.destroy()
    res, _, _ = run(engine, data, ALL, f"SELECT g, COUNT(*), MAX(x) FROM t WHERE {template} GROUP BY g LIMIT 100")
    res.destroy()


def test_value_absent_from_one_segment(engine, data):
    """A value only the big segment's `wide` dictionary holds: alwaysFalse (alwaysTrue for the exclusive leaf) in the
    segments without it."""
    have = set(np.concatenate([np.asarray(v) for v in data[1]["mv"]["wide"]]).tolist())
    v = next(x for x in range(70_000) if x not in have)
    for op in ("=", "!="):
        res, _, _ = run(engine, data, [1, 4], f"SELECT COUNT(*) FROM t WHERE {{wide {op} {v}}}")
        res.destroy()


@pytest.mark.parametrize("policy", ["always", "never"])
def test_mv_leaf_and_inverted_index_leaf(engine, data, policy, monkeypatch):
    monkeypatch.setenv("PINOT_AMD_INV_POLICY", policy)
    for t in ("SELECT COUNT(*), SUM(x) FROM t WHERE {tags IN (1, 4, 7)} AND g IN ('g1', 'g5')",
              "SELECT COUNT(*) FROM t WHERE {tags != 4} AND g = 'g2'"):
        res, _, _ = run(engine, data, ALL, t)
        assert "fwselect" not in res.kernel_info()
        res.destroy()


class _DeviceWords:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i8", "data": (ptr, False), "version": 2,
                                         "strides": None}


def filter_words(engine, segs, add_leaves):
    """The docId bitsets of pinot_amd_execute_filter, one uint64 array per segment."""
    import torch
    from pinot_amd._lib import check, lib
    L = lib()
    qh, rh = C.c_void_p(), C.c_void_p()
    check(L.pinot_amd_query_create(C.byref(qh)))
    keep = []
    add_leaves(L, qh, keep)
    arr = (C.c_void_p * len(segs))(*[s["seg"].handle.value for s in segs])
    check(L.pinot_amd_execute_filter(qh, arr, len(segs), None, C.byref(rh)), "execute_filter")
    out = []
    for i, s in enumerate(segs):
        p, nw = C.c_void_p(), C.c_int64()
        check(L.pinot_amd_result_bitset(rh, i, C.byref(p), C.byref(nw)))
        need = (s["n"] + 63) // 64
        assert nw.value >= need
        w = torch.as_tensor(_DeviceWords(p.value, nw.value), device="cuda").cpu().numpy().view(np.uint64) \
            if need else np.zeros(0, np.uint64)
        out.append(w[:need].copy())
    L.pinot_amd_result_destroy(rh)
    L.pinot_amd_query_destroy(qh)
    return out


def test_execute_filter_bitsets_bit_for_bit(engine, data):
    """FilterPlanNode over MV leaves, and negate = 1 on an EQ / IN leaf = NOT_EQ / NOT_IN."""
    which = [data[i] for i in (0, 1, 3, 4)]
    cases = [(Predicate("EQ", "tags", (1,)), 0), (Predicate("EQ", "tags", (1,)), 1), (Predicate("NOT_EQ", "tags", (1,)), 0),
             (Predicate("IN", "wide", (5, 77, 4000, 31000, 69999)), 1), (Predicate("RANGE", "tags", (), 10, 50, False, True), 0)]
    for pred, neg in cases:
        def add(L, qh, keep, pred=pred, neg=neg):
            from pinot_amd._lib import check
            spec = engine._predicate_spec(pred, which[0]["bufs"].columns[pred.column], False, keep)
            check(L.pinot_amd_query_add_predicate(qh, 0, C.byref(spec), neg), "add_predicate")
        got = filter_words(engine, which, add)
        f = FilterContext.pred(pred)
        if neg:
            f = FilterContext.not_(f)
        for seg, words in zip(which, got):
            exp = R.doc_bitset({pred.column: seg["mv"][pred.column]}, {}, f, seg["n"])
            if seg["n"] % 64:  # (the bits past the last doc are no docs)
                words[-1] &= (np.uint64(1) << np.uint64(seg["n"] % 64)) - np.uint64(1)
            assert np.array_equal(words, exp), (pred, neg, seg["n"])


# ------------------------------------------------------------------------------- aggregations
SIX = "COUNTMV({c}), SUMMV({c}), MINMV({c}), MAXMV({c}), AVGMV({c}), MINMAXRANGEMV({c})"


@pytest.mark.parametrize("col", ["tags", "w", "d"])
@pytest.mark.parametrize("shape", ["all", "group", "filter"])
def test_six_functions(engine, data, col, shape):
    tail = {"all": "", "group": " GROUP BY g LIMIT 100", "filter": " WHERE {tags IN (1, 4, 7, 88)} GROUP BY g LIMIT 100"}[shape]
    head = "SELECT " + ("" if shape == "all" else "g, ")
    fs = () if col == "tags" else (1, 4)  # SUMMV, AVGMV's sum: doubles of w and d
    res, got, exp = run(engine, data, ALL, head + "COUNT(*), " + SIX.format(c=col) + " FROM t" + tail, [col],
                        float_sums=[i + 1 for i in fs])
    for vals in got.values():
        assert type(vals[1]) is int                                    # COUNTMV: a LONG
        assert not any(isinstance(v, float) and math.isnan(v) for v in (vals[3], vals[4]))  # NaN never in MINMV / MAXMV
        assert not any(math.isnan(v) for v in vals[6])
    if col == "d":  # the NaN docs (one per segment) reach SUMMV of their groups only
        assert 1 <= sum(math.isnan(v[2]) for v in got.values()) <= (1 if shape == "all" else 4)
    res.destroy()


def test_countmv_of_single_valued_docs_is_count_star(engine, data):
    res = engine.ServerQueryExecutor().execute("SELECT g, COUNT(*), COUNTMV(one), SUMMV(one) FROM t WHERE tags > 0 "
                                               "GROUP BY g LIMIT 100", [s["seg"] for s in data])
    got = res.groups()
    assert got and all(v[0] == v[1] for v in got.values())
    res.destroy()


def test_exact_values_and_avg_pair(engine, data):
    """h_values_i64: the exact COUNTMV and integer SUMMV; fetch_intermediate: AVGMV's (sum, value count)."""
    ex = engine.ServerQueryExecutor()
    res = ex.execute("SELECT COUNTMV(tags), SUMMV(tags), AVGMV(tags), SUMMV(w) FROM t", [s["seg"] for s in data])
    _, _, vals, vals_i, pairs = res.fetch_arrays()
    cnt = sum(int(reduced(data, i, "tags")[0].sum()) for i in ALL)
    sm = sum(int(reduced(data, i, "tags")[1].sum()) for i in ALL)
    assert (int(vals_i[0]), int(vals_i[1])) == (cnt, sm) and vals[0] == float(cnt) and vals[1] == float(sm)
    assert (pairs[4], pairs[5]) == (float(sm), float(cnt)) and vals[2] == float(sm) / cnt
    assert res.groups()[()][2] == (float(sm), cnt)
    res.destroy()


def test_order_by_summv_through_the_server_table(engine, data):
    t = "SELECT g, SUMMV(tags), COUNTMV(tags) FROM t WHERE {tags > 0} GROUP BY g"
    mv_sql, _, exp = expected(data, ALL, t + " LIMIT 100", ["tags"])  # (every group; the order is checked below)
    mv_sql = R.rewrite(t)[0] + " ORDER BY summv(tags) DESC LIMIT 3"
    res = engine.ServerQueryExecutor(server_trim=True).execute(mv_sql, [s["seg"] for s in data])
    got = res.groups()
    top = sorted(exp, key=lambda k: -exp[k][0])[:3]
    assert len(got) == len(exp)  # trimSize = max(5 * LIMIT, 5000) >= 7 groups: all kept, in the ORDER BY's order
    assert list(got)[:3] == top and got == {k: exp[k] for k in got}
    res.destroy()


def test_filtered_lane_beside_unfiltered(engine, data):
    q = "SELECT SUMMV(tags) FILTER (WHERE tags = 4), COUNTMV(tags), SUMMV(tags) FILTER (WHERE x > 0) FROM t WHERE tags != 88"
    res = engine.ServerQueryExecutor().execute(q, [s["seg"] for s in data])
    f_sum = cnt = x_sum = 0
    for i in ALL:
        c, sm, _, _ = reduced(data, i, "tags")
        for d, vals in enumerate(data[i]["mv"]["tags"]):
            if 88 in vals:
                continue
            cnt += int(c[d])
            f_sum += int(sm[d]) if 4 in vals else 0
            x_sum += int(sm[d]) if data[i]["sv"]["x"][d] > 0 else 0
    assert res.groups()[()] == [float(f_sum), cnt, float(x_sum)]
    res.destroy()


@pytest.mark.parametrize("plan", ["hash", "partitioned"])
def test_twins_are_ordinary_columns_of_every_plan(engine, data, plan, monkeypatch):
    if plan == "hash":
        monkeypatch.setenv("PINOT_AMD_GROUP_PLAN", "hash")
    else:
        monkeypatch.setenv("PINOT_AMD_PARTITIONED", "1")
        monkeypatch.setenv("PINOT_AMD_ATOMIC_HANDOVER", "0")
    monkeypatch.setenv("PINOT_AMD_SELECT", "never")
    res, _, _ = run(engine, data, ALL, "SELECT g, x, COUNT(*), " + SIX.format(c="tags") + ", SUMMV(d) FROM t "
                    "WHERE {tags != 4} GROUP BY g, x LIMIT 100000", ["tags", "d"], float_sums=[7])
    assert plan in res.kernel_info(), res.kernel_info()
    res.destroy()


# ------------------------------------------------------------------------------- plumbing
def test_twins_built_once_plan_cache_and_execute_again(engine):
    rng = np.random.default_rng(5)
    mv, sv = draw_segment(rng, 9000, False)
    bufs = S.build_segment("fresh", {"tags": (mv["tags"], S.INT, {"multi_value": True}),
                                     "g": (sv["g"], S.STRING, {"detect_sorted": False})})
    seg = engine.ImmutableSegment(bufs)
    ex = engine.ServerQueryExecutor()
    q = "SELECT g, COUNTMV(tags), SUMMV(tags), MINMV(tags), MAXMV(tags) FROM t WHERE tags IN (1, 4) GROUP BY g LIMIT 100"
    b0 = seg.device_bytes()
    r1 = ex.execute(q, [seg])
    b1 = seg.device_bytes()
    assert b1 > b0 and "plan_cache" not in r1.plan_timing() and r1.plan_timing()["raw_keys"] > 0
    first = r1.groups()
    bytes1, info = r1.algorithmic_bytes(), r1.kernel_info()
    cb = bufs.columns["tags"]
    assert bytes1 >= cb.total_values * (cb.bits_per_element + 1) / 8 + 2 * ((9000 + 7) // 8)
    assert "$mv" not in info
    for _ in range(2):
        r1.execute_again()
        assert r1.groups() == first and r1.last_kernel_ms() > 0
    r1.destroy()
    r2 = ex.execute(q, [seg])  # the re-issued query: its prepared plan, no new twin
    assert "plan_cache" in r2.plan_timing(), r2.plan_timing()
    assert seg.device_bytes() == b1 and r2.groups() == first
    r2.destroy()
    r3 = ex.execute(q.replace("(1, 4)", "(1, 7)"), [seg])  # another query over the same twins
    assert seg.device_bytes() == b1
    r3.destroy()
    c, sm, mn, mx = R.reductions(mv["tags"], S.INT, True)
    keep = np.array([1 in v or 4 in v for v in mv["tags"]])
    for (g,), vals in first.items():
        m = keep & (sv["g"] == g)
        assert vals == [int(c[m].sum()), float(sm[m].sum()), float(mn[m].min()), float(mx[m].max())]
    seg.destroy()


# ------------------------------------------------------------------------------- refusals
def _refused(engine, query, segs, code, column, **kw):
    from pinot_amd._lib import PinotAmdError, lib
    with pytest.raises(PinotAmdError, match=rf"\({code}\)"):
        engine.ServerQueryExecutor(**kw).execute(query, segs)
    assert column.encode() in lib().pinot_amd_last_error(), lib().pinot_amd_last_error()


def test_refusals(engine, data):
    from pinot_amd._lib import check, lib
    segs = [data[1]["seg"], data[2]["seg"]]
    for q in ("SELECT SUM(tags) FROM t", "SELECT MIN(tags), COUNT(*) FROM t", "SELECT AVG(tags) FROM t GROUP BY g",
              "SELECT MINMAXRANGE(tags) FROM t", "SELECT SUMLONG(tags) FROM t", "SELECT SUM(tags * x) FROM t",
              "SELECT g, COUNT(*) FROM t GROUP BY g, tags", "SELECT tags FROM t LIMIT 5",
              "SELECT g FROM t ORDER BY tags LIMIT 5",
              "SELECT dateTrunc('day', tags, 'MILLISECONDS'), COUNT(*) FROM t GROUP BY dateTrunc('day', tags, 'MILLISECONDS')"):
        _refused(engine, q, segs, EUNSUPPORTED, "tags")
    for q in ("SELECT DISTINCTCOUNT(tags) FROM t", "SELECT PERCENTILE50(tags) FROM t GROUP BY g",
              "SELECT DISTINCTSUM(tags) FROM t", "SELECT DISTINCTAVG(tags) FROM t"):
        _refused(engine, q, segs, EUNSUPPORTED, "tags", distinct_count="native")
    _refused(engine, "SELECT SUMMV(x) FROM t", segs, EUNSUPPORTED, "x")       # an *MV function over an SV column
    _refused(engine, "SELECT COUNTMV(g) FROM t", segs, EINVAL, "g")            # ... over a STRING column
    _refused(engine, "SELECT MAXMV(s) FROM t", segs, EINVAL, "s")
    # the entry points of the single-value functions take none of them; theirs takes nothing else
    qh = C.c_void_p()
    check(lib().pinot_amd_query_create(C.byref(qh)))
    idx = C.c_int32(-1)
    for k, code in enumerate(range(11, 17)):
        assert lib().pinot_amd_query_add_aggregation(qh, code, b"tags", None) == EINVAL
        assert lib().pinot_amd_query_add_aggregation_param(qh, code, b"tags", 0.0, None) == EINVAL
        assert b"pinot_amd_query_add_aggregation_mv" in lib().pinot_amd_last_error()
        assert lib().pinot_amd_query_add_aggregation_mv(qh, code, b"tags", C.byref(idx)) == 0 and idx.value == k
    for code in (-1, 0, 1, 10, 17):
        assert lib().pinot_amd_query_add_aggregation_mv(qh, code, b"tags", None) == EINVAL
    assert lib().pinot_amd_query_add_aggregation_mv(qh, 11, b"*", None) == EINVAL
    assert lib().pinot_amd_query_add_aggregation_mv(qh, 11, None, None) == EINVAL
    assert lib().pinot_amd_query_add_aggregation_mv(None, 11, b"tags", None) == EINVAL
    lib().pinot_amd_query_destroy(qh)
    # a key space installed on an MV column
    with pytest.raises(Exception, match=r"\(-2\)"):
        engine.ServerQueryExecutor().execute("SELECT tags, COUNT(*) FROM t GROUP BY tags", segs,
                                             key_space={"tags": [1, 4]})
    # MV in one segment of the batch, SV in the other
    sv_tags = S.build_segment("svtags", {"tags": (np.arange(50, dtype=np.int32) % 7, S.INT, {"detect_sorted": False}),
                                         "g": (np.array(["g1"] * 50, dtype=object), S.STRING, {"detect_sorted": False}),
                                         "x": (np.arange(50, dtype=np.int32), S.INT, {"dictionary": False})})
    mixed = [data[1]["seg"], engine.ImmutableSegment(sv_tags)]
    _refused(engine, "SELECT COUNT(*) FROM t WHERE tags = 1", mixed, EINVAL, "tags")
    _refused(engine, "SELECT COUNTMV(tags) FROM t", mixed, EINVAL, "tags")
    # nothing was built by a refused query
    b = data[2]["seg"].device_bytes()
    _refused(engine, "SELECT SUMMV(one), SUM(tags) FROM t", [data[2]["seg"]], EUNSUPPORTED, "tags")
    assert data[2]["seg"].device_bytes() == b


def test_dist_refuses_mv_queries(engine, data):
    from pinot_amd import dist
    res = engine.ServerQueryExecutor().execute("SELECT g, COUNT(*) FROM t WHERE tags = 1 GROUP BY g", [data[1]["seg"]])
    with pytest.raises(ValueError, match="multi-value"):
        dist.merge_result(res)
    res.destroy()
    with pytest.raises(ValueError, match="multi-value"):
        dist.merge_groups(parse_sql("SELECT SUMMV(tags) FROM t"), {})
