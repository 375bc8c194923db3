"""LIKE / REGEXP_LIKE on the device: the per-operator dictionary match (dict_regex_match_kernel against the host
runner and tests/regex_ref.py) and whole queries through ServerQueryExecutor against the CPU oracle's answers to the
query rewritten over {0, 1} columns that regex_ref evaluates per doc (the trick of tests/mv_ref.py).

Shapes: dictionaries of 1 / 63 / 64 / 65 / 130 / 5000 values (wave and mask-word edges, a partial last word, past the
64-value accept masks and past 64 set words) whose values have 0, 1, 3, 4 and 5 bytes (the dword edges), one of more
than 256, multi-byte ones, the last ending at the buffer's last byte; 3 segments of about 3000 docs (3 tiles, the last
partial) with different dictionaries, one where nothing matches and one where everything does."""
import ctypes as C

import numpy as np
import pytest

import filtered_aggs_ref
import oracle
import regex_ref as R
import selection_ref
from pinot_amd import segment as S
from pinot_amd.query import canonical_key, final_value, parse_sql

pytestmark = pytest.mark.gpu

from test_gpu_parity import assert_same_groups  # noqa: E402

EINVAL, EUNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from pinot_amd import engine as E
    return E


# ------------------------------------------------------------------------------------------- (a) per operator
CARDS = [1, 63, 64, 65, 130, 5000]
EDGE_VALUES = ["", "a", "abc", "abcd", "abcde", "x" * 300 + "zq", "é", "aé€", "\U0001F600x", "abc\n", "abc\r\n", "K", "ſ",
               "Zq", "/cart9"]
OP_PATTERNS = [("zq", True), ("zq", False), ("^abc", False), ("abc$", False), (".", False), ("^.{3}$", False),
               ("[^a-z]", False), ("é", False), ("^$", False), ("", False), ("(zq|Zq)$", False), ("k", True),
               ("^(a|b)+/?", True), ("\\W", False), ("x{250}z", False), ("^[^é]*$", False), ("^q", False), ("nomatch!", False)]


def dictionary_values(card, seed):
    rng = np.random.default_rng(seed)
    vals = set([""] if card == 1 else EDGE_VALUES[:card])
    alphabet = list("abZq/.x") + ["é", "€"]
    while len(vals) < card:
        vals.add("".join(rng.choice(alphabet, size=int(rng.integers(0, 10)))))
    return sorted(vals, key=lambda s: s.encode("utf-16-be"))


@pytest.fixture(scope="module")
def dict_segments(engine):
    out = {}
    for card in CARDS:
        vals = dictionary_values(card, 100 + card)
        bufs = S.build_segment(f"rxd{card}", {"v": (np.array(vals, dtype=object), S.STRING, {"detect_sorted": False})})
        assert bufs.columns["v"].cardinality == card
        out[card] = (vals, engine.ImmutableSegment(bufs))
    return out


@pytest.mark.parametrize("card", CARDS)
def test_match_dictionary_device_against_host_and_reference(engine, dict_segments, card, monkeypatch):
    vals, seg = dict_segments[card]
    for pat, ci in OP_PATTERNS:
        exp = np.array([R.matches(pat, v, ci) for v in vals], dtype=bool)
        monkeypatch.setenv("PINOT_AMD_REGEX_DEVICE", "always")
        dev = seg.regexp_match_dictionary("v", pat, ci)
        monkeypatch.setenv("PINOT_AMD_REGEX_DEVICE", "never")
        host = seg.regexp_match_dictionary("v", pat, ci)
        assert np.array_equal(dev, host), (pat, ci, np.nonzero(dev != host)[0][:8])
        assert np.array_equal(dev, exp), (pat, ci, [vals[i] for i in np.nonzero(dev != exp)[0][:8]])


def test_device_dictionary_is_built_once_and_counted(engine, monkeypatch):
    vals = dictionary_values(130, 7)
    seg = engine.ImmutableSegment(S.build_segment("rxbytes", {"v": (np.array(vals, dtype=object), S.STRING, {})}))
    before = seg.device_bytes()
    monkeypatch.setenv("PINOT_AMD_REGEX_DEVICE", "never")
    seg.regexp_match_dictionary("v", "zq")
    assert seg.device_bytes() == before  # the host runner stages nothing
    monkeypatch.setenv("PINOT_AMD_REGEX_DEVICE", "always")
    seg.regexp_match_dictionary("v", "zq")
    first = seg.device_bytes()
    payload = sum(len(v.encode()) for v in vals) + 4 * (len(vals) + 1)
    assert first >= before + payload
    seg.regexp_match_dictionary("v", "a.c", True)
    assert seg.device_bytes() == first  # kept with the segment


# ------------------------------------------------------------------------------------------- (b) whole queries
WORDS = ["cart", "pay", "home", "search", "item", "café", "naïve", "login", "help", "Cart", "PAY"]


def draw_strings(rng, count, mode):
    """URL-like values; mode 'none': none holds "zq" in any case, 'all': every one does, 'some': about a third."""
    out = []
    for k in range(count):
        host = "abcd"[int(rng.integers(0, 4))]
        s = f"https://{host}{int(rng.integers(0, 30))}.example/{WORDS[int(rng.integers(0, len(WORDS)))]}{int(rng.integers(0, 50))}"
        if mode == "all" or (mode == "some" and rng.random() < 0.33):
            at = int(rng.integers(0, len(s) + 1))
            s = s[:at] + ["zq", "ZQ", "Zq"][int(rng.integers(0, 3))] + s[at:]
        out.append(s)
    return out


MODES = ["some", "none", "all"]


@pytest.fixture(scope="module")
def data(engine):
    rng = np.random.default_rng(515)
    out = []
    for i, mode in enumerate(MODES):
        n = 3000 - 7 * i
        url_pool = sorted(set(draw_strings(rng, 400, mode)))                     # > 64 values: a dictId set
        brand_pool = [f"b{c}a{k}" for c in "xyz" for k in range(5 + i)] + [f"B{'q' if i != 1 else 'w'}A-{i}"]
        srt_pool = sorted(set(f"s{k:02d}{'zq' if (mode == 'all' or (mode == 'some' and k % 3 == 0)) else ''}"
                              for k in range(40 + i)))
        inv_pool = sorted(set(draw_strings(rng, 100, mode)))
        tag_pool = sorted(set(draw_strings(rng, 90, mode)))
        raw_pool = sorted(set(draw_strings(rng, 150, mode)))
        strings = {
            "url": [url_pool[int(k)] for k in rng.integers(0, len(url_pool), n)],
            "brand": [brand_pool[int(k)] for k in rng.integers(0, len(brand_pool), n)],
            "srt": sorted(srt_pool[int(k)] for k in rng.integers(0, len(srt_pool), n)),
            "inv": [inv_pool[int(k)] for k in rng.integers(0, len(inv_pool), n)],
            "raw": [raw_pool[int(k)] for k in rng.integers(0, len(raw_pool), n)],
            "tags": [[tag_pool[int(k)] for k in rng.integers(0, len(tag_pool), int(rng.integers(1, 4)))] for _ in range(n)],
        }
        nums = {"n": rng.integers(0, 1000, n).astype(np.int32), "g": rng.integers(0, 8, n).astype(np.int32)}
        sv = {"n": (nums["n"], S.INT, {"dictionary": False}), "g": (nums["g"], S.INT, {"detect_sorted": False}),
              "url": (np.array(strings["url"], dtype=object), S.STRING, {"detect_sorted": False})}
        cols = dict(sv)
        cols["brand"] = (np.array(strings["brand"], dtype=object), S.STRING, {"detect_sorted": False})
        cols["srt"] = (np.array(strings["srt"], dtype=object), S.STRING, {})
        cols["inv"] = (np.array(strings["inv"], dtype=object), S.STRING, {"detect_sorted": False, "inverted": True})
        cols["raw"] = (np.array(strings["raw"], dtype=object), S.STRING, {"dictionary": False})
        cols["tags"] = (strings["tags"], S.STRING, {"multi_value": True})
        bufs = S.build_segment(f"rx{i}", cols)
        assert bufs.columns["srt"].is_sorted and bufs.columns["url"].cardinality > 64
        assert bufs.columns["brand"].cardinality <= 64 and not bufs.columns["raw"].has_dictionary
        out.append({"strings": strings, "nums": nums, "sv": sv, "bufs": bufs, "seg": engine.ImmutableSegment(bufs), "n": n})
    return out


_EXPECTED = {}


def expected(data, template):
    """(the library's query, the oracle's matched docs and groups for the rewritten query), computed once."""
    if template not in _EXPECTED:
        sql, sv_sql, leaves = R.rewrite(template)
        segs = [R.oracle_segment(f"o{i}", d["sv"], d["strings"], leaves) for i, d in enumerate(data)]
        nm, groups = oracle.execute(sv_sql, segs)
        _EXPECTED[template] = (sql, nm, groups)
    return _EXPECTED[template]


def run(engine, data, template, float_sums=()):
    sql, nm, exp = expected(data, template)
    res = engine.ServerQueryExecutor().execute(sql, [d["seg"] for d in data])
    try:
        assert res.num_docs_matched() == nm, sql
        assert_same_groups(res.groups(), exp, set(float_sums))
        return res.kernel_info()
    finally:
        res.destroy()


QUERIES = [
    "SELECT COUNT(*), SUM(n) FROM t WHERE {url LIKE '%zq%'} AND n BETWEEN 100 AND 800",          # set leaf AND a range
    "SELECT COUNT(*), MAX(n) FROM t WHERE {brand LIKE 'b_a%'} OR g IN (1, 5)",                    # accept masks OR an IN
    "SELECT COUNT(*), MAX(n) FROM t WHERE {brand LIKE 'bqa-_'} AND g < 7",                        # one value, one segment
    "SELECT COUNT(*), MIN(n) FROM t WHERE {url NOT LIKE '%zq%'}",
    "SELECT COUNT(*), SUM(n) FROM t WHERE NOT {REGEXP_LIKE(url, '/(cart|pay)[0-9]+$')} AND n > 10",
    "SELECT url, COUNT(*), SUM(n) FROM t WHERE {REGEXP_LIKE(url, '(cart|pay)[0-9]*$', 'i')} GROUP BY url",
    "SELECT url, COUNT(*) FROM t WHERE {url LIKE '%zq%'} GROUP BY url",
    "SELECT COUNT(*), SUM(n) FROM t WHERE {srt LIKE 's1%'}",                                      # sorted: a doc range
    "SELECT COUNT(*), SUM(n) FROM t WHERE {srt LIKE '%zq'} AND n < 700",                          # sorted: a dictId set
    "SELECT COUNT(*), SUM(n) FROM t WHERE {srt NOT LIKE 's0_'}",
    "SELECT COUNT(*), SUM(n) FROM t WHERE {raw LIKE '%zq%'} OR {raw LIKE 'https://b1%'}",         # raw STRING
    "SELECT g, COUNT(*) FROM t WHERE {REGEXP_LIKE(raw, 'na.ve[0-9]+$')} GROUP BY g",
    "SELECT COUNT(*), SUM(n) FROM t WHERE {tags LIKE '%zq%'}",                                    # MV: ANY
    "SELECT COUNT(*), SUM(n) FROM t WHERE {tags NOT LIKE '%zq%'} AND n < 900",                    # MV: NOT ANY
    "SELECT g, COUNT(*) FROM t WHERE NOT {REGEXP_LIKE(tags, '^https://[ab]')} OR {url LIKE '%CART%'} GROUP BY g",
]


@pytest.mark.parametrize("runner", ["always", "never"])
@pytest.mark.parametrize("template", QUERIES)
def test_queries(engine, data, template, runner, monkeypatch):
    monkeypatch.setenv("PINOT_AMD_REGEX_DEVICE", runner)
    run(engine, data, template)


@pytest.mark.parametrize("policy", ["always", "never"])
@pytest.mark.parametrize("template", [
    "SELECT COUNT(*), SUM(n) FROM t WHERE {inv LIKE '%zq%'} AND n < 500",
    "SELECT g, COUNT(*) FROM t WHERE {inv NOT LIKE 'https://c%'} GROUP BY g",
    "SELECT COUNT(*) FROM t WHERE {REGEXP_LIKE(inv, 'item[0-9]$')} OR {inv LIKE '%login1_'}",
])
def test_inverted_index_column(engine, data, template, policy, monkeypatch):
    monkeypatch.setenv("PINOT_AMD_INV_POLICY", policy)
    monkeypatch.setenv("PINOT_AMD_REGEX_DEVICE", "always")
    run(engine, data, template)


def _bits(s, leaf_text):
    return R.leaf_bits(list(s[R.leaf_of(leaf_text)[0]]), R.leaf_of(leaf_text)) == 1


# a pattern in a FILTER lane beside an unfiltered aggregation (the oracle reads no FILTER clause: filtered_aggs_ref does)
FILTERED = [
    ("SELECT COUNT(*), SUM(n) FILTER (WHERE url LIKE 'https://a%'), MAX(n) FILTER (WHERE url LIKE '%zq%' AND n < 900) "
     "FROM t WHERE n >= 5", lambda s: s["n"] >= 5,
     [None, lambda s: _bits(s, "url LIKE 'https://a%'"), lambda s: _bits(s, "url LIKE '%zq%'") & (s["n"] < 900)]),
    ("SELECT g, COUNT(*), SUM(n) FILTER (WHERE REGEXP_LIKE(url, 'caf.[0-9]')), MIN(n) FILTER (WHERE tags NOT LIKE '%zq%') "
     "FROM t WHERE NOT REGEXP_LIKE(url, 'help') GROUP BY g LIMIT 1000000", lambda s: ~_bits(s, "REGEXP_LIKE(url, 'help')"),
     [None, lambda s: _bits(s, "REGEXP_LIKE(url, 'caf.[0-9]')"), lambda s: _bits(s, "tags NOT LIKE '%zq%'")]),
]


@pytest.mark.parametrize("runner", ["always", "never"])
@pytest.mark.parametrize("case", range(len(FILTERED)))
def test_filter_lanes(engine, data, case, runner, monkeypatch):
    monkeypatch.setenv("PINOT_AMD_REGEX_DEVICE", runner)
    sql, main, lanes = FILTERED[case]
    qc = parse_sql(sql, pattern_predicates=True)
    arrays = [{"n": d["nums"]["n"], "g": d["nums"]["g"], "url": d["strings"]["url"], "tags": d["strings"]["tags"]} for d in data]
    exp, matched = filtered_aggs_ref.reference(qc, [{k: (v if k in ("url", "tags") else np.asarray(v)) for k, v in a.items()}
                                                    for a in arrays], main, lanes)
    res = engine.ServerQueryExecutor().execute(sql, [d["seg"] for d in data])
    try:
        assert res.num_docs_matched() == matched
        got = {canonical_key(k): [final_value(a.func, p, a.param) for a, p in zip(qc.aggregations, parts)]
               for k, parts in res.groups().items()}
        assert set(got) == set(exp)
        for k in exp:
            for a, x, y in zip(qc.aggregations, got[k], exp[k]):
                assert filtered_aggs_ref.same(x, y, a, False), (sql, k, a.text, x, y)
    finally:
        res.destroy()


def test_one_segment_matches_nothing_and_one_everything(engine, data):
    leaf = R.leaf_of("url LIKE '%zq%'")
    counts = [int(R.leaf_bits(d["strings"]["url"], leaf).sum()) for d in data]
    assert counts[1] == 0 and counts[2] == data[2]["n"] and 0 < counts[0] < data[0]["n"]


@pytest.mark.parametrize("runner", ["always", "never"])
def test_filter_doc_ids(engine, data, runner, monkeypatch):
    monkeypatch.setenv("PINOT_AMD_REGEX_DEVICE", runner)
    for where, cols in [("url LIKE '%zq%' AND n < 600", ["url"]), ("tags NOT LIKE '%zq%'", ["tags"]),
                        ("NOT REGEXP_LIKE(srt, '^s[12]') OR raw LIKE '%zq%'", ["srt", "raw"])]:
        got = engine.ServerQueryExecutor().filter_doc_ids(f"SELECT COUNT(*) FROM t WHERE {where}", [d["seg"] for d in data])
        for d, ids in zip(data, got):
            if cols == ["url"]:
                m = (R.leaf_bits(d["strings"]["url"], R.leaf_of("url LIKE '%zq%'")) == 1) & (d["nums"]["n"] < 600)
            elif cols == ["tags"]:
                m = R.leaf_bits(d["strings"]["tags"], R.leaf_of("tags NOT LIKE '%zq%'")) == 1
            else:
                m = (R.leaf_bits(d["strings"]["srt"], R.leaf_of("REGEXP_LIKE(srt, '^s[12]')")) == 0) | \
                    (R.leaf_bits(d["strings"]["raw"], R.leaf_of("raw LIKE '%zq%'")) == 1)
            assert np.array_equal(np.asarray(ids), np.nonzero(m)[0]), where


@pytest.mark.parametrize("runner", ["always", "never"])
def test_selection_order_by_limit(engine, data, runner, monkeypatch):
    monkeypatch.setenv("PINOT_AMD_REGEX_DEVICE", runner)
    tables = [{"url": np.array(d["strings"]["url"], dtype=object), "n": d["nums"]["n"]} for d in data]
    masks = [(R.leaf_bits(d["strings"]["url"], R.leaf_of("url LIKE '%zq%/%'")) == 1) & (d["nums"]["n"] > 20) for d in data]
    res = engine.ServerQueryExecutor().execute(
        "SELECT url, n FROM t WHERE url LIKE '%zq%/%' AND n > 20 ORDER BY n DESC, url LIMIT 7", [d["seg"] for d in data])
    try:
        rows, origins, matched = selection_ref.select(tables, masks, ["url", "n"], [("n", False), ("url", True)], 7)
        assert res.origins() == origins and selection_ref.same_rows(res.rows(), rows)
        assert res.num_docs_matched() == matched
    finally:
        res.destroy()


# ------------------------------------------------------------------------------------------- (c) identity
def test_two_patterns_of_one_shape_keep_their_own_plans(engine, data, monkeypatch):
    monkeypatch.setenv("PINOT_AMD_REGEX_DEVICE", "always")
    t1 = "SELECT g, COUNT(*), SUM(n) FROM t WHERE {url LIKE '%item1%'} GROUP BY g"
    t2 = "SELECT g, COUNT(*), SUM(n) FROM t WHERE {url LIKE '%item2%'} GROUP BY g"
    t3 = "SELECT g, COUNT(*), SUM(n) FROM t WHERE {REGEXP_LIKE(url, 'item2')} GROUP BY g"  # the same text, case-sensitive
    segs = [d["seg"] for d in data]
    ex = engine.ServerQueryExecutor()
    seen = {}
    for round_ in range(2):
        for t in (t1, t2, t3):
            sql, nm, exp = expected(data, t)
            res = ex.execute(sql, segs)
            assert ("plan_cache" in res.plan_timing()) == (round_ == 1), (t, round_, res.plan_timing())
            assert res.num_docs_matched() == nm
            assert_same_groups(res.groups(), exp)
            seen[t] = nm
            res.destroy()
    assert seen[t1] != seen[t2]  # the two patterns really select different docs


# ------------------------------------------------------------------------------------------- (d) errors
def _spec(engine, column, ptype, pattern):
    from pinot_amd._lib import PredicateSpec
    s = PredicateSpec()
    s.column = column
    s.type = ptype
    s.num_values = 1
    arr = (C.c_char_p * 1)(pattern)
    s.h_values_s = arr
    return s, arr


def test_refusals(engine, data):
    from pinot_amd._lib import PinotAmdError, lib
    L = lib()
    qh = C.c_void_p()
    assert L.pinot_amd_query_create(C.byref(qh)) == 0
    try:
        for pat, code, word in [(b"(?=a)b", EUNSUPPORTED, "look-ahead"), (b"\\bfoo", EUNSUPPORTED, "\\b"),
                                (b"(a)\\1", EUNSUPPORTED, "back-reference"), (b"a{5000}", EUNSUPPORTED, "pattern too complex"),
                                (b"(a", EINVAL, "unclosed group"), (b"a$b", EUNSUPPORTED, "'$'")]:
            s, keep = _spec(engine, b"url", 5, pat)
            assert L.pinot_amd_query_add_predicate(qh, 0, C.byref(s), 0) == code, pat
            assert word in L.pinot_amd_last_error().decode(), (pat, L.pinot_amd_last_error())
        s, keep = _spec(engine, b"url", 6, "é".encode())
        assert L.pinot_amd_query_add_predicate(qh, 0, C.byref(s), 0) == EUNSUPPORTED
        assert "non-ASCII" in L.pinot_amd_last_error().decode()
        s, keep = _spec(engine, b"url", 7, b"a")
        assert L.pinot_amd_query_add_predicate(qh, 0, C.byref(s), 0) == EINVAL  # no such predicate type
        s, keep = _spec(engine, b"url", 5, b"a")
        s.num_values = 2
        assert L.pinot_amd_query_add_predicate(qh, 0, C.byref(s), 0) == EINVAL
    finally:
        L.pinot_amd_query_destroy(qh)
    seg = data[0]["seg"]
    n = C.c_int64()
    # a column that is not STRING: EINVAL from the per-operator call and from a query through the ABI
    assert L.pinot_amd_segment_regexp_match_dictionary(seg.handle, b"g", b"1", 0, None, 0, C.byref(n)) == EINVAL
    assert "not STRING" in L.pinot_amd_last_error().decode()
    assert L.pinot_amd_segment_regexp_match_dictionary(seg.handle, b"url", b"(?i)x", 0, None, 0, C.byref(n)) == EUNSUPPORTED
    assert "inline flags" in L.pinot_amd_last_error().decode()
    assert L.pinot_amd_segment_regexp_match_dictionary(seg.handle, b"nope", b"x", 0, None, 0, C.byref(n)) == EINVAL
    qh = C.c_void_p()
    assert L.pinot_amd_query_create(C.byref(qh)) == 0
    try:
        s, keep = _spec(engine, b"g", 5, b"1")
        assert L.pinot_amd_query_add_predicate(qh, 0, C.byref(s), 0) == 0
        assert L.pinot_amd_query_add_aggregation(qh, 0, None, None) == 0
        arr = (C.c_void_p * 1)(seg.handle)
        rh = C.c_void_p()
        assert L.pinot_amd_execute(qh, arr, 1, None, C.byref(rh)) == EINVAL
        assert "not STRING" in L.pinot_amd_last_error().decode()
    finally:
        L.pinot_amd_query_destroy(qh)
    # Python: ValueError, with the construct named
    ex = engine.ServerQueryExecutor()
    with pytest.raises(ValueError, match="look-behind"):
        ex.execute("SELECT COUNT(*) FROM t WHERE REGEXP_LIKE(url, '(?<=a)b')", [seg])
    with pytest.raises(ValueError, match="non-ASCII"):
        ex.execute("SELECT COUNT(*) FROM t WHERE url LIKE '%é%'", [seg])
    with pytest.raises(ValueError, match="not STRING"):
        ex.execute("SELECT COUNT(*) FROM t WHERE g LIKE '1%'", [seg])
    res = ex.execute("SELECT COUNT(*) FROM t WHERE REGEXP_LIKE(url, 'é')", [seg])
    assert res.num_docs_matched() == sum("é" in u for u in data[0]["strings"]["url"])
    res.destroy()
