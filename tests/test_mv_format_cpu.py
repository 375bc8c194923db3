"""Multi-value columns on the host: FixedBitMVForwardIndexWriter's bytes both ways, segment directories with MV
columns, the *MV functions in the SQL front end. No GPU."""
import os

import numpy as np
import pytest

from pinot_amd import segment as S
from pinot_amd.query import MV_FUNCS, final_value, merge_partial, parse_sql

PINNED_DOCS = [[1, 2], [3], [2, 2, 5], [7], [1, 7]]
PINNED_FWD = bytes.fromhex("00000000B3000512E080")


def test_pinned_bytes_both_ways():
    c = S.build_column("c", PINNED_DOCS, S.INT, multi_value=True)
    assert c.multi_value and c.encoding == "FIXED_BIT_MV"
    assert c.dict_values.tolist() == [1, 2, 3, 5, 7] and c.cardinality == 5 and c.bits_per_element == 3
    assert (c.num_docs, c.total_values, c.max_values) == (5, 9, 3)
    assert c.fwd == PINNED_FWD
    ids = [[0, 1], [2], [1, 1, 3], [4], [0, 4]]
    assert S.mv_fwd_bytes(ids, 3) == PINNED_FWD
    off, got = S.unpack_mv_fwd(PINNED_FWD, 3, 5, 9)
    assert off.tolist() == [0, 2, 3, 6, 7, 9]
    assert [c.dict_values[got[off[d]:off[d + 1]]].tolist() for d in range(5)] == PINNED_DOCS


def random_lists(rng, num_docs, card, max_len):
    lens = rng.integers(1, max_len + 1, num_docs)
    return [rng.integers(0, card, n).tolist() for n in lens]


@pytest.mark.parametrize("bits,num_docs,max_len", [(1, 77, 5), (3, 1000, 8), (7, 513, 3), (17, 300, 9), (5, 3000, 3)])
def test_round_trip(bits, num_docs, max_len):
    rng = np.random.default_rng(bits * 1000 + num_docs)
    docs = random_lists(rng, num_docs, 1 << bits, max_len)
    total = sum(len(d) for d in docs)
    buf = S.mv_fwd_bytes(docs, bits)
    dpc = S.mv_docs_per_chunk(num_docs, total)
    chunks = (num_docs + dpc - 1) // dpc
    assert len(buf) == 4 * chunks + (total + 7) // 8 + (total * bits + 7) // 8
    if num_docs == 3000:
        assert chunks > 1  # 3000 docs of ~2 values: 1024 or 2048 docs per chunk
    off, ids = S.unpack_mv_fwd(buf, bits, num_docs, total)
    assert [ids[off[d]:off[d + 1]].tolist() for d in range(num_docs)] == docs
    # the header: where every docsPerChunk-th doc starts
    starts = np.r_[0, np.cumsum([len(d) for d in docs])[:-1]]
    assert np.frombuffer(buf, dtype=">i4", count=chunks).tolist() == starts[::dpc].tolist()


def test_docs_per_chunk_is_java_int_division():
    # 9 values / 5 docs = 1 in Java's int division: ceil(2048 / 1.0f) = 2048 docs per chunk, not ceil(2048 / 1.8) = 1138
    assert S.mv_docs_per_chunk(5, 9) == 2048
    assert S.mv_docs_per_chunk(3000, 5999) == 2048 and S.mv_docs_per_chunk(3000, 6000) == 1024
    assert S.mv_docs_per_chunk(10, 30) == 683  # ceil(682.67)
    docs = [[0]] * 1137 + [[0, 0]] * 1138  # 2275 docs, 3413 values: avg 1 -> one chunk of 2048 and a second one
    buf = S.mv_fwd_bytes(docs, 1)
    assert np.frombuffer(buf, dtype=">i4", count=2).tolist() == [0, 1137 + 2 * (2048 - 1137)]


def test_unpack_refuses_inconsistent_bytes():
    b = bytearray(PINNED_FWD)
    with pytest.raises(ValueError):
        S.unpack_mv_fwd(bytes(b), 3, 5, 17)          # a wrong value count: the sizes disagree
    b[4] &= 0xDF                                      # value 2 no longer starts a doc
    with pytest.raises(ValueError):
        S.unpack_mv_fwd(bytes(b), 3, 5, 9)
    b = bytearray(PINNED_FWD)
    b[3] = 1                                          # chunk 0 does not start at value 0
    with pytest.raises(ValueError):
        S.unpack_mv_fwd(bytes(b), 3, 5, 9)
    with pytest.raises(ValueError):
        S.mv_fwd_bytes([[1], []], 3)                  # every doc has at least one value


def _metadata(cols, num_docs):
    lines = [f"segment.total.docs = {num_docs}", "segment.name = mvseg"]
    for c in cols:
        lines += [f"column.{c.name}.dataType = {c.stored_type}", f"column.{c.name}.cardinality = {c.cardinality}",
                  f"column.{c.name}.bitsPerElement = {c.bits_per_element}", f"column.{c.name}.hasDictionary = true",
                  f"column.{c.name}.isSorted = false",
                  f"column.{c.name}.isSingleValues = {'false' if c.multi_value else 'true'}"]
        if c.multi_value:
            lines += [f"column.{c.name}.totalNumberOfEntries = {c.total_values}",
                      f"column.{c.name}.maxNumberOfMultiValues = {c.max_values}"]
    return "\n".join(lines) + "\n"


def _columns():
    return [S.build_column("c", PINNED_DOCS, S.INT, multi_value=True),
            S.build_column("s", [["x", "y"], ["y"], ["zz", "x", "x"], ["q"], ["y", "q"]], S.STRING, multi_value=True),
            S.build_column("g", np.array(list("aabba"), dtype=object), S.STRING, detect_sorted=False)]


def _check_loaded(seg):
    assert seg.num_docs == 5 and sorted(seg.columns) == ["c", "g", "s"]
    for want in _columns():
        got = seg.columns[want.name]
        assert (got.multi_value, got.total_values, got.max_values) == (want.multi_value, want.total_values, want.max_values)
        assert (got.fwd, got.dictionary, got.cardinality, got.bits_per_element, got.stored_type) == \
               (want.fwd, want.dictionary, want.cardinality, want.bits_per_element, want.stored_type)
        assert got.encoding == want.encoding
    assert seg.columns["c"].fwd == PINNED_FWD
    assert seg.columns["s"].dict_values.tolist() == ["q", "x", "y", "zz"]


def test_load_segment_dir_v1(tmp_path):
    cols = _columns()
    (tmp_path / "metadata.properties").write_text(_metadata(cols, 5))
    for c in cols:
        (tmp_path / (c.name + ".dict")).write_bytes(c.dictionary)
        (tmp_path / (c.name + (".mv.fwd" if c.multi_value else ".sv.unsorted.fwd"))).write_bytes(c.fwd)
    _check_loaded(S.load_segment_dir(str(tmp_path)))


def test_load_segment_dir_v3(tmp_path):
    cols = _columns()
    v3 = tmp_path / "v3"
    v3.mkdir()
    (v3 / "metadata.properties").write_text(_metadata(cols, 5))
    psf, index_map = bytearray(), []
    marker = S.V3_MAGIC_MARKER.to_bytes(8, "big")
    for c in cols:
        for index, data in (("dictionary", c.dictionary), ("forward_index", c.fwd)):
            index_map += [f"{c.name}.{index}.startOffset = {len(psf)}", f"{c.name}.{index}.size = {len(data) + 8}"]
            psf += marker + data
    (v3 / "index_map").write_text("\n".join(index_map) + "\n")
    (v3 / "columns.psf").write_bytes(bytes(psf))
    _check_loaded(S.load_segment_dir(str(tmp_path)))


def test_raw_mv_column_is_refused(tmp_path):
    (tmp_path / "metadata.properties").write_text(
        "segment.total.docs = 1\ncolumn.r.dataType = INT\ncolumn.r.hasDictionary = false\n"
        "column.r.isSingleValues = false\ncolumn.r.totalNumberOfEntries = 1\ncolumn.r.maxNumberOfMultiValues = 1\n")
    with pytest.raises(NotImplementedError):
        S.load_segment_dir(str(tmp_path))
    with pytest.raises(NotImplementedError):
        S.build_column("r", [[1]], S.INT, dictionary=False, multi_value=True)


SPELLINGS = {"COUNTMV": ["COUNTMV", "countmv", "Count_MV", "COUNT_MV"], "SUMMV": ["SUMMV", "sum_mv", "SumMV"],
             "MINMV": ["MINMV", "min_mv"], "MAXMV": ["MAXMV", "Max_Mv"], "AVGMV": ["AVGMV", "avg_mv"],
             "MINMAXRANGEMV": ["MINMAXRANGEMV", "minMaxRangeMV", "MIN_MAX_RANGE_MV"]}


def test_parse_every_spelling():
    assert set(SPELLINGS) == set(MV_FUNCS)
    for func, words in SPELLINGS.items():
        for w in words:
            qc = parse_sql(f"SELECT {w}(c) FROM t WHERE c IN (1, 3) GROUP BY g")
            (a,) = qc.aggregations
            assert (a.func, a.column, a.alias, a.filter) == (func, "c", None, None)
            assert a.name == f"{func.lower()}(c)"      # the result column name: lower-case function name and (x)


def test_parse_filter_alias_and_order_by():
    qc = parse_sql("SELECT g, SUM_MV(c) FILTER (WHERE c = 2) AS s2, countmv(c) n, AVGMV(c) FROM t WHERE c != 7 "
                   "GROUP BY g ORDER BY summv(c) FILTER(WHERE c = '2') DESC, n LIMIT 3")
    s2, n, avg = qc.aggregations
    assert (s2.func, s2.alias, s2.name) == ("SUMMV", "s2", "s2")
    assert s2.text == "summv(c) FILTER(WHERE c = '2')" and s2.filter.predicate.values == (2,)
    assert (n.func, n.name, n.text) == ("COUNTMV", "n", "countmv(c)")
    assert (avg.func, avg.name) == ("AVGMV", "avgmv(c)")
    assert qc.order_by_targets() == [(1, 0, False), (1, 1, True)]
    assert qc.filter.predicate.type == "NOT_EQ"     # predicates on MV columns need no new syntax


def test_partials_merge_and_finalise():
    assert merge_partial("COUNTMV", 5, 4) == 9 and merge_partial("SUMMV", 14.0, 16.0) == 30.0
    assert merge_partial("MINMV", 1.0, 2.0) == 1.0 and merge_partial("MAXMV", 7.0, 5.0) == 7.0
    assert merge_partial("AVGMV", (14.0, 5), (16.0, 4)) == (30.0, 9)
    assert final_value("AVGMV", (30.0, 9)) == 30.0 / 9 and final_value("AVGMV", (0.0, 0)) == float("-inf")
    assert merge_partial("MINMAXRANGEMV", (1.0, 7.0), (2.0, 7.0)) == (1.0, 7.0)
    assert final_value("MINMAXRANGEMV", (1.0, 7.0)) == 6.0
    assert final_value("MINMAXRANGEMV", (float("inf"), float("-inf"))) == float("-inf")
    assert final_value("COUNTMV", 9) == 9 and final_value("MINMV", float("inf")) == float("inf")
