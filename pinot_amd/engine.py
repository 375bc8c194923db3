"""Host-side mirror of pinot-core's server query execution for the HBM-resident hot path.

Class names follow the reference so that tests and callers read like Pinot:

* :class:`ImmutableSegment` — ``ImmutableSegmentLoader.load`` (pinot-segment-local/.../loader/
  ImmutableSegmentLoader.java): stages a segment's column buffers into HBM through
  ``pinot_amd_segment_add_column``.
* :class:`ServerQueryExecutor` — ``ServerQueryExecutorV1Impl.execute`` -> ``InstancePlanMakerImplV2``
  plan -> per-segment ``AggregationOperator`` / ``GroupByOperator`` -> ``*CombineOperator``
  (pinot-core/.../query/executor/ServerQueryExecutorV1Impl.java). All segments of the call are
  executed in one batched device pass.
* :class:`QueryResult` — ``AggregationGroupByResult`` / ``IntermediateResultsBlock``: per group the
  intermediate results of every aggregation (AVG as (sum, count)), mergeable across servers.
* :class:`SelectionResult` — ``SelectionResultsBlock``: the server's offset + limit rows of a selection query
  (``SelectionOnlyOperator`` / ``SelectionOrderByOperator`` -> ``SelectionOrderByCombineOperator``).

Every computation goes through libpinot_amd.so; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import gc
import math
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import ColumnSpec, KeyTransformSpec, PredicateSpec, XNode, check, lib
from .query import (KEY_TRANSFORMS, MV_FUNCS, TIME_UNITS, TRUNC_UNITS, VALUE_SET_FUNCS, DistinctSize, FinalValue, JavaDouble,
                    QueryContext, expr_columns, expr_postfix, expression, filter_text, fold_distinct_count,
                    hists_from_csr, key_transform, parse_sql, reduce_rows, server_table, sets_from_csr,
                    split_distinct_count, to_cnf)
from .segment import ColumnBuffers, SegmentBuffers, DOUBLE, FLOAT, INT, LONG, STRING

TYPE_CODE = {INT: 0, LONG: 1, FLOAT: 2, DOUBLE: 3, STRING: 4}
ENC_CODE = {"FIXED_BIT": 0, "RAW": 1, "SORTED": 2, "FIXED_BIT_MV": 3}
PRED_CODE = {"EQ": 0, "NOT_EQ": 1, "IN": 2, "NOT_IN": 3, "RANGE": 4, "REGEXP_LIKE": 5}  # (6: REGEXP_LIKE, 'i')
AGG_CODE = {"COUNT": 0, "SUM": 1, "MIN": 2, "MAX": 3, "SUMLONG": 4, "AVG": 5, "MINMAXRANGE": 6,
            "DISTINCTCOUNT": 7, "PERCENTILE": 8, "DISTINCTSUM": 9, "DISTINCTAVG": 10, "DISTINCTCOUNTHLL": 17,
            "COUNTMV": 11, "SUMMV": 12, "MINMV": 13, "MAXMV": 14, "AVGMV": 15, "MINMAXRANGEMV": 16}
EXPR_CODE = {"MUL": 1, "SUB": 2, "ADD": 3}


def key_transform_spec(kt) -> KeyTransformSpec:
    """pinot_amd_key_transform_spec of a query.KeyTransform."""
    s = KeyTransformSpec()
    s.kind = KEY_TRANSFORMS.index(kt.kind)
    s.trunc_unit = TRUNC_UNITS.index(kt.trunc_unit) if kt.trunc_unit else 0
    s.in_unit, s.in_size = TIME_UNITS.index(kt.in_unit), kt.in_size
    s.out_unit, s.out_size = TIME_UNITS.index(kt.out_unit), kt.out_size
    s.gran_unit, s.gran_size = (TIME_UNITS.index(kt.gran_unit) if kt.gran_unit else 0), kt.gran_size
    return s


def _stream_handle(stream) -> Optional[int]:
    if stream is None:
        return None
    return int(getattr(stream, "cuda_stream", stream))


class ImmutableSegment:
    """A segment whose forward indexes, dictionaries and inverted indexes live in HBM."""

    def __init__(self, buffers: SegmentBuffers):
        L = lib()
        self.name = buffers.name
        self.num_docs = buffers.num_docs
        self.columns: Dict[str, ColumnBuffers] = {}
        h = C.c_void_p()
        check(L.pinot_amd_segment_create(buffers.name.encode(), buffers.num_docs, C.byref(h)), "segment_create")
        self._h = h
        for cb in buffers.columns.values():
            self.add_column(cb)

    def add_column(self, cb: ColumnBuffers) -> None:
        spec = ColumnSpec()
        spec.name = cb.name.encode()
        spec.stored_type = TYPE_CODE[cb.stored_type]
        spec.encoding = ENC_CODE[cb.encoding]
        spec.cardinality = cb.cardinality
        spec.bits_per_element = cb.bits_per_element
        keep = [cb.fwd, cb.dictionary, cb.inverted]
        spec.h_fwd = C.cast(C.c_char_p(cb.fwd), C.c_void_p)
        spec.fwd_size = len(cb.fwd)
        if cb.dictionary:
            spec.h_dictionary = C.cast(C.c_char_p(cb.dictionary), C.c_void_p)
            spec.dictionary_size = len(cb.dictionary)
        if cb.inverted:
            spec.h_inverted = C.cast(C.c_char_p(cb.inverted), C.c_void_p)
            spec.inverted_size = len(cb.inverted)
        if cb.multi_value:  # the whole FixedBitMVForwardIndexWriter file, validated on the device
            check(lib().pinot_amd_segment_add_mv_column(self._h, C.byref(spec), cb.total_values, cb.max_values),
                  f"add_mv_column({cb.name})")
        else:
            check(lib().pinot_amd_segment_add_column(self._h, C.byref(spec)), f"add_column({cb.name})")
        del keep
        self.columns[cb.name] = cb

    def mv_info(self, column: str):
        """(totalNumberOfEntries, maxNumberOfMultiValues) of a multi-value column, None for a single-value one."""
        total, mx = C.c_int64(), C.c_int32()
        rc = lib().pinot_amd_segment_column_mv_info(self._h, column.encode(), C.byref(total), C.byref(mx))
        if rc < 0:
            raise KeyError(column)
        return (total.value, mx.value) if rc else None

    @property
    def handle(self):
        return self._h

    def device_bytes(self) -> int:
        return int(lib().pinot_amd_segment_device_bytes(self._h))

    def packed_info(self, column: str):
        """The column's packed twin as {'lo_bits', 'hi_bits', 'base', 'bytes'}, or None without one."""
        lo, hi, base, nbytes = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        rc = lib().pinot_amd_segment_column_packed_info(self._h, column.encode(), C.byref(lo), C.byref(hi),
                                                        C.byref(base), C.byref(nbytes))
        if rc < 0:
            raise KeyError(column)
        if rc == 0:
            return None
        return {"lo_bits": lo.value, "hi_bits": hi.value, "base": base.value, "bytes": nbytes.value}

    def regexp_match_dictionary(self, column: str, pattern: str, case_insensitive: bool = False) -> np.ndarray:
        """DictIdBasedRegexpLikePredicateEvaluator: a bool per dictId of a STRING column, True where the pattern finds
        a match in the value (the runner PINOT_AMD_REGEX_DEVICE selects)."""
        card = self.columns[column].cardinality
        words = np.zeros((card + 31) // 32 + 1, dtype=np.uint32)
        n = C.c_int64()
        check(lib().pinot_amd_segment_regexp_match_dictionary(
            self._h, column.encode(), pattern.encode(), 1 if case_insensitive else 0,
            words.ctypes.data_as(C.POINTER(C.c_uint32)), len(words), C.byref(n)), f"regexp_match_dictionary({column})")
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:card].astype(bool)
        assert int(bits.sum()) == n.value
        return bits

    def column_fwd_ptr(self, column: str) -> int:
        p = lib().pinot_amd_segment_column_fwd(self._h, column.encode())
        if not p:
            raise KeyError(column)
        return int(p)

    def destroy(self) -> None:
        if self._h:
            lib().pinot_amd_segment_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.destroy()
        except Exception:
            pass


def _coerce(value, stored_type: str):
    if stored_type == STRING:
        return str(value)
    if stored_type in (INT, LONG):
        if isinstance(value, float):
            if not value.is_integer():
                raise ValueError(f"non-integral literal {value} for {stored_type} column")
            value = int(value)
        if isinstance(value, str):
            value = int(value)
        return int(value)
    return float(value)


class _ExprColumn:
    """What the engine reads of a column, for an expression's virtual column: a single-value DOUBLE without indexes."""
    stored_type = DOUBLE
    inverted = None
    multi_value = False

    def __init__(self, name: str):
        self.name = name


class _QueryNames:
    """The columns of one library query by the names its calls take: a plain column is itself, an arithmetic
    expression (query.expression) is defined once per query (pinot_amd_query_define_expression) and stands under the
    name the library returned."""

    def __init__(self, qh, first: ImmutableSegment):
        self._qh, self._first, self._defined = qh, first, {}

    def column(self, text: str):
        """The column's buffers (an _ExprColumn for an expression), None when the segment has no such column."""
        e = expression(text)
        if e is None:
            return self._first.columns.get(text)
        for c in expr_columns(e):
            if c not in self._first.columns:
                raise _lib.PinotAmdError(f"unknown column {c!r} in segment {self._first.name} (expression {text})")
        return _ExprColumn(text)

    def abi(self, text: str) -> bytes:
        e = expression(text)
        if e is None:
            return text.encode()
        name = self._defined.get(text)
        if name is None:
            rows = expr_postfix(e)
            nodes = (XNode * len(rows))()
            for n, (kind, nargs, col, lit) in zip(nodes, rows):
                n.kind, n.num_args, n.column, n.literal = kind, nargs, (col.encode() if col is not None else None), lit
            out = C.c_char_p()
            check(lib().pinot_amd_query_define_expression(self._qh, nodes, len(rows), C.byref(out)),
                  f"define_expression({text})")
            name = self._defined[text] = out.value
        return name


def _predicate_spec(pred, column, use_inverted: bool, keep: list, abi_name: Optional[bytes] = None) -> PredicateSpec:
    s = PredicateSpec()
    s.column = abi_name if abi_name is not None else pred.column.encode()
    keep.append(s.column)
    s.type = PRED_CODE[pred.type]
    st = column.stored_type
    if pred.type == "REGEXP_LIKE":
        # the pattern is h_values_s[0]; a refused pattern or a column that is not STRING is the caller's error
        if pred.case_insensitive:
            s.type += 1
        if st != STRING:
            raise ValueError(f"regexp_like on column {pred.column}, which is {st}, not STRING")
        pat = pred.values[0].encode()
        if lib().pinot_amd_regexp_check(pat, 1 if pred.case_insensitive else 0) != 0:
            raise ValueError(lib().pinot_amd_last_error().decode(errors="replace"))
        s.use_inverted_index = 1 if (use_inverted and column.inverted is not None) else 0
        s.num_values = 1
        arr = (C.c_char_p * 1)(pat)
        keep.append(arr)
        s.h_values_s = arr
        return s
    s.use_inverted_index = 1 if (use_inverted and column.inverted is not None and pred.type != "RANGE") else 0
    if pred.type == "RANGE":
        s.lower_unbounded = 1 if pred.lower is None else 0
        s.upper_unbounded = 1 if pred.upper is None else 0
        s.lower_inclusive = 1 if pred.lower_inclusive else 0
        s.upper_inclusive = 1 if pred.upper_inclusive else 0
        for side in ("lower", "upper"):
            v = getattr(pred, side)
            if v is None:
                continue
            v = _coerce(v, st)
            if st == STRING:
                b = v.encode()
                keep.append(b)
                setattr(s, side + "_s", b)
            elif st in (INT, LONG):
                setattr(s, side + "_i", v)
            else:
                setattr(s, side + "_d", v)
        return s
    s.num_values = len(pred.values)
    if st == STRING:
        vals = [_coerce(v, st) for v in pred.values]
        arr = (C.c_char_p * len(vals))(*[v.encode() for v in vals])
        keep.append(arr)
        s.h_values_s = arr
    elif st in (INT, LONG):
        # numpy buffers handed over by pointer: a ctypes array built element by element cost ~0.5 us per literal
        if all(type(v) is int for v in pred.values):
            arr = np.asarray(pred.values, dtype=np.int64)
        else:
            arr = np.asarray([_coerce(v, st) for v in pred.values], dtype=np.int64)
        keep.append(arr)
        s.h_values_i = arr.ctypes.data_as(C.POINTER(C.c_int64))
    else:
        arr = np.asarray([_coerce(v, st) for v in pred.values], dtype=np.float64)
        keep.append(arr)
        s.h_values_d = arr.ctypes.data_as(C.POINTER(C.c_double))
    return s


class DistinctCountResult:
    """Result of a query with DISTINCTCOUNT / PERCENTILE / DISTINCTSUM / DISTINCTAVG aggregations
    (query.split_distinct_count): the base result plus one grouped result per such column, folded into per-group
    value sets and histograms."""

    def __init__(self, qc, base, subs, server_trim: bool = False, column_types=None):
        self.qc, self._base, self._subs = qc, base, subs
        self._column_types = column_types  # column -> stored type (DISTINCTCOUNTHLL hashes by it)
        self._server_trim = server_trim  # the server's combine table over the folded groups

    def num_docs_matched(self) -> int:
        return self._base.num_docs_matched()

    def num_groups_limit_reached(self) -> bool:
        return self._base.num_groups_limit_reached()

    def kernel_info(self) -> str:
        return self._base.kernel_info()

    def _all(self):
        return [self._base] + [r for _, r in self._subs]

    def groups(self):
        g = fold_distinct_count(self.qc, self._base.groups(), [(i, r.groups()) for i, r in self._subs],
                                self._column_types)
        return server_table(self.qc, g) if self._server_trim else g

    def rows(self):
        return reduce_rows(self.qc, self.groups())

    def execute_again(self, stream=None) -> None:
        for r in self._all():
            r.execute_again(stream)

    def last_kernel_ms(self) -> float:
        return sum(r.last_kernel_ms() for r in self._all())

    def algorithmic_bytes(self) -> float:
        return sum(r.algorithmic_bytes() for r in self._all())

    def accumulators(self):
        raise NotImplementedError("DISTINCTCOUNT results merge by value (dist.merge_result merges each of "
                                  "results() with export_groups / merge_groups), not as one accumulator table")

    def results(self):
        """The device results this one folds: the base query, then one per DISTINCTCOUNT (each a GROUP BY
        whose groups are (group key, distinct value) pairs: merged by value across ranks, they union the
        value sets)."""
        return self._all()

    def destroy(self) -> None:
        for r in self._all():
            r.destroy()


class _DeviceWord:
    """One library-owned int64 in HBM seen by torch without a copy (__cuda_array_interface__)."""

    def __init__(self, ptr: int):
        self.__cuda_array_interface__ = {"shape": (1,), "typestr": "<i8", "data": (ptr, False), "version": 2,
                                         "strides": None}


def selfcheck_failures() -> int:
    """Executions of this process whose partitioned self-check failed (pinot_amd_selfcheck_failures)."""
    return int(lib().pinot_amd_selfcheck_failures())


class QueryResult:
    """Results of one executed query plan (kept in HBM until fetched)."""

    def __init__(self, handle, qc: QueryContext, agg_slots: List[tuple], key_types: List[str]):
        self._h = handle
        self.qc = qc
        # per qc aggregation: ('direct', native_idx) | ('avg', sum_idx, count_idx) | ('range', native_idx) |
        # ('distinct', native_idx, stored type of the column): DISTINCTCOUNT executed by the library |
        # ('hist', ...) PERCENTILE | ('dset', ...) DISTINCTSUM / DISTINCTAVG, likewise |
        # ('avgmv', native_idx): AVGMV's AvgPair (sum of values, count of values) from fetch_intermediate
        self._agg_slots = agg_slots
        self._key_types = key_types
        self._merged_reached = None      # numGroupsLimitReached OR-ed over ranks by dist.merge_result

    def execute_again(self, stream=None) -> None:
        self._merged_reached = None
        check(lib().pinot_amd_execute_again(self._h, _stream_handle(stream)), "execute_again")

    def set_merged_limit_reached(self, reached: bool) -> None:
        """The broker ORs numGroupsLimitReached over servers (BrokerReduceService): after a cross-rank
        merge every rank reports the OR of all ranks' flags, until the next execution."""
        self._merged_reached = bool(reached)

    def num_docs_matched(self) -> int:
        out = C.c_int64()
        check(lib().pinot_amd_result_num_docs_matched(self._h, C.byref(out)), "num_docs_matched")
        return out.value

    def num_groups_limit_reached(self) -> bool:
        """GroupByResultsBlock.isNumGroupsLimitReached: more groups than the numGroupsLimit option (after
        dist.merge_result: the OR over every rank's)."""
        if self._merged_reached is not None:
            return self._merged_reached
        out = C.c_int32()
        check(lib().pinot_amd_result_num_groups_limit_reached(self._h, C.byref(out)), "num_groups_limit_reached")
        return bool(out.value)

    def kernel_info(self) -> str:
        """The device plan: 'jit' (fused scan), 'jit-select' / 'jit-wselect' (selection vector; the
        filter on 4-doc tiles / 64-doc bitset words), 'jit-partitioned', 'jit-hash', 'jit-hash-trim';
        ' xN' when the batch ran as N shape launches; ' +lanes(n) table=regs|lds|cu|hbm|hash|hash+lds' for a query
        with filtered aggregations: its n filter lanes and the table its scan aggregates into."""
        return lib().pinot_amd_result_kernel_info(self._h).decode()

    def packed_info(self) -> str:
        """Raw columns the plan streamed through their packed twins: 'column:lo+hi' (plane bits per doc) per
        shape launch, ';' between launches, '' when none."""
        return lib().pinot_amd_result_packed_info(self._h).decode()

    def last_kernel_ms(self) -> float:
        out = C.c_double()
        check(lib().pinot_amd_result_last_kernel_ms(self._h, C.byref(out)), "last_kernel_ms")
        return out.value

    def plan_timing(self) -> Dict[str, float]:
        """Host planning milliseconds per phase of the execute that built this result."""
        txt = lib().pinot_amd_result_plan_timing(self._h).decode()
        return {k: float(v) for k, v in (kv.split("=") for kv in txt.split(";") if kv)}

    def algorithmic_bytes(self) -> float:
        """Algorithmic HBM bytes of the last execution (pinot_amd_result_algorithmic_bytes)."""
        out = C.c_double()
        check(lib().pinot_amd_result_algorithmic_bytes(self._h, C.byref(out)), "algorithmic_bytes")
        return out.value

    def accumulators(self):
        """(ops, num_keys, [device pointers]) of the dense accumulators for a cross-GPU merge."""
        n = C.c_int32()
        nk = C.c_int64()
        check(lib().pinot_amd_result_accumulators(self._h, C.byref(n), C.byref(nk), None, None), "accumulators")
        ptrs = (C.c_void_p * n.value)()
        ops = (C.c_int32 * n.value)()
        check(lib().pinot_amd_result_accumulators(self._h, C.byref(n), C.byref(nk), ptrs, ops), "accumulators")
        return list(ops), nk.value, [int(p) for p in ptrs]

    def check_word(self) -> int:
        """Device address of the execution's self-check word (one int64, 0 = the check held; see
        pinot_amd_result_check_word): a cross-rank merge carries it through its collectives."""
        out = C.c_void_p()
        check(lib().pinot_amd_result_check_word(self._h, C.byref(out)), "check_word")
        return int(out.value)

    def self_check_failed(self) -> bool:
        """Whether the last execution's self-check failed (reads the word without raising: the ranks of a
        merge agree on it before anyone fails)."""
        import torch
        w = torch.as_tensor(_DeviceWord(self.check_word()), device="cuda")
        return bool(int(w.item()) != 0)

    def has_dense_table(self) -> bool:
        """True when the groups live in a dense accumulator table over the key space (mergeable in place
        across ranks with all-reduces); False for hash-table plans and merged results."""
        n = C.c_int32()
        nk = C.c_int64()
        return lib().pinot_amd_result_accumulators(self._h, C.byref(n), C.byref(nk), None, None) == 0

    def export_groups(self, stream=None):
        """This result's groups as device tensors for a cross-rank merge by value
        (pinot_amd_result_export_groups): keys [groups, key_words] and accumulator words [groups, num_acc],
        int64, written on `stream` (synchronised before returning)."""
        import torch
        L = lib()
        kw, na, ng = C.c_int32(), C.c_int32(), C.c_int64()
        sh = _stream_handle(stream)
        check(L.pinot_amd_result_export_groups(self._h, None, None, 0, C.byref(kw), C.byref(na), C.byref(ng), sh),
              "export_groups")
        keys = torch.empty((ng.value, kw.value), dtype=torch.int64, device="cuda")
        acc = torch.empty((ng.value, na.value), dtype=torch.int64, device="cuda")
        if ng.value:
            torch.cuda.current_stream().synchronize()  # the allocations are ordered on torch's stream
            check(L.pinot_amd_result_export_groups(self._h, keys.data_ptr(), acc.data_ptr(), ng.value, C.byref(kw),
                                                   C.byref(na), C.byref(ng), sh), "export_groups")
        return keys, acc

    def merge_groups(self, keys, acc, stream=None) -> None:
        """Fold gathered (keys, acc) rows of every rank into this result (pinot_amd_result_merge_groups):
        until the next execution, groups() are the merged groups. The tensors must be ready on `stream`."""
        assert keys.is_contiguous() and acc.is_contiguous() and keys.shape[0] == acc.shape[0]
        check(lib().pinot_amd_result_merge_groups(self._h, keys.data_ptr(), acc.data_ptr(), keys.shape[0],
                                                  _stream_handle(stream)), "merge_groups")

    def fetch_arrays(self):
        """The groups as flat arrays straight from the library (pinot_amd_result_fetch): (number of groups,
        keys [g * num_group_by + j], final values as double [g * num_aggs + a], exact int64 values, MINMAXRANGE
        pairs or None). groups() turns them into Python values."""
        L = lib()
        ng = C.c_int64()
        check(L.pinot_amd_result_num_groups(self._h, C.byref(ng)), "num_groups")
        n = max(ng.value, 1)
        nk = len(self.qc.group_by)
        nnat = max(len(self._native_aggs), 1)
        keys = np.zeros(n * max(nk, 1), dtype=np.int64)
        vals = np.zeros(n * nnat, dtype=np.float64)
        vals_i = np.zeros(n * nnat, dtype=np.int64)
        got = C.c_int64()
        check(L.pinot_amd_result_fetch(self._h, n, keys.ctypes.data_as(C.POINTER(C.c_int64)),
                                       vals.ctypes.data_as(C.POINTER(C.c_double)),
                                       vals_i.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(got)), "fetch")
        pairs = None
        if any(s[0] in ("range", "avgmv") for s in self._agg_slots):
            pairs = np.zeros(n * nnat * 2, dtype=np.float64)
            got2 = C.c_int64()
            check(L.pinot_amd_result_fetch_intermediate(self._h, n, pairs.ctypes.data_as(C.POINTER(C.c_double)),
                                                        C.byref(got2)), "fetch_intermediate")
        return got, keys, vals, vals_i, pairs

    def distinct_sets(self, native_idx: int, stored_type: str, num_groups: int) -> List[frozenset]:
        """The value sets of library aggregation `native_idx` (a DISTINCTCOUNT), one frozenset per group in fetch
        order (pinot_amd_result_fetch_distinct_values -> query.sets_from_csr)."""
        L = lib()
        total = C.c_int64()
        check(L.pinot_amd_result_fetch_distinct_values(self._h, native_idx, 0, None, None, C.byref(total)),
              "fetch_distinct_values")
        off = np.zeros(num_groups + 1, dtype=np.int64)
        vals = np.zeros(max(total.value, 1), dtype=np.int64)
        check(L.pinot_amd_result_fetch_distinct_values(self._h, native_idx, total.value,
                                                       off.ctypes.data_as(C.POINTER(C.c_int64)),
                                                       vals.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(total)),
              "fetch_distinct_values")
        vals = vals[:total.value]
        strings = None
        if stored_type == STRING:
            strings = {int(i): L.pinot_amd_result_distinct_string(self._h, native_idx, int(i)).decode()
                       for i in np.unique(vals)}
        return sets_from_csr(off, vals, stored_type, strings)

    def hll_registers(self, native_idx: int, num_groups: int) -> List[tuple]:
        """The sketches of library aggregation `native_idx` (a DISTINCTCOUNTHLL), one (log2m, registers bytes) per
        group in fetch order (pinot_amd_result_fetch_hll)."""
        L = lib()
        log2m, ng = C.c_int32(), C.c_int64()
        check(L.pinot_amd_result_fetch_hll(self._h, native_idx, 0, None, C.byref(log2m), C.byref(ng)), "fetch_hll")
        m = 1 << log2m.value
        buf = np.zeros(max(ng.value * m, 1), dtype=np.uint8)
        check(L.pinot_amd_result_fetch_hll(self._h, native_idx, buf.size, buf.ctypes.data, C.byref(log2m), C.byref(ng)),
              "fetch_hll")
        if ng.value != num_groups:
            raise _lib.PinotAmdError(f"fetch_hll: {ng.value} groups, fetch returned {num_groups}")
        raw = buf.tobytes()
        return [(log2m.value, raw[g * m:(g + 1) * m]) for g in range(num_groups)]

    def value_hists(self, native_idx: int, stored_type: str, num_groups: int) -> List[dict]:
        """The histograms of library aggregation `native_idx` (a PERCENTILE), one dict distinct_value -> matching
        docs per group in fetch order (pinot_amd_result_fetch_value_counts -> query.hists_from_csr)."""
        L = lib()
        total = C.c_int64()
        check(L.pinot_amd_result_fetch_value_counts(self._h, native_idx, 0, None, None, None, C.byref(total)),
              "fetch_value_counts")
        off = np.zeros(num_groups + 1, dtype=np.int64)
        vals = np.zeros(max(total.value, 1), dtype=np.int64)
        cnts = np.zeros(max(total.value, 1), dtype=np.int64)
        p64 = C.POINTER(C.c_int64)
        check(L.pinot_amd_result_fetch_value_counts(self._h, native_idx, total.value, off.ctypes.data_as(p64),
                                                    vals.ctypes.data_as(p64), cnts.ctypes.data_as(p64),
                                                    C.byref(total)), "fetch_value_counts")
        return hists_from_csr(off, vals[:total.value], cnts[:total.value], stored_type)

    def groups(self, arrays=None, distinct_sizes: bool = False) -> Dict[tuple, list]:
        """key tuple (group-by values; () for aggregation-only) -> intermediate result per aggregation.
        Converted column-wise (numpy -> Python lists, zipped), not group by group. `arrays`: the output of
        an earlier fetch_arrays() of this execution (not fetched again). distinct_sizes: a library-executed
        DISTINCTCOUNT's partial is only its size (query.DistinctSize, from the fetch) instead of the value set, a
        PERCENTILE's / DISTINCTSUM's / DISTINCTAVG's only its final value (query.FinalValue)."""
        L = lib()
        got, keys, vals, vals_i, pairs = self.fetch_arrays() if arrays is None else arrays
        n = got.value
        nk = len(self.qc.group_by)
        nnat = max(len(self._native_aggs), 1)
        kcols = []
        if nk:
            karr = keys[:n * nk].reshape(n, nk)
            for j in range(nk):
                t = self._key_types[j]
                col = karr[:, j]
                if t == STRING:
                    names = {int(i): L.pinot_amd_result_string_key(self._h, j, int(i)).decode() for i in np.unique(col)}
                    kcols.append([names[i] for i in col.tolist()])
                elif t in (FLOAT, DOUBLE):
                    kcols.append([JavaDouble(x) for x in col.view(np.float64).tolist()])
                else:
                    kcols.append(col.tolist())
            key_tuples = list(zip(*kcols))
        else:
            key_tuples = [()] * n
        v = vals[:n * nnat].reshape(n, nnat)
        vi = vals_i[:n * nnat].reshape(n, nnat)
        acols = []
        for a, slot in zip(self.qc.aggregations, self._agg_slots):
            if slot[0] == "avg":
                acols.append(list(zip(v[:, slot[1]].tolist(), vi[:, slot[2]].tolist())))
            elif slot[0] == "distinct":
                if distinct_sizes:
                    acols.append([DistinctSize(c) for c in vi[:, slot[1]].tolist()])
                else:
                    acols.append(self.distinct_sets(slot[1], slot[2], n))
            elif slot[0] == "hll":  # DISTINCTCOUNTHLL executed by the library: the estimate, or the registers
                if distinct_sizes:
                    acols.append([FinalValue(x) for x in vi[:, slot[1]].tolist()])
                else:
                    acols.append(self.hll_registers(slot[1], n))
            elif slot[0] in ("hist", "dset"):  # PERCENTILE / DISTINCTSUM / DISTINCTAVG executed by the library
                if distinct_sizes:
                    acols.append([FinalValue(x) for x in v[:, slot[1]].tolist()])
                elif slot[0] == "hist":
                    acols.append(self.value_hists(slot[1], slot[2], n))
                else:
                    acols.append(self.distinct_sets(slot[1], slot[2], n))
            elif slot[0] == "range":
                pr = pairs[:n * nnat * 2].reshape(n, nnat, 2)
                acols.append(list(zip(pr[:, slot[1], 0].tolist(), pr[:, slot[1], 1].tolist())))
            elif slot[0] == "avgmv":
                pr = pairs[:n * nnat * 2].reshape(n, nnat, 2)
                acols.append(list(zip(pr[:, slot[1], 0].tolist(), pr[:, slot[1], 1].astype(np.int64).tolist())))
            elif a.func in ("COUNT", "SUMLONG", "COUNTMV"):
                acols.append(vi[:, slot[1]].tolist())
            else:
                acols.append(v[:, slot[1]].tolist())
        # a million small containers would trigger the cyclic GC over and over (none of them is cyclic)
        was = gc.isenabled()
        gc.disable()
        try:
            parts = list(map(list, zip(*acols))) if acols else [[] for _ in range(n)]
            return dict(zip(key_tuples, parts))
        finally:
            if was:
                gc.enable()

    def rows(self) -> List[tuple]:
        # a library-executed DISTINCTCOUNT: the counts come with the fetch, the value sets stay on the device
        return reduce_rows(self.qc, self.groups(distinct_sizes=True))

    def destroy(self) -> None:
        if self._h:
            lib().pinot_amd_result_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.destroy()
        except Exception:
            pass


class SelectionResult:
    """Rows of one executed selection query (SELECT columns [ORDER BY ...] LIMIT n [OFFSET m]).

    columns: the selected columns in select-list order (``*`` expanded); QueryContext.selection_columns gives the
    server's schema order (ORDER BY columns first). The server keeps offset + limit rows; the broker applies the
    offset. Ties of the ORDER BY come in ascending (segment index, docId)."""

    def __init__(self, handle, qc: QueryContext, columns: List[str], types: List[str]):
        self._h = handle
        self.qc = qc
        self.columns = columns
        self._types = types

    def execute_again(self, stream=None) -> None:
        check(lib().pinot_amd_execute_again(self._h, _stream_handle(stream)), "execute_again")

    def num_docs_matched(self) -> int:
        """numDocsScanned: every matching doc with ORDER BY, the rows returned without."""
        out = C.c_int64()
        check(lib().pinot_amd_result_num_docs_matched(self._h, C.byref(out)), "num_docs_matched")
        return out.value

    def kernel_info(self) -> str:
        """'jit-topk' (rows pruned in LDS) or 'jit-topk-sort', ' xN' for N launches run."""
        return lib().pinot_amd_result_kernel_info(self._h).decode()

    def packed_info(self) -> str:
        return lib().pinot_amd_result_packed_info(self._h).decode()

    def last_kernel_ms(self) -> float:
        out = C.c_double()
        check(lib().pinot_amd_result_last_kernel_ms(self._h, C.byref(out)), "last_kernel_ms")
        return out.value

    def algorithmic_bytes(self) -> float:
        out = C.c_double()
        check(lib().pinot_amd_result_algorithmic_bytes(self._h, C.byref(out)), "algorithmic_bytes")
        return out.value

    def plan_timing(self) -> Dict[str, float]:
        txt = lib().pinot_amd_result_plan_timing(self._h).decode()
        return {k: float(v) for k, v in (kv.split("=") for kv in txt.split(";") if kv)}

    def fetch_arrays(self):
        """(rows, segment index per row, docId per row, values [rows, columns] in fetch's key encoding)."""
        L = lib()
        n = C.c_int64()
        check(L.pinot_amd_result_num_rows(self._h, C.byref(n)), "num_rows")
        cap = max(n.value, 1)
        nc = max(len(self.columns), 1)
        seg = np.zeros(cap, dtype=np.int32)
        doc = np.zeros(cap, dtype=np.int32)
        vals = np.zeros(cap * nc, dtype=np.int64)
        got = C.c_int64()
        p32 = C.POINTER(C.c_int32)
        check(L.pinot_amd_result_fetch_rows(self._h, cap, seg.ctypes.data_as(p32), doc.ctypes.data_as(p32),
                                            vals.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(got)), "fetch_rows")
        g = got.value
        return g, seg[:g], doc[:g], vals[:g * nc].reshape(g, nc)

    def origins(self) -> List[tuple]:
        """(segment index in the batch, docId) of every row."""
        _, seg, doc, _ = self.fetch_arrays()
        return list(zip(seg.tolist(), doc.tolist()))

    def rows(self) -> List[tuple]:
        """The server's offset + limit rows, values in select-list order: STRINGs as str, FLOAT as Python floats of
        the float32 value, DOUBLE as float, INT / LONG as int."""
        L = lib()
        g, _, _, vals = self.fetch_arrays()
        cols = []
        for j, t in enumerate(self._types):
            col = np.ascontiguousarray(vals[:, j])
            if t == STRING:
                names = {int(i): L.pinot_amd_result_selection_string(self._h, j, int(i)).decode() for i in np.unique(col)}
                cols.append([names[i] for i in col.tolist()])
            elif t in (FLOAT, DOUBLE):
                cols.append(col.view(np.float64).tolist())
            else:
                cols.append(col.tolist())
        return list(zip(*cols)) if g else []

    def destroy(self) -> None:
        if self._h:
            lib().pinot_amd_result_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.destroy()
        except Exception:
            pass


class DistinctResult:
    """Rows of one executed distinct query (SELECT DISTINCT columns [WHERE] [ORDER BY ...] LIMIT n).

    columns: the distinct columns in select-list order. rows(): at most LIMIT distinct rows in the ORDER BY's order
    (ties by ascending global group key); without ORDER BY the first LIMIT rows held, in ascending global key order.
    Values are typed like group keys (JavaDouble for FLOAT / DOUBLE); STRING values are resolved for the returned
    rows only."""

    def __init__(self, handle, qc: QueryContext, columns: List[str], types: List[str]):
        self._h = handle
        self.qc = qc
        self.columns = columns
        self._types = types

    def execute_again(self, stream=None) -> None:
        check(lib().pinot_amd_execute_again(self._h, _stream_handle(stream)), "execute_again")

    def num_docs_matched(self) -> int:
        """The docs matching the filter in the segments actually scanned (the dictionary-only answer: the sum of
        min(LIMIT, cardinality) over the segments, as DictionaryBasedDistinctOperator reports)."""
        out = C.c_int64()
        check(lib().pinot_amd_result_num_docs_matched(self._h, C.byref(out)), "num_docs_matched")
        return out.value

    def kernel_info(self) -> str:
        """'jit-distinct-lds' / '-wide' / '-hbm' (' xN' for N != 1 launches run), the hash plan's name, or
        'distinct-dictionary'."""
        return lib().pinot_amd_result_kernel_info(self._h).decode()

    def packed_info(self) -> str:
        return lib().pinot_amd_result_packed_info(self._h).decode()

    def last_kernel_ms(self) -> float:
        out = C.c_double()
        check(lib().pinot_amd_result_last_kernel_ms(self._h, C.byref(out)), "last_kernel_ms")
        return out.value

    def algorithmic_bytes(self) -> float:
        out = C.c_double()
        check(lib().pinot_amd_result_algorithmic_bytes(self._h, C.byref(out)), "algorithmic_bytes")
        return out.value

    def plan_timing(self) -> Dict[str, float]:
        txt = lib().pinot_amd_result_plan_timing(self._h).decode()
        return {k: float(v) for k, v in (kv.split("=") for kv in txt.split(";") if kv)}

    def fetch_arrays(self):
        """(rows, values [rows, columns] in fetch's key encoding), in result order."""
        L = lib()
        ng = C.c_int64()
        check(L.pinot_amd_result_num_groups(self._h, C.byref(ng)), "num_groups")
        cap = max(ng.value, 1)
        nc = len(self.columns)
        keys = np.zeros(cap * nc, dtype=np.int64)
        got = C.c_int64()
        check(L.pinot_amd_result_fetch(self._h, cap, keys.ctypes.data_as(C.POINTER(C.c_int64)), None, None,
                                       C.byref(got)), "fetch")
        g = got.value
        return g, keys[:g * nc].reshape(g, nc)

    def rows(self) -> List[tuple]:
        L = lib()
        g, vals = self.fetch_arrays()
        cols = []
        for j, t in enumerate(self._types):
            col = np.ascontiguousarray(vals[:, j])
            if t == STRING:
                names = {int(i): L.pinot_amd_result_string_key(self._h, j, int(i)).decode() for i in np.unique(col)}
                cols.append([names[i] for i in col.tolist()])
            elif t in (FLOAT, DOUBLE):
                cols.append([JavaDouble(x) for x in col.view(np.float64).tolist()])
            else:
                cols.append(col.tolist())
        return list(zip(*cols)) if g else []

    def destroy(self) -> None:
        if self._h:
            lib().pinot_amd_result_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.destroy()
        except Exception:
            pass


class ServerQueryExecutor:
    """Compiles a QueryContext and runs it over a list of HBM-resident segments.

    server_trim: apply the server's combine table to GROUP BY results like GroupByCombineOperator's
    IndexedTable (LIMIT groups without ORDER BY; the top max(5 * LIMIT, minServerGroupTrimSize) by the
    ORDER BY otherwise; pinot_amd_query_set_result_limit). Off by default: every group is returned,
    which is what a multi-server broker reduce over exact partials wants.

    distinct_count: how a query with DISTINCTCOUNT, PERCENTILE, DISTINCTSUM or DISTINCTAVG aggregations (each
    where DISTINCTCOUNT is named below) runs. "mirror" (default): split here into the
    base query and one (group, value) query per DISTINCTCOUNT, every pair fetched and folded into Python sets
    (DistinctCountResult; the path multi-GPU merges use). "native": the whole query goes to the library, which
    runs the same queries and folds them on the device (PINOT_AMD_AGG_DISTINCTCOUNT); rows() then fetches only
    the counts, groups() the value sets as CSR."""

    def __init__(self, use_inverted_index: bool = True, server_trim: bool = False, distinct_count: str = "mirror"):
        if distinct_count not in ("mirror", "native"):
            raise ValueError(f"distinct_count must be 'mirror' or 'native', not {distinct_count!r}")
        self.use_inverted_index = use_inverted_index
        self.server_trim = server_trim
        self.distinct_count = distinct_count

    def filter_doc_ids(self, query, segments: Sequence[ImmutableSegment], stream=None) -> List[np.ndarray]:
        """FilterPlanNode -> BlockDocIdSet: ascending matching docIds of each segment (the filter
        runs on the device into a dense bitset, compacted with ballot / prefix sums)."""
        import torch
        qc = parse_sql(query, pattern_predicates=True) if isinstance(query, str) else query
        L = lib()
        qh, _ = self._compile(qc, segments)
        try:
            arr = (C.c_void_p * len(segments))(*[s.handle.value for s in segments])
            rh = C.c_void_p()
            check(L.pinot_amd_execute_filter(qh, arr, len(segments), _stream_handle(stream), C.byref(rh)),
                  "execute_filter")
        finally:
            L.pinot_amd_query_destroy(qh)
        out = []
        try:
            for i, seg in enumerate(segments):
                p = C.c_void_p()
                nw = C.c_int64()
                check(L.pinot_amd_result_bitset(rh, i, C.byref(p), C.byref(nw)), "result_bitset")
                ids = torch.empty(max(seg.num_docs, 1), dtype=torch.int32, device="cuda")
                cnt = C.c_int64()
                check(L.pinot_amd_bitset_to_doc_ids(p.value, seg.num_docs, ids.data_ptr(), C.byref(cnt),
                                                    _stream_handle(stream)), "bitset_to_doc_ids")
                out.append(ids[:cnt.value].cpu().numpy())
        finally:
            L.pinot_amd_result_destroy(rh)
        return out

    def _compile(self, qc: QueryContext, segments: Sequence[ImmutableSegment]):
        L = lib()
        first = segments[0]
        qh = C.c_void_p()
        check(L.pinot_amd_query_create(C.byref(qh)), "query_create")
        keep: list = []
        names = _QueryNames(qh, first)
        try:
            for ci, clause in enumerate(qc.cnf):
                for pred, neg in clause:
                    col = names.column(pred.column)
                    if col is None:
                        raise _lib.PinotAmdError(f"unknown column {pred.column!r} in segment {first.name}")
                    spec = _predicate_spec(pred, col, self.use_inverted_index, keep, names.abi(pred.column))
                    check(L.pinot_amd_query_add_predicate(qh, ci, C.byref(spec), 1 if neg else 0), "add_predicate")
        except Exception:
            L.pinot_amd_query_destroy(qh)
            raise
        return qh, names

    def execute(self, query, segments: Sequence[ImmutableSegment], stream=None, key_space=None):
        """Run a query over HBM-resident segments. key_space (optional): group-by column -> the values of
        its global key space (dist.global_key_space: the union of every rank's dictionaries), so that
        every rank's dense group table indexes the same groups."""
        qc = parse_sql(query, pattern_predicates=True) if isinstance(query, str) else query
        if key_space is not None and qc.expressions():
            raise ValueError(f"a query with arithmetic expressions ({', '.join(qc.expressions())}) takes no key_space: "
                             "the cross-rank merge does not cover it")
        if qc.has_filtered_aggregations():
            if key_space is not None:
                raise _lib.PinotAmdError("a query with filtered aggregations (FILTER (WHERE ...)) takes no key_space: the "
                                         "cross-rank merge does not cover it")
            for a in qc.aggregations:  # (distinct_count="native": the library refuses it, EUNSUPPORTED)
                if a.func in VALUE_SET_FUNCS and self.distinct_count != "native":
                    raise _lib.PinotAmdError(f"FILTER (WHERE ...) in a query with {a.func} is not supported: the value-set "
                                             "queries do not take the lanes' predicates")
        if qc.is_selection():
            if key_space is not None:
                raise _lib.PinotAmdError("a selection query takes no key_space (its rows merge by value at the broker)")
            return self._execute_selection(qc, segments, stream)
        if qc.is_distinct():
            if key_space is not None:
                raise _lib.PinotAmdError("a distinct query takes no key_space (there is no multi-GPU merge of its rows)")
            return self._execute_distinct(qc, segments, stream)
        if any(a.func in VALUE_SET_FUNCS for a in qc.aggregations) and self.distinct_count == "native":
            if key_space is not None:
                raise _lib.PinotAmdError("distinct_count='native' takes no key_space: results of several ranks merge "
                                         "their value sets by union on the mirror path (distinct_count='mirror', "
                                         "DistinctCountResult.results())")
            for a in qc.aggregations:
                if a.func in VALUE_SET_FUNCS and (a.expr is not None or a.column == "*"):
                    raise ValueError(f"{a.func} takes one column")
            return self._execute(qc, segments, stream, None)
        if any(a.func in VALUE_SET_FUNCS for a in qc.aggregations):
            # the device queries run untrimmed (a result limit on a (group, value) sub-query would cut value
            # sets); the server's combine table applies to the folded groups (DistinctCountResult.groups)
            trim = self.server_trim and bool(qc.group_by)
            if trim and qc.safe_trim() and qc.limit >= qc.sort_aggregate_limit_threshold \
                    and not qc.server_return_final_result:
                raise _lib.PinotAmdError("DISTINCTCOUNT with a segment-level safe trim (ORDER BY = GROUP BY, LIMIT >= "
                                         "sortAggregateLimitThreshold) is not supported with server_trim")
            base, subs = split_distinct_count(qc)
            return DistinctCountResult(qc, self._execute(base, segments, stream, key_space, server_trim=False),
                                       [(i, self._execute(sq, segments, stream, key_space, server_trim=False))
                                        for i, sq in subs], server_trim=trim,
                                       column_types={a.column: segments[0].columns[a.column].stored_type
                                                     for a in qc.aggregations
                                                     if a.func == "DISTINCTCOUNTHLL" and a.column in segments[0].columns})
        return self._execute(qc, segments, stream, key_space)

    def _execute_selection(self, qc: QueryContext, segments: Sequence[ImmutableSegment], stream=None) -> SelectionResult:
        """SelectionPlanNode: the selected columns as the library's output columns, the ORDER BY, LIMIT and OFFSET."""
        if not segments:
            raise ValueError("no segments")
        L = lib()
        first = segments[0]
        columns = qc.select_list(first)
        if not columns:
            raise ValueError("a selection query needs a column")
        qh, names = self._compile(qc, segments)
        try:
            cbs = {}
            for c in columns + [c for c, _ in qc.order_by]:
                cbs[c] = names.column(c)
                if cbs[c] is None:
                    raise _lib.PinotAmdError(f"unknown column {c!r} in segment {first.name}")
            for c in columns:
                check(L.pinot_amd_query_add_selection(qh, names.abi(c), None), "add_selection")
            for c, asc in qc.order_by:
                check(L.pinot_amd_query_add_selection_order_by(qh, names.abi(c), 1 if asc else 0), "add_selection_order_by")
            check(L.pinot_amd_query_set_selection_limit(qh, qc.limit, qc.offset), "set_selection_limit")
            arr = (C.c_void_p * len(segments))(*[s.handle.value for s in segments])
            rh = C.c_void_p()
            check(L.pinot_amd_execute(qh, arr, len(segments), _stream_handle(stream), C.byref(rh)), "execute")
        finally:
            L.pinot_amd_query_destroy(qh)
        return SelectionResult(rh, qc, columns, [cbs[c].stored_type for c in columns])

    def _execute_distinct(self, qc: QueryContext, segments: Sequence[ImmutableSegment], stream=None) -> DistinctResult:
        """DistinctPlanNode: the distinct columns as the library's keys, the ORDER BY over them, the LIMIT."""
        if not segments:
            raise ValueError("no segments")
        L = lib()
        first = segments[0]
        qh, names = self._compile(qc, segments)
        try:
            for g in qc.group_by:
                kt = key_transform(g)
                if kt is not None:
                    spec = key_transform_spec(kt)
                    check(L.pinot_amd_query_add_group_by_transform(qh, kt.column.encode(), C.byref(spec)),
                          f"add_group_by_transform({g})")
                    continue
                if names.column(g) is None:
                    raise _lib.PinotAmdError(f"unknown column {g!r} in segment {first.name}")
                check(L.pinot_amd_query_add_group_by(qh, names.abi(g)), "add_group_by")
            for kind, idx, asc in qc.order_by_targets():
                check(L.pinot_amd_query_add_order_by(qh, kind, idx, 1 if asc else 0), "add_order_by")
            check(L.pinot_amd_query_set_distinct(qh, qc.limit), "set_distinct")
            arr = (C.c_void_p * len(segments))(*[s.handle.value for s in segments])
            rh = C.c_void_p()
            check(L.pinot_amd_execute(qh, arr, len(segments), _stream_handle(stream), C.byref(rh)), "execute")
        finally:
            L.pinot_amd_query_destroy(qh)
        types = [LONG if key_transform(g) is not None else DOUBLE if expression(g) is not None
                 else first.columns[g].stored_type for g in qc.group_by]
        return DistinctResult(rh, qc, list(qc.group_by), types)

    @staticmethod
    def _set_key_space(qh, column: str, stored_type: str, values) -> None:
        n = len(values)
        vi = vd = vs = None
        if stored_type == STRING:
            vs = (C.c_char_p * max(n, 1))(*[str(v).encode() for v in values])
        elif stored_type in (FLOAT, DOUBLE):
            vd = (C.c_double * max(n, 1))(*[float(v) for v in values])
        else:
            vi = (C.c_int64 * max(n, 1))(*[int(v) for v in values])
        check(lib().pinot_amd_query_set_group_key_values(qh, column.encode(), TYPE_CODE[stored_type], n, vi, vd, vs),
              f"set_group_key_values({column})")

    def _execute(self, qc, segments: Sequence[ImmutableSegment], stream=None, key_space=None,
                 server_trim=None) -> QueryResult:
        if not segments:
            raise ValueError("no segments")
        server_trim = self.server_trim if server_trim is None else server_trim
        L = lib()
        first = segments[0]
        qh = C.c_void_p()
        check(L.pinot_amd_query_create(C.byref(qh)), "query_create")
        keep: list = []
        names = _QueryNames(qh, first)
        try:
            for ci, clause in enumerate(qc.cnf):
                for pred, neg in clause:
                    col = names.column(pred.column)
                    if col is None:
                        raise _lib.PinotAmdError(f"unknown column {pred.column!r} in segment {first.name}")
                    spec = _predicate_spec(pred, col, self.use_inverted_index, keep, names.abi(pred.column))
                    check(L.pinot_amd_query_add_predicate(qh, ci, C.byref(spec), 1 if neg else 0), "add_predicate")
            for g in qc.group_by:
                kt = key_transform(g)
                if kt is not None:  # a time-bucket key: bound by its spec, its key space the union over the batch
                    if key_space is not None:
                        raise _lib.PinotAmdError(f"GROUP BY {g} takes no key_space (a transformed key's space is "
                                                 "the union over the batch)")
                    spec = key_transform_spec(kt)
                    check(L.pinot_amd_query_add_group_by_transform(qh, kt.column.encode(), C.byref(spec)),
                          f"add_group_by_transform({g})")
                    continue
                check(L.pinot_amd_query_add_group_by(qh, names.abi(g)), "add_group_by")
                if key_space is not None and g in key_space:
                    self._set_key_space(qh, g, first.columns[g].stored_type, key_space[g])
            check(L.pinot_amd_query_set_num_groups_limit(qh, qc.num_groups_limit), "set_num_groups_limit")
            if qc.filtered_aggregations_skip_empty_groups:
                check(L.pinot_amd_query_set_filtered_aggregations_skip_empty_groups(qh, 1),
                      "set_filtered_aggregations_skip_empty_groups")
            if server_trim and qc.group_by:
                check(L.pinot_amd_query_set_result_limit(qh, qc.limit, qc.min_server_group_trim_size,
                                                         qc.group_trim_threshold), "set_result_limit")
                check(L.pinot_amd_query_set_server_options(qh, 1 if qc.server_return_final_result else 0,
                                                           qc.sort_aggregate_limit_threshold), "set_server_options")
                check(L.pinot_amd_query_set_segment_trim(qh, qc.min_segment_group_trim_size), "set_segment_trim")
            native = []
            agg_slots = []

            def add(func, column, expr=None, param=None, filt=None):
                # (a filtered aggregation: its lane -- the filter's text -- is part of the library aggregation's identity)
                key = (func, column) if param is None else (func, column, param)
                if filt is not None:
                    key += ("FILTER", filter_text(filt))
                if key in native:
                    return native.index(key)
                idx = C.c_int32()
                abi_col = column.encode() if (expr is not None or column == "*") else names.abi(column)
                if func == "DISTINCTCOUNTHLL":  # its own entry point: the literal is log2m
                    check(L.pinot_amd_query_add_aggregation_hll(qh, abi_col, int(param), C.byref(idx)),
                          f"add_aggregation_hll({column})")
                elif func in MV_FUNCS:  # the multi-value functions' entry point
                    check(L.pinot_amd_query_add_aggregation_mv(qh, AGG_CODE[func], column.encode(), C.byref(idx)),
                          f"add_aggregation_mv({func})")
                elif AGG_CODE[func] > AGG_CODE["DISTINCTCOUNT"]:  # the functions with a literal argument's entry point
                    check(L.pinot_amd_query_add_aggregation_param(qh, AGG_CODE[func], abi_col,
                                                                  0.0 if param is None else param, C.byref(idx)),
                          f"add_aggregation_param({func})")
                elif expr is None:
                    check(L.pinot_amd_query_add_aggregation(qh, AGG_CODE[func], abi_col, C.byref(idx)),
                          f"add_aggregation({func})")
                else:
                    check(L.pinot_amd_query_add_aggregation_expr(qh, AGG_CODE[func], EXPR_CODE[expr[0]],
                                                                 expr[1].encode(), expr[2].encode(), C.byref(idx)),
                          f"add_aggregation_expr({func} {column})")
                for ci, clause in enumerate(to_cnf(filt)):
                    for pred, neg in clause:
                        col = names.column(pred.column)
                        if col is None:
                            raise _lib.PinotAmdError(f"unknown column {pred.column!r} in segment {first.name}")
                        spec = _predicate_spec(pred, col, self.use_inverted_index, keep, names.abi(pred.column))
                        check(L.pinot_amd_query_add_aggregation_filter_predicate(qh, idx.value, ci, C.byref(spec),
                                                                                 1 if neg else 0),
                              "add_aggregation_filter_predicate")
                native.append(key)
                return idx.value

            for a in qc.aggregations:
                if a.func == "AVG":
                    # (with FILTER: the sum and the count of the aggregation's lane)
                    agg_slots.append(("avg", add("SUM", a.column, a.expr, None, a.filter), add("COUNT", "*", None, None, a.filter)))
                elif a.func == "DISTINCTCOUNT":  # the library folds the value sets (distinct_count="native")
                    col = names.column(a.column)
                    if col is None:
                        raise _lib.PinotAmdError(f"unknown column {a.column!r} in segment {first.name}")
                    agg_slots.append(("distinct", add("DISTINCTCOUNT", a.column, None, None, a.filter), col.stored_type))
                elif a.func == "DISTINCTCOUNTHLL":  # the library builds and folds the registers
                    if names.column(a.column) is None:
                        raise _lib.PinotAmdError(f"unknown column {a.column!r} in segment {first.name}")
                    agg_slots.append(("hll", add(a.func, a.column, None, a.param, a.filter)))
                elif a.func in VALUE_SET_FUNCS:    # PERCENTILE / DISTINCTSUM / DISTINCTAVG, likewise
                    col = names.column(a.column)
                    if col is None:
                        raise _lib.PinotAmdError(f"unknown column {a.column!r} in segment {first.name}")
                    agg_slots.append(("hist" if a.func == "PERCENTILE" else "dset",
                                      add(a.func, a.column, None, a.param, a.filter), col.stored_type))  # (a FILTER: refused there)
                elif a.func == "MINMAXRANGE":  # MinMaxRangePair (min, max), NaN-skipping, in the library
                    agg_slots.append(("range", add("MINMAXRANGE", a.column, a.expr, None, a.filter)))
                elif a.func in MV_FUNCS:  # over the column's per-doc twins, in the library
                    if a.expr is not None or a.column == "*":
                        raise ValueError(f"{a.func} takes one multi-value column")
                    kind = {"AVGMV": "avgmv", "MINMAXRANGEMV": "range"}.get(a.func, "direct")
                    agg_slots.append((kind, add(a.func, a.column, None, None, a.filter)))
                else:
                    agg_slots.append(("direct", add(a.func, a.column, a.expr, None, a.filter)))
            if not qc.aggregations and qc.group_by:
                add("COUNT", "*")  # DISTINCT-style group-by still needs the group presence count
            if server_trim and qc.group_by:
                for kind, idx, asc in qc.order_by_targets():
                    if kind == 1:  # the library aggregation whose final value orders (AVG: sum / count)
                        a = qc.aggregations[idx]
                        idx = add(a.func, a.column, a.expr, a.param, a.filter)
                    check(L.pinot_amd_query_add_order_by(qh, kind, idx, 1 if asc else 0), "add_order_by")
            arr = (C.c_void_p * len(segments))(*[s.handle.value for s in segments])
            rh = C.c_void_p()
            check(L.pinot_amd_execute(qh, arr, len(segments), _stream_handle(stream), C.byref(rh)), "execute")
        finally:
            L.pinot_amd_query_destroy(qh)
        key_types = [LONG if key_transform(g) is not None else DOUBLE if expression(g) is not None
                     else first.columns[g].stored_type for g in qc.group_by]
        res = QueryResult(rh, qc, agg_slots, key_types)
        res._native_aggs = native
        # the multi-value columns the query filters on (dist.merge_result refuses such a result)
        res.mv_columns = sorted({p.column for clause in qc.cnf for p, _ in clause
                                 if getattr(first.columns.get(p.column), "multi_value", False)})
        return res
