"""bench.py's cpu_baseline leg times oracle.cpu_plan (the oracle's C work for one segment, set up
once). Its matched-doc count must equal oracle.execute's on the same segment and query, and the
timed closure must be re-runnable (the inverted leaves' bitsets are rebuilt each call)."""
import numpy as np
import pytest

import oracle
from helpers import SV_FILTER, random_segment, sv_segment


@pytest.mark.parametrize("use_inverted", [True, False])
@pytest.mark.parametrize("query", [
    "SELECT COUNT(*), SUM(column1), MAX(column3) FROM t" + SV_FILTER,
    "SELECT column11, COUNT(*), SUM(column1) FROM t" + SV_FILTER + " GROUP BY column11",
    "SELECT column6, column7, SUM(column1) FROM t WHERE column17 IN (635553468, 1225000000) GROUP BY column6, column7",
])
def test_cpu_plan_matches_execute(query, use_inverted):
    seg = sv_segment()
    run = oracle.cpu_plan(query, seg, use_inverted)
    exp, _ = oracle.execute(query, [seg], use_inverted)
    assert run() == exp
    assert run() == exp


def test_cpu_plan_inverted_or():
    rng = np.random.default_rng(5)
    seg = random_segment(rng, 50_000, bits_cards=(300, 200, 100), inverted=("d0", "d1", "d2"))
    q = ("SELECT COUNT(*), SUM(r_int) FROM t WHERE d0 IN (3, 10, 17, 24, 500) AND "
         "(d1 IN (3, 52, 101) OR d2 IN (10, 17, 24, 31))")
    exp, _ = oracle.execute(q, [seg])
    run = oracle.cpu_plan(q, seg)
    assert exp > 0 and run() == exp and run() == exp


@pytest.mark.parametrize("info,want", [
    ("jit", "pinot_scan_jit"),
    ("jit-select", "pinot_select+pinot_gather"),
    ("jit-wselect", "pinot_select(word-level)+pinot_gather"),
    ("jit-fwselect", "roaring_select_kernel"),
    ("jit-partitioned+admit-seq", "pinot_admit_seq"),
    ("jit-partitioned+admit", "pinot_first_doc"),
    ("jit-hash-trim", "hash_merge_kernel"),
    ("jit x3", "(3 shape launches)"),
])
def test_bench_kernel_labels(info, want):
    """bench.py names the kernels a plan ran from its kernel_info (round-2 advisor: mislabelled lines)."""
    bench = _bench_module()
    assert want in bench.plan_kernels(info), bench.plan_kernels(info)


def _bench_module():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(os.path.dirname(os.path.dirname(__file__)), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


@pytest.mark.parametrize("budget", [1 << 20, 4096])
def test_bench_dump_outputs(tmp_path, budget):
    """bench.py --dump-outputs: rows sorted by key whatever order the plan fetched them in (two builds compare row
    for row), float64 files, and a fixed seeded sample of the sorted rows when they exceed the byte budget."""
    import ctypes
    import os
    from types import SimpleNamespace
    bench = _bench_module()
    rng = np.random.default_rng(3)
    n, nk, na = 300, 2, 3
    keys = np.stack([rng.integers(0, 20, n), rng.permutation(n)], axis=1).astype(np.int64)  # distinct rows
    vals = keys[:, :1] * 0.5 + keys[:, 1:] * np.arange(1, na + 1)[None, :]
    res = SimpleNamespace(qc=SimpleNamespace(group_by=["a", "b"]), _native_aggs=[None] * na, _key_types=["INT", "INT"])
    dumps = []
    for trial in range(2):  # the same groups fetched in two different orders
        p = rng.permutation(n)
        k, v = keys[p], vals[p]
        arrays = (ctypes.c_int64(n), k.reshape(-1).copy(), v.reshape(-1).copy(), v.astype(np.int64).reshape(-1), None)
        d = str(tmp_path / f"d{trial}")
        bench.dump_outputs(d, "", res, arrays, 1234, budget)
        dumps.append({f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))})
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= budget
    a, b = dumps
    assert set(a) == {"keys", "values", "values_exact", "num_docs_matched"} | ({"sample_rows"} if budget == 4096 else set())
    for name in a:
        assert a[name].dtype == np.float64 and np.array_equal(a[name], b[name]), name
    order = np.lexsort((keys[:, 1], keys[:, 0]))
    rows = order if budget != 4096 else order[a["sample_rows"].astype(np.int64)]
    assert 0 < len(rows) <= n and (budget != 4096 or len(rows) < n)
    assert np.array_equal(a["keys"], keys[rows]) and np.array_equal(a["values"], vals[rows])
    assert np.array_equal(a["values_exact"], vals[rows].astype(np.int64)) and a["num_docs_matched"].tolist() == [1234.0]
