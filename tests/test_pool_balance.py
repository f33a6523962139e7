"""Every query gives back to the device/pinned buffer pool what it took,
on its error exits as on success ("Who owns pooled blocks").

yt_gpu_debug_pool_blocks_in_use() is read before and after each call and must
be the same; each case runs twice in a row, so the second run works on the
blocks the first one returned. Beside the balance each case asserts the rows
(against the oracle, or against plain Python for string projections, which
the oracle does not evaluate) or the error the other suites expect for that
shape. All errors here are ordinary refusals and user errors.

Not covered: the "tie set too large" refusal of a multi-key ORDER BY needs
more than 2^17 rows with one order key, far above the few thousand rows used
here. Events do not show in this counter; that no exit leaks one is a
property of the code (PoolScope owns them), not something measured here."""
import ctypes as C

import numpy as np
import pytest

import ytsaurus_amd as y
from ytsaurus_amd import _abi
from ytsaurus_amd._abi import (SCAN_PATH_PROJ_COMPACT, SCAN_PATH_STR_DENSE,
                               SCAN_PATH_STR_GENERAL, VT_INT64, VT_STRING)

import test_partition_modes as pm
import test_versioned as tv

CAPACITY = "ytql error %d" % _abi.YT_ERR_CAPACITY


def in_use():
    return int(_abi.gpu_lib().yt_gpu_debug_pool_blocks_in_use())


def scan_path():
    return _abi.gpu_lib().yt_gpu_debug_last_scan_path()


def balanced(fn):
    """fn() twice; each run leaves the pool's count where it found it"""
    out = None
    for _ in range(2):
        before = in_use()
        out = fn()
        assert in_use() == before
    return out


def fails(match, fn):
    def run():
        with pytest.raises(RuntimeError, match=match):
            fn()
    balanced(run)


def same_rows(got, want):
    assert y.sort_rows(got) == y.sort_rows(want)


def test_counter_is_exported():
    assert in_use() >= 0


# ---- shared data (built once; never modified) ----

_CACHE = {}


def cached(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def _str_table():
    """6000 rows in key segments of 2048 that the value column shares; 300
    keys and 2 % null keys; int64 values with 10 % nulls; g = key index."""
    rng = np.random.default_rng(501)
    n = 6000
    ki = rng.integers(0, 300, n)
    kn = rng.random(n) < 0.02
    keys = [None if kn[i] else "k%04d" % ki[i] for i in range(n)]
    v = rng.integers(-1000, 1000, n, dtype=np.int64)
    vn = (rng.random(n) < 0.10).astype(np.uint8)
    g = np.where(kn, 0, ki).astype(np.int64)
    return y.Chunk([y.encode_string(keys, max_segment_values=2048),
                    y.encode_int64(v, vn, max_segment_values=2048),
                    y.encode_int64(g, max_segment_values=2048)], n)


def _wide_table():
    """6000 rows, 3000 distinct keys: more than the 2048 slots a merge table
    starts with under a small max_groups_hint"""
    rng = np.random.default_rng(502)
    n = 6000
    ki = rng.permutation(n) % 3000
    keys = ["w%05d" % k for k in ki]
    v = rng.integers(1, 1000, n, dtype=np.int64)
    return y.Chunk([y.encode_string(keys, max_segment_values=2048),
                    y.encode_int64(v, max_segment_values=2048)], n)


def str_table():
    return cached("str", _str_table)


def wide_table():
    return cached("wide", _wide_table)


def dense_plan():
    return y.Plan(keys=[y.col(0)], aggs=[y.agg_sum(y.col(1)), y.agg_sum1()])


def general_plan():
    return y.Plan(filter=y.col(1) > -500, keys=[y.col(0)],
                  aggs=[y.agg_sum(y.col(1)), y.agg_sum1()])


def key_bytes(rows):
    return sum(len(r[0]) for r in rows if r[0] is not None)


# ---- run_string_group, specialised ----

@pytest.mark.gpu
def test_string_group_specialised(cuda):
    chunk = str_table()
    dev = chunk.c_device(cuda)
    plan = dense_plan()
    want, _ = y.oracle_execute(plan, chunk)
    assert any(r[0] is None for r in want)       # the null row is written
    need = key_bytes(want)

    def run(**kw):
        got, st = y.gpu_execute(plan, dev, max_groups_hint=1024, **kw)
        assert scan_path() == SCAN_PATH_STR_DENSE
        return got, st

    got, _ = balanced(lambda: run(pool_bytes=need))          # sliced emit
    same_rows(got, want)
    # the limited emit: every row fits under the limit, the null row included
    got, st = balanced(lambda: run(output_row_limit=len(want) + 5))
    same_rows(got, want)
    assert st.incomplete_output == 0
    fails(CAPACITY, lambda: run(out_capacity=len(want) - 1,
                                output_row_limit=len(want) + 5))
    fails("string pool too small", lambda: run(pool_bytes=need - 1))


@pytest.mark.gpu
def test_string_group_specialised_table_grows(cuda):
    chunk = wide_table()
    plan = dense_plan()
    want, _ = y.oracle_execute(plan, chunk)
    assert len(want) == 3000
    dev = chunk.c_device(cuda)

    def run():
        got, _ = y.gpu_execute(plan, dev, max_groups_hint=1)
        assert scan_path() == SCAN_PATH_STR_DENSE
        return got

    same_rows(balanced(run), want)


# ---- run_string_group, general ----

@pytest.mark.gpu
def test_string_group_general(cuda):
    chunk = str_table()
    dev = chunk.c_device(cuda)
    plan = general_plan()
    want, _ = y.oracle_execute(plan, chunk)
    need = key_bytes(want)

    def run(p=plan, **kw):
        got, _ = y.gpu_execute(p, dev, max_groups_hint=1024, **kw)
        assert scan_path() == SCAN_PATH_STR_GENERAL
        return got

    same_rows(balanced(lambda: run(pool_bytes=need)), want)
    fails("rowset too small", lambda: run(out_capacity=len(want) - 1))
    fails("string pool too small", lambda: run(pool_bytes=need - 1))
    div0 = y.Plan(filter=(y.col(1) // (y.col(2) - y.col(2))) > 0,
                  keys=[y.col(0)], aggs=[y.agg_sum1()])
    fails("Division by zero", lambda: run(div0))


@pytest.mark.gpu
def test_string_group_general_table_grows(cuda):
    """max_groups_hint = 1 starts the merge table at 2048 slots; 3000 keys
    overflow it, so the slot table and the aggregate records beside it are
    replaced at least once"""
    chunk = wide_table()
    plan = y.Plan(filter=y.col(1) > 0, keys=[y.col(0)],
                  aggs=[y.agg_sum(y.col(1)), y.agg_sum1()])
    want, _ = y.oracle_execute(plan, chunk)
    assert len(want) == 3000
    dev = chunk.c_device(cuda)

    def run():
        got, _ = y.gpu_execute(plan, dev, max_groups_hint=1)
        assert scan_path() == SCAN_PATH_STR_GENERAL
        return got

    same_rows(balanced(run), want)


# ---- yt_gpu_query_partial_str and yt_gpu_merge_states_str ----

def partial(cuda, chunk, plan, cap):
    """the one-partition bottom query: (states, pool, counts, pool bytes)"""
    states_t = cuda.zeros((max(cap, 1), 4), dtype=cuda.int64, device="cuda")
    pool_cap = 64 * (chunk.row_count + 16)
    pool_t = cuda.zeros(pool_cap, dtype=cuda.uint8, device="cuda")
    counts, pbytes, _ = y.gpu_partial_str(plan, chunk.c_device(cuda), 1,
                                          states_t.data_ptr(), cap,
                                          pool_t.data_ptr(), pool_cap,
                                          max_groups_hint=4096)
    return states_t, pool_t, counts, pbytes


@pytest.mark.gpu
def test_partial_str(cuda):
    chunk = str_table()
    plan = dense_plan()
    want, _ = y.oracle_execute(plan, chunk)
    states_t, pool_t, counts, pbytes = balanced(
        lambda: partial(cuda, chunk, plan, chunk.row_count + 16))
    assert counts == [len(want)] and pbytes == [key_bytes(want)]
    got, _ = y.gpu_merge_str(plan, states_t.data_ptr(), counts,
                             pool_t.data_ptr(), pbytes,
                             col_types=[VT_STRING, VT_INT64],
                             max_groups_hint=4096)
    same_rows(got, want)
    fails("state/pool buffer too small",
          lambda: partial(cuda, chunk, plan, len(want) - 1))


@pytest.mark.gpu
def test_merge_states_str(cuda):
    chunk = str_table()
    plan = dense_plan()
    want, _ = y.oracle_execute(plan, chunk)
    need = key_bytes(want)
    states_t, pool_t, counts, pbytes = partial(cuda, chunk, plan,
                                               chunk.row_count + 16)

    def merge(**kw):
        got, _ = y.gpu_merge_str(plan, states_t.data_ptr(), counts,
                                 pool_t.data_ptr(), pbytes,
                                 col_types=[VT_STRING, VT_INT64],
                                 max_groups_hint=4096, **kw)
        return got

    same_rows(balanced(lambda: merge(pool_capacity=need)), want)
    fails("output rowset too small",
          lambda: merge(out_capacity=len(want) - 1))
    fails("string pool too small", lambda: merge(pool_capacity=need - 1))


@pytest.mark.gpu
def test_merge_states_str_table_grows(cuda):
    chunk = wide_table()
    plan = dense_plan()
    want, _ = y.oracle_execute(plan, chunk)
    states_t, pool_t, counts, pbytes = partial(cuda, chunk, plan,
                                               chunk.row_count + 16)
    assert counts == [3000]

    def merge():
        got, _ = y.gpu_merge_str(plan, states_t.data_ptr(), counts,
                                 pool_t.data_ptr(), pbytes,
                                 col_types=[VT_STRING, VT_INT64],
                                 max_groups_hint=1)       # 2048 slots
        return got

    same_rows(balanced(merge), want)


# ---- run_scan_topk ----

@pytest.mark.gpu
def test_topk(cuda):
    rng = np.random.default_rng(503)
    n = 5000
    d = rng.standard_normal(n) * 1e6
    v = rng.integers(0, 10**9, n, dtype=np.int64)
    chunk = y.Chunk([y.encode_double(d), y.encode_int64(v)], n)
    plan = y.Plan(projects=[y.col(0), y.col(1)], order_by=[(0, True)],
                  limit=77, offset=3)
    want, _ = y.oracle_execute(plan, chunk)
    dev = chunk.c_device(cuda)
    got, _ = balanced(lambda: y.gpu_execute(plan, dev))
    assert got == want and len(got) == 77
    d2 = d.copy()
    d2[123] = np.nan
    bad = y.Chunk([y.encode_double(d2), y.encode_int64(v)], n)
    bad_dev = bad.c_device(cuda)
    fails("NaN", lambda: y.gpu_execute(plan, bad_dev))


# ---- run_scan_project, host compaction ----

@pytest.mark.gpu
def test_scan_project_host_compaction(cuda):
    rng = np.random.default_rng(504)
    n = 5000
    a = rng.integers(-1000, 1000, n, dtype=np.int64)
    b = rng.integers(1, 100, n, dtype=np.int64)
    chunk = y.Chunk([y.encode_int64(a, max_segment_values=2048),
                     y.encode_int64(b, max_segment_values=2048)], n)
    dev = chunk.c_device(cuda)
    plan = y.Plan(filter=y.col(0) > 0, projects=[y.col(0), y.col(0) // y.col(1)])
    want, _ = y.oracle_execute(plan, chunk)
    assert 0 < len(want) < n

    def run(p=plan, **kw):
        got, _ = y.gpu_execute(p, dev, **kw)
        assert scan_path() == 0
        return got

    assert balanced(run) == want
    fails(CAPACITY, lambda: run(out_capacity=len(want) - 1))
    div0 = y.Plan(projects=[y.col(0) // (y.col(1) - y.col(1))])
    fails("Division by zero", lambda: run(div0))


# ---- scan_project_compact ----

def _proj_table():
    rng = np.random.default_rng(505)
    n = 700
    s = [None if rng.random() < 0.05 else b"name-%03d" % (i % 90)
         for i in range(n)]
    v = [int(x) for x in rng.integers(0, 1000, n)]
    chunk = y.Chunk([y.encode_string(s, max_segment_values=256),
                     y.encode_int64(np.array(v, dtype=np.int64),
                                    max_segment_values=256)], n)
    want = [(s[i], v[i]) for i in range(n) if v[i] > 500]
    return chunk, want


@pytest.mark.gpu
def test_scan_project_compact(cuda, monkeypatch):
    chunk, want = cached("proj", _proj_table)
    need = key_bytes(want)
    assert need > 0 and len(want) > 200
    dev = chunk.c_device(cuda)
    plan = y.Plan(filter=y.col(1) > 500, projects=[y.col(0), y.col(1)])

    def run(**kw):
        kw.setdefault("out_capacity", chunk.row_count + 16)
        got, _ = y.gpu_execute(plan, dev, **kw)
        assert scan_path() == SCAN_PATH_PROJ_COMPACT
        return got

    assert balanced(lambda: run(pool_bytes=need)) == want
    fails(CAPACITY, lambda: run(out_capacity=len(want) - 1))
    fails(CAPACITY, lambda: run(pool_bytes=need - 1))
    # eleven windows: the per-window blocks go back after each of them
    monkeypatch.setenv("YTQL_PROJ_WINDOW", "64")
    assert balanced(lambda: run(pool_bytes=need)) == want
    fails(CAPACITY, lambda: run(pool_bytes=need - 1))


# ---- partitioned GROUP BY ----

@pytest.mark.gpu
def test_partitioned_fallback_rung(cuda):
    """E2 of test_partition_modes: both partitioned rungs overflow,
    run_partitioned gives its buffers back and k_scan_fast finishes"""
    case = pm.E2
    chunk = case.chunk()        # owns the device tensors behind `dev`
    dev = chunk.c_device(cuda)
    plan = case.plan()

    def run():
        got, st = y.gpu_execute(plan, dev, max_groups_hint=case.hint)
        assert scan_path() == case.bits
        assert st.kernel_scan_launches == case.launches
        return got

    same_rows(balanced(run), case.rows())


@pytest.mark.gpu
def test_partitioned_capacity_error(cuda):
    case = pm.DP
    chunk = case.chunk()        # owns the device tensors behind `dev`
    dev = chunk.c_device(cuda)
    plan = case.plan()
    want = case.rows()

    def run(**kw):
        got, _ = y.gpu_execute(plan, dev, max_groups_hint=case.hint, **kw)
        assert scan_path() == case.bits
        return got

    same_rows(balanced(run), want)
    fails(CAPACITY, lambda: run(out_capacity=len(want) - 1))


# ---- versioned scan: the chunk handle keeps its blob ----

@pytest.mark.gpu
def test_versioned_scan_chunk_handle(cuda):
    rng = np.random.default_rng(506)
    rows, col = tv._gen(rng, 2000)
    _, vis = tv._model(rows, 500)
    assert 0 < sum(vis) < 2000

    def run():
        before = in_use()
        sc = y.gpu_versioned_scan_chunk(col, 500)
        assert sc.row_count == sum(vis)
        assert in_use() == before + 1            # the blob, and nothing else
        _abi.gpu_lib().yt_gpu_scan_chunk_free(C.byref(sc.chunk), sc._handle)
        sc._handle = C.c_void_p()                # freed: __del__ finds nothing

    balanced(run)
