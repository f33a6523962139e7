"""General string-key GROUP BY on the GPU: WHERE clause, the whole aggregate
family (sum / sum(1) / min / max / avg / first over expressions), DirectRle
key segments, mixed key layouts in one column, ragged segmentation, the
two-phase bottom query with a filter, and the refusals that remain.

Every GPU result is compared with the CPU oracle on the same chunk after
sorting by key. Integer, count, min, max and avg-of-int results are exact;
double sums and averages are within 1e-6 relative (atomic add order is not
fixed; values are drawn from [0, 1) so cancellation cannot defeat the
bound). Each test also pins the kernel set through
yt_gpu_debug_last_scan_path()."""
import ctypes as C
import os

import numpy as np
import pytest

import ytsaurus_amd as y
from ytsaurus_amd import _abi
from ytsaurus_amd._abi import (YtStateRow, VT_STRING, VT_INT64,
                               SCAN_PATH_STR_DENSE, SCAN_PATH_STR_GENERAL)


def scan_path():
    return _abi.gpu_lib().yt_gpu_debug_last_scan_path()


def rkey(r):
    return (r[0] is None, r[0] or b"")


def assert_rows(got, want, approx_cols=()):
    """rows equal after sorting by key; columns in approx_cols (doubles
    summed by atomics) within 1e-6 relative, everything else exact."""
    got = sorted(got, key=rkey)
    want = sorted(want, key=rkey)
    assert [r[0] for r in got] == [r[0] for r in want]
    for g, w in zip(got, want):
        assert len(g) == len(w)
        for c in range(1, len(w)):
            if c in approx_cols and w[c] is not None:
                assert g[c] is not None, (w[0], c)
                assert g[c] == pytest.approx(w[c], rel=1e-6, abs=0), (w[0], c)
            else:
                assert g[c] == w[c], (w[0], c, g[c], w[c])


def run_both(plan, chunk, cuda, approx_cols=(), path=SCAN_PATH_STR_GENERAL,
             hint=None):
    hint = hint or chunk.row_count + 16
    got, st = y.gpu_execute(plan, chunk.c_device(cuda), max_groups_hint=hint,
                            out_capacity=chunk.row_count + 16)
    assert scan_path() == path
    want, _ = y.oracle_execute(plan, chunk)
    assert_rows(got, want, approx_cols)
    return got, want, st


def seg_types(col):
    return [col._cenc.segments[j].type for j in range(col._cenc.segment_count)]


# ---- shared data (built once; never modified) ----

_CACHE = {}


def base_data():
    """20 000 rows, 300 keys, ~2 % null keys; col1 int64 with 10 % nulls,
    col2 double in [0,1) with 5 % nulls, g = 7*key_index (0 for null keys).
    Key segments of 8192 rows, col1 segments of 5000: ragged."""
    if "base" in _CACHE:
        return _CACHE["base"]
    rng = np.random.default_rng(1234)
    n = 20_000
    ki = rng.integers(0, 300, n)
    kn = rng.random(n) < 0.02
    keys = [None if kn[i] else "k%04d" % ki[i] for i in range(n)]
    v1 = rng.integers(-1000, 1000, n, dtype=np.int64)
    v1n = (rng.random(n) < 0.10).astype(np.uint8)
    # one group whose every col1 is null
    v1n[(ki == 17) & ~kn] = 1
    v2 = rng.random(n)
    v2n = (rng.random(n) < 0.05).astype(np.uint8)
    g = np.where(kn, 0, 7 * ki).astype(np.int64)
    chunk = y.Chunk([y.encode_string(keys, max_segment_values=8192),
                     y.encode_int64(v1, v1n, max_segment_values=5000),
                     y.encode_double(v2, v2n),
                     y.encode_int64(g)], n)
    _CACHE["base"] = chunk
    return chunk


def rle_keys():
    """1500 runs of 4 rows; key index i % 1200 so the first 300 keys come
    back in the second segment; every 37th run is null."""
    keys = []
    for i in range(1500):
        k = None if i % 37 == 0 else "long-string-key-number-%06d" % (i % 1200)
        keys += [k] * 4
    return keys


def rle_data():
    if "rle" in _CACHE:
        return _CACHE["rle"]
    keys = rle_keys()
    n = len(keys)
    rng = np.random.default_rng(77)
    v1 = rng.integers(-1000, 1000, n, dtype=np.int64)
    v1n = (rng.random(n) < 0.10).astype(np.uint8)
    chunk = y.Chunk([y.encode_string(keys, max_segment_values=4096),
                     y.encode_int64(v1, v1n)], n)
    _CACHE["rle"] = chunk
    return chunk


# ---- 1. the WHERE clause ----

@pytest.mark.gpu
def test_filter_honoured(cuda):
    chunk = base_data()
    plan = y.Plan(filter=y.col(1) > 0, keys=[y.col(0)],
                  aggs=[y.agg_sum(y.col(1)), y.agg_sum1()])
    got, want, st = run_both(plan, chunk, cuda)
    # the filter really removed rows (and the all-null group 17 with them)
    assert sum(r[2] for r in got) < chunk.row_count * 0.6
    assert b"k0017" not in {r[0] for r in got}
    assert st.rows_read == chunk.row_count
    assert st.grouped_row_count == len(want)


@pytest.mark.gpu
def test_filter_removes_whole_keys(cuda):
    chunk = base_data()
    plan = y.Plan(filter=y.col(3) < 1050, keys=[y.col(0)],
                  aggs=[y.agg_sum(y.col(1)), y.agg_sum1()])
    got, _, _ = run_both(plan, chunk, cuda)
    names = {r[0] for r in got}
    assert b"k0149" in names and b"k0150" not in names
    assert len(got) == 150 + 1          # keys 0..149 and the null key (g = 0)
    assert all(r[2] > 0 for r in got)   # absent, not present with a zero count


@pytest.mark.gpu
def test_filter_removes_every_row(cuda):
    chunk = base_data()
    plan = y.Plan(filter=y.col(3) < 0, keys=[y.col(0)],
                  aggs=[y.agg_sum(y.col(1)), y.agg_sum1()])
    got, want, _ = run_both(plan, chunk, cuda)
    assert got == [] and want == []


@pytest.mark.gpu
def test_filter_kleene_logic_and_division_by_zero(cuda):
    chunk = base_data()
    # null col1 OR true stays true, null OR false is null (row dropped)
    plan = y.Plan(filter=(y.col(1) > 0).or_(y.col(2) < 0.3).and_(
                      (y.col(3) % 2 == 0).not_()),
                  keys=[y.col(0)], aggs=[y.agg_sum(y.col(1)), y.agg_sum1()])
    run_both(plan, chunk, cuda)
    plan = y.Plan(filter=(y.col(1) // (y.col(3) - y.col(3))) > 0,
                  keys=[y.col(0)], aggs=[y.agg_sum1()])
    with pytest.raises(RuntimeError, match="Division by zero"):
        y.gpu_execute(plan, chunk.c_device(cuda), max_groups_hint=4096)
    rc, _, _ = y.oracle_execute(plan, chunk, expect_error=True)
    assert rc == _abi.YT_ERR_DIV_ZERO


@pytest.mark.gpu
def test_group_row_limit_matches_specialised_path(cuda):
    """group_row_limit marks the output incomplete the same way on both
    kernel sets (the identity merge still completes)"""
    chunk = base_data()
    dev = chunk.c_device(cuda)
    aggs = [y.agg_sum(y.col(3)), y.agg_sum1()]      # col3: one 20000-row segment
    chunk2 = y.Chunk([chunk.columns[0],
                      y.encode_int64(np.arange(20_000, dtype=np.int64),
                                     max_segment_values=8192)], 20_000)
    dense = y.Plan(keys=[y.col(0)], aggs=[y.agg_sum(y.col(1)), y.agg_sum1()])
    _, st_d = y.gpu_execute(dense, chunk2.c_device(cuda), max_groups_hint=1024,
                            group_row_limit=50)
    assert scan_path() == SCAN_PATH_STR_DENSE
    general = y.Plan(filter=y.col(3) >= 0, keys=[y.col(0)], aggs=aggs)
    _, st_g = y.gpu_execute(general, dev, max_groups_hint=1024,
                            group_row_limit=50)
    assert scan_path() == SCAN_PATH_STR_GENERAL
    assert st_d.incomplete_output == 1 and st_g.incomplete_output == 1
    assert st_d.grouped_row_count == st_g.grouped_row_count == 301
    _, st_g = y.gpu_execute(general, dev, max_groups_hint=1024)
    assert st_g.incomplete_output == 0


# ---- 2. aggregate family ----

@pytest.mark.gpu
def test_aggregate_family(cuda):
    chunk = base_data()
    plan = y.Plan(filter=(y.col(1) > -500).and_(y.col(2) < 0.9),
                  keys=[y.col(0)],
                  aggs=[y.agg_min(y.col(1)), y.agg_max(y.col(2)),
                        y.agg_avg(y.col(1)), y.agg_sum(y.col(1) * 2 + 1)])
    got, _, _ = run_both(plan, chunk, cuda)
    assert any(r[0] is None for r in got)            # null key group present


@pytest.mark.gpu
def test_group_with_all_null_argument(cuda):
    chunk = base_data()
    plan = y.Plan(filter=y.col(2) < 0.9, keys=[y.col(0)],
                  aggs=[y.agg_min(y.col(1)), y.agg_avg(y.col(1)),
                        y.agg_sum1(), y.agg_avg(y.col(2))])
    got, _, _ = run_both(plan, chunk, cuda, approx_cols=(4,))
    row = [r for r in got if r[0] == b"k0017"][0]
    assert row[1] is None and row[2] is None and row[3] > 0


# ---- 3. first() ----

@pytest.mark.gpu
def test_first(cuda):
    chunk = base_data()
    plan = y.Plan(filter=y.col(1) > -900, keys=[y.col(0)],
                  aggs=[y.agg_first(y.col(3)), y.agg_sum(y.col(1)),
                        y.agg_sum(y.col(2)), y.agg_sum1()])
    run_both(plan, chunk, cuda, approx_cols=(3,))


# ---- 4. uint64 and boolean arguments ----

@pytest.mark.gpu
def test_uint64_and_boolean_arguments(cuda):
    rng = np.random.default_rng(4321)
    n = 9000
    ki = rng.integers(0, 120, n)
    keys = ["u%03d" % k for k in ki]
    u = (rng.integers(0, 1 << 40, n, dtype=np.uint64)
         + np.uint64(1 << 63))                       # every value >= 2^63
    un = (rng.random(n) < 0.08).astype(np.uint8)
    b = (ki % 3 == 0) & (rng.random(n) < 0.5)        # keys with no true at all
    bn = (rng.random(n) < 0.1).astype(np.uint8)
    chunk = y.Chunk([y.encode_string(keys, max_segment_values=4096),
                     y.encode_int64(u.view(np.int64), un, unsigned=True,
                                    max_segment_values=3000),
                     y.encode_bool(b, bn)], n)
    plan = y.Plan(keys=[y.col(0)],
                  aggs=[y.agg_sum(y.col(1)), y.agg_min(y.col(1)),
                        y.agg_max(y.col(1)), y.agg_max(y.col(2))])
    got, _, _ = run_both(plan, chunk, cuda)
    assert all(r[2] is None or r[2] >= 1 << 63 for r in got)
    assert {r[4] for r in got} >= {True, False}


# ---- 5. DirectRle keys ----

@pytest.mark.gpu
def test_direct_rle_keys(cuda):
    chunk = rle_data()
    types = seg_types(chunk.columns[0])
    assert len(types) == 2 and _abi.SEG_DIRECT_RLE in types, types
    plan = y.Plan(keys=[y.col(0)], aggs=[y.agg_sum(y.col(1)), y.agg_sum1()])
    got, _, _ = run_both(plan, chunk, cuda)
    assert len(got) == len(set(rle_keys()))      # None counts as the null group
    plan = y.Plan(filter=y.col(1) > -200, keys=[y.col(0)],
                  aggs=[y.agg_sum(y.col(1)), y.agg_min(y.col(1)),
                        y.agg_sum1()])
    run_both(plan, chunk, cuda)


# ---- 6. mixed layouts in one column ----

@pytest.mark.gpu
def test_mixed_layouts_in_one_column(cuda):
    keys = (["k%03d" % (i % 50) for i in range(8192)]
            + ["z%06d" % i for i in range(8192)]
            + rle_keys())
    n = len(keys)
    rng = np.random.default_rng(66)
    v1 = rng.integers(-1000, 1000, n, dtype=np.int64)
    v1n = (rng.random(n) < 0.10).astype(np.uint8)
    chunk = y.Chunk([y.encode_string(keys, max_segment_values=4096),
                     y.encode_int64(v1, v1n, max_segment_values=7000)], n)
    types = seg_types(chunk.columns[0])
    assert len(set(types)) >= 3, types
    plan = y.Plan(filter=y.col(1) < 600, keys=[y.col(0)],
                  aggs=[y.agg_min(y.col(1)), y.agg_max(y.col(1)),
                        y.agg_sum1()])
    run_both(plan, chunk, cuda)


# ---- 7. composition with ORDER BY / HAVING / WITH TOTALS ----

def compose_data(with_null):
    rng = np.random.default_rng(707)
    n = 12_000
    ki = rng.integers(0, 200, n)
    keys = ["c%03d" % k for k in ki]
    if with_null:
        keys[5] = None
    v1 = rng.integers(-1000, 1000, n, dtype=np.int64)
    v1n = (rng.random(n) < 0.05).astype(np.uint8)
    return y.Chunk([y.encode_string(keys, max_segment_values=4096),
                    y.encode_int64(v1, v1n, max_segment_values=5000)], n)


@pytest.mark.gpu
def test_order_by_limit(cuda):
    chunk = compose_data(False)
    plan = y.Plan(filter=y.col(1) < 990, keys=[y.col(0)],
                  aggs=[y.agg_min(y.col(1)), y.agg_sum1()],
                  order_by=[(1, True), (0, False)], limit=10)
    got, _ = y.gpu_execute(plan, chunk.c_device(cuda), max_groups_hint=1024)
    assert scan_path() == SCAN_PATH_STR_GENERAL
    want, _ = y.oracle_execute(plan, chunk)
    assert len(want) == 10
    assert got == want                       # ordered output: no re-sorting


@pytest.mark.gpu
def test_with_totals_and_having(cuda):
    chunk = compose_data(False)
    plan = y.Plan(filter=y.col(1) > -990, keys=[y.col(0)],
                  aggs=[y.agg_sum(y.col(1)), y.agg_max(y.col(1))],
                  with_totals=True, having=y.col(2) > 900)
    got, _ = y.gpu_execute(plan, chunk.c_device(cuda), max_groups_hint=1024)
    assert scan_path() == SCAN_PATH_STR_GENERAL
    want, _ = y.oracle_execute(plan, chunk)
    assert 1 < len(want) < 201               # HAVING kept some, dropped some
    assert got[-1] == want[-1]               # the totals row comes last
    assert_rows(got[:-1], want[:-1])


@pytest.mark.gpu
def test_null_key_forbidden_under_order_by(cuda):
    chunk = compose_data(True)
    plan = y.Plan(filter=y.col(1) < 990, keys=[y.col(0)],
                  aggs=[y.agg_min(y.col(1)), y.agg_sum1()],
                  order_by=[(1, True), (0, False)], limit=10)
    with pytest.raises(RuntimeError,
                       match="Null values are forbidden in group key"):
        y.gpu_execute(plan, chunk.c_device(cuda), max_groups_hint=1024)
    rc, _, _ = y.oracle_execute(plan, chunk, expect_error=True)
    assert rc != _abi.YT_OK


# ---- 8. two-phase bottom query with a filter ----

def filtered_sum_plan():
    return y.Plan(filter=y.col(1) > 0, keys=[y.col(0)],
                  aggs=[y.agg_sum(y.col(1)), y.agg_sum1()])


def partial_on_gpu(cuda, chunk, world, plan):
    cap = chunk.row_count + 16
    states_t = cuda.zeros((cap, 4), dtype=cuda.int64, device="cuda")
    pool_cap = 64 * cap
    pool_t = cuda.zeros(pool_cap, dtype=cuda.uint8, device="cuda")
    counts, pbytes, _ = y.gpu_partial_str(plan, chunk.c_device(cuda), world,
                                          states_t.data_ptr(), cap,
                                          pool_t.data_ptr(), pool_cap,
                                          max_groups_hint=4096)
    return states_t, pool_t, counts, pbytes


@pytest.mark.gpu
def test_two_phase_with_filter_gpu_merge(cuda):
    chunk = base_data()
    plan = filtered_sum_plan()
    states_t, pool_t, counts, pbytes = partial_on_gpu(cuda, chunk, 1, plan)
    assert scan_path() == SCAN_PATH_STR_GENERAL
    got, _ = y.gpu_merge_str(plan, states_t.data_ptr(), counts,
                             pool_t.data_ptr(), pbytes,
                             col_types=[VT_STRING, VT_INT64],
                             max_groups_hint=4096)
    want, _ = y.oracle_execute(plan, chunk)
    assert_rows(got, want)


@pytest.mark.gpu
def test_two_phase_with_filter_oracle_merge(cuda):
    chunk = rle_data()                       # DirectRle keys, ragged value col
    plan = filtered_sum_plan()
    world = 2
    states_t, pool_t, counts, pbytes = partial_on_gpu(cuda, chunk, world, plan)
    assert scan_path() == SCAN_PATH_STR_GENERAL
    h_states = states_t.cpu().numpy().tobytes()
    h_pool = bytes(pool_t.cpu().numpy().tobytes())
    union = []
    for p in range(world):
        rbase = sum(counts[:p]) * C.sizeof(YtStateRow)
        bbase = sum(pbytes[:p])
        sb = h_states[rbase:rbase + counts[p] * C.sizeof(YtStateRow)]
        arr = (YtStateRow * max(counts[p], 1)).from_buffer_copy(
            sb or bytes(C.sizeof(YtStateRow)))
        union += y.oracle_merge_str(
            plan, [(arr, counts[p], h_pool[bbase:bbase + pbytes[p]], pbytes[p])])
    want, _ = y.oracle_execute(plan, chunk)
    assert_rows(union, want)


@pytest.mark.gpu
def test_two_phase_min_still_refused(cuda):
    chunk = rle_data()
    plan = y.Plan(keys=[y.col(0)], aggs=[y.agg_min(y.col(1)), y.agg_sum1()])
    with pytest.raises(RuntimeError, match="min/max/avg/first"):
        partial_on_gpu(cuda, chunk, 1, plan)


# ---- 9. refusals ----

@pytest.mark.gpu
def test_string_column_in_filter_refused(cuda):
    chunk = rle_data()
    plan = y.Plan(filter=y.col(0) == y.col(0), keys=[y.col(0)],
                  aggs=[y.agg_sum1()])
    with pytest.raises(RuntimeError, match="string column inside a filter"):
        y.gpu_execute(plan, chunk.c_device(cuda), max_groups_hint=4096)


@pytest.mark.gpu
def test_first_of_string_column_refused(cuda):
    chunk = rle_data()
    plan = y.Plan(keys=[y.col(0)], aggs=[y.agg_first(y.col(0)), y.agg_sum1()])
    with pytest.raises(RuntimeError, match="string"):
        y.gpu_execute(plan, chunk.c_device(cuda), max_groups_hint=4096)


# ---- 10. the specialised path keeps its plans ----

@pytest.mark.gpu
@pytest.mark.parametrize("int_sum", [False, True])
def test_old_path_untouched(cuda, int_sum):
    """the shapes of test_gpu_parity's test_string_group_by_gpu and
    test_string_group_by_gpu_int_sum stay on the specialised kernels"""
    n = 60_000
    if int_sum:
        rng = np.random.default_rng(18)
        keyset = ["s%d" % i for i in range(500)]
        keys = [keyset[int(i)] for i in rng.integers(0, 500, n)]
        vals = rng.integers(-10**9, 10**9, n, dtype=np.int64)
        chunk = y.Chunk([y.encode_string(keys, max_segment_values=8192),
                         y.encode_int64(vals, max_segment_values=8192)], n)
    else:
        rng = np.random.default_rng(17)
        keyset = ["key-%05d" % i for i in range(300)]
        kidx = rng.integers(0, 300, n)
        kn = rng.random(n) < 0.02
        keys = [None if kn[i] else keyset[int(kidx[i])] for i in range(n)]
        vals = rng.random(n)
        vn = (rng.random(n) < 0.05).astype(np.uint8)
        chunk = y.Chunk([y.encode_string(keys, max_segment_values=20000),
                         y.encode_double(vals, vn, max_segment_values=20000)], n)
    plan = y.Plan(keys=[y.col(0)], aggs=[y.agg_sum(y.col(1)), y.agg_sum1()])
    run_both(plan, chunk, cuda, approx_cols=() if int_sum else (1,),
             path=SCAN_PATH_STR_DENSE, hint=1024)


# ---- 11. without a device ----

def test_constants_and_no_gpu():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(repo, "include", "ytql_gpu.h")).read()
    assert "YT_SCAN_PATH_STR_DENSE   = 1 << 9" in hdr
    assert "YT_SCAN_PATH_STR_GENERAL = 1 << 10" in hdr
    assert SCAN_PATH_STR_DENSE == 1 << 9
    assert SCAN_PATH_STR_GENERAL == 1 << 10
    if y.gpu_available():
        return                               # the rest is about no device
    chunk = rle_data()
    plan = y.Plan(filter=y.col(1) > 0, keys=[y.col(0)],
                  aggs=[y.agg_min(y.col(1)), y.agg_sum1()])
    with pytest.raises(RuntimeError,
                       match="ytql error %d:" % _abi.YT_ERR_NO_GPU):
        y.gpu_execute(plan, chunk.c_host())
