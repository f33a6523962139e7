"""Multi-key GROUP BY with STRING keys on the GPU: every
result is compared with the Python model of test_multikey_strings_cpu.py,
which that file checks against the CPU oracle on the same data. Unordered
results compare after y.sort_rows, ORDER BY results exactly (they order on
all key columns, so the order is total); doubles within 1e-6 relative,
everything else bit-exact. Where the reference raises "Null values are
forbidden in group key", the GPU must raise it too.

A plan takes at most 4 aggregates, so "all six" are two plans
(six_aggs_spec)."""
import numpy as np
import pytest

import ytsaurus_amd as y
from ytsaurus_amd import _abi
from ytsaurus_amd._abi import (SCAN_PATH_GENERIC, SCAN_PATH_STR_IDS,
                               SCAN_PATH_STR_DENSE, SCAN_PATH_STR_GENERAL,
                               VT_STRING, VT_INT64)

import test_multikey_strings_cpu as m
from test_multikey_strings_cpu import Spec

pytestmark = pytest.mark.gpu

CAPACITY = "ytql error %d" % _abi.YT_ERR_CAPACITY
UNSUPPORTED = "ytql error %d" % _abi.YT_ERR_UNSUPPORTED
STR_PATH = SCAN_PATH_GENERIC | SCAN_PATH_STR_IDS

_DEV = {}


def dev(data, cuda):
    """the data set's device chunk, uploaded once"""
    if id(data) not in _DEV:
        _DEV[id(data)] = (data, data.chunk.c_device(cuda))
    return _DEV[id(data)][1]


def scan_path():
    return _abi.gpu_lib().yt_gpu_debug_last_scan_path()


def blocks():
    return int(_abi.gpu_lib().yt_gpu_debug_pool_blocks_in_use())


def gpu(spec, data, cuda, **kw):
    kw.setdefault("max_groups_hint", 4096)
    base = blocks()
    try:
        return y.gpu_execute(spec.plan(), dev(data, cuda), **kw)
    finally:
        assert blocks() == base     # success, refusal or capacity error


def check(spec, data, cuda, ordered=False, **kw):
    """GPU == model, or both raise the null-key error"""
    want = m.with_null_error(lambda: m.model(spec, data.rows))
    got = m.with_null_error(lambda: gpu(spec, data, cuda, **kw))
    if isinstance(want, str) or isinstance(got, str):
        assert want == m.NULL_KEY_ERROR and got == m.NULL_KEY_ERROR, (got, want)
        return want, None
    rows, st = got
    assert scan_path() == STR_PATH
    m.same_rows(rows, want, ordered=ordered, totals=spec.totals is not None)
    return want, st


def fails(code, text, fn):
    base = blocks()
    with pytest.raises(RuntimeError) as e:
        fn()
    assert code in str(e.value) and text in str(e.value), str(e.value)
    assert blocks() == base


SUMS = [("sum", 2), ("sum1", None)]


# ---- 1. the golden ----

def test_golden_group_order2_on_gpu(cuda):
    # GroupByOrderBy2, the data and rows of test_golden3.py
    a = list(range(1, 10))
    bs = [b"a", b"a", b"b", b"a", b"b", b"a", b"b", b"b", b"a"]
    c = [1, 2, 3, 4, 1, 2, 3, 4, 1]
    d = m.Data([("i", a, 0), ("s", bs, 0), ("i", c, 0)])
    spec = Spec([1, 2], [("sum", 0)], order=[(0, False), (1, False)], limit=6)
    rows, _ = gpu(spec, d, cuda, max_groups_hint=64)
    assert rows == [(b"a", 1, 10), (b"a", 2, 8), (b"a", 4, 4),
                    (b"b", 1, 5), (b"b", 3, 10), (b"b", 4, 8)]
    assert scan_path() == STR_PATH


# ---- 2. cross-segment identity, every layout ----

@pytest.mark.parametrize("layout,seg", m.LAYOUT_CASES)
def test_layouts(cuda, layout, seg):
    d = m.layout_data(layout, seg)
    types = d.seg_types(0)
    if layout == "mixed":
        assert len(set(types)) >= 3, types
    else:
        assert set(types) == {m.LAYOUT_TYPE[layout]}, types
    want, st = check(m.shape_specs()["sum_avg_min_sum1"], d, cuda)
    assert y.gpu_debug_last_strkey()[1] == 37
    assert len({r[0] for r in want if r[0] is not None}) == 37
    assert st.rows_read == d.n and st.rows_written == len(want)
    assert st.grouped_row_count == len(want)
    check(m.shape_specs()["two_string_columns"], d, cuda)
    assert y.gpu_debug_last_strkey()[1] == 37 + 3


# ---- 3. nulls ----

def test_nulls(cuda):
    d = m.null_data()
    want, _ = check(Spec([0, 1], [("sum", 3), ("sum1", None)]), d, cuda)
    keys = {r[:2] for r in want}
    assert {(b"a", None), (None, 1), (None, None), (b"", 1), (b"", None)} <= keys
    # a string column of nulls only: no distinct string, one code
    check(Spec([2, 1], [("sum1", None)]), d, cuda)
    assert y.gpu_debug_last_strkey()[1] == 0
    check(Spec([0, 2], [("sum", 3)]), d, cuda)
    assert y.gpu_debug_last_strkey()[1] == 2


# ---- 4. width edges ----

@pytest.mark.parametrize("dcount", m.WIDTH_D)
def test_widths(cuda, dcount):
    want, _ = check(Spec([0, 1], SUMS), m.width_data(dcount), cuda)
    assert y.gpu_debug_last_strkey()[1] == dcount
    assert len(want) == 2 * dcount
    check(Spec([1, 0], SUMS), m.width_data(dcount), cuda)


def test_62_bits_accepted_63_refused(cuda):
    # 3 strings: codes 0..3, 2 bits; the int key's component is 60 / 61 wide
    check(Spec([0, 1], [("sum", 2)]), m.wide_data(60), cuda)
    check(Spec([1, 0], [("sum", 2)]), m.wide_data(60), cuda)
    fails(UNSUPPORTED, "62 bits",
          lambda: gpu(Spec([0, 1], [("sum", 2)]), m.wide_data(61), cuda))


# ---- 5. position and count, 6. plan shapes ----

@pytest.mark.parametrize("name", sorted(m.shape_specs()))
def test_shapes(cuda, name):
    check(m.shape_specs()[name], m.layout_data("dict_dense", 100), cuda)
    check(m.shape_specs()[name], m.layout_data("mixed", 64), cuda)


def test_six_aggregates(cuda):
    for spec in m.six_aggs_spec():
        check(spec, m.layout_data("dict_dense", 100), cuda)
        check(spec, m.layout_data("mixed", 64), cuda)


def test_string_predicates_and_in_lists(cuda):
    s = m.strings37()
    pfx = b"0123456789abcdef"
    some = [s[0], s[1], s[3], s[7], s[20], b"not-in-the-column"]
    where = {
        "prefix_on_key": (y.is_prefix(pfx, y.col(0)),
                          lambda r: r[0] is not None and r[0].startswith(pfx)),
        "in_on_key": (y.isin(y.col(0), some), lambda r: r[0] in some),
        "prefix_on_other": (y.is_prefix(b"gre", y.col(4)),
                            lambda r: r[4] is not None and r[4].startswith(b"gre")),
        "in_on_other": (y.isin(y.col(4), [b"", b"red"]),
                        lambda r: r[4] in (b"", b"red")),
    }
    for name, w in where.items():
        for d in (m.layout_data("dict_dense", 100), m.layout_data("mixed", 64)):
            want, _ = check(Spec([0, 1], SUMS, where=w), d, cuda)
            assert 0 < len(want) < len(m.model(Spec([0, 1], SUMS), d.rows)), name
            check(Spec([4, 0], SUMS, where=w), d, cuda)


@pytest.mark.parametrize("name", sorted(m.totals_specs()))
def test_totals(cuda, name):
    spec = m.totals_specs()[name]
    want, _ = check(spec, m.no_allnull_data(), cuda)
    assert all(v is None for v in want[-1][:2])
    # (null, null) groups: refused as the reference refuses them
    assert check(spec, m.layout_data("dict_dense", 100), cuda)[0] == m.NULL_KEY_ERROR


@pytest.mark.parametrize("name", sorted(m.order_specs()))
def test_order_by(cuda, name):
    spec = m.order_specs()[name]
    want, _ = check(spec, m.no_allnull_data(), cuda, ordered=True)
    assert len(want) > 0
    assert check(spec, m.layout_data("dict_dense", 100), cuda,
                 ordered=True)[0] == m.NULL_KEY_ERROR


# ---- 7. limits and statistics ----

def dict_entries(keys, seg, nrows):
    """entries of the dictionary segments that hold rows [0, nrows)"""
    return sum(len({k for k in keys[a:a + seg] if k is not None})
               for a in range(0, nrows, seg))


def test_input_row_limit(cuda):
    d = m.layout_data("dict_dense", 100)
    spec = Spec([0, 1], SUMS)
    keep = 1050
    rows, st = gpu(spec, d, cuda, input_row_limit=keep)
    m.same_rows(rows, m.model(spec, d.rows[:keep]))
    assert st.incomplete_input == 1 and st.rows_read == keep
    entries, distinct = y.gpu_debug_last_strkey()
    keys = [r[0] for r in d.rows]
    assert entries == dict_entries(keys, 100, keep)
    assert entries < dict_entries(keys, 100, d.n)
    assert distinct == len({k for k in keys[:1100] if k is not None})


def test_output_row_limit(cuda):
    d = m.layout_data("dict_dense", 100)
    spec = Spec([0, 1], SUMS)
    want = m.model(spec, d.rows)
    rows, st = gpu(spec, d, cuda, output_row_limit=50)
    assert len(rows) == 50 and len(set(rows)) == 50
    assert set(rows) <= set(want)
    assert st.incomplete_output == 1
    rows, st = gpu(spec, d, cuda, output_row_limit=len(want))
    assert st.incomplete_output == 0
    m.same_rows(rows, want)


def test_capacity_errors_and_exact_pool(cuda):
    d = m.layout_data("dict_dense", 100)
    spec = Spec([0, 1], SUMS)
    want = m.model(spec, d.rows)
    need = sum(len(r[0]) for r in want if r[0] is not None)
    rs, st = gpu(spec, d, cuda, pool_bytes=need, raw_rowset=True)
    assert rs.string_pool_used == need
    m.same_rows(y.rows_from_rowset(rs), want)
    fails(CAPACITY, "string pool too small",
          lambda: gpu(spec, d, cuda, pool_bytes=need - 1))
    fails(CAPACITY, "", lambda: gpu(spec, d, cuda, out_capacity=len(want) - 1))
    # two string keys: both components' bytes are counted
    spec2 = Spec([0, 4], SUMS)
    want2 = m.model(spec2, d.rows)
    need2 = sum(len(v) for r in want2 for v in r[:2] if v is not None)
    rs, _ = gpu(spec2, d, cuda, pool_bytes=need2, raw_rowset=True)
    assert rs.string_pool_used == need2
    fails(CAPACITY, "string pool too small",
          lambda: gpu(spec2, d, cuda, pool_bytes=need2 - 1))
    # a group table too small for the 50,000 groups
    fails(CAPACITY, "max_groups_hint",
          lambda: gpu(spec, m.big_data(), cuda, max_groups_hint=100))


# ---- 8. diagnostics ----

def test_diagnostics(cuda):
    d = m.layout_data("dict_dense", 100)
    keys = [r[0] for r in d.rows]
    check(Spec([0, 1], SUMS), d, cuda)
    entries, distinct = y.gpu_debug_last_strkey()
    assert entries == dict_entries(keys, 100, d.n)
    assert entries < d.n // 2 and distinct == 37
    check(Spec([0, 1], SUMS), m.layout_data("dict_dense", 4096), cuda)
    assert y.gpu_debug_last_strkey() == (37, 37)
    # a single string key and an integer multi-key plan: their old paths, 0 / 0
    gpu(Spec([0], SUMS), d, cuda)
    assert scan_path() in (SCAN_PATH_STR_DENSE, SCAN_PATH_STR_GENERAL)
    assert y.gpu_debug_last_strkey() == (0, 0)
    rows, _ = gpu(Spec([1, 5], SUMS), d, cuda)
    m.same_rows(rows, m.model(Spec([1, 5], SUMS), d.rows))
    assert scan_path() == SCAN_PATH_GENERIC
    assert y.gpu_debug_last_strkey() == (0, 0)


# ---- 9. several full segments ----

def test_several_full_segments(cuda):
    d = m.big_data()
    assert len(d.seg_types(0)) == 3
    want, st = check(Spec([0, 1], SUMS), d, cuda, max_groups_hint=100_000)
    assert len(want) == 50_000 and st.grouped_row_count == 50_000
    assert y.gpu_debug_last_strkey()[1] == 1000


# ---- 10. refusals, 11. pool balance (fails() and gpu() check it) ----

def test_refusals(cuda):
    d = m.layout_data("dict_dense", 100)
    dc = dev(d, cuda)

    def run(**plan_kw):
        kw = dict(keys=[y.col(0), y.col(1)], aggs=[y.agg_sum(y.col(2))])
        kw.update(plan_kw)
        return y.gpu_execute(y.Plan(**kw), dc, max_groups_hint=4096)

    dim = y.Chunk([y.encode_int64(np.arange(5, dtype=np.int64)),
                   y.encode_int64(np.arange(5, dtype=np.int64) * 10)], 5)
    dimdev = dim.c_device(cuda)
    join_plan = y.Plan(keys=[y.col(0), y.col(1)], aggs=[y.agg_sum(y.col(2))],
                       join=y.Join(dim, 1, 0, [1]))
    fails(UNSUPPORTED, "a string key beside a join",
          lambda: y.gpu_execute(join_plan, dc, max_groups_hint=4096,
                                join_foreign=dimdev))
    fails(UNSUPPORTED, "post-projections on a plan with a string key",
          lambda: run(projects=[y.col(1), y.col(2)]))
    fails(UNSUPPORTED, "HAVING over string values",
          lambda: run(having=y.col(0) == y.lit_str(b"x")))
    fails(UNSUPPORTED, "HAVING over string values",
          lambda: run(having=y.col(0) == y.col(1)))
    fails(UNSUPPORTED, "plain key columns",
          lambda: run(keys=[y.col(0) + 1, y.col(1)]))
    fails(UNSUPPORTED, "string column inside an aggregate argument",
          lambda: run(aggs=[y.agg_sum(y.col(4))]))

    plan = y.Plan(keys=[y.col(0), y.col(1)],
                  aggs=[y.agg_sum(y.col(2)), y.agg_sum1()])
    fails(UNSUPPORTED, "cannot be exchanged", lambda: y.gpu_key_ranges(plan, dc))
    states = cuda.zeros(32 * 1024, dtype=cuda.uint8, device="cuda")
    ranges = ([0, 0], [40, 10])
    fails(UNSUPPORTED, "cannot be exchanged",
          lambda: y.gpu_partial_mk(plan, dc, 2, states.data_ptr(), 1024, ranges))
    fails(UNSUPPORTED, "cannot be exchanged",
          lambda: y.gpu_merge_mk(plan, states.data_ptr(), 0, ranges,
                                 col_types=[VT_STRING, VT_INT64, VT_INT64]))
