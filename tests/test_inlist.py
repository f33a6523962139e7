"""IN lists in WHERE on the GPU: numeric expressions and string columns.

Every reference here is plain Python: set membership answers the IN leaf per
row (None in the list matches a null cell; the answer is never null), and a
few lines of Python do the GROUP BY / scan / ORDER BY around it. Nothing on
the reference side calls the library. Integer sums wrap modulo 2^64 as the
engine's do; no floating point is involved, so every comparison is exact.

Numeric chunks have 10,000 rows in segments of 4096 + 4096 + 1808 rows (1808
is no multiple of 64). String chunks are those of test_string_predicates:
20,000 rows in ten segments, the last of 1568 rows, dictionaries of 63, 64,
65 and 300 entries."""
import ctypes as C

import numpy as np
import pytest

import ytsaurus_amd as y
from ytsaurus_amd import _abi
from ytsaurus_amd._abi import (VT_STRING, VT_INT64, VT_DOUBLE, VT_BOOLEAN,
                               SEG_DICTIONARY_DENSE, SEG_DICTIONARY_RLE,
                               SEG_DIRECT_DENSE, SEG_DIRECT_RLE)

import test_string_predicates as sp
from test_string_predicates import c, seg_types

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = _abi.YT_ERR_UNSUPPORTED, _abi.YT_ERR_INVALID_PLAN
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
M64 = (1 << 64) - 1
N = 10_000
SEG = 4096
EXTREMES = [0, -1, I64_MIN, I64_MAX]


def lib():
    return _abi.gpu_lib()


def wrap(v):
    v &= M64
    return v - (1 << 64) if v >= (1 << 63) else v


# ---------------------------------------------------------------------
# numeric data: column 0 = the operand in one of six forms, 1 = int64 value
# with 10 % nulls, 2 = int64 key 0..6, 3 = a string column, 4 = double

def operand_values(form, rng):
    """N python values (int / bool / None) of the operand column"""
    if form == "direct_dense":
        v = [int(x) for x in rng.integers(I64_MIN, I64_MAX, N, dtype=np.int64)]
        v[:4] = EXTREMES
        v[5000:5004] = EXTREMES
        v[9996:10000] = EXTREMES
    elif form == "dict_dense":
        pop = EXTREMES + [int(x) for x in
                          rng.integers(I64_MIN, I64_MAX, 36, dtype=np.int64)]
        v = [pop[i] for i in rng.integers(0, len(pop), N)]
    elif form == "direct_rle":
        v = []
        while len(v) < N:
            x = int(rng.integers(I64_MIN, I64_MAX, dtype=np.int64))
            if len(v) % 1024 < 32:
                x = EXTREMES[(len(v) // 8) % 4]
            v += [x] * 8
        v = v[:N]
    elif form == "dict_rle":
        pop = EXTREMES + [int(x) for x in
                          rng.integers(I64_MIN, I64_MAX, 12, dtype=np.int64)]
        v = []
        while len(v) < N:
            v += [pop[int(rng.integers(0, len(pop)))]] * 8
        v = v[:N]
    elif form == "uint64":
        v = [int(x) for x in rng.integers(0, 1 << 63, N, dtype=np.uint64) * 2 + 1]
        for at in (0, 5000, 9990):
            v[at:at + 4] = [0, 1 << 63, M64, (1 << 63) + 1]
    elif form == "boolean":
        v = [bool(x) for x in rng.integers(0, 2, N)]
    else:
        raise AssertionError(form)
    if form in ("direct_rle", "dict_rle"):
        for s in range(64, N, 640):                  # null runs
            v[s:s + 8] = [None] * 8
    else:
        v = [None if (i % 97 == 13) else x for i, x in enumerate(v)]
    return v


FORMS = {"direct_dense": SEG_DIRECT_DENSE, "dict_dense": SEG_DICTIONARY_DENSE,
         "direct_rle": SEG_DIRECT_RLE, "dict_rle": SEG_DICTIONARY_RLE,
         "uint64": SEG_DIRECT_DENSE, "boolean": None}
_NUM = {}
_DEV = {}


class NumData:
    def __init__(self, form):
        rng = np.random.default_rng(sorted(FORMS).index(form) + 50)
        self.form = form
        self.x = operand_values(form, rng)
        nulls = np.array([a is None for a in self.x], dtype=np.uint8)
        if form == "boolean":
            col0 = y.encode_bool(np.array([bool(a) for a in self.x], np.uint8),
                                 nulls, max_segment_values=SEG)
        elif form == "uint64":
            arr = np.array([a or 0 for a in self.x], dtype=np.uint64)
            col0 = y.encode_int64(arr.view(np.int64), nulls,
                                  max_segment_values=SEG, unsigned=True)
        else:
            arr = np.array([a or 0 for a in self.x], dtype=np.int64)
            col0 = y.encode_int64(arr, nulls, max_segment_values=SEG)
        r2 = np.random.default_rng(7)
        v = r2.integers(-1000, 1000, N, dtype=np.int64)
        vn = r2.random(N) < 0.10
        self.v = [None if n else int(a) for a, n in zip(v, vn)]
        self.k = [int(a) for a in r2.integers(0, 7, N)]
        self.s = [None if i % 50 == 7 else b"t%02d" % (i % 23) for i in range(N)]
        self.chunk = y.Chunk([
            col0,
            y.encode_int64(v, vn.astype(np.uint8), max_segment_values=SEG),
            y.encode_int64(np.array(self.k, dtype=np.int64),
                           max_segment_values=SEG),
            y.encode_string(self.s, max_segment_values=SEG),
            y.encode_double(r2.random(N), max_segment_values=SEG)], N)


def num(form):
    if form not in _NUM:
        _NUM[form] = NumData(form)
    return _NUM[form]


def num_dev(cuda, form):
    if form not in _DEV:
        _DEV[form] = num(form).chunk.c_device(cuda)
    return _DEV[form]


def str_dev(cuda, name):
    return sp.dev_chunk(cuda, name)


# ---------------------------------------------------------------------
# the Python reference

def ref_in(values, lst):
    """per-row answer of `value IN lst`: never None"""
    members = set(a for a in lst if a is not None)
    has_null = any(a is None for a in lst)
    return [has_null if a is None else (a in members) for a in values]


def ref_group(keys, vals, mask):
    """SELECT k, sum(v), sum(1) WHERE mask GROUP BY k"""
    acc = {}
    for k, v, m in zip(keys, vals, mask):
        if not m:
            continue
        s, nn, cnt = acc.get(k, (0, 0, 0))
        if v is not None:
            s, nn = s + v, nn + 1
        acc[k] = (s, nn, cnt + 1)
    return [(k, wrap(s) if nn else None, cnt) for k, (s, nn, cnt) in acc.items()]


def group_plan(f, key=2, val=1, **kw):
    return y.Plan(filter=f, keys=[c(key)], aggs=[y.agg_sum(c(val)), y.agg_sum1()],
                  **kw)


def run(cuda, plan, dev, **kw):
    kw.setdefault("max_groups_hint", 4096)
    got, _ = y.gpu_execute(plan, dev, **kw)
    return got


def same_groups(got, want):
    assert y.sort_rows(got) == y.sort_rows(want)


def in_list(form, d, size, with_null, rng):
    """a list of `size` values: some of the column's (the extremes among
    them), the rest misses, duplicates from 63 on; plus None"""
    present = [a for a in d.x if a is not None]
    if form == "boolean":
        lst = [[True], [False, False]][size - 1] if size <= 2 else [True] * size
    else:
        # hits come from one half of the distinct values, so that a long
        # list over a small dictionary still leaves rows out
        half = sorted(set(present))
        half = half[:len(half) // 2]
        hits = present[:4] + [half[int(i)] for i in
                              rng.integers(0, len(half), max(size // 3, 1))]
        if form == "uint64":
            miss = [int(a) for a in rng.integers(0, 1 << 63, size,
                                                 dtype=np.uint64) * 2]
        else:
            miss = [int(a) for a in rng.integers(I64_MIN, I64_MAX, size,
                                                 dtype=np.int64)]
        lst = (hits + miss)[:size]
        if size >= 63:
            lst[10:14] = lst[20:24]
    return lst + ([None] if with_null else [])


def as_values(form, lst):
    """the list as y.isin takes it: long lists as numpy arrays"""
    if form == "boolean" or None in lst or len(lst) < 1000:
        return lst, form == "uint64"
    dt = np.uint64 if form == "uint64" else np.int64
    return np.array(lst, dtype=dt), False


@pytest.mark.parametrize("size", [1, 2, 1000, 100_000])
@pytest.mark.parametrize("form", list(FORMS))
def test_numeric_in_filters_an_int_key_group_by(cuda, form, size):
    d = num(form)
    if FORMS[form] is not None:
        assert seg_types(d.chunk.columns[0]) == [FORMS[form]] * 3, form
    rng = np.random.default_rng(size)
    for with_null in (False, True):
        lst = in_list(form, d, size, with_null, rng)
        vals, unsigned = as_values(form, lst)
        plan = group_plan(y.isin(c(0), vals, unsigned=unsigned))
        mask = ref_in(d.x, lst)
        assert 0 < sum(mask) < N
        same_groups(run(cuda, plan, num_dev(cuda, form)),
                    ref_group(d.k, d.v, mask))


def test_numeric_extremes_one_by_one(cuda):
    d = num("direct_dense")
    for v in EXTREMES:
        mask = ref_in(d.x, [v])
        assert sum(mask) == 3
        same_groups(run(cuda, group_plan(c(0).isin([v])),
                        num_dev(cuda, "direct_dense")),
                    ref_group(d.k, d.v, mask))
    du = num("uint64")
    for v in (0, 1 << 63, M64):
        mask = ref_in(du.x, [v])
        assert sum(mask) == 3
        same_groups(run(cuda, group_plan(c(0).isin([v], unsigned=True)),
                        num_dev(cuda, "uint64")),
                    ref_group(du.k, du.v, mask))


def test_empty_and_null_only_numeric_lists(cuda):
    d = num("dict_dense")
    dev = num_dev(cuda, "dict_dense")
    assert run(cuda, group_plan(c(0).isin([])), dev) == []
    mask = [a is None for a in d.x]
    same_groups(run(cuda, group_plan(c(0).isin([None, None])), dev),
                ref_group(d.k, d.v, mask))
    # NOT over the empty list keeps every row, the null cells included
    same_groups(run(cuda, group_plan(c(0).isin([]).not_()), dev),
                ref_group(d.k, d.v, [True] * N))


def test_not_in_and_in_beside_other_predicates(cuda):
    d = num("dict_dense")
    dev = num_dev(cuda, "dict_dense")
    pop = sorted(set(a for a in d.x if a is not None))
    lst = pop[::3] + [12345]
    inn = ref_in(d.x, lst)
    # NOT IN is never null: a null cell is kept unless the list holds null
    same_groups(run(cuda, group_plan(c(0).isin(lst).not_()), dev),
                ref_group(d.k, d.v, [not m for m in inn]))
    same_groups(run(cuda, group_plan(c(0).isin(lst + [None]).not_()), dev),
                ref_group(d.k, d.v, [not m for m in ref_in(d.x, lst + [None])]))
    # AND / OR with a range predicate (v null: the comparison is false for
    # `v > 100`, null < any value)
    rng_ = [v is not None and v > 100 for v in d.v]
    same_groups(run(cuda, group_plan(c(0).isin(lst).and_(c(1) > 100)), dev),
                ref_group(d.k, d.v, [a and b for a, b in zip(inn, rng_)]))
    same_groups(run(cuda, group_plan(c(0).isin(lst).or_(c(1) > 100)), dev),
                ref_group(d.k, d.v, [a or b for a, b in zip(inn, rng_)]))
    # with a string predicate, and with a string IN, in one filter
    pre = [None if s is None else s.startswith(b"t1") for s in d.s]
    f = c(0).isin(lst).and_(y.is_prefix(b"t1", c(3)))
    same_groups(run(cuda, group_plan(f), dev),
                ref_group(d.k, d.v, [a and bool(b) for a, b in zip(inn, pre)]))
    sin = ref_in(d.s, [b"t03", b"t22", None])
    f = c(0).isin(lst).or_(c(3).isin([b"t03", b"t22", None]))
    same_groups(run(cuda, group_plan(f), dev),
                ref_group(d.k, d.v, [a or b for a, b in zip(inn, sin)]))
    # two lists over two columns
    kin = ref_in(d.k, [1, 5])
    f = c(0).isin(lst).and_(c(2).isin([1, 5]).not_())
    same_groups(run(cuda, group_plan(f), dev),
                ref_group(d.k, d.v, [a and not b for a, b in zip(inn, kin)]))


def py_mod(a, b):
    """the engine's int64 %: truncated toward zero"""
    r = abs(a) % abs(b)
    return -r if a < 0 else r


def test_numeric_in_over_an_expression_wherever_one_compiles(cuda):
    d = num("direct_dense")
    dev = num_dev(cuda, "direct_dense")
    m10 = [None if a is None else py_mod(a, 10) for a in d.x]
    lst = [0, 3, -7, None]
    inn = ref_in(m10, lst)
    assert 0 < sum(inn) < N
    # in the filter
    same_groups(run(cuda, group_plan((c(0) % 10).isin(lst)), dev),
                ref_group(d.k, d.v, inn))
    # as a group key: a boolean key that is never null
    got = run(cuda, y.Plan(keys=[(c(0) % 10).isin(lst)],
                           aggs=[y.agg_sum(c(1)), y.agg_sum1()]), dev)
    same_groups(got, ref_group(inn, d.v, [True] * N))
    assert sorted(r[0] for r in got) == [False, True]
    # inside a sum argument: the sum of the 0/1 answers, read as raw bits
    # (the value's type tag is the argument's, BOOLEAN)
    rs, _ = y.gpu_execute(y.Plan(keys=[c(2)],
                                 aggs=[y.agg_sum((c(0) % 10).isin(lst)),
                                       y.agg_sum1()]),
                          dev, max_groups_hint=4096, raw_rowset=True)
    got = sorted((rs.values[r * 3].data.i64, rs.values[r * 3 + 1].data.u64,
                  rs.values[r * 3 + 2].data.i64) for r in range(rs.row_count))
    want = {}
    for k, m in zip(d.k, inn):
        a, b = want.get(k, (0, 0))
        want[k] = (a + int(m), b + 1)
    assert got == sorted((k, a, b) for k, (a, b) in want.items())
    # as a projection of a plain scan, in row order
    got = run(cuda, y.Plan(filter=c(2) == 4,
                           projects=[c(1), (c(0) % 10).isin(lst)]),
              dev, out_capacity=N + 16)
    assert got == [(v, m) for v, m, k in zip(d.v, inn, d.k) if k == 4]
    # ... and under ORDER BY ... LIMIT
    got = run(cuda, y.Plan(filter=(c(0) % 10).isin(lst),
                           projects=[c(1), c(2)],
                           order_by=[(0, True), (1, False)], limit=20), dev)
    rows = [(v, k) for v, k, m in zip(d.v, d.k, inn) if m]
    rows.sort(key=lambda r: ((1, 0) if r[0] is None else (0, -r[0]), r[1]))
    assert got == rows[:20]


def test_numeric_in_in_having(cuda):
    d = num("dict_rle")
    dev = num_dev(cuda, "dict_rle")
    groups = ref_group(d.k, d.v, [True] * N)
    plan = y.Plan(keys=[c(2)], aggs=[y.agg_sum(c(1)), y.agg_sum1()],
                  having=c(0).isin([0, 3, 5, 99]))
    same_groups(run(cuda, plan, dev), [g for g in groups if g[0] in (0, 3, 5)])
    counts = sorted(g[2] for g in groups)
    keep = [counts[0], counts[3], counts[3], -1]
    plan = y.Plan(keys=[c(2)], aggs=[y.agg_sum(c(1)), y.agg_sum1()],
                  having=c(2).isin(keep).not_().or_(c(0).isin([None])))
    same_groups(run(cuda, plan, dev), [g for g in groups if g[2] not in keep])


def test_numeric_in_on_a_foreign_column(cuda):
    d = num("dict_dense")
    dev = num_dev(cuda, "dict_dense")
    # keys 0..4 have a foreign row; the value of key 2 is null. LEFT join:
    # rows with key 5 or 6 see a null foreign value
    fk = np.arange(5, dtype=np.int64)
    fv = fk * 10
    foreign = y.Chunk([y.encode_int64(fk),
                       y.encode_int64(fv, np.array([0, 0, 1, 0, 0], np.uint8))], 5)
    fdev = foreign.c_device(cuda)
    fval = {0: 0, 1: 10, 2: None, 3: 30, 4: 40, 5: None, 6: None}
    for lst in ([10, 40, 77], [10, None]):
        plan = y.Plan(filter=c(5).isin(lst), keys=[c(2)],
                      aggs=[y.agg_sum(c(1)), y.agg_sum1()],
                      join=y.Join(foreign, 2, 0, [1], is_left=True))
        mask = ref_in([fval[k] for k in d.k], lst)
        same_groups(run(cuda, plan, dev, join_foreign=fdev),
                    ref_group(d.k, d.v, mask))


# ---------------------------------------------------------------------
# string IN. Columns of sp.data(): 0 string (the layouts), 1 int64 with
# nulls, 2 double, 3 int64 key 0..6, 4 second string column, 5 int64 key 0..4

def sdata(name):
    d = sp.data(name)
    v1 = [None if n else int(a) for a, n in zip(d.raw["v1"], d.raw["v1n"])]
    return d, v1, [int(a) for a in d.raw["k3"]]


def last_entries():
    return lib().yt_gpu_debug_last_strpred_entries()


def last_mode():
    return lib().yt_gpu_debug_last_inlist_mode()


def sample_list(texts, rng, k):
    """k distinct values of the column plus as many misses: a last-byte
    neighbour of each, which has the same length"""
    present = sorted(set(t for t in texts if t))
    pick = [present[int(i)] for i in rng.permutation(len(present))[:k]]
    near = [t[:-1] + bytes([t[-1] ^ 1]) for t in pick]
    return pick + [t for t in near if t not in set(present)]


@pytest.mark.parametrize("layout", list(sp.LAYOUTS))
def test_string_in_over_every_layout(cuda, layout):
    d, v1, k3 = sdata(layout)
    assert seg_types(d.chunk.columns[0]) == sp.LAYOUTS[layout][1]
    assert d.chunk.columns[0].segments[-1].row_count % 64 != 0
    dev = str_dev(cuda, layout)
    rng = np.random.default_rng(5)
    base = sample_list(d.cols[0], rng, 40)
    for lst in (base, base + [None], base + [b""], [b"", None] + base[:3]):
        mask = ref_in(d.cols[0], lst)
        assert 0 < sum(mask) < sp.N
        same_groups(run(cuda, group_plan(c(0).isin(lst), key=3), dev),
                    ref_group(k3, v1, mask))
        assert last_entries() > 0 and last_mode() == 1
        same_groups(run(cuda, group_plan(c(0).isin(lst).not_(), key=3), dev),
                    ref_group(k3, v1, [not m for m in mask]))


def test_five_values_the_list_an_or_of_eq_cannot_hold(cuda):
    d, v1, k3 = sdata("dict_dense")
    lst = [b"", b"s-key-0005", b"s-key-0100", b"\xff\xfe-high", b"nope"]
    mask = ref_in(d.cols[0], lst)
    assert len({t for t, m in zip(d.cols[0], mask) if m}) == 4
    same_groups(run(cuda, group_plan(c(0).isin(lst), key=3),
                    str_dev(cuda, "dict_dense")), ref_group(k3, v1, mask))
    # the entry pass saw every dictionary entry once
    assert last_entries() == sum(
        len({t for t in d.cols[0][s:s + sp.SEG] if t is not None})
        for s in range(0, sp.N, sp.SEG))


def test_lists_on_both_sides_of_the_lds_budget(cuda):
    """1024 slots of 16 bytes fit the 16 KiB the entry kernel stages: 512
    distinct strings probe in LDS (mode 1), 513 in global memory (mode 2)"""
    d, v1, k3 = sdata("mixed")
    dev = str_dev(cuda, "mixed")
    present = sorted(set(t for t in d.cols[0] if t is not None))
    assert len(present) > 700
    for count, mode in ((512, 1), (513, 2), (3000, 2)):
        lst = present[:count // 2] + [b"absent-%05d" % i
                                      for i in range(count - count // 2)]
        assert len(set(lst)) == count
        mask = ref_in(d.cols[0], lst)
        assert 0 < sum(mask) < sp.N
        same_groups(run(cuda, group_plan(c(0).isin(lst), key=3), dev),
                    ref_group(k3, v1, mask))
        assert last_mode() == mode, count
    # duplicates do not count against the budget
    lst = (present[:300] + present[:300]) * 2
    same_groups(run(cuda, group_plan(c(0).isin(lst), key=3), dev),
                ref_group(k3, v1, ref_in(d.cols[0], lst)))
    assert last_mode() == 1


def test_null_only_string_list_takes_no_bitmap(cuda):
    d, v1, k3 = sdata("dict_rle")
    dev = str_dev(cuda, "dict_rle")
    mask = [t is None for t in d.cols[0]]
    same_groups(run(cuda, group_plan(c(0).isin([None, None]), key=3), dev),
                ref_group(k3, v1, mask))
    assert last_entries() == 0 and last_mode() == 0
    assert run(cuda, group_plan(c(0).isin([]), key=3), dev) == []
    assert last_entries() == 0 and last_mode() == 0
    same_groups(run(cuda, group_plan(c(0).isin([None]).not_(), key=3), dev),
                ref_group(k3, v1, [not m for m in mask]))


def test_string_in_on_every_plan_shape(cuda):
    d, v1, k3 = sdata("mixed")
    dev = str_dev(cuda, "mixed")
    s0, s4 = d.cols[0], d.cols[4]
    k5 = [int(a) for a in d.raw["k5"]]
    rng = np.random.default_rng(8)
    lst = sample_list(s0, rng, 60) + [None]
    m0 = ref_in(s0, lst)
    lst4 = [b"h03", b"h17", b"h39", b"h40", b""]
    m4 = ref_in(s4, lst4)
    assert 0 < sum(m0) < sp.N and 0 < sum(m4) < sp.N
    # string-key GROUP BY: the list on the key column, and on another one
    got = run(cuda, group_plan(c(0).isin(lst), key=0), dev,
              max_groups_hint=sp.N, out_capacity=sp.N + 16)
    assert sp.scan_path() == _abi.SCAN_PATH_STR_GENERAL
    same_groups(got, ref_group(s0, v1, m0))
    got = run(cuda, group_plan(c(4).isin(lst4), key=0), dev,
              max_groups_hint=sp.N, out_capacity=sp.N + 16)
    same_groups(got, ref_group(s0, v1, m4))
    # plain scan that projects the string column
    got = run(cuda, y.Plan(filter=c(0).isin(lst), projects=[c(0), c(1)]), dev,
              out_capacity=sp.N + 16)
    assert sp.scan_path() == _abi.SCAN_PATH_PROJ_COMPACT
    assert got == [(s, v) for s, v, m in zip(s0, v1, m0) if m]
    # ORDER BY ... LIMIT
    got = run(cuda, y.Plan(filter=c(0).isin(lst).and_(c(4).isin(lst4).not_()),
                           projects=[c(1), c(3), c(5)],
                           order_by=[(0, False), (1, True), (2, False)],
                           limit=25), dev)
    rows = [(v, a, b) for v, a, b, x, z in zip(v1, k3, k5, m0, m4) if x and not z]
    rows.sort(key=lambda r: ((0, 0) if r[0] is None else (1, r[0]), -r[1], r[2]))
    assert got == rows[:25]
    # a bottom query and its front query
    plan = group_plan(c(0).isin(lst), key=3)
    states = cuda.zeros((1024, 4), dtype=cuda.int64, device="cuda")
    counts, _ = y.gpu_partial(plan, dev, 3, states.data_ptr(), 1024,
                              max_groups_hint=4096)
    assert last_entries() > 0
    got, _ = y.gpu_merge(plan, states.data_ptr(), sum(counts),
                         max_groups_hint=4096,
                         col_types=[VT_STRING, VT_INT64, VT_DOUBLE, VT_INT64])
    same_groups(got, ref_group(k3, v1, m0))
    # input_row_limit inside a segment: 7000 = 3 segments of 2048 + 856 rows
    cut = sp.ROW_LIMIT
    got = run(cuda, plan, dev, input_row_limit=cut)
    same_groups(got, ref_group(k3[:cut], v1[:cut], m0[:cut]))
    got = run(cuda, y.Plan(filter=c(0).isin(lst), projects=[c(0), c(3)]), dev,
              input_row_limit=cut, out_capacity=sp.N + 16)
    assert got == [(s, k) for s, k, m in zip(s0[:cut], k3[:cut], m0[:cut]) if m]


def test_four_bitmaps_pass_and_a_fifth_is_refused(cuda):
    d, v1, k3 = sdata("dict_dense")
    dev = str_dev(cuda, "dict_dense")
    s0, s4 = d.cols[0], d.cols[4]
    a = [b"s-key-0010", b"s-key-0011", b""]
    b = [b"h01", b"h02", b"h03"]
    cc = [b"s-key-0200", None]
    f = c(0).isin(a).or_(c(4).isin(b)).or_(c(0).isin(cc)).or_(
        y.is_prefix(b"s-key-02", c(0)))
    pre = [t is not None and t.startswith(b"s-key-02") for t in s0]
    mask = [w or x or z or p for w, x, z, p in
            zip(ref_in(s0, a), ref_in(s4, b), ref_in(s0, cc), pre)]
    same_groups(run(cuda, group_plan(f, key=3), dev), ref_group(k3, v1, mask))
    # a null-only list needs no bitmap and still fits
    same_groups(run(cuda, group_plan(f.or_(c(4).isin([None])), key=3), dev),
                ref_group(k3, v1, [m or t is None for m, t in zip(mask, s4)]))
    refused(cuda, group_plan(f.or_(c(4).isin([b"h09"])), key=3),
            UNSUPPORTED, "more than 4 string predicates")


# ---------------------------------------------------------------------
# refusals

def refused(cuda, plan, code, message, dev=None, **kw):
    with pytest.raises(RuntimeError,
                       match=r"ytql error %d: .*%s" % (code, message)):
        y.gpu_execute(plan, dev or str_dev(cuda, "dict_dense"),
                      max_groups_hint=4096, **kw)


def test_refusals(cuda):
    aggs = [y.agg_sum1()]
    grp = dict(keys=[c(3)], aggs=aggs)
    # tuple operands, a DOUBLE operand
    refused(cuda, y.Plan(filter=y.isin((c(1), c(3)), [1]), **grp),
            UNSUPPORTED, "tuple operand")
    refused(cuda, y.Plan(filter=c(2).isin([1]), **grp), UNSUPPORTED, "DOUBLE")
    refused(cuda, y.Plan(filter=(c(2) + 1.0).isin([1]), **grp),
            UNSUPPORTED, "DOUBLE")
    # a string operand that is no plain column of the primary chunk
    refused(cuda, y.Plan(filter=y.isin(y.lit_str(b"a"), [b"a"]), **grp),
            UNSUPPORTED, "plain string column")
    # a string IN outside the filter: the messages string predicates get
    refused(cuda, y.Plan(keys=[c(0).isin([b"a"])], aggs=aggs),
            UNSUPPORTED, "string column inside a filter or key expression")
    refused(cuda, y.Plan(keys=[c(3)], aggs=[y.agg_sum(c(0).isin([b"a"]))]),
            UNSUPPORTED, "string column inside an aggregate argument")
    refused(cuda, y.Plan(keys=[c(0)], aggs=[y.agg_max(c(4).isin([None]))]),
            UNSUPPORTED, "string column inside an aggregate argument")
    refused(cuda, y.Plan(projects=[c(1), c(0).isin([b"a"])]), UNSUPPORTED,
            "inside a projection")
    refused(cuda, y.Plan(keys=[c(3)], aggs=aggs, having=c(1).isin([b"x"])),
            UNSUPPORTED, "HAVING over string values")
    # ... and inside a comparison in the filter it is no leaf
    refused(cuda, y.Plan(filter=c(0).isin([b"a"]) == c(1).isin([1]), **grp),
            INVALID, "type mismatch")
    # beside a join
    fk = np.arange(7, dtype=np.int64)
    foreign = y.Chunk([y.encode_int64(fk), y.encode_int64(fk * 10)], 7)
    plan = y.Plan(filter=c(0).isin([b"a"]), keys=[c(3)],
                  aggs=[y.agg_sum(c(sp.NCOLS))], join=y.Join(foreign, 3, 0, [1]))
    refused(cuda, plan, UNSUPPORTED, "not this round",
            join_foreign=foreign.c_device(cuda))
    # a fifth numeric list
    five = c(1).isin([1])
    for i in range(2, 6):
        five = five.or_(c(3).isin([i]))
    refused(cuda, y.Plan(filter=five, **grp), UNSUPPORTED,
            "more than 4 numeric IN lists")
    four = c(1).isin([1]).or_(c(3).isin([2])).or_(c(5).isin([3]))
    y.gpu_execute(y.Plan(filter=four, keys=[c(3).isin([1, 2])], aggs=aggs),
                  str_dev(cuda, "dict_dense"), max_groups_hint=4096)
    # over the length cap, numeric and string; duplicates do not count
    big = np.arange((1 << 20) + 1, dtype=np.int64)
    refused(cuda, y.Plan(filter=c(1).isin(big), **grp), UNSUPPORTED, "1048576")
    y.gpu_execute(y.Plan(filter=c(1).isin(np.concatenate([big[:-1], big[:9]])),
                         **grp),
                  str_dev(cuda, "dict_dense"), max_groups_hint=4096)
    # a malformed list
    e = c(1).isin([1, 2, 3])
    e.c.list_len = -1
    refused(cuda, y.Plan(filter=e, **grp), INVALID, "list")
    e = c(1).isin([1, 2, 3])
    e.c.list = None
    refused(cuda, y.Plan(filter=e, **grp), INVALID, "list")
    e = c(0).isin([b"a"])
    e.c.list = None
    refused(cuda, y.Plan(filter=e, **grp), INVALID, "list")
    # literals of another type than the operand
    refused(cuda, y.Plan(filter=c(1).isin([1, b"x"]), **grp), INVALID,
            "type mismatch")
    refused(cuda, y.Plan(filter=c(1).isin([1], unsigned=True), **grp), INVALID,
            "type mismatch")
    refused(cuda, y.Plan(filter=c(1).isin([True]), **grp), INVALID,
            "type mismatch")
    refused(cuda, y.Plan(filter=c(1).isin([1.5]), **grp), INVALID,
            "type mismatch")
    refused(cuda, y.Plan(filter=c(0).isin([b"a", 1]), **grp), INVALID,
            "type mismatch")
    refused(cuda, y.Plan(filter=(c(1) > 0).isin([1]), **grp), INVALID,
            "type mismatch")
    refused(cuda, y.Plan(keys=[c(3)], aggs=aggs, having=c(0).isin([True])),
            INVALID, "")
    # the bottom queries carry the same refusals
    states = cuda.zeros((64, 4), dtype=cuda.int64, device="cuda")
    with pytest.raises(RuntimeError, match="ytql error 7: .*DOUBLE"):
        y.gpu_partial(y.Plan(filter=c(2).isin([1]), **grp),
                      str_dev(cuda, "dict_dense"), 2, states.data_ptr(), 64)


def test_pool_balance(cuda):
    dev = str_dev(cuda, "dict_dense")
    ndev = num_dev(cuda, "dict_dense")
    aggs = [y.agg_sum1()]
    base = lib().yt_gpu_debug_pool_blocks_in_use()
    # a successful run of each form
    run(cuda, group_plan(c(0).isin([1, 2, None])), ndev)
    assert lib().yt_gpu_debug_pool_blocks_in_use() == base
    run(cuda, group_plan(c(0).isin([b"s-key-0010", b"x"]), key=3), dev)
    assert lib().yt_gpu_debug_pool_blocks_in_use() == base
    run(cuda, group_plan(c(0).isin([b"s-key-%04d" % i for i in range(600)]),
                         key=0), dev, max_groups_hint=sp.N,
        out_capacity=sp.N + 16)
    assert last_mode() == 2
    assert lib().yt_gpu_debug_pool_blocks_in_use() == base
    run(cuda, y.Plan(filter=c(0).isin([b"s-key-0010"]).and_(c(1).isin([5, 7])),
                     projects=[c(0), c(1)]), dev, out_capacity=sp.N + 16)
    assert lib().yt_gpu_debug_pool_blocks_in_use() == base
    # refusals after the tables were uploaded: a division by zero that the
    # scan meets, in each kernel family, and a HAVING list of another type
    bad = c(0).isin([b"s-key-0010", b""]).or_((c(1) % (c(3) - c(3))).isin([1]))
    for plan in (y.Plan(filter=bad, keys=[c(3)], aggs=aggs),
                 y.Plan(filter=bad, keys=[c(0)], aggs=aggs),
                 y.Plan(filter=bad, projects=[c(0), c(1)]),
                 y.Plan(filter=bad, projects=[c(1), c(3)],
                        order_by=[(0, False)], limit=5)):
        with pytest.raises(RuntimeError, match="ytql error 8"):
            y.gpu_execute(plan, dev, max_groups_hint=sp.N,
                          out_capacity=sp.N + 16)
        assert lib().yt_gpu_debug_pool_blocks_in_use() == base
    with pytest.raises(RuntimeError, match="ytql error 1"):
        y.gpu_execute(y.Plan(filter=c(1).isin([1, 2, 3]), keys=[c(3)], aggs=aggs,
                             having=c(0).isin([True])), dev, max_groups_hint=4096)
    assert lib().yt_gpu_debug_pool_blocks_in_use() == base
    # refusals at compile time hold nothing either
    refused(cuda, y.Plan(filter=c(1).isin([1]).and_(c(2).isin([1])),
                         keys=[c(3)], aggs=aggs), UNSUPPORTED, "DOUBLE")
    assert lib().yt_gpu_debug_pool_blocks_in_use() == base


def test_raw_c_abi(cuda):
    """yt_gpu_query_execute through ctypes alone: hand-built YtExpr nodes and
    YtValue lists, a string list and a numeric list under one AND"""
    d, v1, k3 = sdata("dict_dense")
    dev = str_dev(cuda, "dict_dense")
    texts = [b"s-key-0042", b"", b"zz"]
    bufs = [C.create_string_buffer(t, max(len(t), 1)) for t in texts]
    slist = (_abi.YtValue * 4)()
    for i, (t, b) in enumerate(zip(texts, bufs)):
        slist[i].type = VT_STRING
        slist[i].length = len(t)
        slist[i].data.u64 = C.addressof(b)
    slist[3].type = _abi.VT_NULL
    nlist = (_abi.YtValue * 3)()
    for i, v in enumerate((0, 2, 5)):
        nlist[i].type = VT_INT64
        nlist[i].data.i64 = v
    col0 = _abi.YtExpr(op=_abi.EX_COLUMN, col=0)
    col5 = _abi.YtExpr(op=_abi.EX_COLUMN, col=5)
    col3 = _abi.YtExpr(op=_abi.EX_COLUMN, col=3)
    in_s = _abi.YtExpr(op=_abi.EX_IN, a=C.pointer(col0), list=slist, list_len=4)
    in_n = _abi.YtExpr(op=_abi.EX_IN, a=C.pointer(col5), list=nlist, list_len=3)
    both = _abi.YtExpr(op=_abi.EX_AND, a=C.pointer(in_s), b=C.pointer(in_n))
    keys = (C.POINTER(_abi.YtExpr) * 1)(C.pointer(col3))
    agg = _abi.YtAgg(func=_abi.AGG_SUM1)
    aggs = (C.POINTER(_abi.YtAgg) * 1)(C.pointer(agg))
    plan = _abi.YtPlan(filter=C.pointer(both), key_count=1, keys=keys,
                       agg_count=1, aggs=aggs, totals_mode=1)
    vals = (_abi.YtValue * (64 * 2))()
    rs = _abi.YtRowset(values=vals, capacity_rows=64)
    opts = _abi.YtExecOptions(max_groups_hint=4096)
    st = _abi.YtStatistics()
    err = C.create_string_buffer(512)
    rc = lib().yt_gpu_query_execute(C.byref(plan), C.byref(dev), C.byref(opts),
                                    C.byref(rs), C.byref(st), err, 512)
    assert rc == _abi.YT_OK, err.value
    assert rs.column_count == 2
    got = sorted((vals[r * 2].data.i64, vals[r * 2 + 1].data.i64)
                 for r in range(rs.row_count))
    k5 = [int(a) for a in d.raw["k5"]]
    mask = [a and b for a, b in zip(ref_in(d.cols[0], texts + [None]),
                                    ref_in(k5, [0, 2, 5]))]
    want = sorted((k, n) for k, _, n in ref_group(k3, v1, mask))
    assert got == want and len(want) == 7
