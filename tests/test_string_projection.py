"""Plain scans that return STRING columns: SELECT name, v WHERE ... with and
without ORDER BY ... LIMIT (device compaction and byte gather).

Reference: every chunk is built from Python lists, and the expected result is
literally [(cols...) for each row i that satisfies the filter], computed in
Python in input row order (the 2^20-row case does the same with numpy).
Comparison is exact: values, nulls, lengths and order. Filters are the
string-predicate leaves of test_string_predicates.py (its ref_leaf answers
them) and integer comparisons by the engine's relational rule (its ref_rel);
the chunk builders that force each string layout come from that file too.

SCAN_PATH_PROJ_COMPACT is imported at the top: without the feature this file
fails at collection."""
import ctypes as C

import numpy as np
import pytest

import ytsaurus_amd as y
from ytsaurus_amd import _abi
from ytsaurus_amd._abi import SCAN_PATH_PROJ_COMPACT, VT_NULL, VT_STRING

import test_string_predicates as sp
from test_string_predicates import c, gpu_expr, ref_leaf, ref_rel, seg_types

CAPACITY, UNSUPPORTED = _abi.YT_ERR_CAPACITY, _abi.YT_ERR_UNSUPPORTED
LONG = bytes((i * 7 + 3) % 251 for i in range(5000))     # holds 0x00 and >= 0x80
SPECIAL = [b"", b"\x00", b"a\x00b\x00", b"\x80\xff\xfe", b"\xc3\xa9t\xc3\xa9"]


# ---------------------------------------------------------------------
# filters: one description, a GPU expression and a Python answer per row
#   ("leaf", spec)            a string-predicate leaf of test_string_predicates
#   ("int", col, op, k)       integer column against a literal
#   ("and" | "or", a, b)
# Kleene logic; a row passes when the answer is True.

def flt_expr(f):
    if f is None:
        return None
    if f[0] == "leaf":
        return gpu_expr(f[1])
    if f[0] == "int":
        a = c(f[1])
        return {"==": a.__eq__, "!=": a.__ne__, "<": a.__lt__, "<=": a.__le__,
                ">": a.__gt__, ">=": a.__ge__}[f[2]](f[3])
    a, b = flt_expr(f[1]), flt_expr(f[2])
    return a.and_(b) if f[0] == "and" else a.or_(b)


def flt_rows(f, cols, n):
    """per-row True / False / None"""
    if f is None:
        return [True] * n
    if f[0] == "leaf":
        return ref_leaf(f[1], cols)
    if f[0] == "int":
        return [ref_rel(f[2], v, f[3]) for v in cols[f[1]]]
    a, b = flt_rows(f[1], cols, n), flt_rows(f[2], cols, n)
    if f[0] == "and":
        return [False if (p is False or q is False) else
                (None if (p is None or q is None) else True)
                for p, q in zip(a, b)]
    return [True if (p is True or q is True) else
            (None if (p is None or q is None) else False)
            for p, q in zip(a, b)]


def expected(cols, n, f, proj, limit_rows=None):
    n = n if limit_rows is None else min(n, limit_rows)
    sel = flt_rows(f, {k: v[:n] for k, v in cols.items()}, n)
    return [tuple(cols[p][i] for p in proj) for i in range(n) if sel[i] is True]


# ---------------------------------------------------------------------
# chunks: cols = {index: list of Python values (None = null)}

class Table:
    def __init__(self, cols, enc, n):
        """enc: the encoded columns, or a chunk that holds them already"""
        self.cols, self.n = cols, n
        self.chunk = enc if isinstance(enc, y.Chunk) else y.Chunk(enc, n)
        self._dev = None

    def dev(self, cuda):
        if self._dev is None:
            self._dev = self.chunk.c_device(cuda)
        return self._dev


def int_col(vals, seg=0):
    arr = np.array([0 if v is None else v for v in vals], dtype=np.int64)
    nulls = np.array([v is None for v in vals], dtype=np.uint8)
    return y.encode_int64(arr, nulls, max_segment_values=seg)


def scan_path():
    return _abi.gpu_lib().yt_gpu_debug_last_scan_path()


def run(cuda, t, proj, f=None, compact=True, **kw):
    """the plan on the GPU: (rows, stats, string_pool_used)"""
    plan = y.Plan(filter=flt_expr(f), projects=[c(p) for p in proj])
    kw.setdefault("out_capacity", t.n + 16)
    rs, st = y.gpu_execute(plan, t.dev(cuda), raw_rowset=True, **kw)
    assert scan_path() == (SCAN_PATH_PROJ_COMPACT if compact else 0)
    return y.rows_from_rowset(rs), st, rs.string_pool_used


def pool_bytes_of(rows):
    return sum(len(v) for r in rows for v in r if isinstance(v, bytes))


def check(cuda, t, proj, f=None, **kw):
    want = expected(t.cols, t.n, f, proj, kw.get("input_row_limit") or None)
    got, st, used = run(cuda, t, proj, f, **kw)
    assert len(got) == len(want)
    assert got == want
    assert used == pool_bytes_of(want)
    assert st.rows_written == len(want)
    return want


# ---------------------------------------------------------------------
# the four layouts, with the awkward values written over whole runs so that
# the writer's layout choice stays what test_string_predicates established

def with_special(strings):
    """SPECIAL values over the first runs of segment 1 (rows 2048..), the
    5000-byte string over one run of segment 2"""
    out = list(strings)

    def overwrite_run(at, value):
        end = at
        while end < len(out) and out[end] == out[at]:
            end += 1
        out[at:end] = [value] * (end - at)
        return end

    at = sp.SEG + 64
    for v in SPECIAL:
        while out[at] is None:
            at += 1
        at = overwrite_run(at, v)
    at = 2 * sp.SEG + 64
    while out[at] is None:
        at += 1
    overwrite_run(at, LONG)
    return out


_LAYOUT = {}


def layout_table(name):
    if name not in _LAYOUT:
        gen, _ = sp.LAYOUTS[name]
        strings = with_special(sp._bytes_list(gen(np.random.default_rng(99))))
        rng = np.random.default_rng(5)
        v = [None if rng.random() < 0.1 else int(x)
             for x in rng.integers(-1000, 1000, sp.N)]
        cols = {0: strings, 1: v}
        _LAYOUT[name] = Table(cols, [y.encode_string(strings, max_segment_values=sp.SEG),
                                     int_col(v, 5000)], sp.N)
    return _LAYOUT[name]


@pytest.mark.parametrize("layout", list(sp.LAYOUTS))
def test_layouts_are_what_the_cases_assume(layout):
    t = layout_table(layout)
    assert seg_types(t.chunk.columns[0]) == sp.LAYOUTS[layout][1]
    s = t.cols[0]
    assert all(v in s for v in SPECIAL) and LONG in s
    assert any(v is None for v in s)
    assert t.chunk.columns[1].segments[0].row_count == 5000


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(sp.LAYOUTS))
def test_layouts(cuda, layout):
    """DictionaryDense, DictionaryRle, DirectDense, DirectRle and all four in
    one column: nulls, a segment of nulls only, empty strings, bytes 0x00 and
    >= 0x80, a 5000-byte value; 2048-row string segments against 5000-row
    integer segments"""
    t = layout_table(layout)
    assert seg_types(t.chunk.columns[0]) == sp.LAYOUTS[layout][1]
    want = check(cuda, t, [0, 1])
    assert len(want) == sp.N
    want = check(cuda, t, [1, 0], ("int", 1, ">", 0))
    assert 0 < len(want) < sp.N
    check(cuda, t, [0], ("leaf", ("isnull", 0, "==")))        # nulls only
    want = check(cuda, t, [0], ("leaf", ("cmp", 0, "<=", b"\x00", False)))
    assert {r[0] for r in want} == {None, b"", b"\x00"}


@pytest.mark.gpu
def test_long_string_among_short_ones(cuda):
    """one 5000-byte string among 1-byte ones: the wave that holds it copies
    lane-strided, its neighbours one lane per string"""
    s = [bytes([97 + (i * 5) % 26]) for i in range(300)]
    s[131] = LONG
    s[7] = None
    t = Table({0: s, 1: list(range(300))}, [y.encode_string(s), int_col(range(300))],
              300)
    check(cuda, t, [0, 1])
    check(cuda, t, [1, 0], ("int", 1, ">=", 131))
    want = check(cuda, t, [0], ("int", 1, "==", 131))
    assert want == [(LONG,)]


# ---------------------------------------------------------------------
# sizes around every scan boundary (tile = 2048 rows, 256 threads x 8 rows,
# waves of 64), each with nothing / everything / every other row / only the
# last row passing

SIZES = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 8191, 8192, 8193]


def sized_table(n):
    rng = np.random.default_rng(n)
    pop = [b"", b"x", b"\x00\x80", b"key-%d" % n] + \
          [b"v%03d" % i + b"." * (i % 37) for i in range(60)]
    s = [None if rng.random() < 0.05 else pop[int(rng.integers(0, len(pop)))]
         for _ in range(n)]
    s[n - 1] = b"last-%d" % n
    idx = list(range(n))
    return Table({0: s, 1: idx, 2: [i % 2 for i in idx]},
                 [y.encode_string(s, max_segment_values=1000), int_col(idx),
                  int_col([i % 2 for i in idx])], n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_selectivities(cuda, n):
    t = sized_table(n)
    got, _, used = run(cuda, t, [0, 1], ("int", 1, "<", 0))
    assert got == [] and used == 0
    assert len(check(cuda, t, [0, 1], ("int", 1, ">=", 0))) == n
    assert len(check(cuda, t, [1, 0], ("int", 2, "==", 0))) == (n + 1) // 2
    assert check(cuda, t, [0, 1], ("int", 1, "==", n - 1)) == \
        [(b"last-%d" % n, n - 1)]


# ---------------------------------------------------------------------
# 2^20 rows: 512 tiles, more than the one scanning workgroup has threads

def values_view(rs):
    dt = np.dtype([("id", "<u2"), ("type", "u1"), ("flags", "u1"),
                   ("length", "<u4"), ("data", "<u8")])
    n = rs.row_count * rs.column_count
    return np.frombuffer(rs._buf, dtype=dt, count=n).reshape(rs.row_count,
                                                             rs.column_count)


@pytest.mark.gpu
def test_second_level_scan_loops(cuda):
    n, k = 1 << 20, 1000
    rng = np.random.default_rng(20)
    kid = rng.integers(0, k, n)
    lens_k = (4 + np.arange(k) % 9).astype(np.uint32)       # 4..12 bytes
    begins_k = np.concatenate([[0], np.cumsum(lens_k)[:-1]]).astype(np.uint64)
    blob = b"".join((b"%04d" % i + b"abcdefgh")[:int(lens_k[i])] for i in range(k))
    null = rng.random(n) < 0.03
    v = rng.integers(0, 3000, n)
    chunk = y.Chunk([y.encode_string_raw(blob, begins_k[kid],
                                         np.where(null, 0, lens_k[kid]),
                                         null.astype(np.uint8)),
                     y.encode_int64(v)], n)
    plan = y.Plan(filter=c(1) < 1000, projects=[c(0), c(1)])
    rs, st = y.gpu_execute(plan, chunk.c_device(cuda), raw_rowset=True,
                           out_capacity=n // 2)
    assert scan_path() == SCAN_PATH_PROJ_COMPACT
    keep = np.flatnonzero(v < 1000)
    assert 0.30 * n < len(keep) < 0.37 * n
    assert rs.row_count == len(keep) and rs.column_count == 2
    vals = values_view(rs)
    knull = null[keep]
    want_len = np.where(knull, 0, lens_k[kid[keep]]).astype(np.int64)
    assert np.array_equal(vals["type"][:, 0],
                          np.where(knull, VT_NULL, VT_STRING))
    assert np.array_equal(vals["length"][:, 0], want_len)
    assert np.array_equal(vals["data"][:, 1].astype(np.int64), v[keep])
    assert rs.string_pool_used == int(want_len.sum())
    base = C.addressof(rs._pool)
    offs = np.concatenate([[0], np.cumsum(want_len)[:-1]])
    nn = ~knull
    assert np.array_equal(vals["data"][nn, 0].astype(np.int64) - base, offs[nn])
    blob_np = np.frombuffer(blob, dtype=np.uint8)
    src = begins_k[kid[keep][nn]].astype(np.int64)
    ln = want_len[nn]
    pos = np.repeat(src - offs[nn], ln) + np.arange(int(ln.sum()))
    got_pool = np.frombuffer(rs._pool, dtype=np.uint8,
                             count=rs.string_pool_used)
    assert np.array_equal(got_pool, blob_np[pos])


# ---------------------------------------------------------------------
# plan shapes over the mixed-layout data of test_string_predicates:
# 0 string (2048-row segments), 1 int64 with nulls (5000-row segments),
# 2 double with nulls, 3 int64, 4 second string (4096-row segments), 5 int64

_SHAPES = {}


def shapes_table():
    if "t" not in _SHAPES:
        d = sp.data("mixed")
        raw = d.raw
        cols = {0: d.cols[0], 4: d.cols[4],
                1: [None if m else int(v) for v, m in zip(raw["v1"], raw["v1n"])],
                2: [None if m else float(v) for v, m in zip(raw["v2"], raw["v2n"])],
                3: [int(v) for v in raw["k3"]], 5: [int(v) for v in raw["k5"]]}
        _SHAPES["t"] = Table(cols, d.chunk, sp.N)
    return _SHAPES["t"]


@pytest.mark.gpu
def test_shapes(cuda):
    t = shapes_table()
    pre = ("leaf", ("prefix", 0, b"s-key-00"))
    # two different string columns with numeric columns between
    want = check(cuda, t, [0, 1, 2, 4, 3], ("int", 3, "<", 4))
    assert 0 < len(want) < sp.N
    # the same string column twice
    check(cuda, t, [0, 5, 0], ("int", 5, "==", 2))
    # the projected column is the predicate's column
    want = check(cuda, t, [0, 1], pre)
    assert want and all(r[0].startswith(b"s-key-00") for r in want)
    check(cuda, t, [4, 0], ("and", pre, ("leaf", ("like", 4, b"h_5", None))))
    # no filter
    assert len(check(cuda, t, [4])) == sp.N
    # numeric-only projections stay on the uncompacted path
    want = expected(t.cols, t.n, pre, [1, 3])
    got, _, used = run(cuda, t, [1, 3], pre, compact=False)
    assert got == want and used == 0


@pytest.mark.gpu
def test_ragged_segmentation(cuda):
    """string column in 1000-row segments, integer column in 4096-row ones"""
    n = 9500
    rng = np.random.default_rng(8)
    s = [None if rng.random() < 0.04 else b"r%05d" % int(rng.integers(0, 400))
         for _ in range(n)]
    v = [int(x) for x in rng.integers(-50, 50, n)]
    t = Table({0: s, 1: v}, [y.encode_string(s, max_segment_values=1000),
                             int_col(v, 4096)], n)
    assert [g.row_count for g in t.chunk.columns[0].segments][:2] == [1000, 1000]
    assert t.chunk.columns[1].segments[0].row_count == 4096
    check(cuda, t, [0, 1], ("int", 1, ">", 10))
    check(cuda, t, [1, 0], ("leaf", ("cmp", 0, ">=", b"r00200", False)))


@pytest.mark.gpu
def test_window_boundary(cuda, monkeypatch):
    """10 000 rows through 4096-row windows: identical to the one-window run"""
    t = layout_table("mixed")
    plan = y.Plan(filter=c(1) > -500, projects=[c(0), c(1)])

    def go():
        rs, _ = y.gpu_execute(plan, t.dev(cuda), raw_rowset=True,
                              out_capacity=sp.N, input_row_limit=10_000)
        assert scan_path() == SCAN_PATH_PROJ_COMPACT
        return y.rows_from_rowset(rs), rs.string_pool_used

    monkeypatch.delenv("YTQL_PROJ_WINDOW", raising=False)
    one = go()
    monkeypatch.setenv("YTQL_PROJ_WINDOW", "4096")
    three = go()
    monkeypatch.undo()
    assert three == one
    assert one[0] == expected(t.cols, t.n, ("int", 1, ">", -500), [0, 1], 10_000)


# ---------------------------------------------------------------------
# limits

@pytest.mark.gpu
def test_input_row_limit_cuts_inside_a_segment(cuda):
    t = layout_table("mixed")
    for lim in (1, 2048 + 700, 3 * 2048 + 1):      # inside segments 0, 1 and 3
        want = check(cuda, t, [0, 1], ("int", 1, "<", 300), input_row_limit=lim)
        assert len(want) <= lim


@pytest.mark.gpu
def test_output_row_limit(cuda):
    t = layout_table("dict_dense")
    f = ("int", 1, ">", 0)
    full = expected(t.cols, t.n, f, [1, 0])
    for lim in (1, 777, len(full) - 1):
        got, st, used = run(cuda, t, [1, 0], f, output_row_limit=lim)
        assert got == full[:lim]
        assert st.incomplete_output == 1
        assert used == pool_bytes_of(full[:lim])
    got, st, used = run(cuda, t, [1, 0], f, output_row_limit=len(full) + 5)
    assert got == full and st.incomplete_output == 0


@pytest.mark.gpu
def test_capacity_limits(cuda):
    t = layout_table("direct_dense")
    f = ("int", 1, ">", 500)
    want = expected(t.cols, t.n, f, [0, 1])
    need = pool_bytes_of(want)
    assert need > 0
    got, _, used = run(cuda, t, [0, 1], f, pool_bytes=need)
    assert got == want and used == need
    with pytest.raises(RuntimeError, match="ytql error %d" % CAPACITY):
        run(cuda, t, [0, 1], f, pool_bytes=need - 1)
    with pytest.raises(RuntimeError, match="ytql error %d" % CAPACITY):
        run(cuda, t, [0, 1], f, out_capacity=len(want) - 1)
    got, _, _ = run(cuda, t, [0, 1], f, out_capacity=len(want))
    assert got == want


@pytest.mark.gpu
def test_zero_capacity_pool_with_nothing_to_store(cuda):
    s = [None, b"", None, b"", b""] * 600
    t = Table({0: s, 1: list(range(3000))}, [y.encode_string(s),
                                             int_col(range(3000))], 3000)
    want = expected(t.cols, t.n, None, [0, 1])
    got, _, used = run(cuda, t, [0, 1], pool_bytes=0)
    assert got == want and used == 0
    assert {r[0] for r in got} == {None, b""}


# ---------------------------------------------------------------------
# ORDER BY int column LIMIT / OFFSET carrying a string column. Column 1 is
# the order key (unique, three nulls), column 2 a unique tie-breaker so that
# the null keys have an order too.

def order_table():
    if "o" not in _SHAPES:
        n = 6000
        rng = np.random.default_rng(77)
        key = [int(x) for x in rng.permutation(n) - 2500]
        for i in (17, 2900, 5999):
            key[i] = None
        tie = [int(x) for x in rng.permutation(n)]
        s = [None if rng.random() < 0.05 else
             (LONG[:int(rng.integers(0, 90))] if i % 50 == 0 else b"o%04d" % (i % 700))
             for i in range(n)]
        _SHAPES["o"] = Table({0: s, 1: key, 2: tie},
                             [y.encode_string(s, max_segment_values=1024),
                              int_col(key), int_col(tie)], n)
    return _SHAPES["o"]


def ordered(rows, desc):
    """the engine's order: null < any value; descending inverts it"""
    rows = sorted(rows, key=lambda r: r[2])
    return sorted(rows, key=lambda r: (r[1] is not None, r[1] or 0),
                  reverse=desc)


@pytest.mark.gpu
@pytest.mark.parametrize("desc", [False, True])
def test_order_by_carries_strings(cuda, desc):
    t = order_table()
    for f, limit, offset in ((None, 40, 0), (None, 25, 2),
                             (("int", 2, ">=", 3000), 30, 7),
                             (("leaf", ("prefix", 0, b"o00")), 50, 5),
                             (None, t.n, t.n - 20)):
        plan = y.Plan(filter=flt_expr(f), projects=[c(0), c(1), c(2)],
                      order_by=[(1, desc), (2, False)], limit=limit,
                      offset=offset)
        rs, _ = y.gpu_execute(plan, t.dev(cuda), raw_rowset=True,
                              out_capacity=t.n)
        assert scan_path() == 0
        got = y.rows_from_rowset(rs)
        want = ordered(expected(t.cols, t.n, f, [0, 1, 2]), desc)
        want = want[offset:offset + limit]
        assert want and got == want
        assert rs.string_pool_used == pool_bytes_of(want)
    # the three null keys are in the first slice ascending, the last descending
    assert sum(k is None for k in t.cols[1]) == 3


@pytest.mark.gpu
def test_order_by_limits(cuda):
    t = order_table()
    plan = y.Plan(projects=[c(0), c(1), c(2)], order_by=[(1, False), (2, False)],
                  limit=100)
    want = ordered(expected(t.cols, t.n, None, [0, 1, 2]), False)[:100]
    need = pool_bytes_of(want)
    rs, _ = y.gpu_execute(plan, t.dev(cuda), raw_rowset=True, pool_bytes=need)
    assert y.rows_from_rowset(rs) == want and rs.string_pool_used == need
    with pytest.raises(RuntimeError, match="ytql error %d" % CAPACITY):
        y.gpu_execute(plan, t.dev(cuda), pool_bytes=need - 1)
    rs, st = y.gpu_execute(plan, t.dev(cuda), raw_rowset=True,
                           output_row_limit=9)
    assert y.rows_from_rowset(rs) == want[:9] and st.incomplete_output == 1
    assert rs.string_pool_used == pool_bytes_of(want[:9])


# ---------------------------------------------------------------------
# refusals

def refused(cuda, plan, message, **kw):
    with pytest.raises(RuntimeError,
                       match=r"ytql error %d: .*%s" % (UNSUPPORTED, message)):
        y.gpu_execute(plan, sp.dev_chunk(cuda, "dict_dense"), **kw)


@pytest.mark.gpu
def test_refusals(cuda):
    # a string column inside a projection expression
    refused(cuda, y.Plan(projects=[c(1), c(0) + 1]),
            "string column inside a projection expression")
    refused(cuda, y.Plan(projects=[c(0) == c(4)]),
            "string column inside a projection expression")
    # string literals and predicates keep the message of before
    refused(cuda, y.Plan(projects=[c(1), c(0) == b"x"]), "inside a projection")
    # a string ORDER BY column in a plain scan, first key or later
    refused(cuda, y.Plan(projects=[c(0), c(1)], order_by=[(0, False)], limit=5),
            "ORDER BY on a string column")
    refused(cuda, y.Plan(projects=[c(1), c(4)],
                         order_by=[(0, False), (1, True)], limit=5),
            "ORDER BY on a string column")
    # beside a join, and a foreign string column
    fk = np.arange(7, dtype=np.int64)
    foreign = y.Chunk([y.encode_int64(fk),
                       y.encode_string([b"f%d" % i for i in range(7)])], 7)
    fdev = foreign.c_device(cuda)
    refused(cuda, y.Plan(projects=[c(0), c(3)], join=y.Join(foreign, 3, 0, [0])),
            "string projection beside a join", join_foreign=fdev)
    refused(cuda, y.Plan(projects=[c(1), c(sp.NCOLS)],
                         join=y.Join(foreign, 3, 0, [1])),
            "foreign string column", join_foreign=fdev)
    refused(cuda, y.Plan(projects=[c(sp.NCOLS) + 1],
                         join=y.Join(foreign, 3, 0, [1])),
            "string column inside a projection expression", join_foreign=fdev)


# ---------------------------------------------------------------------
# fuzz: 20 seeded cases

PREDS = [None,
         ("int", 1, ">", 0),
         ("int", 3, "<=", 2),
         ("leaf", ("prefix", 0, b"s-key")),
         ("leaf", ("substr", 2, b"1")),
         ("leaf", ("isnull", 0, "!=")),
         ("and", ("leaf", ("cmp", 0, ">=", b"s-key-0030", False)),
          ("int", 1, "<", 400)),
         ("or", ("leaf", ("like", 2, b"%7", None)), ("int", 3, "==", 0))]


def fuzz_table(seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 20_001))
    seg = int(rng.choice([256, 1000, 2048, 4096]))
    s0 = []
    while len(s0) < n:
        rows = min(seg, n - len(s0))
        kind = int(rng.integers(0, 5))
        if rows < 8 or kind == 4:
            s0 += [None if rng.random() < 0.3 else SPECIAL[int(rng.integers(0, 5))]
                   for _ in range(rows)]
        elif kind == 0:
            s0 += sp.seg_dict_dense(rng, min(65, rows), rows)
        elif kind == 1:
            s0 += sp.seg_dict_rle(rng, 30, rows)
        elif kind == 2:
            s0 += sp.seg_direct_dense(rng, b"s-key", rows)
        else:
            s0 += sp.seg_direct_rle(rng, b"s-key", rows)
    s2 = [None if rng.random() < 0.1 else b"t%d" % int(rng.integers(0, 5000))
          for _ in range(n)]
    v1 = [None if rng.random() < 0.1 else int(x)
          for x in rng.integers(-1000, 1000, n)]
    v3 = [int(x) for x in rng.integers(0, 6, n)]
    t = Table({0: s0, 1: v1, 2: s2, 3: v3},
              [y.encode_string(s0, max_segment_values=seg), int_col(v1, 3000),
               y.encode_string(s2), int_col(v3)], n)
    f = PREDS[int(rng.integers(0, len(PREDS)))]
    proj = [int(p) for p in rng.choice(4, size=int(rng.integers(1, 6)))]
    if not ({0, 2} & set(proj)):
        proj[int(rng.integers(0, len(proj)))] = int(rng.choice([0, 2]))
    return t, f, proj


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(20))
def test_fuzz(cuda, seed):
    t, f, proj = fuzz_table(seed)
    check(cuda, t, proj, f)
