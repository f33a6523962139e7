"""Multi-key GROUP BY with STRING keys: the data sets, the plans and the
reference model that tests/test_multikey_strings.py runs on the GPU, checked
here against the CPU oracle (no GPU needed).

The reference is a small Python model: a dict keyed by the tuple of key
values, with the aggregate semantics the README states — sum / min / max /
avg skip nulls and are null over no value, sum(1) counts rows, avg is
double(sum) / count, first is the one distinct non-null value of its group
(the data keeps it unique per group wherever first is asked for). HAVING,
WITH TOTALS (both modes) and ORDER BY ... LIMIT/OFFSET follow the reference's
order of operations; a group whose keys are all null is an error under WITH
TOTALS and ORDER BY ("Null values are forbidden in group key").

The oracle has no string predicates and no IN lists, so plans with those are
checked on the GPU against the model alone."""
import numpy as np
import pytest

import ytsaurus_amd as y
from ytsaurus_amd._abi import (SEG_DICTIONARY_DENSE, SEG_DICTIONARY_RLE,
                               SEG_DIRECT_DENSE, SEG_DIRECT_RLE)

NULL_KEY_ERROR = "Null values are forbidden in group key"

# ---------------------------------------------------------------------
# the model

class Spec:
    """One plan, for y.Plan and for the model. keys: column indices. aggs:
    (name, column or None). where / having: (expression, Python predicate
    over the input row / the output row) or None. totals: None, "before" or
    "after" (HAVING). order: [(output column, desc)], with limit / offset."""

    def __init__(self, keys, aggs=(), where=None, having=None, totals=None,
                 order=(), limit=0, offset=0):
        self.keys = list(keys)
        self.aggs = list(aggs)
        self.where = where
        self.having = having
        self.totals = totals
        self.order = list(order)
        self.limit = limit
        self.offset = offset

    def plan(self):
        mk = {"sum": y.agg_sum, "min": y.agg_min, "max": y.agg_max,
              "avg": y.agg_avg, "first": y.agg_first}
        aggs = [y.agg_sum1() if f == "sum1" else mk[f](y.col(c))
                for f, c in self.aggs]
        return y.Plan(filter=self.where[0] if self.where else None,
                      keys=[y.col(k) for k in self.keys], aggs=aggs,
                      having=self.having[0] if self.having else None,
                      with_totals=self.totals is not None,
                      totals_after_having=self.totals == "after",
                      order_by=self.order, limit=self.limit, offset=self.offset)


def _agg(name, vals):
    nn = [v for v in vals if v is not None]
    if name == "sum1":
        return len(vals)
    if not nn:
        return None
    if name == "sum":
        return sum(nn)
    if name == "min":
        return min(nn)
    if name == "max":
        return max(nn)
    if name == "avg":
        return float(sum(nn)) / len(nn)
    if name == "first":
        assert len(set(nn)) == 1, "first() needs one distinct value per group"
        return nn[0]
    raise KeyError(name)


def _fold_totals(spec, rows):
    nk = len(spec.keys)
    out = [None] * nk
    for a, (name, _) in enumerate(spec.aggs):
        vals = [r[nk + a] for r in rows]
        fold = {"sum1": "sum", "sum": "sum", "min": "min", "max": "max"}[name]
        t = _agg(fold, vals)
        out.append(0 if (name == "sum1" and t is None) else t)
    return tuple(out)


def _order(rows, order):
    for c, desc in reversed(order):
        # null < any value; a descending key inverts the whole comparison
        rows = sorted(rows, key=lambda r: (r[c] is not None,
                                           r[c] if r[c] is not None else 0),
                      reverse=bool(desc))
    return rows


def model(spec, rows):
    """rows: list of input tuples -> list of output tuples [keys..., aggs...];
    the totals row, when there is one, comes last"""
    groups = {}
    for r in rows:
        if spec.where and not spec.where[1](r):
            continue
        groups.setdefault(tuple(r[k] for k in spec.keys), []).append(r)
    out = []
    for k, rs in groups.items():
        out.append(k + tuple(_agg(f, [r[c] if c is not None else 1 for r in rs])
                             for f, c in spec.aggs))
    if (spec.totals or spec.order) and any(
            all(v is None for v in r[:len(spec.keys)]) for r in out):
        raise RuntimeError(NULL_KEY_ERROR)
    had = len(out) > 0
    tot = None
    if spec.totals == "before":
        tot = _fold_totals(spec, out)
    if spec.having:
        out = [r for r in out if spec.having[1](r)]
    if spec.totals == "after":
        tot = _fold_totals(spec, out)
    if spec.order:
        out = _order(out, spec.order)[spec.offset:spec.offset + spec.limit]
    if spec.totals and had:
        out.append(tot)
    return out


def same_rows(got, want, ordered=False, totals=False):
    """bit-exact but for doubles, which compare within 1e-6 relative; an
    unordered result is compared after y.sort_rows (the totals row, the last
    one, stays where it is)"""
    got, want = list(got), list(want)
    assert len(got) == len(want), (len(got), len(want))
    if not ordered:
        tg, tw = ([got.pop()], [want.pop()]) if totals and want else ([], [])
        got, want = y.sort_rows(got) + tg, y.sort_rows(want) + tw
    for g, w in zip(got, want):
        assert len(g) == len(w), (g, w)
        for a, b in zip(g, w):
            if isinstance(b, float):
                assert isinstance(a, float), (g, w)
                assert a == pytest.approx(b, rel=1e-6, abs=0), (g, w)
            else:
                assert type(a) is type(b) and a == b, (g, w)


# ---------------------------------------------------------------------
# data sets (built once, never modified)

class Data:
    """cols: (kind, values, max_segment_values); kind 's' string, 'i' int64,
    'u' uint64, 'b' boolean, 'd' double; None is null"""

    def __init__(self, cols):
        self.cols = cols
        self.n = len(cols[0][1])
        self.rows = list(zip(*[c[1] for c in cols]))
        enc = []
        for kind, vals, seg in cols:
            nulls = np.array([v is None for v in vals], dtype=np.uint8)
            if kind == "s":
                enc.append(y.encode_string(vals, max_segment_values=seg))
            elif kind == "d":
                enc.append(y.encode_double(
                    np.array([0.0 if v is None else v for v in vals]), nulls,
                    max_segment_values=seg))
            elif kind == "b":
                enc.append(y.encode_bool(
                    np.array([bool(v) for v in vals], dtype=np.uint8), nulls,
                    max_segment_values=seg))
            else:
                enc.append(y.encode_int64(
                    np.array([0 if v is None else v for v in vals],
                             dtype=np.uint64 if kind == "u" else np.int64)
                    .astype(np.int64), nulls, max_segment_values=seg,
                    unsigned=kind == "u"))
        self.chunk = y.Chunk(enc, self.n)

    def seg_types(self, c):
        col = self.chunk.columns[c]
        return [col._cenc.segments[j].type
                for j in range(col._cenc.segment_count)]


_CACHE = {}


def cached(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def strings37():
    """37 distinct strings of length 0..40: the empty string, pairs that
    share their first 16 bytes (decided by the slot's prefix when the length
    is <= 16, by the owner's bytes above), pairs that differ in byte 15"""
    def make():
        rng = np.random.default_rng(5)
        s = [b"", b"x", b"\x00", b"0123456789abcdef", b"0123456789abcdeF",
             b"0123456789abcdefg", b"0123456789abcdefh",
             b"0123456789abcdef" + b"z" * 24, b"0123456789abcdef" + b"y" * 24]
        while len(s) < 37:
            n = int(rng.integers(1, 41))
            v = bytes(rng.integers(97, 123, n).astype(np.uint8))
            if v not in s:
                s.append(v)
        assert len(set(s)) == 37 and max(map(len, s)) == 40
        assert any(len(v) <= 16 for v in s) and any(len(v) > 16 for v in s)
        return s
    return cached("s37", make)


N_LAYOUT = 4000
LAYOUT_TYPE = {"dict_dense": SEG_DICTIONARY_DENSE, "dict_rle": SEG_DICTIONARY_RLE,
               "direct_dense": SEG_DIRECT_DENSE, "direct_rle": SEG_DIRECT_RLE}
# the key segment sizes at which the writer stores the recipe below purely in
# the named layout (asserted); 64 and 4096 give the uniform-shift segment
# lookup, 100 the binary search. With 37 distinct strings no segment of 100
# or 4096 rows is cheaper in DirectDense than in a dictionary, and no segment
# of 64 rows in runs is cheaper in DictionaryRle than in DirectRle.
LAYOUT_SEGS = {"dict_dense": (64, 100, 4096), "dict_rle": (100, 4096),
               "direct_dense": (64,), "direct_rle": (64, 100),
               "mixed": (64, 100)}
LAYOUT_CASES = [(l, s) for l in LAYOUT_SEGS for s in LAYOUT_SEGS[l]]


def layout_keys(layout, n=N_LAYOUT):
    s = strings37()
    rng = np.random.default_rng(17)
    if layout == "dict_dense":
        return [None if rng.random() < 0.03 else s[j]
                for j in rng.integers(0, 37, n)]
    if layout == "dict_rle":       # runs of 8, three strings per 320 rows
        return [None if (i // 8) % 29 == 0 else
                s[((i // 8) % 3 + 3 * (i // 320)) % 37] for i in range(n)]
    if layout == "direct_rle":     # runs of 4, every run another string
        return [None if (i // 4) % 41 == 0 else s[(i // 4) % 37]
                for i in range(n)]
    if layout == "direct_dense":   # per 64 rows: 37 distinct strings, 27 nulls
        return [s[(i % 64 + i // 64) % 37] if i % 64 < 37 else None
                for i in range(n)]
    if layout == "mixed":
        keys = []
        for part in ("dict_dense", "direct_dense", "direct_rle", "dict_rle"):
            keys += layout_keys(part, 3200)[:1024]
        return keys[:n]
    raise KeyError(layout)


def layout_data(layout, seg):
    """cols: 0 key string (segments of `seg` rows), 1 small int key 0..4 with
    3 % nulls (segments of 1000), 2 int64 with 10 % nulls (one segment),
    3 double in [0, 1) with 5 % nulls, 4 second string of 3 values + null
    (segments of 512), 5 boolean key, 6 = 7 * index of the key string (the
    same for every row of a group keyed by col 0; null beside a null key)"""
    def make():
        keys = layout_keys(layout)
        n = len(keys)
        rng = np.random.default_rng(23)
        idx = {v: i for i, v in enumerate(strings37())}
        k = [None if rng.random() < 0.03 else int(v) for v in rng.integers(0, 5, n)]
        v = [None if rng.random() < 0.10 else int(x)
             for x in rng.integers(-1000, 1000, n)]
        d = [None if rng.random() < 0.05 else float(x) for x in rng.random(n)]
        s2 = [(b"red", b"green-and-a-long-tail-past-16", b"", None)[int(j)]
              for j in rng.integers(0, 4, n)]
        b = [None if rng.random() < 0.02 else bool(x) for x in rng.integers(0, 2, n)]
        g = [None if key is None else 7 * idx[key] for key in keys]
        return Data([("s", keys, seg), ("i", k, 1000), ("i", v, 0), ("d", d, 0),
                     ("s", s2, 512), ("b", b, 0), ("i", g, 0)])
    return cached("layout-%s-%d" % (layout, seg), make)


def null_data():
    """every null combination of (string, int), b"" beside null, and col 2
    a string column of nulls only"""
    def make():
        pairs = [(b"a", 1), (b"a", None), (None, 1), (None, None), (b"", 1),
                 (b"", None), (b"a", 2), (None, 2), (b"", 2)]
        rng = np.random.default_rng(3)
        pick = [pairs[int(j)] for j in rng.integers(0, len(pairs), 600)]
        pick[:len(pairs)] = pairs
        return Data([("s", [p[0] for p in pick], 64),
                     ("i", [p[1] for p in pick], 100),
                     ("s", [None] * 600, 64),
                     ("i", [int(x) for x in rng.integers(-50, 50, 600)], 0)])
    return cached("nulls", make)


def no_allnull_data():
    """layout_data("dict_dense", 100) without the rows whose keys of columns
    0 and 1 are both null"""
    def make():
        d = layout_data("dict_dense", 100)
        keep = [i for i, r in enumerate(d.rows) if r[0] is not None or r[1] is not None]
        return Data([(k, [v[i] for i in keep], s) for k, v, s in d.cols])
    return cached("nulls-no-allnull", make)


WIDTH_D = (1, 2, 3, 4, 255, 256, 257)


def width_data(dcount):
    """dcount distinct strings beside an int key of span 1 (values 7, 8)"""
    def make():
        n = max(2 * dcount + 10, 600)
        rng = np.random.default_rng(dcount)
        ids = list(range(dcount)) * 2 + [int(x) for x in
                                         rng.integers(0, dcount, n - 2 * dcount)]
        keys = [b"w%05d" % (i * 7919) for i in ids]
        return Data([("s", keys, 128),
                     # every (string, int) pair occurs
                     ("i", [7] * dcount + [8] * dcount +
                      [7 + int(x) for x in rng.integers(0, 2, n - 2 * dcount)], 0),
                     ("i", [int(x) for x in rng.integers(-9, 9, n)], 0)])
    return cached("width-%d" % dcount, make)


def wide_data(int_bits):
    """3 distinct strings (codes 0..3: 2 bits) beside an int key whose
    component is int_bits wide. The packer bounds a column's zigzag range by
    its segments' minimum and bit width, so a column stored int_bits - 1 bits
    wide from 0 (zigzag values up to 2^(int_bits-1) - 2 here) has span
    2^(int_bits-1) - 1, and its codes 0 .. span + 1 need int_bits bits."""
    def make():
        n = 300
        rng = np.random.default_rng(int_bits)
        hi = ((1 << (int_bits - 1)) - 2) // 2    # zigzag(hi) = 2^(bits-1) - 2
        vals = [0, hi] + [int(x) for x in rng.integers(0, 1000, n - 2)]
        keys = [(b"p", b"q", b"r")[i % 3] for i in range(n)]
        return Data([("s", keys, 64), ("i", vals, 0),
                     ("i", [int(x) for x in rng.integers(-9, 9, n)], 0)])
    return cached("wide-%d" % int_bits, make)


def big_data():
    """300,000 rows in the default 128 Ki segments: 1,000 strings x 50 ints"""
    def make():
        n = 300_000
        rng = np.random.default_rng(99)
        si = rng.integers(0, 1000, n)
        ii = rng.integers(0, 50, n)
        si[:50_000] = np.arange(50_000) // 50      # every pair occurs
        ii[:50_000] = np.arange(50_000) % 50
        keys = [b"key-%04d-with-a-tail-past-16-bytes" % i if i % 2 else b"k%04d" % i
                for i in map(int, si)]
        return Data([("s", keys, 0),
                     ("i", [int(x) for x in ii], 0),
                     ("i", [int(x) for x in rng.integers(-1000, 1000, n)], 0)])
    return cached("big", make)


# ---------------------------------------------------------------------
# the plans both files run (name -> Spec over layout_data's columns)

def shape_specs():
    ge = (y.col(1) >= 2, lambda r: r[1] is not None and r[1] >= 2)
    return {
        "sum_avg_min_sum1": Spec([0, 1], [("sum", 2), ("avg", 3), ("min", 2),
                                          ("sum1", None)]),
        "str_last": Spec([1, 0], [("sum", 2), ("sum1", None)]),
        "str_middle_of_three": Spec([1, 0, 5], [("max", 2), ("sum1", None)]),
        "str_last_of_four": Spec([1, 5, 1, 0], [("sum", 3)]),
        "two_string_columns": Spec([0, 4], [("sum", 2), ("sum1", None)]),
        "same_column_twice": Spec([0, 0], [("min", 3), ("sum1", None)]),
        "distinct": Spec([0, 1]),
        "numeric_filter": Spec([0, 1], [("sum", 2), ("sum1", None)], where=ge),
        "having": Spec([0, 1], [("sum", 2), ("sum1", None)],
                       having=(y.col(3) > 20, lambda r: r[3] > 20)),
    }


def six_aggs_spec():
    """all six aggregates in one plan is more than the 4 a plan takes: two
    plans cover them; first(col 6) is unique per group of key col 0"""
    return [Spec([0, 1], [("sum", 2), ("sum1", None), ("min", 3), ("max", 2)]),
            Spec([0, 1], [("avg", 2), ("first", 6), ("max", 3), ("avg", 3)])]


def totals_specs():
    hv = (y.col(3) > 20, lambda r: r[3] > 20)
    aggs = [("sum", 2), ("sum1", None), ("min", 2), ("max", 3)]
    return {"totals": Spec([0, 1], aggs, totals="before"),
            "totals_before_having": Spec([0, 1], aggs, having=hv, totals="before"),
            "totals_after_having": Spec([0, 1], aggs, having=hv, totals="after")}


def order_specs():
    aggs = [("sum", 2), ("sum1", None)]
    return {"order_str_asc_int_desc": Spec([0, 1], aggs,
                                           order=[(0, False), (1, True)],
                                           limit=40, offset=7),
            "order_desc_offset": Spec([1, 0], aggs, order=[(1, True), (0, False)],
                                      limit=1000, offset=3)}


def with_null_error(fn):
    """fn() -> rows, or the string NULL_KEY_ERROR when it raised that"""
    try:
        return fn()
    except RuntimeError as e:
        assert NULL_KEY_ERROR in str(e), e
        return NULL_KEY_ERROR


def check_oracle(spec, data, ordered=False):
    want = with_null_error(lambda: model(spec, data.rows))
    got = with_null_error(lambda: y.oracle_execute(spec.plan(), data.chunk)[0])
    if isinstance(want, str) or isinstance(got, str):
        assert got == want
        return want
    same_rows(got, want, ordered=ordered, totals=spec.totals is not None)
    return want


# ---------------------------------------------------------------------
# CPU tests: the layouts are what the GPU tests say, and model == oracle

@pytest.mark.parametrize("layout,seg", LAYOUT_CASES)
def test_layouts_are_what_they_claim(layout, seg):
    d = layout_data(layout, seg)
    types = d.seg_types(0)
    assert len(types) > 1 or seg == 4096
    if layout == "mixed":
        assert len(set(types)) >= 3, types
    else:
        assert set(types) == {LAYOUT_TYPE[layout]}, (layout, seg, types)
    keys = [r[0] for r in d.rows]
    assert len({k for k in keys if k is not None}) == 37
    assert None in keys and b"" in keys
    # ragged against the int columns
    assert len(d.seg_types(1)) == 4 and len(d.seg_types(2)) == 1


@pytest.mark.parametrize("layout,seg", LAYOUT_CASES)
def test_model_is_oracle_layouts(layout, seg):
    d = layout_data(layout, seg)
    check_oracle(shape_specs()["sum_avg_min_sum1"], d)
    check_oracle(shape_specs()["two_string_columns"], d)


@pytest.mark.parametrize("name", sorted(shape_specs()))
def test_model_is_oracle_shapes(name):
    check_oracle(shape_specs()[name], layout_data("dict_dense", 100))


def test_model_is_oracle_six_aggregates():
    for spec in six_aggs_spec():
        check_oracle(spec, layout_data("dict_dense", 100))
        check_oracle(spec, layout_data("mixed", 64))


@pytest.mark.parametrize("name", sorted(totals_specs()))
def test_model_is_oracle_totals(name):
    # the layout data holds (null, null) rows: the reference refuses them
    # under WITH TOTALS, the oracle and the model with it
    assert check_oracle(totals_specs()[name],
                        layout_data("dict_dense", 100)) == NULL_KEY_ERROR
    want = check_oracle(totals_specs()[name], no_allnull_data())
    assert all(v is None for v in want[-1][:2])


@pytest.mark.parametrize("name", sorted(order_specs()))
def test_model_is_oracle_order(name):
    assert check_oracle(order_specs()[name],
                        layout_data("dict_dense", 100), True) == NULL_KEY_ERROR
    want = check_oracle(order_specs()[name], no_allnull_data(), True)
    assert len(want) > 0


def test_model_is_oracle_nulls():
    d = null_data()
    want = check_oracle(Spec([0, 1], [("sum", 3), ("sum1", None)]), d)
    keys = {r[:2] for r in want}
    assert {(b"a", None), (None, 1), (None, None), (b"", 1), (b"", None)} <= keys
    # a column of nulls only beside the int key, and beside the string key
    check_oracle(Spec([2, 1], [("sum1", None)]), d)
    check_oracle(Spec([0, 2], [("sum", 3)]), d)


@pytest.mark.parametrize("dcount", WIDTH_D)
def test_model_is_oracle_widths(dcount):
    want = check_oracle(Spec([0, 1], [("sum", 2), ("sum1", None)]),
                        width_data(dcount))
    assert len({r[0] for r in want}) == dcount


def test_model_is_oracle_wide_and_big():
    for bits in (60, 61):
        check_oracle(Spec([0, 1], [("sum", 2)]), wide_data(bits))
    want = check_oracle(Spec([0, 1], [("sum", 2), ("sum1", None)]), big_data())
    assert len(want) == 50_000
