"""Equi-join on STRING keys (include/ytql_gpu.h YtJoin): a string hash table
over the foreign rows, one probe per dictionary entry of the primary key
column, and a per-row lookup of the cached answer.

The oracle refuses string join keys, so the yardstick is a Python model of
join + plan (join_rows and the helpers below). The model itself is pinned
without a GPU: every case has an INTEGER TWIN — each distinct string mapped
to a distinct int64, null to null — and the model on the strings must equal
oracle_execute on the twin. The GPU cases then compare the product with the
model exactly: all data is integer sums and counts, so no tolerance is
involved.

Semantics (cg_routines/registry.cpp MultiJoinOpHelper): null joins null, the
empty string is a key and not null, INNER drops misses, LEFT null-extends,
duplicate foreign keys expand to one joined row per match."""
import collections

import numpy as np
import pytest

import ytsaurus_amd as y
from ytsaurus_amd import _abi
from ytsaurus_amd._abi import (SEG_DICTIONARY_DENSE, SEG_DICTIONARY_RLE,
                               SEG_DIRECT_DENSE, SEG_DIRECT_RLE, YtStateRow)


# ---------------------------------------------------------------------
# the model

def join_rows(fact_cols, items):
    """fact_cols: list of columns (python lists). items: list of dicts
    {pkey, fkeys, fvals (list of columns), left}. Returns the joined rows,
    [fact columns..., item 0 values..., item 1 values...], in fact row order,
    the matches of one fact row in foreign row order."""
    n = len(fact_cols[0])
    rows = [tuple(c[i] for c in fact_cols) for i in range(n)]
    for it in items:
        idx = collections.defaultdict(list)
        for r, k in enumerate(it["fkeys"]):
            idx[k].append(r)              # None is a key too: null joins null
        out = []
        for row in rows:
            m = idx.get(row[it["pkey"]], [])
            for r in m:
                out.append(row + tuple(c[r] for c in it["fvals"]))
            if not m and it["left"]:
                out.append(row + (None,) * len(it["fvals"]))
        rows = out
    return rows


def _sum(vals):
    vals = [v for v in vals if v is not None]
    return sum(vals) if vals else None


def group_rows(rows, key, aggs, where=None, having=None, totals=False):
    """key: column index or None (global aggregate). aggs: list of
    ("sum", col) / ("sum1",). having: predicate over the output row. totals:
    append (None, aggregates over every grouped row) after the groups."""
    if where:
        rows = [r for r in rows if where(r)]

    def fold(rs):
        return tuple(len(rs) if a[0] == "sum1" else _sum(r[a[1]] for r in rs)
                     for a in aggs)
    if key is None:
        return [fold(rows)] if rows else []
    groups = collections.OrderedDict()
    for r in rows:
        groups.setdefault(r[key], []).append(r)
    out = [(k,) + fold(rs) for k, rs in groups.items()]
    if having:
        out = [r for r in out if having(r)]
    if totals:
        out.append((None,) + fold(rows))
    return out


# ---------------------------------------------------------------------
# cases: python columns -> encoded chunks, as strings or as the integer twin

class Case:
    """fact: list of (kind, values, max_segment_values); kind 's' = bytes or
    None, 'i' = int or None. items: list of dicts {pkey, fkey (index into
    fcols), fcols: like fact, vals: foreign value column indices, left}."""

    def __init__(self, fact, items):
        self.fact = fact
        self.items = items
        self.n = len(fact[0][1])
        self._built = {}
        strings = set()
        for kind, vals, _ in fact + [c for it in items for c in it["fcols"]]:
            if kind == "s":
                strings.update(v for v in vals if v is not None)
        # distinct strings -> distinct int64, far apart and signed
        self.twin_of = {s: (i * 0x9E3779B97F4A7C15 + 12345) % (1 << 62) - (1 << 61)
                        for i, s in enumerate(sorted(strings))}
        assert len(set(self.twin_of.values())) == len(self.twin_of)

    def _enc(self, col, twin):
        kind, vals, seg = col
        if kind == "s" and not twin:
            return y.encode_string(list(vals), max_segment_values=seg)
        if kind == "s":
            vals = [None if v is None else self.twin_of[v] for v in vals]
        return y.encode_int64(
            np.array([0 if v is None else v for v in vals], dtype=np.int64),
            np.array([v is None for v in vals], dtype=np.uint8),
            max_segment_values=seg)

    def chunks(self, twin=False):
        """(fact chunk, [foreign chunk per item]); built once per flavour"""
        if twin not in self._built:
            fact = y.Chunk([self._enc(c, twin) for c in self.fact], self.n)
            foreign = [y.Chunk([self._enc(c, twin) for c in it["fcols"]],
                               len(it["fcols"][0][1])) for it in self.items]
            self._built[twin] = (fact, foreign)
        return self._built[twin]

    def joins(self, foreign, left=None):
        return [y.Join(foreign[i], it["pkey"], it["fkey"], it["vals"],
                       is_left=it["left"] if left is None else left)
                for i, it in enumerate(self.items)]

    def joined(self, left=None, limit=None):
        cols = [c[1] if limit is None else c[1][:limit] for c in self.fact]
        return join_rows(cols, [
            {"pkey": it["pkey"], "fkeys": it["fcols"][it["fkey"]][1],
             "fvals": [it["fcols"][v][1] for v in it["vals"]],
             "left": it["left"] if left is None else left}
            for it in self.items])


_CACHE = {}


def cached(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def seg_types(col):
    return [col._cenc.segments[j].type for j in range(col._cenc.segment_count)]


SPECIAL = [b"", b"\x00", b"\x00\x00", b"a\x00b", b"abc", b"abcd",
           b"same-but-last-x", b"same-but-last-y",
           b"sixteen-byte-stem-tail-A", b"sixteen-byte-stem-tail-B"]


def dim_table(keys, rng, nulls=1, dups=()):
    """foreign columns [key 's', fval 'i' (5 % null), fcat 'i' in 0..6] over
    `keys` shuffled, plus `nulls` null keys and the keys in `dups` again"""
    fk = list(keys) + [None] * nulls + list(dups)
    fk = [fk[i] for i in rng.permutation(len(fk))]
    fval = [None if rng.random() < 0.05 else int(v)
            for v in rng.integers(-10**6, 10**6, len(fk))]
    fcat = [int(v) for v in rng.integers(0, 7, len(fk))]
    return [("s", fk, 0), ("i", fval, 0), ("i", fcat, 0)]


def fact_table(keys, rng, seg, vseg=0):
    """fact columns [key 's', g 'i' in 0..11 (3 % null), v 'i']"""
    n = len(keys)
    g = [None if rng.random() < 0.03 else int(v) for v in rng.integers(0, 12, n)]
    v = [int(x) for x in rng.integers(-1000, 1000, n)]
    return [("s", list(keys), seg), ("i", g, vseg), ("i", v, vseg)]


def layout_keys(layout, rng):
    """fact keys that the writer stores in the named layout (asserted by the
    tests), with the special strings, nulls and keys missing from the
    foreign side among them. Returns (fact keys, foreign keys)."""
    if layout == "dict_dense":
        pool = SPECIAL + [b"k%03d" % i for i in range(30)]
        keys = [pool[i] for i in rng.integers(0, len(pool), 3000)]
        keys = [None if rng.random() < 0.03 else k for k in keys]
        return keys, pool[:25] + [b"only-foreign"]
    if layout == "dict_rle":
        pool = SPECIAL[:4] + [b"a-long-dictionary-rle-key-%02d" % i for i in range(4)]
        keys = []
        while len(keys) < 2048:
            k = pool[int(rng.integers(0, len(pool)))]
            keys += [None if rng.random() < 0.1 else k] * 8
        return keys, pool[:6] + [b"only-foreign"]
    if layout == "direct_dense":
        keys = [b"row-%05d" % i for i in rng.permutation(1500)]
        keys[7], keys[800], keys[801] = b"", None, b"\x00"
        return keys, [b"row-%05d" % i for i in range(0, 1500, 2)] + [b"", b"\x00"]
    if layout == "direct_rle":
        keys = []
        for i in range(400):
            k = None if i % 41 == 0 else b"a-long-direct-rle-run-key-%05d" % i
            keys += [k] * 4
        return keys, [b"a-long-direct-rle-run-key-%05d" % i for i in range(0, 400, 3)]
    raise KeyError(layout)


LAYOUT_SEG = {"dict_dense": 64, "dict_rle": 256, "direct_dense": 64,
              "direct_rle": 256}
LAYOUT_TYPE = {"dict_dense": SEG_DICTIONARY_DENSE, "dict_rle": SEG_DICTIONARY_RLE,
               "direct_dense": SEG_DIRECT_DENSE, "direct_rle": SEG_DIRECT_RLE}
LAYOUTS = list(LAYOUT_SEG)


def layout_case(layout):
    def make():
        rng = np.random.default_rng(LAYOUTS.index(layout) + 11)
        keys, fkeys = layout_keys(layout, rng)
        return Case(fact_table(keys, rng, LAYOUT_SEG[layout]),
                    [{"pkey": 0, "fkey": 0, "fcols": dim_table(fkeys, rng),
                      "vals": [1, 2], "left": False}])
    return cached("layout-" + layout, make)


def mixed_case():
    """one key column that holds at least three layouts, ragged against the
    5,000-row value segments; duplicate foreign keys, a duplicated null and a
    duplicated empty string"""
    def make():
        rng = np.random.default_rng(21)
        keys, fkeys = [], []
        for layout in ("dict_dense", "direct_dense", "direct_rle", "dict_rle"):
            k, f = layout_keys(layout, rng)
            keys += k[:1024]
            fkeys += f
        fkeys = sorted(set(fkeys))
        dups = [b"", None, b"k001", b"k001", b"row-00002"]
        return Case(fact_table(keys, rng, 256, vseg=5000),
                    [{"pkey": 0, "fkey": 0,
                      "fcols": dim_table(fkeys, rng, nulls=1, dups=dups),
                      "vals": [1, 2], "left": False}])
    return cached("mixed", make)


def dup_foreign_case():
    """a foreign key column in a DICTIONARY layout: 300 foreign rows over 24
    keys, so every key — null and the empty string among them — is held by
    about 12 rows and a fact row expands to as many joined rows"""
    def make():
        rng = np.random.default_rng(25)
        pool = SPECIAL[:6] + [b"d%02d" % i for i in range(20)]
        keys = [pool[i] for i in rng.integers(0, len(pool), 1000)]
        keys = [None if rng.random() < 0.04 else k for k in keys]
        fpool = pool[:22] + [None, b"only-foreign"]
        fk = [fpool[i] for i in rng.integers(0, len(fpool), 300)]
        fcols = [("s", fk, 0),
                 ("i", [int(v) for v in rng.integers(-1000, 1000, 300)], 0),
                 ("i", [int(v) for v in rng.integers(0, 7, 300)], 0)]
        return Case(fact_table(keys, rng, 64, vseg=5000),
                    [{"pkey": 0, "fkey": 0, "fcols": fcols, "vals": [1, 2],
                      "left": False}])
    return cached("dup-foreign", make)


def unique_case():
    """unique foreign keys (a plain scan and ORDER BY need that), 1,000 fact
    rows in 64-row key segments against one value segment"""
    def make():
        rng = np.random.default_rng(31)
        pool = SPECIAL + [b"u%03d" % i for i in range(60)]
        keys = [pool[i] for i in rng.integers(0, len(pool), 1000)]
        keys = [None if rng.random() < 0.03 else k for k in keys]
        fact = fact_table(keys, rng, 64, vseg=5000)
        fact[2] = ("i", list(range(1000)), 5000)        # v: a unique row id
        fcols = dim_table(pool[:50], rng, nulls=1)
        # distinct non-null values: ORDER BY over them has no ties between keys
        fcols[1] = ("i", [1000 * i + 7 for i in range(len(fcols[0][1]))], 0)
        return Case(fact, [{"pkey": 0, "fkey": 0, "fcols": fcols,
                            "vals": [1, 2], "left": False}])
    return cached("unique", make)


def wave_case():
    """four 130-row key segments whose dictionaries hold 1, 63, 64 and 65
    entries: the boundaries of a wave's worth of entries"""
    def make():
        rng = np.random.default_rng(41)
        keys = []
        for d in (1, 63, 64, 65):
            seg = [b"w%02d-%03d" % (d, i % d) for i in range(130)]
            keys += [seg[i] for i in rng.permutation(130)]
        fkeys = sorted(set(keys))[::2]
        return Case(fact_table(keys, rng, 130),
                    [{"pkey": 0, "fkey": 0, "fcols": dim_table(fkeys, rng, nulls=0),
                      "vals": [1, 2], "left": False}])
    return cached("wave", make)


def null_side_case(which):
    """fact: a null fact key, no null foreign key; foreign: the reverse"""
    def make():
        rng = np.random.default_rng(51)
        keys = [b"n%02d" % (i % 20) for i in range(1000)]
        if which == "fact":
            for i in range(0, 1000, 9):
                keys[i] = None
        return Case(fact_table(keys, rng, 64),
                    [{"pkey": 0, "fkey": 0,
                      "fcols": dim_table([b"n%02d" % i for i in range(15)], rng,
                                         nulls=0 if which == "fact" else 2),
                      "vals": [1, 2], "left": False}])
    return cached("null-" + which, make)


def two_item_case(kind):
    """str_int: string item 0, integer item 1 keyed on item 0's fcat (plan
    column 4). str_str: two string items on two primary string columns.
    int_str: integer item 0 on g, string item 1 on the key column."""
    def make():
        rng = np.random.default_rng(61)
        pool = SPECIAL + [b"t%03d" % i for i in range(40)]
        keys = [pool[i] for i in rng.integers(0, len(pool), 2000)]
        keys = [None if rng.random() < 0.03 else k for k in keys]
        fact = fact_table(keys, rng, 64)
        pool2 = [b"", b"second-%02d" % 0] + [b"second-%02d" % i for i in range(1, 9)]
        k2 = [pool2[i] for i in rng.integers(0, len(pool2), 2000)]
        fact.append(("s", [None if rng.random() < 0.05 else k for k in k2], 128))
        sdim = dim_table(pool[:40], rng, nulls=1)                 # fcat 0..6
        idim = [("i", [0, 1, 2, 3, 4, None], 0),
                ("i", [10, 11, 12, 13, 14, 19], 0)]
        gdim = [("i", list(range(0, 10)) + [None], 0),
                ("i", [100 + i for i in range(11)], 0)]
        sdim2 = [("s", pool2[:7] + [None], 0),
                 ("i", [200 + i for i in range(8)], 0)]
        P = len(fact)
        if kind == "str_int":
            items = [{"pkey": 0, "fkey": 0, "fcols": sdim, "vals": [1, 2], "left": True},
                     {"pkey": P + 1, "fkey": 0, "fcols": idim, "vals": [1], "left": False}]
        elif kind == "str_str":
            items = [{"pkey": 0, "fkey": 0, "fcols": sdim, "vals": [1, 2], "left": False},
                     {"pkey": 3, "fkey": 0, "fcols": sdim2, "vals": [1], "left": True}]
        else:
            items = [{"pkey": 1, "fkey": 0, "fcols": gdim, "vals": [1], "left": True},
                     {"pkey": 0, "fkey": 0, "fcols": sdim[:2], "vals": [1], "left": False}]
        return Case(fact, items)
    return cached("two-" + kind, make)


def big_case():
    """the grid-stride case: 100,000 fact rows over 3,000 keys in 8,192-row
    segments, 20,000 foreign rows (a table far larger than LDS)"""
    def make():
        rng = np.random.default_rng(71)
        ki = rng.integers(0, 3000, 100_000)
        keys = [b"big-key-%06d" % k for k in ki]
        fkeys = [b"big-key-%06d" % k for k in rng.permutation(30_000)[:20_000]]
        fcols = [("s", fkeys, 8192),
                 ("i", [int(v) for v in rng.integers(-1000, 1000, 20_000)], 8192),
                 ("i", [int(v) for v in rng.integers(0, 7, 20_000)], 8192)]
        g = [int(v) for v in rng.integers(0, 12, 100_000)]
        v = [int(x) for x in rng.integers(-1000, 1000, 100_000)]
        return Case([("s", keys, 8192), ("i", g, 0), ("i", v, 0)],
                    [{"pkey": 0, "fkey": 0, "fcols": fcols, "vals": [1, 2],
                      "left": False}])
    return cached("big", make)


# ---------------------------------------------------------------------
# plan shapes over the standard column space: 0 key, 1 g, 2 v | 3 fval, 4 fcat

def shape(name, joins):
    """(plan, model over the joined rows) of a named plan shape"""
    if name == "group_fact":
        return (y.Plan(keys=[y.col(1)], join=joins,
                       aggs=[y.agg_sum(y.col(3)), y.agg_sum(y.col(2)), y.agg_sum1()]),
                lambda rows: group_rows(rows, 1, [("sum", 3), ("sum", 2), ("sum1",)]))
    if name == "group_foreign":
        return (y.Plan(keys=[y.col(4)], join=joins,
                       aggs=[y.agg_sum(y.col(2)), y.agg_sum1()]),
                lambda rows: group_rows(rows, 4, [("sum", 2), ("sum1",)]))
    if name == "global":
        return (y.Plan(aggs=[y.agg_sum(y.col(3)), y.agg_sum1()], join=joins),
                lambda rows: group_rows(rows, None, [("sum", 3), ("sum1",)]))
    if name == "filter_foreign":
        return (y.Plan(filter=y.col(3) > 0, keys=[y.col(1)], join=joins,
                       aggs=[y.agg_sum(y.col(3)), y.agg_sum1()]),
                lambda rows: group_rows(rows, 1, [("sum", 3), ("sum1",)],
                                        where=lambda r: r[3] is not None and r[3] > 0))
    if name == "having":
        return (y.Plan(keys=[y.col(4)], join=joins, having=y.col(2) > 100,
                       aggs=[y.agg_sum(y.col(2)), y.agg_sum1()]),
                lambda rows: group_rows(rows, 4, [("sum", 2), ("sum1",)],
                                        having=lambda r: r[2] > 100))
    if name == "totals":
        # WITH TOTALS forbids a null group key: the filter drops null g
        return (y.Plan(filter=y.col(1) >= 0, keys=[y.col(1)], join=joins,
                       with_totals=True,
                       aggs=[y.agg_sum(y.col(3)), y.agg_sum1()]),
                lambda rows: group_rows(rows, 1, [("sum", 3), ("sum1",)],
                                        where=lambda r: r[1] is not None,
                                        totals=True))
    raise KeyError(name)


GROUP_SHAPES = ["group_fact", "group_foreign", "global", "filter_foreign",
                "having", "totals"]


def same(got, want, totals=False):
    if totals:
        assert got[-1] == want[-1]
        got, want = got[:-1], want[:-1]
    assert y.sort_rows(got) == y.sort_rows(want)


def oracle_twin(case, plan_of, left=None):
    fact, foreign = case.chunks(twin=True)
    plan = plan_of(case.joins(foreign, left))
    rows, _ = y.oracle_execute(plan, fact)
    return rows


def gpu_rows(case, plan_of, cuda, left=None, **kw):
    fact, foreign = case.chunks()
    plan = plan_of(case.joins(foreign, left))
    kw.setdefault("max_groups_hint", 4096)
    got, _ = y.gpu_execute(plan, fact.c_device(cuda),
                           join_foreign=[f.c_device(cuda) for f in foreign], **kw)
    return got


def scan_plan(joins):
    return y.Plan(projects=[y.col(2), y.col(1), y.col(3), y.col(4)], join=joins)


def scan_model(rows):
    return [(r[2], r[1], r[3], r[4]) for r in rows]


def order_plan(joins):
    return y.Plan(projects=[y.col(2), y.col(3)], order_by=[(1, True)], limit=10,
                  join=joins)


def check_order(got, rows):
    """the ordered foreign values are the model's; every row is a joined row
    (rows that share a foreign value tie, and any of them may be returned)"""
    want = sorted((r[3] for r in rows), reverse=True)[:10]
    assert [r[1] for r in got] == want
    src = collections.Counter((r[2], r[3]) for r in rows)
    for r in got:
        assert src[tuple(r)] > 0
        src[tuple(r)] -= 1


# ---------------------------------------------------------------------
# the model against the oracle on the integer twin (no GPU)

def test_model_semantics_by_hand():
    rows = join_rows([[b"", None, b"x", b"y"], [1, 2, 3, 4]],
                     [{"pkey": 0, "fkeys": [None, b"", b"x", b"x"],
                       "fvals": [[10, 20, 30, 40]], "left": False}])
    assert rows == [(b"", 1, 20), (None, 2, 10), (b"x", 3, 30), (b"x", 3, 40)]
    rows = join_rows([[b"y", None]], [{"pkey": 0, "fkeys": [b""], "fvals": [[1]],
                                       "left": True}])
    assert rows == [(b"y", None), (None, None)]


@pytest.mark.parametrize("left", [False, True], ids=["inner", "left"])
@pytest.mark.parametrize("name", LAYOUTS + ["mixed", "dup-foreign", "wave",
                                            "null-fact", "null-foreign"])
def test_model_equals_oracle_on_the_integer_twin(name, left):
    case = {"mixed": mixed_case, "wave": wave_case,
            "dup-foreign": dup_foreign_case,
            "null-fact": lambda: null_side_case("fact"),
            "null-foreign": lambda: null_side_case("foreign")}.get(
                name, lambda: layout_case(name))()
    for sh in GROUP_SHAPES:
        want = shape(sh, None)[1](case.joined(left))
        got = oracle_twin(case, lambda j: shape(sh, j)[0], left)
        same(got, want, totals=sh == "totals")
        assert want, (name, sh)


@pytest.mark.parametrize("left", [False, True], ids=["inner", "left"])
def test_model_equals_oracle_scan_and_order(left):
    case = unique_case()
    rows = case.joined(left)
    assert oracle_twin(case, scan_plan, left) == scan_model(rows)
    check_order(oracle_twin(case, order_plan, False), case.joined(False))


@pytest.mark.parametrize("kind", ["str_int", "str_str", "int_str"])
def test_model_equals_oracle_two_items(kind):
    case = two_item_case(kind)
    plan_of, model = two_item_plan(case)
    same(oracle_twin(case, plan_of), model(case.joined()))


def two_item_plan(case):
    """group by g, summing the LAST appended column and counting"""
    last = len(case.fact) + sum(len(it["vals"]) for it in case.items) - 1
    return (lambda j: y.Plan(keys=[y.col(1)], join=j,
                             aggs=[y.agg_sum(y.col(last)), y.agg_sum1()]),
            lambda rows: group_rows(rows, 1, [("sum", last), ("sum1",)]))


def test_oracle_refuses_string_join_keys():
    """the reason this file has a model of its own"""
    case = null_side_case("fact")
    fact, foreign = case.chunks()
    plan = shape("group_fact", case.joins(foreign))[0]
    rc, _, _ = y.oracle_execute(plan, fact, expect_error=True)
    assert rc != _abi.YT_OK


def test_layout_cells_hold_their_layout():
    """so that a writer change cannot silently empty a cell"""
    for layout in LAYOUTS:
        types = seg_types(layout_case(layout).chunks()[0].columns[0])
        assert set(types) == {LAYOUT_TYPE[layout]}, (layout, types)
        assert len(types) > 1
    types = seg_types(mixed_case().chunks()[0].columns[0])
    assert len(set(types)) >= 3, types
    # foreign key columns: direct dense, and a dictionary layout
    assert set(seg_types(mixed_case().chunks()[1][0].columns[0])) == \
        {SEG_DIRECT_DENSE}
    assert set(seg_types(dup_foreign_case().chunks()[1][0].columns[0])) == \
        {SEG_DICTIONARY_DENSE}
    wave = seg_types(wave_case().chunks()[0].columns[0])
    assert len(wave) == 4 and set(wave) <= {SEG_DICTIONARY_DENSE,
                                            SEG_DICTIONARY_RLE}, wave


# ---------------------------------------------------------------------
# GPU

@pytest.mark.gpu
@pytest.mark.parametrize("left", [False, True], ids=["inner", "left"])
@pytest.mark.parametrize("layout", LAYOUTS + ["mixed", "dup-foreign"])
def test_gpu_layout_cells(cuda, layout, left):
    """every primary key layout alone and mixed, through every grouped plan
    shape; the foreign keys are direct dense, and a dictionary in dup-foreign.
    mixed and dup-foreign hold duplicate foreign keys, a duplicated null and
    a duplicated empty string"""
    case = {"mixed": mixed_case, "dup-foreign": dup_foreign_case}.get(
        layout, lambda: layout_case(layout))()
    rows = case.joined(left)
    for sh in GROUP_SHAPES:
        got = gpu_rows(case, lambda j: shape(sh, j)[0], cuda, left)
        same(got, shape(sh, None)[1](rows), totals=sh == "totals")
    inserted, entries = y.gpu_debug_last_strjoin()
    fkeys = case.items[0]["fcols"][0][1]
    assert inserted == sum(k is not None for k in fkeys)
    assert 0 < entries <= case.n


@pytest.mark.gpu
def test_gpu_wave_boundaries(cuda):
    case = wave_case()
    for left in (False, True):
        got = gpu_rows(case, lambda j: shape("group_fact", j)[0], cuda, left)
        same(got, shape("group_fact", None)[1](case.joined(left)))
    assert y.gpu_debug_last_strjoin()[1] == 1 + 63 + 64 + 65


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["fact", "foreign"])
def test_gpu_null_on_one_side_only(cuda, which):
    case = null_side_case(which)
    for left in (False, True):
        for sh in ("group_fact", "global"):
            got = gpu_rows(case, lambda j: shape(sh, j)[0], cuda, left)
            same(got, shape(sh, None)[1](case.joined(left)))


@pytest.mark.gpu
@pytest.mark.parametrize("left", [False, True], ids=["inner", "left"])
def test_gpu_scan_and_order(cuda, left):
    case = unique_case()
    rows = case.joined(left)
    assert gpu_rows(case, scan_plan, cuda, left, out_capacity=2048) == \
        scan_model(rows)
    check_order(gpu_rows(case, order_plan, cuda, False), case.joined(False))


@pytest.mark.gpu
def test_gpu_duplicates_refused_outside_group_by(cuda):
    case = mixed_case()
    for plan_of in (scan_plan, order_plan):
        with pytest.raises(RuntimeError, match="duplicate foreign keys with "
                                               "ORDER BY / plain scan"):
            gpu_rows(case, plan_of, cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["str_int", "str_str", "int_str"])
def test_gpu_two_items(cuda, kind):
    case = two_item_case(kind)
    plan_of, model = two_item_plan(case)
    same(gpu_rows(case, plan_of, cuda), model(case.joined()))
    n_str = sum(it["fcols"][it["fkey"]][0] == "s" for it in case.items)
    inserted, _ = y.gpu_debug_last_strjoin()
    assert inserted == sum(k is not None for it in case.items
                           if it["fcols"][it["fkey"]][0] == "s"
                           for k in it["fcols"][it["fkey"]][1])
    assert n_str == (2 if kind == "str_str" else 1)


@pytest.mark.gpu
def test_gpu_input_row_limit_cuts_the_key_column(cuda):
    """500 of 1,000 rows: the limit falls inside the 8th 64-row key segment;
    only the kept segments' entries are probed"""
    case = unique_case()
    got = gpu_rows(case, lambda j: shape("group_fact", j)[0], cuda,
                   input_row_limit=500)
    same(got, shape("group_fact", None)[1](case.joined(limit=500)))
    _, entries = y.gpu_debug_last_strjoin()
    full = gpu_rows(case, lambda j: shape("group_fact", j)[0], cuda)
    assert len(full) and 0 < entries < y.gpu_debug_last_strjoin()[1]


@pytest.mark.gpu
@pytest.mark.parametrize("left", [False, True], ids=["inner", "left"])
def test_gpu_bottom_query(cuda, left):
    """yt_gpu_query_partial states, merged by the oracle, equal the model"""
    case = mixed_case()
    fact, foreign = case.chunks()
    mk = lambda j: y.Plan(keys=[y.col(1)], join=j,
                          aggs=[y.agg_sum(y.col(3)), y.agg_sum1()])
    cap = 4096
    states_t = cuda.zeros((cap, 4), dtype=cuda.int64, device="cuda")
    counts, _ = y.gpu_partial(mk(case.joins(foreign, left)), fact.c_device(cuda),
                              2, states_t.data_ptr(), cap, max_groups_hint=4096,
                              join_foreign=[f.c_device(cuda) for f in foreign])
    total = sum(counts)
    raw = states_t.cpu().numpy()[:max(total, 1)].tobytes()
    arr = (YtStateRow * max(total, 1)).from_buffer_copy(raw)
    got = y.oracle_merge(mk(None), [(arr, total)])
    same(got, group_rows(case.joined(left), 1, [("sum", 3), ("sum1",)]))


@pytest.mark.gpu
def test_gpu_grid_stride_and_entry_count(cuda):
    case = big_case()
    fact, _ = case.chunks()
    assert set(seg_types(fact.columns[0])) == {SEG_DICTIONARY_DENSE}
    keys = case.fact[0][1]
    want_entries = sum(len(set(keys[a:a + 8192])) for a in range(0, len(keys), 8192))
    for sh in ("group_fact", "group_foreign"):
        got = gpu_rows(case, lambda j: shape(sh, j)[0], cuda)
        same(got, shape(sh, None)[1](case.joined()))
    inserted, entries = y.gpu_debug_last_strjoin()
    assert inserted == 20_000
    assert entries == want_entries and entries < 50_000     # rows: 100,000


# ---- refusals, each with the pool left as it was found ----

def in_use():
    return int(_abi.gpu_lib().yt_gpu_debug_pool_blocks_in_use())


def refused(match, fn):
    before = in_use()
    with pytest.raises(RuntimeError, match=match):
        fn()
    assert in_use() == before


@pytest.mark.gpu
def test_gpu_refusals_and_pool_balance(cuda):
    case = unique_case()
    fact, foreign = case.chunks()
    dfact = fact.c_device(cuda)
    dfor = foreign[0].c_device(cuda)
    twin_for = case.chunks(twin=True)[1][0].c_device(cuda)
    group = lambda j: y.Plan(keys=[y.col(1)], aggs=[y.agg_sum1()], join=j)

    def run(plan, jf):
        return y.gpu_execute(plan, dfact, max_groups_hint=1024, join_foreign=jf)

    # a successful join gives everything back
    before = in_use()
    run(group(y.Join(foreign[0], 0, 0, [1, 2])), dfor)
    assert in_use() == before
    # STRING against INT64, both directions
    refused("join: key type mismatch",
            lambda: run(group(y.Join(foreign[0], 1, 0, [1])), dfor))
    refused("join: key type mismatch",
            lambda: run(group(y.Join(foreign[0], 0, 1, [1])), dfor))
    refused("join: key type mismatch",
            lambda: run(group(y.Join(case.chunks(twin=True)[1][0], 0, 0, [1])),
                        twin_for))
    # a string key naming an appended foreign column: item 0 would have to
    # append the string, and string foreign values stay refused
    refused("join: string foreign values not this round",
            lambda: run(group([y.Join(foreign[0], 0, 0, [0]),
                               y.Join(foreign[0], 3, 0, [1])]), [dfor, dfor]))
    # an appended INT64 column against a string foreign key
    refused("join: key type mismatch",
            lambda: run(group([y.Join(foreign[0], 0, 0, [1]),
                               y.Join(foreign[0], 3, 0, [1])]), [dfor, dfor]))
    # a string-key GROUP BY beside a string join
    refused("join with string group keys",
            lambda: run(y.Plan(keys=[y.col(0)], aggs=[y.agg_sum1()],
                               join=y.Join(foreign[0], 0, 0, [1])), dfor))
    # a string predicate beside a string join
    refused("string predicate beside a join",
            lambda: run(y.Plan(filter=y.col(0) == y.lit_str(b"abc"),
                               keys=[y.col(1)], aggs=[y.agg_sum1()],
                               join=y.Join(foreign[0], 0, 0, [1])), dfor))
    # a string projection beside a string join
    refused("string projection beside a join",
            lambda: run(y.Plan(projects=[y.col(0), y.col(3)],
                               join=y.Join(foreign[0], 0, 0, [1])), dfor))
