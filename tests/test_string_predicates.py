"""WHERE over string columns on the GPU: relational ops against a string or
null literal, is_prefix, is_substr and LIKE.

How parity is checked: the CPU oracle has no string literals, so it cannot
run these plans. Every chunk here is built from Python lists; a small
reference in this file answers each string-predicate leaf per row as True,
False or None (bytes comparison, startswith, `in`, LIKE translated to an `re`
pattern) and that answer is appended to the chunk as a boolean mask column
with nulls. The GPU result of the plan with the string predicate must equal
the oracle's result of the SAME plan with each leaf replaced by col(mask):
Python vouches for the leaf, the oracle for everything around it (Kleene
logic, aggregates, ORDER BY, totals). Integers, counts, min and max are
exact; double sums (values from [0, 1), atomic add order not fixed) are
within 1e-6 relative.

The matchers themselves are also driven on the CPU through yt_strpred_eval
(the host build of the code the GPU entry pass runs) against the same
reference, on seeded random cases."""
import ctypes as C
import re
from collections import namedtuple

import numpy as np
import pytest

import ytsaurus_amd as y
from ytsaurus_amd import _abi
from ytsaurus_amd._abi import (VT_STRING, VT_INT64, VT_DOUBLE,
                               SCAN_PATH_GENERIC, SCAN_PATH_STR_GENERAL,
                               EX_EQ, EX_NE, EX_LT, EX_LE, EX_GT, EX_GE,
                               EX_LIT_STRING, EX_IS_PREFIX, EX_IS_SUBSTR,
                               EX_LIKE)

REL = {"==": EX_EQ, "!=": EX_NE, "<": EX_LT, "<=": EX_LE, ">": EX_GT,
       ">=": EX_GE}


# ---------------------------------------------------------------------
# the Python reference for one leaf

def ref_rel(op, a, b):
    """a op b over bytes-or-None, the engine's non-canonical relational rule:
    null < any value, null == null, the result is never null"""
    if a is None or b is None:
        lt = a is None and b is not None
        eq = a is None and b is None
    else:
        lt, eq = a < b, a == b          # bytes: unsigned, shorter is less
    return {"==": eq, "!=": not eq, "<": lt, "<=": lt or eq,
            ">": not (lt or eq), ">=": not lt}[op]


def like_regex(pattern, escape):
    """LIKE pattern -> compiled bytes regex; None when the pattern ends in a
    lone escape (an invalid plan)"""
    out = []
    i = 0
    while i < len(pattern):
        c = pattern[i:i + 1]
        if escape is not None and c == escape:
            if i + 1 >= len(pattern):
                return None
            out.append(re.escape(pattern[i + 1:i + 2]))
            i += 2
            continue
        out.append(b".*" if c == b"%" else b"." if c == b"_" else re.escape(c))
        i += 1
    return re.compile(b"".join(out), re.DOTALL)


def ref_leaf(spec, cols):
    """per-row answers (True / False / None) of one string-predicate leaf"""
    kind, col = spec[0], spec[1]
    texts = cols[col]
    if kind == "cmp":
        _, _, op, lit, flipped = spec
        if flipped:
            return [ref_rel(op, lit, t) for t in texts]
        return [ref_rel(op, t, lit) for t in texts]
    if kind == "isnull":
        return [ref_rel(spec[2], t, None) for t in texts]
    if kind == "prefix":
        return [None if t is None else t.startswith(spec[2]) for t in texts]
    if kind == "substr":
        return [None if t is None else spec[2] in t for t in texts]
    if kind == "like":
        rx = like_regex(spec[2], spec[3])
        return [None if t is None else rx.fullmatch(t) is not None
                for t in texts]
    raise AssertionError(kind)


# ---------------------------------------------------------------------
# predicate specs: one description, two expressions
#   leaves  ("cmp", col, op, literal, literal_on_the_left)
#           ("isnull", col, "==" | "!=")
#           ("prefix", col, literal) ("substr", col, literal)
#           ("like", col, pattern, escape-or-None)
#   ("int", fn)  an ordinary expression, the same in both plans
#   ("and", a, b) ("or", a, b) ("not", a)

LEAVES = ("cmp", "isnull", "prefix", "substr", "like")


def spec_leaves(spec, out=None):
    out = [] if out is None else out
    if spec[0] in LEAVES:
        out.append(spec)
    elif spec[0] in ("and", "or"):
        spec_leaves(spec[1], out)
        spec_leaves(spec[2], out)
    elif spec[0] == "not":
        spec_leaves(spec[1], out)
    return out


def gpu_expr(spec):
    kind = spec[0]
    if kind == "cmp":
        _, col, op, lit, flipped = spec
        a, b = (y.lit_str(lit), y.col(col)) if flipped else (y.col(col), lit)
        return {"==": a.__eq__, "!=": a.__ne__, "<": a.__lt__, "<=": a.__le__,
                ">": a.__gt__, ">=": a.__ge__}[op](b)
    if kind == "isnull":
        return y.col(spec[1]) == None if spec[2] == "==" \
            else y.col(spec[1]) != None       # noqa: E711
    if kind == "prefix":
        return y.is_prefix(spec[2], y.col(spec[1]))
    if kind == "substr":
        return y.is_substr(spec[2], y.col(spec[1]))
    if kind == "like":
        return y.like(y.col(spec[1]), spec[2], escape=spec[3])
    if kind == "int":
        return spec[1]()
    if kind == "and":
        return gpu_expr(spec[1]).and_(gpu_expr(spec[2]))
    if kind == "or":
        return gpu_expr(spec[1]).or_(gpu_expr(spec[2]))
    if kind == "not":
        return gpu_expr(spec[1]).not_()
    raise AssertionError(kind)


def mask_expr(spec, first_mask, counter=None):
    """the same tree with the i-th leaf (spec_leaves order) replaced by
    col(first_mask + i)"""
    counter = [0] if counter is None else counter
    kind = spec[0]
    if kind in LEAVES:
        e = y.col(first_mask + counter[0])
        counter[0] += 1
        return e
    if kind == "int":
        return spec[1]()
    if kind == "not":
        return mask_expr(spec[1], first_mask, counter).not_()
    a = mask_expr(spec[1], first_mask, counter)
    b = mask_expr(spec[2], first_mask, counter)
    return a.and_(b) if kind == "and" else a.or_(b)


def kleene(spec, cols, n):
    """per-row Kleene value of the spec with every ("int", ...) operand left
    out (an AND / OR with one keeps its other side): used only to count what
    the string leaves select on their own"""
    kind = spec[0]
    if kind in LEAVES:
        return ref_leaf(spec, cols)
    if kind == "int":
        return None
    if kind == "not":
        return [None if v is None else not v for v in kleene(spec[1], cols, n)]
    a, b = kleene(spec[1], cols, n), kleene(spec[2], cols, n)
    if a is None or b is None:
        return a if b is None else b
    if kind == "and":
        return [False if (x is False or z is False) else
                (None if (x is None or z is None) else True)
                for x, z in zip(a, b)]
    return [True if (x is True or z is True) else
            (None if (x is None or z is None) else False)
            for x, z in zip(a, b)]


# ---------------------------------------------------------------------
# data. Columns: 0 string (the predicate column, 2048-row segments),
# 1 int64 with 10 % nulls (5000-row segments: ragged against column 0),
# 2 double in [0, 1) with 5 % nulls, 3 int64 key 0..6, 4 second string
# column (4096-row segments), 5 int64 key 0..4. Mask columns go after.

N = 20_000
SEG = 2048
ROW_LIMIT = 7000
NCOLS = 6
_DATA = {}
Data = namedtuple("Data", "name cols raw chunk")


def _bytes_list(v):
    return [None if s is None else (s if isinstance(s, bytes) else s.encode())
            for s in v]


# the dictionary population: the empty string and two strings with bytes
# >= 0x80 (unsigned order), then ordinary keys
def population(k):
    special = [b"", b"\xff\xfe-high", b"\x80abc"]
    return (special + [b"s-key-%04d" % i for i in range(k)])[:k] if k >= 8 \
        else [b"s-key-%04d" % i for i in range(k)]


def seg_dict_dense(rng, k, rows):
    pop = population(k)
    idx = np.concatenate([np.arange(k), rng.integers(0, k, rows - k)])
    rng.shuffle(idx)
    return [None if rng.random() < 0.02 else pop[i] for i in idx]


def seg_dict_rle(rng, k, rows, run=3):
    pop = population(k)
    out, r = [], 0
    while len(out) < rows:
        out += [None if rng.random() < 0.02 else pop[r % k]] * run
        r += 1
    return out[:rows]


def seg_direct_dense(rng, tag, rows):
    return [None if rng.random() < 0.02 else b"%s-u%05d" % (tag, i)
            for i in range(rows)]


def seg_direct_rle(rng, tag, rows, run=4):
    out, r = [], 0
    while len(out) < rows:
        out += [None if rng.random() < 0.02
                else b"%s-long-unique-run-%06d" % (tag, r)] * run
        r += 1
    return out[:rows]


def seg_all_null(rows):
    return [None] * rows


def seg_rows():
    return [min(SEG, N - s) for s in range(0, N, SEG)]     # 9 x 2048 + 1568


def strings_dict_dense(rng):
    ks = [300, 63, 64, 65, None, 8, 300, 300, 300, 300]
    return sum([seg_all_null(r) if k is None else seg_dict_dense(rng, k, r)
                for k, r in zip(ks, seg_rows())], [])


def strings_dict_rle(rng):
    ks = [1, 63, 64, 65, 300, None, 300, 8, 300, 300]
    return sum([seg_all_null(r) if k is None
                else seg_dict_rle(rng, k, r, run=8 if k < 100 else 3)
                for k, r in zip(ks, seg_rows())], [])


def strings_direct_dense(rng):
    return sum([seg_all_null(r) if i == 4
                else seg_direct_dense(rng, b"s%d" % (i % 3), r)
                for i, r in enumerate(seg_rows())], [])


def strings_direct_rle(rng):
    return sum([seg_all_null(r) if i == 4
                else seg_direct_rle(rng, b"s%d" % (i % 3), r,
                                    run=3 if i == 2 else 4)
                for i, r in enumerate(seg_rows())], [])


def strings_mixed(rng):
    out = []
    for i, r in enumerate(seg_rows()):
        out += seg_all_null(r) if i == 8 else \
            [seg_dict_dense(rng, 65, r), seg_dict_rle(rng, 300, r),
             seg_direct_dense(rng, b"s-key", r),
             seg_direct_rle(rng, b"s-key", r)][i % 4]
    return out


DD, DR, XD, XR = (_abi.SEG_DICTIONARY_DENSE, _abi.SEG_DICTIONARY_RLE,
                  _abi.SEG_DIRECT_DENSE, _abi.SEG_DIRECT_RLE)
# the all-null segment and the one-key segment come out as DictionaryRle
# (an empty / one-entry dictionary under one run per null gap)
LAYOUTS = {
    "dict_dense": (strings_dict_dense, [DD, DD, DD, DD, DR, DD, DD, DD, DD, DD]),
    "dict_rle": (strings_dict_rle, [DR] * 10),
    "direct_dense": (strings_direct_dense, [XD, XD, XD, XD, DR, XD, XD, XD, XD, XD]),
    "direct_rle": (strings_direct_rle, [XR, XR, XR, XR, DR, XR, XR, XR, XR, XR]),
    "mixed": (strings_mixed, [DD, DR, XD, XR, DD, DR, XD, XR, DR, DR]),
}
NULL_SEG = {"dict_dense": 4, "dict_rle": 5, "direct_dense": 4,
            "direct_rle": 4, "mixed": 8}


def raw_columns():
    """the non-predicate columns: the same in every data set"""
    rng = np.random.default_rng(4321)
    return dict(
        v1=rng.integers(-1000, 1000, N, dtype=np.int64),
        v1n=(rng.random(N) < 0.10).astype(np.uint8),
        v2=rng.random(N),
        v2n=(rng.random(N) < 0.05).astype(np.uint8),
        k3=rng.integers(0, 7, N, dtype=np.int64),
        s4=[None if rng.random() < 0.02 else b"h%02d" % ((i * 7) % 40)
            for i in range(N)],
        k5=rng.integers(0, 5, N, dtype=np.int64))


def build_data(name, strings, raw, n=N):
    raw = {k: v[:n] for k, v in raw.items()}
    cols = {0: _bytes_list(strings)[:n], 4: raw["s4"]}
    chunk = y.Chunk([y.encode_string(cols[0], max_segment_values=SEG),
                     y.encode_int64(raw["v1"], raw["v1n"],
                                    max_segment_values=5000),
                     y.encode_double(raw["v2"], raw["v2n"]),
                     y.encode_int64(raw["k3"]),
                     y.encode_string(raw["s4"], max_segment_values=4096),
                     y.encode_int64(raw["k5"])], n)
    return Data(name, cols, raw, chunk)


def data(name):
    if name not in _DATA:
        if name.startswith("first7000:"):
            # the first 7000 rows of a data set as a chunk of their own: what
            # input_row_limit = 7000 must see (the cut falls inside column
            # 0's fourth segment, column 1's second, and the only segment of
            # columns 2, 3 and 5)
            full = data(name.split(":")[1])
            _DATA[name] = build_data(name, full.cols[0], full.raw, n=ROW_LIMIT)
        else:
            gen, _ = LAYOUTS[name]
            _DATA[name] = build_data(name, gen(np.random.default_rng(99)),
                                     raw_columns())
    return _DATA[name]


def seg_types(col):
    return [col._cenc.segments[j].type for j in range(col._cenc.segment_count)]


def with_masks(d, spec):
    """the chunk plus one boolean mask column (with nulls) per leaf"""
    extra = []
    for leaf in spec_leaves(spec):
        ans = ref_leaf(leaf, d.cols)
        vals = np.array([1 if a else 0 for a in ans], dtype=np.uint8)
        nulls = np.array([1 if a is None else 0 for a in ans], dtype=np.uint8)
        extra.append(y.encode_bool(vals, nulls))
    return y.Chunk(list(d.chunk.columns) + extra, d.chunk.row_count)


# ---------------------------------------------------------------------
# plan shapes

def c(i):
    return y.col(i)


Shape = namedtuple("Shape", "plan approx ordered path")
SHAPES = {
    # int64-key GROUP BY: sum, min, sum(1)
    "group": Shape(lambda f: y.Plan(filter=f, keys=[c(3)],
                                    aggs=[y.agg_sum(c(1)), y.agg_min(c(1)),
                                          y.agg_sum1()]),
                   (), False, SCAN_PATH_GENERIC),
    "global": Shape(lambda f: y.Plan(filter=f,
                                     aggs=[y.agg_sum(c(2)), y.agg_sum1(),
                                           y.agg_max(c(1))]),
                    (0,), False, SCAN_PATH_GENERIC),
    "two_key": Shape(lambda f: y.Plan(filter=f, keys=[c(3), c(5)],
                                      aggs=[y.agg_sum(c(1)), y.agg_sum1()]),
                     (), False, SCAN_PATH_GENERIC),
    "project": Shape(lambda f: y.Plan(filter=f, projects=[c(1), c(3), c(2)]),
                     (), True, None),
    "topk": Shape(lambda f: y.Plan(filter=f, projects=[c(1), c(3), c(5)],
                                   order_by=[(0, False), (1, True), (2, False)],
                                   limit=25),
                  (), True, None),
    "totals": Shape(lambda f: y.Plan(filter=f, keys=[c(3)],
                                     aggs=[y.agg_sum(c(1)), y.agg_sum1()],
                                     with_totals=True),
                    (), False, SCAN_PATH_GENERIC),
    "str_key": Shape(lambda f: y.Plan(filter=f, keys=[c(0)],
                                      aggs=[y.agg_sum(c(1)), y.agg_min(c(1)),
                                            y.agg_sum1()]),
                     (), False, SCAN_PATH_STR_GENERAL),
    # the state row of the bottom queries: one sum and the row count
    "partial": Shape(lambda f: y.Plan(filter=f, keys=[c(3)],
                                      aggs=[y.agg_sum(c(1)), y.agg_sum1()]),
                     (), False, None),
    "partial_str": Shape(lambda f: y.Plan(filter=f, keys=[c(0)],
                                          aggs=[y.agg_sum(c(1)), y.agg_sum1()]),
                         (), False, None),
}


# ---------------------------------------------------------------------
# the case table

Case = namedtuple("Case", "name group data shape spec")
MID = {}


def mid_of(name):
    """a literal equal to an entry: the median distinct non-null text"""
    if name not in MID:
        vals = sorted({t for t in data(name).cols[0] if t is not None})
        MID[name] = vals[len(vals) // 2]
    return MID[name]


def matrix_specs(mid):
    specs = []
    for op in REL:
        specs.append(("%s_right" % op, ("cmp", 0, op, mid, False)))
        specs.append(("%s_left" % op, ("cmp", 0, op, mid, True)))
    specs += [
        ("eq_null", ("isnull", 0, "==")),
        ("ne_null", ("isnull", 0, "!=")),
        ("prefix", ("prefix", 0, mid[:-2])),
        ("substr", ("substr", 0, mid[-3:-1])),
        ("like_head", ("like", 0, mid[:-2] + b"_%", None)),
        ("like_tail", ("like", 0, b"%" + mid[-2:-1] + b"_", None)),
    ]
    return specs


def int_pos():
    return c(1) > 0


def dbl_low():
    return c(2) < 0.5


def build_cases():
    cases = []
    for layout in LAYOUTS:
        for nm, spec in matrix_specs(mid_of(layout)):
            cases.append(Case("%s-%s" % (layout, nm), "layout_" + layout,
                              layout, "group", spec))
    mid = mid_of("dict_dense")
    longlit = mid + b"z" * 80
    edge = [
        ("eq_empty_literal", ("cmp", 0, "==", b"", False)),
        ("gt_empty_literal", ("cmp", 0, ">", b"", False)),
        ("lt_empty_literal", ("cmp", 0, "<", b"", False)),       # nulls only
        ("prefix_empty_literal", ("prefix", 0, b"")),
        ("substr_empty_literal", ("substr", 0, b"")),
        ("like_empty_pattern", ("like", 0, b"", None)),
        ("eq_entry", ("cmp", 0, "==", mid, False)),
        ("le_proper_prefix", ("cmp", 0, "<=", mid[:-1], False)),
        ("gt_proper_prefix", ("cmp", 0, ">", mid[:-1], False)),
        ("lt_entry_is_prefix", ("cmp", 0, "<", mid + b"x", False)),
        ("ge_entry_is_prefix", ("cmp", 0, ">=", mid + b"x", False)),
        ("lt_long_literal", ("cmp", 0, "<", longlit, False)),
        ("gt_long_literal", ("cmp", 0, ">", longlit, False)),
        ("empty_eq_long_literal", ("cmp", 0, "==", longlit, False)),
        ("empty_substr_long_literal", ("substr", 0, longlit)),
        ("all_lt_ff", ("cmp", 0, "<", b"\xff\xff", False)),
        ("ge_ff", ("cmp", 0, ">=", b"\xff", False)),
        ("lt_80", ("cmp", 0, "<", b"\x80", False)),
        ("ge_80_left", ("cmp", 0, "<=", b"\x80", True)),
        ("like_escape", ("like", 0, b"s\\-key\\-00_%", b"\\")),
        ("like_high_byte", ("like", 0, b"_\xfe%", None)),
    ]
    for nm, spec in edge:
        cases.append(Case("edge-" + nm, "edge", "dict_dense", "group", spec))

    p = ("prefix", 0, b"s-key-01")                  # null for a null text
    lk = ("like", 0, b"%-key-0_5%", None)
    kle = [
        ("and_int", ("and", p, ("int", int_pos))),
        ("or_int", ("or", p, ("int", int_pos))),
        ("not", ("not", p)),
        ("not_like", ("not", lk)),
        ("two_columns", ("and", ("cmp", 0, "<", mid, False),
                         ("prefix", 4, b"h1"))),
        ("same_twice", ("or", ("and", p, ("int", int_pos)),
                        ("and", p, ("int", dbl_low)))),
        ("null_rule_or_null_result", ("or", ("cmp", 0, "!=", mid, False), lk)),
        ("four_predicates", ("or", ("and", p, lk),
                             ("and", ("substr", 4, b"3"),
                              ("cmp", 4, ">=", b"h2", True)))),
    ]
    for nm, spec in kle:
        cases.append(Case("kleene-" + nm, "kleene", "dict_dense", "group", spec))

    ge = ("cmp", 0, ">=", mid, False)
    for shape in ("global", "two_key", "project", "topk", "totals"):
        cases.append(Case("shape-" + shape, "shape", "dict_dense", shape, ge))
    cases.append(Case("shape-project-mixed", "shape", "mixed", "project",
                      ("like", 0, b"s%5_", None)))
    cases.append(Case("shape-str_key-on-key", "shape", "dict_dense", "str_key",
                      ("and", p, ("int", int_pos))))
    cases.append(Case("shape-str_key-on-key-mixed", "shape", "mixed", "str_key",
                      ("substr", 0, b"-00")))
    cases.append(Case("shape-str_key-on-second-column", "shape", "dict_dense",
                      "str_key", ("prefix", 4, b"h1")))
    cases.append(Case("shape-str_key-is-null", "shape", "dict_dense",
                      "str_key", ("isnull", 0, "!=")))
    cases.append(Case("rowlimit-group", "rowlimit", "first7000:dict_dense",
                      "group", ge))
    cases.append(Case("rowlimit-str_key", "rowlimit", "first7000:dict_dense",
                      "str_key", p))
    cases.append(Case("rowlimit-project", "rowlimit", "first7000:dict_dense",
                      "project", lk))
    cases.append(Case("rowlimit-direct-group", "rowlimit",
                      "first7000:direct_dense", "group",
                      ("cmp", 0, "<", mid_of("direct_dense"), False)))
    cases.append(Case("rowlimit-direct-str_key", "rowlimit",
                      "first7000:direct_dense", "str_key",
                      ("like", 0, b"s_-u0%7", None)))
    cases.append(Case("bottom-int-key", "bottom", "dict_dense", "partial",
                      ("and", lk, ("int", int_pos))))
    cases.append(Case("bottom-str-key", "bottom_str", "mixed", "partial_str",
                      ("prefix", 0, b"s-key-0")))
    return cases


CASES = build_cases()


def cases_of(group):
    return [k for k in CASES if k.group == group]


def oracle_rows(case):
    d = data(case.data)
    plan = SHAPES[case.shape].plan(mask_expr(case.spec, NCOLS))
    rows, _ = y.oracle_execute(plan, with_masks(d, case.spec))
    return rows


def assert_same(case, got, want):
    shape = SHAPES[case.shape]
    if shape.ordered:
        assert got == want, case.name
        return
    if case.shape == "totals":
        assert got[-1] == want[-1], case.name
        got, want = got[:-1], want[:-1]
    got, want = y.sort_rows(got), y.sort_rows(want)
    assert len(got) == len(want), (case.name, len(got), len(want))
    nkeys = 0 if case.shape == "global" else 1
    for g, w in zip(got, want):
        for i, (gv, wv) in enumerate(zip(g, w)):
            if i - nkeys in shape.approx and wv is not None:
                assert gv == pytest.approx(wv, rel=1e-6, abs=0), (case.name, w)
            else:
                assert gv == wv, (case.name, g, w)


# ---------------------------------------------------------------------
# CPU tests

def test_matcher_fuzz():
    """yt_strpred_eval against the Python reference on 5000 seeded cases over
    the alphabet a b % _ \\ : wildcards and escapes collide all the time.
    Half of the texts are derived from the literal so that matches are
    common for every operator."""
    rng = np.random.default_rng(20261)
    alpha = [b"a", b"b", b"%", b"_", b"\\"]
    ops = list(REL) + ["prefix", "substr", "like", "like_esc"]

    def rnd(lo=0):
        ln = int(rng.integers(lo, 13))
        return b"".join(alpha[i] for i in rng.integers(0, 5, ln))

    def derived(op, lit):
        if op.startswith("like"):
            esc = b"\\" if op == "like_esc" else None
            out, i = b"", 0
            while i < len(lit):
                ch = lit[i:i + 1]
                if esc is not None and ch == esc:
                    out += lit[i + 1:i + 2]
                    i += 2
                    continue
                out += rnd()[:3] if ch == b"%" else \
                    alpha[int(rng.integers(0, 5))] if ch == b"_" else ch
                i += 1
            return out[:12]
        if op == "prefix":
            return (lit + rnd())[:12]
        if op == "substr":
            return (rnd()[:2] + lit + rnd())[:12]
        return lit if rng.random() < 0.5 else (lit + rnd())[:12]

    hits = misses = errors = 0
    for _ in range(5000):
        op = ops[int(rng.integers(0, len(ops)))]
        lit = rnd()
        text = derived(op, lit) if rng.random() < 0.5 else rnd()
        assert len(text) <= 12 and len(lit) <= 12
        if op in REL:
            want = ref_rel(op, text, lit)
            got = y.strpred_eval(REL[op], text, lit)
        elif op == "prefix":
            want = text.startswith(lit)
            got = y.strpred_eval(EX_IS_PREFIX, text, lit)
        elif op == "substr":
            want = lit in text
            got = y.strpred_eval(EX_IS_SUBSTR, text, lit)
        else:
            esc = b"\\" if op == "like_esc" else None
            rx = like_regex(lit, esc)
            got = y.strpred_eval(EX_LIKE, text, lit, escape=esc)
            if rx is None:
                assert got < 0, (text, lit)
                errors += 1
                continue
            want = rx.fullmatch(text) is not None
        assert got == int(want), (op, text, lit, got, want)
        hits += bool(want)
        misses += not want
    total = hits + misses
    assert hits >= 0.10 * total and misses >= 0.10 * total, (hits, misses)
    assert errors > 0            # lone trailing escapes did occur


EXPLICIT_LIKE = [
    # text, pattern, escape
    (b"", b"", None), (b"a", b"", None), (b"", b"%", None), (b"abc", b"%", None),
    (b"", b"%%", None), (b"abc", b"%%", None), (b"abc", b"a%%c", None),
    (b"abc", b"abc%", None), (b"abc", b"ab%", None), (b"ab", b"abc%", None),
    (b"", b"_", None), (b"a", b"_", None), (b"ab", b"_", None),
    (b"50%", b"50\\%", b"\\"), (b"50x", b"50\\%", b"\\"),
    (b"a_b", b"a\\_b", b"\\"), (b"axb", b"a\\_b", b"\\"),
    (b"a\\b", b"a\\\\b", b"\\"), (b"a%b", b"a%%b", b"%"),
    (b"aababab", b"%ab%ab_", None), (b"aabababx", b"%ab%ab_", None),
    (b"abababab", b"%ab%ab_", None), (b"mississippi", b"m%iss%ip_i", None),
    (b"mississippi", b"%s_s%p", None), (b"a\nb", b"a_b", None),
    (b"\xff\x80z", b"\xff_z", None), (b"\xc3\xa9", b"_", None),
    (b"\xc3\xa9", b"__", None), (b"x\xfe", b"%\xfe", None),
    (b"a\\", b"a\\", None),
]


def test_matcher_explicit_cases():
    for text, pat, esc in EXPLICIT_LIKE:
        want = like_regex(pat, esc).fullmatch(text) is not None
        assert y.strpred_eval(EX_LIKE, text, pat, escape=esc) == int(want), \
            (text, pat, esc)
    # a pattern that ends in a lone escape is an error, whatever the text
    for text in (b"", b"a", b"a\\"):
        assert y.strpred_eval(EX_LIKE, text, b"a\\", escape=b"\\") < 0
        assert y.strpred_eval(EX_LIKE, text, b"\\", escape=b"\\") < 0
    # an unknown operator
    assert y.strpred_eval(99, b"a", b"a") < 0
    # the length tie-break and unsigned bytes, all six operators
    for a, b in ((b"ab", b"abc"), (b"abc", b"ab"), (b"ab", b"ab"), (b"", b""),
                 (b"", b"a"), (b"\x7f", b"\x80"), (b"\xff", b"a"),
                 (b"a\xff", b"a\x00b")):
        for op, code in REL.items():
            assert y.strpred_eval(code, a, b) == int(ref_rel(op, a, b)), (op, a, b)
    # the empty literal is a prefix and a substring of everything
    for text in (b"", b"a", b"\xff"):
        assert y.strpred_eval(EX_IS_PREFIX, text, b"") == 1
        assert y.strpred_eval(EX_IS_SUBSTR, text, b"") == 1
    assert y.strpred_eval(EX_IS_PREFIX, b"ab", b"abc") == 0
    assert y.strpred_eval(EX_IS_SUBSTR, b"xxabab", b"aba") == 1
    assert y.strpred_eval(EX_IS_SUBSTR, b"xxabab", b"abb") == 0


def test_builders():
    e = y.col(0) == b"x\x00y"
    assert e.c.op == EX_EQ and e.c.a.contents.op == _abi.EX_COLUMN
    lit = e.c.b.contents
    assert lit.op == EX_LIT_STRING and lit.lit_len == 3
    assert C.string_at(lit.lit_str, lit.lit_len) == b"x\x00y"
    e = y.col(0) < "k0100é"                       # str: UTF-8 encoded
    assert e.c.op == EX_LT
    assert C.string_at(e.c.b.contents.lit_str, e.c.b.contents.lit_len) == \
        "k0100é".encode()
    assert y.lit_str(b"").c.lit_len == 0
    e = y.is_prefix(b"//home/", y.col(2))
    assert e.c.op == EX_IS_PREFIX and e.c.a.contents.op == EX_LIT_STRING
    assert e.c.b.contents.op == _abi.EX_COLUMN and e.c.b.contents.col == 2
    e = y.is_substr("ab", y.col(1))
    assert e.c.op == EX_IS_SUBSTR and e.c.a.contents.lit_len == 2
    e = y.like(y.col(0), b"x\\%%", escape=b"\\")
    assert e.c.op == EX_LIKE and e.c.lit_i64 == 92
    assert e.c.a.contents.op == _abi.EX_COLUMN
    assert e.c.b.contents.op == EX_LIT_STRING
    assert y.like(y.col(0), "x%").c.lit_i64 == -1
    with pytest.raises(ValueError):
        y.like(y.col(0), "x", escape=b"ab")
    with pytest.raises(TypeError):
        y.col(0) == object()


def test_expr_layout_is_appended():
    """the two new YtExpr fields sit after `b`: every older offset stands"""
    f = _abi.YtExpr
    assert (f.op.offset, f.col.offset, f.lit_i64.offset, f.lit_dbl.offset,
            f.a.offset, f.b.offset) == (0, 4, 8, 16, 24, 32)
    assert f.lit_str.offset == 40 and f.lit_len.offset == 48
    assert C.sizeof(f) == 56


def test_oracle_refuses_string_nodes():
    d = data("dict_dense")
    for flt in (y.col(0) == b"x", (y.col(1) > 0).and_(y.is_prefix(b"a", y.col(0))),
                y.like(y.col(0), b"a%").not_()):
        plan = y.Plan(filter=flt, keys=[c(3)], aggs=[y.agg_sum1()])
        with pytest.raises(NotImplementedError):
            y.oracle_execute(plan, d.chunk)
        with pytest.raises(NotImplementedError):
            y.oracle_partial(plan, d.chunk, 2)
        with pytest.raises(NotImplementedError):
            y.oracle_merge(plan, [])
    plan = y.Plan(filter=y.is_substr(b"a", c(0)), keys=[c(0)],
                  aggs=[y.agg_sum1()])
    with pytest.raises(NotImplementedError):
        y.oracle_partial_str(plan, d.chunk, 2)
    with pytest.raises(NotImplementedError):
        y.oracle_merge_str(plan, [])
    plan = y.Plan(filter=y.col(0) != "a", keys=[c(3), c(5)], aggs=[y.agg_sum1()])
    with pytest.raises(NotImplementedError):
        y.oracle_partial_mk(plan, d.chunk, 2, ([0, 0], [9, 9]))
    with pytest.raises(NotImplementedError):
        y.oracle_merge_mk(plan, [], ([0, 0], [9, 9]))


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layouts_are_what_the_cases_assume(layout):
    d = data(layout)
    assert seg_types(d.chunk.columns[0]) == LAYOUTS[layout][1]
    assert [s.row_count for s in d.chunk.columns[0].segments] == seg_rows()
    assert d.chunk.columns[1].segments[0].row_count == 5000
    nulls = sum(t is None for t in d.cols[0])
    assert 0.015 * N < nulls - SEG < 0.03 * N        # ~2 % beside the null segment
    ns = NULL_SEG[layout] * SEG
    assert all(t is None for t in d.cols[0][ns:ns + SEG])
    if layout == "dict_dense":
        assert {b"", b"\xff\xfe-high", b"\x80abc"} <= set(d.cols[0])
        per_seg = [len({t for t in d.cols[0][s:s + SEG] if t is not None})
                   for s in range(0, N, SEG)]
        assert per_seg[:6] == [300, 63, 64, 65, 0, 8]
    if layout == "dict_rle":
        per_seg = [len({t for t in d.cols[0][s:s + SEG] if t is not None})
                   for s in range(0, N, SEG)]
        assert per_seg[:6] == [1, 63, 64, 65, 300, 0]


@pytest.mark.parametrize("group", sorted({k.group for k in CASES}))
def test_case_table_is_sane(group):
    """every case's string leaves select some rows but not all (cases named
    empty / all are exempt), and the oracle's run of the mask plan returns
    rows: no case passes by comparing two empty results"""
    names = [k.name for k in CASES]
    assert len(names) == len(set(names))
    for case in cases_of(group):
        d = data(case.data)
        n = d.chunk.row_count
        sel = sum(v is True for v in kleene(case.spec, d.cols, n))
        tag = case.name.split("-", 1)[1]
        if tag.startswith("empty"):
            assert sel == 0, case.name
        elif tag.startswith("all"):
            assert sel == n, case.name
        else:
            assert 1 <= sel <= n - 1, (case.name, sel)
            assert len(oracle_rows(case)) >= 1, case.name


# ---------------------------------------------------------------------
# GPU tests

_DEV = {}


def dev_chunk(cuda, name):
    if name not in _DEV:
        _DEV[name] = data(name).chunk.c_device(cuda)
    return _DEV[name]


def scan_path():
    return _abi.gpu_lib().yt_gpu_debug_last_scan_path()


def last_entries():
    return _abi.gpu_lib().yt_gpu_debug_last_strpred_entries()


def run_case(cuda, case, **kw):
    shape = SHAPES[case.shape]
    plan = shape.plan(gpu_expr(case.spec))
    d = data(case.data)
    got, st = y.gpu_execute(plan, dev_chunk(cuda, case.data),
                            max_groups_hint=4096,
                            out_capacity=d.chunk.row_count + 16, **kw)
    if shape.path is not None:
        assert scan_path() == shape.path, case.name
    assert_same(case, got, oracle_rows(case))
    return got, st


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layout_matrix(cuda, layout):
    """every operator, the literal on either side, == / != null and the three
    functions over one string layout (and over all four mixed in one column):
    dictionary sizes 1, 63, 64, 65 and 300, a segment of nulls only, 2 % null
    texts, 2048-row string segments against 5000-row value segments"""
    assert seg_types(data(layout).chunk.columns[0]) == LAYOUTS[layout][1]
    group = cases_of("layout_" + layout)
    assert len(group) == 18
    for case in group:
        run_case(cuda, case)


@pytest.mark.gpu
def test_predicate_is_evaluated_per_entry(cuda):
    """a 300-key dictionary column of 20 000 rows in 8192-row segments: the
    entry pass touches the dictionaries, not the rows"""
    rng = np.random.default_rng(31)
    keys = [None if rng.random() < 0.02 else b"k%04d" % int(rng.integers(0, 300))
            for _ in range(N)]
    chunk = y.Chunk([y.encode_string(keys, max_segment_values=8192),
                     y.encode_int64(rng.integers(0, 9, N, dtype=np.int64))], N)
    assert seg_types(chunk.columns[0]) == [DD, DD, DD]
    dev = chunk.c_device(cuda)
    entries = sum(len({t for t in keys[s:s + 8192] if t is not None})
                  for s in range(0, N, 8192))
    assert 600 <= entries <= 900 < N

    def run(flt):
        plan = y.Plan(filter=flt, keys=[c(1)], aggs=[y.agg_sum1()])
        got, _ = y.gpu_execute(plan, dev, max_groups_hint=64)
        return sum(r[1] for r in got)

    assert run(c(0) < b"k0150") == sum(ref_rel("<", t, b"k0150") for t in keys)
    assert last_entries() == entries
    run(y.is_prefix(b"k00", c(0)).or_(y.like(c(0), b"%9")))
    assert last_entries() == 2 * entries          # summed over predicates
    assert run(c(0) == None) == sum(t is None for t in keys)   # noqa: E711
    assert last_entries() == 0                    # a constant per row: no pass
    run(c(1) > 3)
    assert last_entries() == 0


@pytest.mark.gpu
def test_literal_edge_cases(cuda):
    for case in cases_of("edge"):
        run_case(cuda, case)


@pytest.mark.gpu
def test_kleene_composition(cuda):
    for case in cases_of("kleene"):
        run_case(cuda, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases_of("shape"), ids=lambda k: k.name)
def test_plan_shapes(cuda, case):
    got, _ = run_case(cuda, case)
    if case.shape == "topk":
        assert len(got) == 25
    if case.shape == "totals":
        assert len(got) == 7 + 1


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases_of("rowlimit"), ids=lambda k: k.name)
def test_input_row_limit_cuts_the_segment_list(cuda, case):
    """input_row_limit = 7000 on the 20 000-row chunk equals the plan on the
    first 7000 rows: only the kept segments are laid out and evaluated, and
    the segment the limit cuts is still read by its own layout"""
    shape = SHAPES[case.shape]
    plan = shape.plan(gpu_expr(case.spec))
    full = case.data.split(":")[1]
    got, st = y.gpu_execute(plan, dev_chunk(cuda, full),
                            max_groups_hint=N, out_capacity=N,
                            input_row_limit=ROW_LIMIT)
    if case.shape == "group":
        assert st.incomplete_input == 1
    assert_same(case, got, oracle_rows(case))
    kept = data(full).cols[0][:4 * SEG]             # segments 0..3 are kept
    if full == "direct_dense":
        assert last_entries() == 4 * SEG            # an entry per stored row
    else:
        assert last_entries() == sum(
            len({t for t in kept[s:s + SEG] if t is not None})
            for s in range(0, 4 * SEG, SEG))


@pytest.mark.gpu
def test_bottom_query_int_key(cuda):
    case, = cases_of("bottom")
    d = data(case.data)
    plan = SHAPES[case.shape].plan(gpu_expr(case.spec))
    cap = 1024
    states_t = cuda.zeros((cap, 4), dtype=cuda.int64, device="cuda")
    counts, _ = y.gpu_partial(plan, dev_chunk(cuda, case.data), 3,
                              states_t.data_ptr(), cap, max_groups_hint=4096)
    assert last_entries() > 0
    got, _ = y.gpu_merge(plan, states_t.data_ptr(), sum(counts),
                         max_groups_hint=4096,
                         col_types=[VT_STRING, VT_INT64, VT_DOUBLE, VT_INT64])
    assert_same(case, got, oracle_rows(case))
    assert len(got) == 7 and d.chunk.row_count == N


@pytest.mark.gpu
def test_bottom_query_multi_key(cuda):
    case = Case("bottom-two-key", "bottom", "dict_dense", "two_key",
                ("cmp", 0, ">=", mid_of("dict_dense"), False))
    plan = SHAPES["two_key"].plan(gpu_expr(case.spec))
    dev = dev_chunk(cuda, case.data)
    ranges = y.gpu_key_ranges(plan, dev)
    cap = 1024
    states_t = cuda.zeros((cap, 4), dtype=cuda.int64, device="cuda")
    counts, _ = y.gpu_partial_mk(plan, dev, 2, states_t.data_ptr(), cap, ranges,
                                 max_groups_hint=4096)
    assert last_entries() > 0
    got, _ = y.gpu_merge_mk(plan, states_t.data_ptr(), sum(counts), ranges,
                            max_groups_hint=4096)
    want = oracle_rows(case)
    assert y.sort_rows(got) == y.sort_rows(want) and len(want) == 35


@pytest.mark.gpu
def test_bottom_query_string_key(cuda):
    case, = cases_of("bottom_str")
    d = data(case.data)
    plan = SHAPES[case.shape].plan(gpu_expr(case.spec))
    cap = d.chunk.row_count + 16
    states_t = cuda.zeros((cap, 4), dtype=cuda.int64, device="cuda")
    pool_cap = 64 * cap
    pool_t = cuda.zeros(pool_cap, dtype=cuda.uint8, device="cuda")
    counts, pbytes, _ = y.gpu_partial_str(plan, dev_chunk(cuda, case.data), 1,
                                          states_t.data_ptr(), cap,
                                          pool_t.data_ptr(), pool_cap,
                                          max_groups_hint=N)
    assert scan_path() == SCAN_PATH_STR_GENERAL
    assert last_entries() > 0
    got, _ = y.gpu_merge_str(plan, states_t.data_ptr(), counts,
                             pool_t.data_ptr(), pbytes,
                             col_types=[VT_STRING, VT_INT64, VT_DOUBLE,
                                        VT_INT64, VT_STRING, VT_INT64],
                             max_groups_hint=N)
    assert_same(case, got, oracle_rows(case))
    assert all(r[0] is not None and r[0].startswith(b"s-key-0") for r in got)


UNSUPPORTED, INVALID = _abi.YT_ERR_UNSUPPORTED, _abi.YT_ERR_INVALID_PLAN


def refused(cuda, plan, code, message, **kw):
    with pytest.raises(RuntimeError,
                       match=r"ytql error %d: .*%s" % (code, message)):
        y.gpu_execute(plan, dev_chunk(cuda, "dict_dense"),
                      max_groups_hint=4096, **kw)


@pytest.mark.gpu
def test_refusals(cuda):
    aggs = [y.agg_sum1()]
    grp = dict(keys=[c(3)], aggs=aggs)
    # string column against string column: the message of before
    refused(cuda, y.Plan(filter=c(0) == c(4), **grp), UNSUPPORTED,
            "string column inside a filter")
    refused(cuda, y.Plan(filter=y.is_prefix(b"a", c(0)).and_(c(0) < c(4)), **grp),
            UNSUPPORTED, "string column inside a filter")
    # a string literal against a non-string operand, or in arithmetic
    refused(cuda, y.Plan(filter=c(1) == b"x", **grp), INVALID, "type mismatch")
    refused(cuda, y.Plan(filter=y.lit_str(b"a") < c(2), **grp), INVALID,
            "type mismatch")
    refused(cuda, y.Plan(filter=(c(1) + b"x") > 0, **grp), INVALID,
            "type mismatch")
    refused(cuda, y.Plan(filter=y.lit_str(b"a") == y.lit_str(b"a"), **grp),
            INVALID, "type mismatch")
    refused(cuda, y.Plan(filter=y.is_prefix(b"a", c(1)), **grp), INVALID,
            "type mismatch")
    refused(cuda, y.Plan(filter=y.is_substr(c(0), b"a"), **grp), INVALID,
            "type mismatch")
    refused(cuda, y.Plan(filter=y.like(y.lit_str(b"a"), c(0)), **grp), INVALID,
            "type mismatch")
    refused(cuda, y.Plan(filter=y.like(c(0), b"ab\\", escape=b"\\"), **grp),
            INVALID, "lone escape")
    # outside the filter
    refused(cuda, y.Plan(keys=[y.is_prefix(b"s", c(0))], aggs=aggs),
            UNSUPPORTED, "string column inside a filter or key expression")
    refused(cuda, y.Plan(keys=[c(1) + b"x"], aggs=aggs),
            UNSUPPORTED, "string column inside a filter or key expression")
    refused(cuda, y.Plan(keys=[c(3)], aggs=[y.agg_sum(c(0) == b"x")]),
            UNSUPPORTED, "string column inside an aggregate argument")
    refused(cuda, y.Plan(keys=[c(0)], aggs=[y.agg_max(y.like(c(4), b"h%"))]),
            UNSUPPORTED, "string column inside an aggregate argument")
    refused(cuda, y.Plan(projects=[c(1), c(0) == b"x"]), UNSUPPORTED,
            "inside a projection")
    refused(cuda, y.Plan(keys=[c(3)], aggs=aggs, having=c(1) == b"x"),
            UNSUPPORTED, "HAVING over string values")
    # more than four predicates with a bitmap
    five = c(0) == b"a"
    for lit in (b"b", b"c", b"d", b"e"):
        five = five.or_(c(0) == lit)
    refused(cuda, y.Plan(filter=five, **grp), UNSUPPORTED,
            "more than 4 string predicates")
    # beside a join
    fk = np.arange(7, dtype=np.int64)
    foreign = y.Chunk([y.encode_int64(fk), y.encode_int64(fk * 10)], 7)
    plan = y.Plan(filter=c(0) == b"a", keys=[c(3)], aggs=[y.agg_sum(c(NCOLS))],
                  join=y.Join(foreign, 3, 0, [1]))
    refused(cuda, plan, UNSUPPORTED, "not this round",
            join_foreign=foreign.c_device(cuda))
    # the bottom queries carry the same refusals
    states_t = cuda.zeros((64, 4), dtype=cuda.int64, device="cuda")
    with pytest.raises(RuntimeError, match="ytql error 1: .*type mismatch"):
        y.gpu_partial(y.Plan(filter=c(1) == b"x", keys=[c(3)], aggs=aggs),
                      dev_chunk(cuda, "dict_dense"), 2, states_t.data_ptr(), 64)
