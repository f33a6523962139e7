"""Expression semantics against an independent model (tests/expr_model.py).

The oracle (eval_expr), the host evaluator (heval) and the device interpreter
(eval_prog) are each held against the plain-Python model, not against one
another. Inputs are the cross product of per-type edge values as two columns
a, b of one type; every chunk is [k, a, b, g]: k the row number, g = k % 3.
Each chunk is encoded whole, in one-row segments (the smallest the encoder
makes: a column of many segments, found by binary search) and, for the scan
site, in two-row segments (uniform power-of-two segments: found by shift).

Comparison: integers and booleans must be equal, doubles equal in every bit,
and any two NaNs count as equal. NaN is kept out of the group-key, ORDER BY
and min/max sites, because the engine refuses NaN order keys, and -0.0 out of
min/max, where the engine's order map need not keep the sign of a zero that
equals another; rows whose modelled result is one of those are left out of
the chunk that site runs on. Sums and averages over doubles use dyadic values
whose every partial sum is exact, so the order of accumulation cannot matter.

Division by zero: a plan fails with YT_ERR_DIV_ZERO exactly when the model
meets a zero divisor on a row that passes the filter. Division is kept out of
AND / OR operands: whether those skip their right operand is not pinned here.
"""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import expr_model as M
import ytsaurus_amd as y
from expr_model import BOOL, DBL, I64, U64
from ytsaurus_amd import _abi, api

INT64_MIN, INT64_MAX = -2**63, 2**63 - 1

EDGES = {
    I64: [INT64_MIN, INT64_MIN + 1, -1, 0, 1, 2**31, 2**53 + 1, INT64_MAX, None],
    U64: [0, 1, 2**63 - 1, 2**63, 2**64 - 1, None],
    DBL: [-math.inf, -1.5, -0.0, 0.0, 5e-324, 5.0, 2.0**53, math.inf, math.nan,
          None],
    BOOL: [0, 1, None],
}
# sums and averages over doubles: every partial sum of 25 products, sums or
# differences of these is a multiple of 1/16 below 2**53, hence exact
DYADIC = [-1.5, 0.25, 5.0, 1048576.0, None]

A, B = ("col", 1), ("col", 2)
NULL = ("null",)
LITS = [("lit", 5), ("lit", -1), ("lit", 0), ("lit", 2**63 - 1), ("litf", 5.0)]

VT = {I64: _abi.VT_INT64, U64: _abi.VT_UINT64, DBL: _abi.VT_DOUBLE,
      BOOL: _abi.VT_BOOLEAN}
TV = {v: k for k, v in VT.items()}

OPS = {"+": "__add__", "-": "__sub__", "*": "__mul__", "//": "__floordiv__",
       "%": "__mod__", "==": "__eq__", "!=": "__ne__", "<": "__lt__",
       "<=": "__le__", ">": "__gt__", ">=": "__ge__", "and": "and_", "or": "or_"}


def to_api(e):
    k = e[0]
    if k == "col":
        return y.col(e[1])
    if k == "lit":
        return y.lit(e[1])
    if k == "litf":
        return y.litf(e[1])
    if k == "null":
        return y.null()
    if k == "not":
        return to_api(e[1]).not_()
    return getattr(to_api(e[1]), OPS[k])(to_api(e[2]))


# ---- data ----------------------------------------------------------------

def encode(t, vals, seg):
    nulls = np.array([v is None for v in vals], np.uint8)
    if t == DBL:
        return y.encode_double(np.array([0.0 if v is None else v for v in vals]),
                               nulls, max_segment_values=seg)
    ints = [0 if v is None else v for v in vals]
    if t == BOOL:
        return y.encode_bool(np.array(ints, np.uint8), nulls,
                             max_segment_values=seg)
    if t == U64:
        return y.encode_int64(np.array(ints, np.uint64).view(np.int64), nulls,
                              max_segment_values=seg, unsigned=True)
    return y.encode_int64(np.array(ints, np.int64), nulls, max_segment_values=seg)


class Data:
    """rows = the cross product of `edges` x `edges` (or the given subset of
    it) as columns a, b of type t beside k and g"""

    def __init__(self, t, edges=None, keep=None):
        self.t = t
        pairs = list(itertools.product(edges or EDGES[t], repeat=2))
        if keep is not None:
            pairs = [p for i, p in enumerate(pairs) if i in keep]
        self.n = len(pairs)
        self.col_types = [I64, t, t, I64]
        val = lambda v: None if v is None else (t, v)     # noqa: E731
        self.rows = [[(I64, i), val(a), val(b), (I64, i % 3)]
                     for i, (a, b) in enumerate(pairs)]
        self._pairs = pairs
        self._chunks = {}

    def chunk(self, seg):
        if seg not in self._chunks:
            n = self.n
            ks = list(range(n))
            self._chunks[seg] = y.Chunk(
                [encode(I64, ks, seg),
                 encode(self.t, [p[0] for p in self._pairs], seg),
                 encode(self.t, [p[1] for p in self._pairs], seg),
                 encode(I64, [k % 3 for k in ks], seg)], n)
        return self._chunks[seg]


_DATA = {}


def data(t, edges=None):
    key = (t, None if edges is None else tuple(map(repr, edges)))
    if key not in _DATA:
        _DATA[key] = Data(t, edges)
    return _DATA[key]


def data_without(d, bad_rows, edges=None):
    """d without the rows in bad_rows (k renumbered), cached"""
    if not bad_rows:
        return d
    keep = frozenset(range(d.n)) - frozenset(bad_rows)
    key = (d.t, None if edges is None else tuple(map(repr, edges)), keep)
    if key not in _DATA:
        _DATA[key] = Data(d.t, edges, keep)
    return _DATA[key]


# ---- the expression matrix -------------------------------------------------

def matrix(ops=M.ARITH + M.REL):
    """all ops in the forms col.col, col.lit, lit.col, col.null, null.col"""
    out = []
    for op in ops:
        out.append((op, A, B))
        for lit in LITS:
            out.append((op, A, lit))
            out.append((op, lit, A))
        out.append((op, A, NULL))
        out.append((op, NULL, A))
    return out


LOGIC = [("and", A, B), ("or", A, B), ("not", A), ("not", ("and", A, B)),
         ("or", ("not", A), B)]

NESTED_INT = [
    ("and", ("<", ("+", A, B), ("lit", 5)), (">=", A, ("lit", 0))),
    ("or", ("==", ("*", A, ("lit", 3)), B), ("not", ("<", B, NULL))),
    ("and", (">", ("-", A, ("lit", 1)), B), ("or", ("!=", B, ("lit", 0)), NULL)),
    ("<=", ("*", ("+", A, ("lit", 1)), ("-", B, ("lit", 1))), ("lit", 0)),
]
# doubling is exact, so each node rounds at most once whatever is fused
NESTED_DBL = [
    ("and", ("<", ("+", ("*", A, ("litf", 2.0)), ("litf", 1.0)), B),
     (">=", A, ("lit", 0))),
    ("or", (">", ("*", A, ("lit", 2)), ("+", B, B)), ("not", ("<", B, NULL))),
]


def expressions(t):
    ex = matrix()
    if t in (BOOL, I64):
        ex += LOGIC                   # Kleene tables; integers as truth values
    if t in (I64, U64):
        ex += NESTED_INT
    if t == DBL:
        ex += NESTED_DBL
    return ex


# integers that face the other column types, and what else must be refused
MIXED_TYPES = [I64, DBL, I64, U64, I64]          # [k, d, i, u, g]
D_, I_, U_ = ("col", 1), ("col", 2), ("col", 3)
MISMATCHES = [
    ("+", D_, I_), ("*", I_, D_), ("<", I_, U_), ("+", U_, I_), ("==", D_, U_),
    ("<", ("lit", -1), U_), ("+", ("litf", 1.0), I_), ("<", I_, ("litf", 5.0)),
    ("*", U_, ("litf", 2.0)), (">", ("+", D_, ("lit", 1)), I_),
    ("-", ("+", NULL, D_), I_),
]


def model_outcome(d, exprs, flt=None):
    """("ok", per-expression value lists) | ("div0", None) | (verdict, None)"""
    v = M.verdict(list(exprs) + ([flt] if flt is not None else []), d.col_types)
    if v != "ok":
        return v, None
    try:
        res = []
        for row in d.rows:
            if flt is not None and not M.passes(M.evaluate(flt, d.col_types, row)):
                res.append(None)
                continue
            res.append([M.evaluate(e, d.col_types, row) for e in exprs])
        return "ok", res
    except M.DivZero:
        return "div0", None


RC = {"type mismatch": _abi.YT_ERR_INVALID_PLAN,
      "unsupported": _abi.YT_ERR_UNSUPPORTED,
      "too deep": _abi.YT_ERR_UNSUPPORTED,
      "too long": _abi.YT_ERR_INVALID_PLAN,
      "div0": _abi.YT_ERR_DIV_ZERO}


# ---- running plans ---------------------------------------------------------

_DT = np.dtype([("id", "<u2"), ("type", "u1"), ("flags", "u1"),
                ("length", "<u4"), ("bits", "<u8")])


def decode(rs):
    n, nc = rs.row_count, rs.column_count
    if n == 0:
        return []
    buf = np.ctypeslib.as_array(
        C.cast(rs.values, C.POINTER(C.c_uint8)), shape=(n * nc * 16,))
    arr = buf.view(_DT).reshape(n, nc)
    types, bits = arr["type"].tolist(), arr["bits"].tolist()
    dbls = arr["bits"].view(np.float64).tolist()
    rows = []
    for r in range(n):
        row = []
        for c in range(nc):
            t = types[r][c]
            if t == _abi.VT_NULL:
                row.append(None)
            elif t == _abi.VT_DOUBLE:
                row.append((DBL, dbls[r][c]))
            elif t == _abi.VT_INT64:
                b = bits[r][c]
                row.append((I64, b - 2**64 if b >> 63 else b))
            else:
                row.append((TV[t], bits[r][c]))
        rows.append(row)
    return rows


def run_oracle(plan, chunk):
    keep = api._attach_join(plan, lambda c: c.c_host())
    ch = chunk.c_host()
    rs = api.make_rowset(512, 8)
    st = api.YtStatistics()
    err = C.create_string_buffer(256)
    rc = _abi.oracle_lib().yto_execute(C.byref(plan.c), C.byref(ch), C.byref(rs),
                                       C.byref(st), 1, err, 256)
    del keep
    return rc, err.value.decode(), decode(rs) if rc == 0 else None


class Gpu:
    """the GPU entry over device copies of the chunks it is given"""

    def __init__(self, torch):
        self.torch = torch
        self._dev = {}

    def dev(self, chunk):
        if id(chunk) not in self._dev:
            self._dev[id(chunk)] = (chunk, chunk.c_device(self.torch))
        return self._dev[id(chunk)][1]

    def __call__(self, plan, chunk, join_foreign=None):
        keep = api._attach_join_dev(plan, join_foreign)
        opts = api.YtExecOptions(max_groups_hint=1024)
        rs = api.make_rowset(512, 8, pool_bytes=4096)
        st = api.YtStatistics()
        err = C.create_string_buffer(512)
        dch = self.dev(chunk)
        rc = _abi.gpu_lib().yt_gpu_query_execute(
            C.byref(plan.c), C.byref(dch), C.byref(opts), C.byref(rs),
            C.byref(st), err, 512)
        del keep
        return rc, err.value.decode(), decode(rs) if rc == 0 else None


def pool_blocks():
    return int(_abi.gpu_lib().yt_gpu_debug_pool_blocks_in_use())


def assert_same_rows(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for g, w in zip(got, want):
        assert len(g) == len(w), (what, g, w)
        for x, z in zip(g, w):
            assert M.same(x, z), (what, g, w)


def by_k(rows):
    return sorted(rows, key=lambda r: r[0][1])


def describe(e):
    return repr(e)


# ---- sites -----------------------------------------------------------------
# Each takes run (run_oracle or a Gpu), the data, a chunk of it, and checks one
# plan against the model: the refusal, the division by zero, or the rows.

def expect_refusal(rc, msg, outcome, what):
    assert rc == RC[outcome], (what, outcome, rc, msg)
    if outcome == "type mismatch":
        assert "type mismatch" in msg, (what, msg)
    if outcome == "too deep":
        assert str(M.STACK_SLOTS) in msg, (what, msg)


def site_scan(run, d, chunk, exprs, flt=None):
    """filter + projections [k, exprs...] of a plain scan"""
    what = ("scan", d.t, flt, exprs)
    outcome, res = model_outcome(d, exprs, flt)
    plan = y.Plan(filter=None if flt is None else to_api(flt),
                  projects=[y.col(0)] + [to_api(e) for e in exprs])
    rc, msg, rows = run(plan, chunk)
    if outcome != "ok":
        expect_refusal(rc, msg, outcome, what)
        return outcome
    assert rc == 0, (what, rc, msg)
    want = [[d.rows[i][0]] + vals for i, vals in enumerate(res) if vals is not None]
    assert_same_rows(rows, want, what)          # input row order
    return outcome


def site_filter(run, d, chunk, e):
    return site_scan(run, d, chunk, [], flt=e)


def site_having(run, d, chunk, e):
    """HAVING over the group rows [k, first(a), first(b)]: one row each"""
    what = ("having", d.t, e)
    outcome, res = model_outcome(d, [], flt=e)
    plan = y.Plan(keys=[y.col(0)],
                  aggs=[y.agg_first(y.col(1)), y.agg_first(y.col(2))],
                  having=to_api(e))
    rc, msg, rows = run(plan, chunk)
    if outcome != "ok":
        expect_refusal(rc, msg, outcome, what)
        return outcome
    assert rc == 0, (what, rc, msg)
    want = [d.rows[i][:3] for i, vals in enumerate(res) if vals is not None]
    assert_same_rows(by_k(rows), want, what)
    return outcome


def nonzero_divisor_filter(e):
    """for a division by a column: the filter that keeps its divisor non-zero
    (null divisors pass: null != 0 is true, and the quotient is null)"""
    if e[0] in ("//", "%") and e[2][0] == "col":
        return ("!=", e[2], ("lit", 0))
    return None


# ---- check 1: the oracle against the model (no GPU) ------------------------

@pytest.mark.parametrize("seg", [0, 1])
@pytest.mark.parametrize("t", [I64, U64, DBL, BOOL])
def test_oracle_matrix(t, seg):
    d = data(t)
    chunk = d.chunk(seg)
    seen = set()
    pack = []
    for e in expressions(t):
        outcome = site_filter(run_oracle, d, chunk, e)
        seen.add(outcome)
        assert site_having(run_oracle, d, chunk, e) == outcome
        if outcome == "ok" and model_outcome(d, [e])[0] == "ok":
            pack.append(e)
        else:
            # alone: its refusal, or its division by zero ...
            seen.add(site_scan(run_oracle, d, chunk, [e]))
            # ... and the rows once the filter keeps the divisor non-zero
            flt = nonzero_divisor_filter(e)
            if flt is not None and M.verdict([e], d.col_types) == "ok":
                assert site_scan(run_oracle, d, chunk, [e], flt) == "ok"
        if len(pack) == 7:
            site_scan(run_oracle, d, chunk, pack)
            pack = []
    if pack:
        site_scan(run_oracle, d, chunk, pack)
    # the matrix meets every outcome it is meant to
    assert "ok" in seen
    if t != DBL:
        assert {"div0", "type mismatch"} <= seen
    else:
        assert "unsupported" in seen


def test_oracle_issue_table():
    """the rows of the table that opened this work"""
    dv = [-1.5, 0.0, 3.0, 7.5, 100.0]
    ch = y.Chunk([y.encode_double(np.array(dv)),
                  y.encode_int64(np.arange(1, 6, dtype=np.int64))], 5)
    run = lambda **kw: run_oracle(y.Plan(**kw), ch)       # noqa: E731
    rc, _, rows = run(filter=y.col(0) > 5, projects=[y.col(0)])
    assert rc == 0 and rows == [[(DBL, 7.5)], [(DBL, 100.0)]]
    for proj in (y.lit(2) * y.col(0), y.col(0) * 2):
        rc, _, rows = run(projects=[proj])
        assert rc == 0 and rows == [[(DBL, 2 * v)] for v in dv]
    for kw in (dict(projects=[y.col(0) + y.col(1)]),
               dict(aggs=[y.agg_sum(y.col(1) * y.col(0))])):
        rc, msg, _ = run(**kw)
        assert rc == _abi.YT_ERR_INVALID_PLAN and "type mismatch" in msg
    rc, _, rows = run(keys=[y.col(1)], aggs=[y.agg_avg(y.col(0))],
                      having=y.col(1) > 5)
    assert rc == 0 and by_k(rows) == [[(I64, 4), (DBL, 7.5)], [(I64, 5), (DBL, 100.0)]]
    u = np.array([1, 2**63 + 5], np.uint64)
    chu = y.Chunk([y.encode_int64(u.view(np.int64), unsigned=True)], 2)
    for flt in (y.lit(3) < y.col(0), y.col(0) > 3):
        rc, _, rows = run_oracle(y.Plan(filter=flt, projects=[y.col(0)]), chu)
        assert rc == 0 and rows == [[(U64, 2**63 + 5)]]


def mixed_chunk(with_string=False):
    key = ("mixed", with_string)
    if key not in _DATA:
        n = 12
        cols = [encode(I64, list(range(n)), 0),
                encode(DBL, [float(i) - 3.5 for i in range(n)], 0),
                encode(I64, [i - 4 for i in range(n)], 0),
                encode(U64, [i + 2**63 for i in range(n)], 0),
                encode(I64, [i % 3 for i in range(n)], 0)]
        if with_string:
            cols.append(y.encode_string(["s%d" % (i % 3) for i in range(n)]))
        _DATA[key] = y.Chunk(cols, n)
    return _DATA[key]


def refusal_plans(e, string_key=False):
    """the mismatching expression at every site an expression can stand at"""
    x = to_api(e)
    key = y.col(5) if string_key else y.col(4)
    plans = {
        "filter": dict(filter=x, projects=[y.col(0)]),
        "projection": dict(projects=[y.col(0), x]),
        "order by": dict(projects=[x, y.col(0)], order_by=[(0, False)], limit=5),
        "grouped filter": dict(filter=x, keys=[key], aggs=[y.agg_sum1()]),
        "having": dict(keys=[y.col(0)],
                       aggs=[y.agg_first(y.col(1)), y.agg_first(y.col(2)),
                             y.agg_first(y.col(3))],
                       having=x),
    }
    if not string_key:
        plans["key"] = dict(keys=[x], aggs=[y.agg_sum1()])
    if e[0] in M.ARITH:
        for name, f in (("sum", y.agg_sum), ("min", y.agg_min),
                        ("max", y.agg_max), ("avg", y.agg_avg)):
            plans[name] = dict(keys=[key], aggs=[f(x)])
    return plans


@pytest.mark.parametrize("e", MISMATCHES, ids=describe)
def test_oracle_refuses_mismatch(e):
    assert M.verdict([e], MIXED_TYPES) == "type mismatch"
    for site, kw in refusal_plans(e).items():
        rc, msg, _ = run_oracle(y.Plan(**kw), mixed_chunk())
        assert rc == _abi.YT_ERR_INVALID_PLAN and "type mismatch" in msg, (site, rc, msg)


# ---- check 2: the GPU against the model, one family per site ---------------

@pytest.fixture(scope="module")
def gpu(cuda):
    return Gpu(cuda)


def site_list(t):
    """a list short enough to run one plan per expression at every site:
    every op in the forms col.col, col.lit, lit.col, col.null"""
    lit = ("litf", 5.0) if t == DBL else ("lit", 5)
    big = ("lit", 2**63 - 1)
    out = []
    for op in M.ARITH + M.REL:
        out += [(op, A, B), (op, A, lit), (op, big, A), (op, A, NULL)]
    return [e for e in out if M.verdict([e], data(t).col_types) == "ok"]


@pytest.mark.gpu
@pytest.mark.parametrize("seg", [0, 1, 2])
@pytest.mark.parametrize("t", [I64, U64, DBL, BOOL])
def test_gpu_scan(gpu, t, seg):
    """filter and projection of a plain scan: the whole matrix"""
    d = data(t)
    chunk = d.chunk(seg)
    pack = []
    for e in expressions(t):
        outcome = site_filter(gpu, d, chunk, e)
        if outcome == "ok" and model_outcome(d, [e])[0] == "ok":
            pack.append(e)
        else:
            site_scan(gpu, d, chunk, [e])
            flt = nonzero_divisor_filter(e)
            if flt is not None and M.verdict([e], d.col_types) == "ok":
                assert site_scan(gpu, d, chunk, [e], flt) == "ok"
        if len(pack) == 7:
            site_scan(gpu, d, chunk, pack)
            pack = []
    if pack:
        site_scan(gpu, d, chunk, pack)
    assert _abi.gpu_lib().yt_gpu_debug_last_scan_path() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("seg", [0, 1])
@pytest.mark.parametrize("t", [I64, U64, DBL, BOOL])
def test_gpu_having(gpu, t, seg):
    """HAVING: the host evaluator over group rows. The rows come from
    first(), which copies; NaN and -0.0 stay in."""
    d = data(t)
    chunk = d.chunk(seg)
    for e in site_list(t) + (LOGIC if t in (BOOL, I64) else []):
        site_having(gpu, d, chunk, e)


def is_nan(v):
    return v is not None and v[0] == DBL and math.isnan(v[1])


def is_neg_zero(v):
    return v is not None and v[0] == DBL and v[1] == 0.0 and math.copysign(1, v[1]) < 0


def usable(d, e, flt, bad, edges=None):
    """(outcome, data, per-row value or None when filtered) with the rows
    whose value `bad` rejects taken out of the data"""
    outcome, res = model_outcome(d, [e], flt)
    if outcome != "ok":
        return outcome, d, None
    drop = [i for i, v in enumerate(res) if v is not None and bad(v[0])]
    d2 = data_without(d, drop, edges)
    outcome, res = model_outcome(d2, [e], flt)
    return outcome, d2, [None if v is None else v[0] for v in res]


def key_of(v):
    return None if v is None else (v[0], M.bits_of(v))


@pytest.mark.gpu
@pytest.mark.parametrize("seg", [0, 1])
@pytest.mark.parametrize("t", [I64, U64, DBL, BOOL])
def test_gpu_group_key(gpu, t, seg):
    """one expression as the group key; groups are told apart by bits. Rows
    whose key is NaN are left out: the engine refuses NaN order keys."""
    d0 = data(t)
    for e in site_list(t):
        flt = nonzero_divisor_filter(e)
        outcome, d, vals = usable(d0, e, flt, is_nan)
        assert outcome == "ok", e
        want = {}
        for i, v in enumerate(vals):
            if flt is None or M.passes(M.evaluate(flt, d.col_types, d.rows[i])):
                want[key_of(v)] = want.get(key_of(v), 0) + 1
        plan = y.Plan(filter=None if flt is None else to_api(flt),
                      keys=[to_api(e)], aggs=[y.agg_sum1()])
        rc, msg, rows = gpu(plan, d.chunk(seg))
        assert rc == 0, (e, rc, msg)
        got = {key_of(r[0]): r[1] for r in rows}
        assert len(got) == len(rows), e
        assert got == {k: (I64, c) for k, c in want.items()}, e
        st = M.static_type(e, d.col_types)
        assert all(r[0] is None or r[0][0] == st for r in rows), (e, st)


def order_key(v):
    """the comparer of ORDER BY: null first, then by value in the type's order"""
    if v is None:
        return (0, 0)
    return (1, v[1])


@pytest.mark.gpu
@pytest.mark.parametrize("seg", [0, 1])
@pytest.mark.parametrize("t", [I64, U64, DBL, BOOL])
def test_gpu_order_by(gpu, t, seg):
    """the ORDER BY expression of scan + ORDER BY ... LIMIT; rows whose key
    is NaN are left out (a NaN order key is an error)"""
    d0 = data(t)
    for n, e in enumerate(site_list(t)):
        flt = nonzero_divisor_filter(e)
        outcome, d, vals = usable(d0, e, flt, is_nan)
        assert outcome == "ok", e
        live = [(v, d.rows[i][0]) for i, v in enumerate(vals)
                if flt is None or M.passes(M.evaluate(flt, d.col_types, d.rows[i]))]
        desc = bool(n % 2)
        limit = len(live) if n % 3 else 7
        want = sorted((order_key(v) for v, _ in live), reverse=desc)[:limit]
        plan = y.Plan(filter=None if flt is None else to_api(flt),
                      projects=[to_api(e), y.col(0)],
                      order_by=[(0, desc)], limit=limit)
        rc, msg, rows = gpu(plan, d.chunk(seg))
        assert rc == 0, (e, rc, msg)
        assert [order_key(r[0]) for r in rows] == want, (e, desc, limit)
        # each row still carries its own value
        by = {k[1]: v for v, k in live}
        for r in rows:
            assert M.same(r[0], by[r[1][1]]), (e, r)


def agg_model(func, t, vals):
    """vals: the argument's values over one group's rows"""
    nn = [v for v in vals if v is not None]
    if not nn:
        return None
    if func in ("min", "max"):
        pick = min if func == "min" else max
        return pick(nn, key=lambda v: v[1])
    if t == DBL:
        s = (DBL, math.fsum(v[1] for v in nn))      # exact by construction
    else:
        s = M._from_bits(t, sum(M.bits_of(v) for v in nn))
    if func == "sum":
        return s
    return (DBL, float(s[1]) / float(len(nn)))      # double(sum) / count


def check_aggregates(gpu, d, chunk, e, flt, key_col, vals, path=None):
    t = M.static_type(e, d.col_types)
    funcs = [("min", y.agg_min), ("max", y.agg_max)]
    if t != BOOL:
        funcs = [("sum", y.agg_sum)] + funcs + [("avg", y.agg_avg)]
    x = to_api(e)
    plan = y.Plan(filter=None if flt is None else to_api(flt),
                  keys=[y.col(key_col)], aggs=[f(x) for _, f in funcs])
    rc, msg, rows = gpu(plan, chunk)
    assert rc == 0, (e, rc, msg)
    if path is not None:
        assert _abi.gpu_lib().yt_gpu_debug_last_scan_path() == path
    groups = {}
    for i, v in enumerate(vals):
        if flt is None or M.passes(M.evaluate(flt, d.col_types, d.rows[i])):
            groups.setdefault(i % 3, []).append(v)
    assert len(rows) == len(groups), (e, rows)
    for r in rows:
        g = r[0][1] if path is None else int(r[0][1])
        for (name, _), got in zip(funcs, r[1:]):
            want = agg_model(name, t, groups[g])
            assert M.same(got, want), (e, name, g, got, want)
            # the state and output type follow the static type
            if got is not None:
                assert got[0] == (DBL if name == "avg" else t), (e, name, got)


def agg_cases(t):
    """(data, edges) and the argument expressions of the aggregate sites"""
    lit = ("litf", 5.0) if t == DBL else ("lit", 5)
    ops = ("+", "-", "*") if t == DBL else M.ARITH
    edges = DYADIC if t == DBL else None
    out = []
    for op in ops:
        out += [(op, A, B), (op, A, lit), (op, lit, A), (op, NULL, A)]
    d = data(t, edges)
    return d, edges, [e for e in out if M.verdict([e], d.col_types) == "ok"]


@pytest.mark.gpu
@pytest.mark.parametrize("seg", [0, 1])
@pytest.mark.parametrize("t", [I64, U64, DBL, BOOL])
def test_gpu_aggregate_argument(gpu, t, seg):
    """sum, min, max and avg of one expression, grouped by g = k % 3. Rows
    whose argument is NaN or -0.0 are left out (min / max: the engine refuses
    NaN order keys and need not keep a zero's sign); double sums run over
    DYADIC, where every partial sum is exact."""
    d0, edges, exprs = agg_cases(t)
    for e in exprs:
        flt = nonzero_divisor_filter(e)
        outcome, d, vals = usable(d0, e, flt, lambda v: is_nan(v) or is_neg_zero(v),
                                  edges)
        assert outcome == "ok", e
        check_aggregates(gpu, d, d.chunk(seg), e, flt, 3, vals)


def string_chunk(d, seg):
    key = ("str", id(d), seg)
    if key not in _DATA:
        base = d.chunk(seg)
        s = y.encode_string(["%d" % (k % 3) for k in range(d.n)],
                            max_segment_values=seg)
        _DATA[key] = y.Chunk(list(base.columns) + [s], d.n)
    return _DATA[key]


class StrKey:
    """a Gpu whose rows come back with the string key "0".."2" as a number"""

    def __init__(self, gpu):
        self.gpu = gpu

    def __call__(self, plan, chunk):
        rc, msg, rs = run_gpu_raw(self.gpu, plan, chunk)
        if rc:
            return rc, msg, None
        keys = [r[0] for r in api.rows_from_rowset(rs)]
        rows = decode_skip_strings(rs)
        for r, k in zip(rows, keys):
            r[0] = (I64, int(k))
        return rc, msg, rows


def run_gpu_raw(gpu, plan, chunk):
    opts = api.YtExecOptions(max_groups_hint=1024)
    rs = api.make_rowset(512, 8, pool_bytes=4096)
    st = api.YtStatistics()
    err = C.create_string_buffer(512)
    dch = gpu.dev(chunk)
    plan.c.join = None
    rc = _abi.gpu_lib().yt_gpu_query_execute(
        C.byref(plan.c), C.byref(dch), C.byref(opts), C.byref(rs),
        C.byref(st), err, 512)
    return rc, err.value.decode(), rs


def decode_skip_strings(rs):
    """decode() with the STRING values (column 0) left as None"""
    n, nc = rs.row_count, rs.column_count
    for r in range(n):
        v = rs.values[r * nc]
        if v.type == _abi.VT_STRING:
            v.type = _abi.VT_NULL
    return decode(rs)


@pytest.mark.gpu
@pytest.mark.parametrize("t", [I64, U64, DBL])
def test_gpu_string_group_general(gpu, t):
    """filter and aggregate argument of a string-key GROUP BY: the general
    kernels (YT_SCAN_PATH_STR_GENERAL)"""
    d0, edges, exprs = agg_cases(t)
    rel = [(op, A, B) for op in M.REL] + [("<", ("lit", 0), A), (">=", A, NULL)]
    for n, e in enumerate(exprs):
        flt = nonzero_divisor_filter(e) or rel[n % len(rel)]
        outcome, d, vals = usable(d0, e, flt, lambda v: is_nan(v) or is_neg_zero(v),
                                  edges)
        assert outcome == "ok", e
        check_aggregates(StrKey(gpu), d, string_chunk(d, n % 2), e, flt, 4, vals,
                         path=_abi.SCAN_PATH_STR_GENERAL)


@pytest.mark.gpu
@pytest.mark.parametrize("is_left", [False, True])
def test_gpu_join_foreign_columns(gpu, is_left):
    """expressions over a foreign DOUBLE and a foreign UINT64 column"""
    n = 40
    prim = y.Chunk([encode(I64, [None if k == 7 else k for k in range(n)], 0)], n)
    fk = list(range(0, n, 2)) + [None]                  # odd keys find no row
    dv = [EDGES[DBL][i % len(EDGES[DBL])] for i in range(len(fk))]
    uv = [EDGES[U64][i % len(EDGES[U64])] for i in range(len(fk))]
    foreign = y.Chunk([encode(I64, fk, 0), encode(DBL, dv, 0), encode(U64, uv, 0)],
                      len(fk))
    types = [I64, DBL, U64]
    look = {k: i for i, k in enumerate(fk)}
    rows = []
    for k in range(n):
        kk = None if k == 7 else k
        i = look.get(kk)
        if i is None:
            if not is_left:
                continue
            rows.append([(I64, kk), None, None])
            continue
        rows.append([None if kk is None else (I64, kk),
                     None if dv[i] is None else (DBL, dv[i]),
                     None if uv[i] is None else (U64, uv[i])])
    Dc, Uc = ("col", 1), ("col", 2)
    exprs = [("*", ("lit", 2), Dc), ("+", Dc, ("lit", 5)), (">", Dc, ("lit", 5)),
             ("-", Uc, ("lit", 1)), ("<", ("lit", 3), Uc), ("//", ("lit", 2**63 - 1), Uc),
             ("+", NULL, Dc)]
    flt = ("!=", Uc, ("lit", 0))         # the divisor of the sixth projection
    assert M.verdict(exprs + [flt], types) == "ok"
    want = []
    for row in rows:
        if M.passes(M.evaluate(flt, types, row)):
            want.append([row[0]] + [M.evaluate(e, types, row) for e in exprs])
    join = y.Join(foreign, 0, 0, [1, 2], is_left=is_left)
    plan = y.Plan(filter=to_api(flt),
                  projects=[y.col(0)] + [to_api(e) for e in exprs], join=join)
    rc, msg, got = gpu(plan, prim, join_foreign=gpu.dev(foreign))
    assert rc == 0, (rc, msg)
    assert_same_rows(got, want, "join")
    # static result types: 2 * d and null + d are DOUBLE, u - 1 is UINT64
    for r in got:
        for v, t in zip(r[1:], [DBL, DBL, BOOL, U64, BOOL, U64, DBL]):
            assert v is None or v[0] == t
    base = pool_blocks()
    for e in [("+", Dc, Uc), ("<", Uc, ("lit", -1)), ("==", Dc, ("col", 0))]:
        assert M.verdict([e], types) == "type mismatch"
        plan = y.Plan(projects=[y.col(0), to_api(e)], join=join)
        rc, msg, _ = gpu(plan, prim, join_foreign=gpu.dev(foreign))
        assert rc == _abi.YT_ERR_INVALID_PLAN and "type mismatch" in msg, (e, rc, msg)
        assert pool_blocks() == base


# ---- check 5: refusals -----------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("e", MISMATCHES, ids=describe)
def test_gpu_refuses_mismatch(gpu, e):
    """every site, integer and string group key; nothing stays taken"""
    base = pool_blocks()
    for string_key in (False, True):
        chunk = mixed_chunk(with_string=string_key)
        for site, kw in refusal_plans(e, string_key).items():
            rc, msg, _ = gpu(y.Plan(**kw), chunk)
            assert rc == _abi.YT_ERR_INVALID_PLAN and "type mismatch" in msg, \
                (site, string_key, rc, msg)
            assert pool_blocks() == base, (site, string_key)


# ---- check 6: depth and length ---------------------------------------------

def right_nested(op, leaves):
    e = A
    for _ in range(leaves - 1):
        e = (op, A, e)
    return e


def left_deep(op, leaves):
    e = A
    for _ in range(leaves - 1):
        e = (op, e, A)
    return e


def test_model_depth_and_length():
    assert M.stack_need(right_nested("+", 12)) == 12
    assert M.stack_need(right_nested("+", 13)) == 13
    assert M.program_len(right_nested("+", 13)) == 25
    assert M.stack_need(left_deep("+", 25)) == 2
    assert M.program_len(left_deep("+", 24)) == 47
    assert M.verdict([right_nested("+", 13)], [I64, I64]) == "too deep"
    assert M.verdict([left_deep("+", 24)], [I64, I64]) == "ok"
    assert M.verdict([left_deep("+", 25)], [I64, I64]) == "too long"


@pytest.mark.gpu
def test_gpu_depth_and_length(gpu):
    """12 slots evaluate, 13 are refused before any kernel; 47 instructions
    evaluate, 49 are refused"""
    d = data(I64)
    chunk = d.chunk(0)
    base = pool_blocks()

    def scan(flt, proj):
        plan = y.Plan(filter=None if flt is None else to_api(flt),
                      projects=[to_api(proj)])
        return gpu(plan, chunk)

    def want(flt, proj):
        return [[M.evaluate(proj, d.col_types, r)] for r in d.rows
                if flt is None or M.passes(M.evaluate(flt, d.col_types, r))]

    deep12 = right_nested("+", 12)
    assert M.verdict([deep12], d.col_types) == "ok"
    rc, msg, rows = scan(None, deep12)
    assert rc == 0, (rc, msg)
    assert_same_rows(rows, want(None, deep12), "12 slots, projection")
    flt12 = (">", right_nested("+", 12), ("lit", 0))
    assert M.stack_need(flt12) == 12
    rc, msg, rows = scan(flt12, A)
    assert rc == 0, (rc, msg)
    assert_same_rows(rows, want(flt12, A), "12 slots, filter")
    and12 = right_nested("and", 12)               # the filter's own AND chain
    rc, msg, rows = scan(and12, A)
    assert rc == 0, (rc, msg)
    assert_same_rows(rows, want(and12, A), "12 slots, AND chain")

    for flt, proj in ((None, right_nested("+", 13)),
                      ((">", right_nested("+", 13), ("lit", 0)), A),
                      (right_nested("and", 13), A),
                      (right_nested("or", 13), A)):
        assert M.verdict([proj] + ([flt] if flt else []), d.col_types) == "too deep"
        rc, msg, _ = scan(flt, proj)
        expect_refusal(rc, msg, "too deep", (flt, proj))
        assert pool_blocks() == base
    for kw in (dict(keys=[to_api(right_nested("+", 13))], aggs=[y.agg_sum1()]),
               dict(keys=[y.col(3)], aggs=[y.agg_sum(to_api(right_nested("*", 13)))])):
        rc, msg, _ = gpu(y.Plan(**kw), chunk)
        expect_refusal(rc, msg, "too deep", kw)
        assert pool_blocks() == base

    long24 = left_deep("+", 24)
    assert M.verdict([long24], d.col_types) == "ok"
    rc, msg, rows = scan(None, long24)
    assert rc == 0, (rc, msg)
    assert_same_rows(rows, want(None, long24), "47 instructions")
    long25 = left_deep("+", 25)
    assert M.verdict([long25], d.col_types) == "too long"
    rc, msg, _ = scan(None, long25)
    expect_refusal(rc, msg, "too long", long25)
    assert "too long" in msg
    assert pool_blocks() == base


def test_oracle_types_before_rows():
    """typing is judged before any row is read: a plan that is mistyped and
    would divide by zero is a type mismatch"""
    e = ("+", ("//", I_, ("lit", 0)), D_)
    rc, msg, _ = run_oracle(y.Plan(projects=[to_api(e)]), mixed_chunk())
    assert rc == _abi.YT_ERR_INVALID_PLAN and "type mismatch" in msg
