"""IN lists on the CPU: the lookup tables a query builds (inlist.h), driven
through yt_inlist_eval_i64 / yt_inlist_eval_str — the host build of the probes
the GPU runs, over a table built exactly as the product builds it — against
Python set membership. No GPU.

Contract under test (include/ytql_gpu.h): the answer is true iff the operand
equals a listed value; a null operand matches a null in the list; duplicates
mean nothing; the empty list is false; strings compare on length and bytes."""
import ctypes as C

import numpy as np
import pytest

import ytsaurus_amd as y
from ytsaurus_amd import _abi

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SIZES = [0, 1, 2, 63, 64, 65, 1000, 100_000]


def eval_i64(lst, has_null, values, nulls):
    """lst, values: numpy int64 or uint64 arrays (raw 64-bit patterns)"""
    lst = np.ascontiguousarray(lst).view(np.uint64)
    values = np.ascontiguousarray(values).view(np.uint64)
    nulls = np.ascontiguousarray(nulls, dtype=np.uint8)
    out = np.full(len(values), 7, dtype=np.uint8)
    rc = _abi.gpu_lib().yt_inlist_eval_i64(
        lst.ctypes.data, len(lst), int(has_null), values.ctypes.data,
        nulls.ctypes.data, len(values), out.ctypes.data)
    assert rc == _abi.YT_OK
    return out


def pack(strings):
    """list of bytes-or-None -> (bytes, ends int64 array, nulls uint8 array)"""
    ends = np.cumsum([0 if s is None else len(s) for s in strings],
                     dtype=np.int64)
    nulls = np.array([s is None for s in strings], dtype=np.uint8)
    return b"".join(s for s in strings if s is not None), ends, nulls


def eval_str(lst, texts):
    lb, le, ln = pack(lst)
    tb, te, tn = pack(texts)
    out = np.full(len(texts), 7, dtype=np.uint8)
    rc = _abi.gpu_lib().yt_inlist_eval_str(
        lb, le.ctypes.data, ln.ctypes.data, len(lst),
        tb, te.ctypes.data, tn.ctypes.data, len(texts), out.ctypes.data)
    assert rc == _abi.YT_OK
    return out


EXTREME_I64 = np.array([0, -1, I64_MIN, I64_MAX, 1, I64_MIN + 1, I64_MAX - 1],
                       dtype=np.int64)
EXTREME_U64 = np.array([0, 1, (1 << 63), (1 << 63) + 1, (1 << 64) - 1,
                        (1 << 63) - 1, 0x8000000000000001], dtype=np.uint64)


def num_list(rng, size, dtype):
    """`size` values with duplicates; the extremes first when there is room"""
    if size == 0:
        return np.zeros(0, dtype=dtype)
    if dtype == np.int64:
        body = rng.integers(-5000, 5000, size, dtype=np.int64) * 7919
        ext = EXTREME_I64
    else:
        body = rng.integers(0, 1 << 63, size, dtype=np.uint64) * np.uint64(2) \
            + np.uint64(1)
        ext = EXTREME_U64
    if size >= 63:
        body[:len(ext)] = ext
        body[len(ext):len(ext) + 5] = body[20:25]         # duplicates
    return body


@pytest.mark.parametrize("dtype", [np.int64, np.uint64], ids=["int64", "uint64"])
@pytest.mark.parametrize("size", SIZES)
def test_numeric_lists_against_a_python_set(size, dtype):
    rng = np.random.default_rng(1000 + size)
    lst = num_list(rng, size, dtype)
    ext = EXTREME_I64 if dtype == np.int64 else EXTREME_U64
    # operands: every list value (hits), the extremes, near misses, randoms
    miss = (lst[:2000].astype(dtype) + dtype(1)) if size else lst
    rnd = rng.integers(-5000, 5000, 3000).astype(np.int64).view(np.uint64) \
        .astype(np.uint64).view(dtype)
    values = np.concatenate([lst[:5000], ext, miss, rnd]).astype(dtype)
    nulls = (rng.random(len(values)) < 0.05).astype(np.uint8)
    members = set(lst.view(np.uint64).tolist())
    for has_null in (False, True):
        got = eval_i64(lst, has_null, values, nulls)
        want = np.array([has_null if nl else (v in members)
                         for v, nl in zip(values.view(np.uint64).tolist(),
                                          nulls)], dtype=np.uint8)
        assert np.array_equal(got, want), (size, has_null)
        if size:
            assert want.sum() > 0 and (want == 0).sum() > 0


def test_numeric_empty_marker_is_never_a_member():
    """whatever value the builder takes for 'empty', a probe for it answers
    by the list: a list that holds the obvious candidates still works"""
    lst = np.array([0x8000000000000000 + i for i in range(300)] + [0, 2**64 - 1],
                   dtype=np.uint64)
    values = np.array([0x8000000000000000 + i for i in range(298, 310)] +
                      [0, 1, 2**64 - 1, 2**64 - 2], dtype=np.uint64)
    got = eval_i64(lst, False, values, np.zeros(len(values), dtype=np.uint8))
    members = set(lst.tolist())
    assert got.tolist() == [int(v in members) for v in values.tolist()]


def test_numeric_list_over_the_cap():
    lst = np.arange((1 << 20) + 1, dtype=np.int64)
    out = np.zeros(1, dtype=np.uint8)
    one = np.zeros(1, dtype=np.uint64)
    rc = _abi.gpu_lib().yt_inlist_eval_i64(
        lst.ctypes.data, len(lst), 0, one.ctypes.data, None, 1, out.ctypes.data)
    assert rc == _abi.YT_ERR_UNSUPPORTED
    # duplicates do not count: the same values twice are exactly at the cap
    lst = np.concatenate([np.arange(1 << 20, dtype=np.int64)] * 2)
    rc = _abi.gpu_lib().yt_inlist_eval_i64(
        lst.ctypes.data, len(lst), 0, one.ctypes.data, None, 1, out.ctypes.data)
    assert rc == _abi.YT_OK and out[0] == 1


FIXED_STRINGS = [b"", b"a", b"ab", b"abc", b"abd", b"xyzw-long-tail-A",
                 b"xyzw-long-tail-B", b"\x00", b"\x00\x00", b"a\x00b",
                 b"\xff\xfe"]


def str_list(rng, size):
    out = [b"k%07d-%d" % (int(v), int(v) % 3)
           for v in rng.integers(0, 10 * size + 10, size)]
    if size >= 63:
        out[:len(FIXED_STRINGS)] = FIXED_STRINGS
        out[30:33] = out[40:43]                           # duplicates
    return out


@pytest.mark.parametrize("size", SIZES)
def test_string_lists_against_a_python_set(size):
    rng = np.random.default_rng(2000 + size)
    lst = str_list(rng, size)
    # texts: list values, the fixed strings, last-byte and length neighbours
    near = [s[:-1] + bytes([s[-1] ^ 1]) for s in lst[:1500] if s] + \
           [s + b"x" for s in lst[:500]] + [s[:-1] for s in lst[:500] if s]
    texts = lst[:4000] + FIXED_STRINGS + near + \
        [b"k%07d-0" % int(v) for v in rng.integers(0, 10 * size + 10, 1500)]
    texts = [None if rng.random() < 0.05 else t for t in texts]
    for with_null in (False, True):
        full = lst + ([None, None] if with_null else [])
        order = rng.permutation(len(full))
        full = [full[i] for i in order]
        members = set(lst)
        got = eval_str(full, texts)
        want = [int(with_null) if t is None else int(t in members) for t in texts]
        assert got.tolist() == want, (size, with_null)
        if size:
            assert sum(want) > 0 and want.count(0) > 0


def test_string_probe_chains():
    """3000 strings in 8192 slots: chains form. The test finds them by the
    product's own hash so that it proves the chains exist — splitmix64 over
    FNV-1a, restated here — and then checks members and near misses."""
    rng = np.random.default_rng(31)
    lst = [b"chain-%05d" % i for i in rng.permutation(40_000)[:3000]]

    def h(b):
        x = 0xCBF29CE484222325
        for ch in b:
            x = ((x ^ ch) * 0x100000001B3) & (2**64 - 1)
        x = (x + 0x9E3779B97F4A7C15) & (2**64 - 1)
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
        return x ^ (x >> 31)

    homes = [h(s) & 8191 for s in lst]
    assert len(set(homes)) < len(homes) - 100          # many shared home slots
    texts = lst + [b"chain-%05d" % i for i in range(40_000, 43_000)] + \
        [s[:-1] + b"x" for s in lst[:1000]]
    members = set(lst)
    got = eval_str(lst, texts)
    assert got.tolist() == [int(t in members) for t in texts]


def test_empty_and_null_only_lists():
    texts = [b"", b"a", None]
    assert eval_str([], texts).tolist() == [0, 0, 0]
    assert eval_str([None], texts).tolist() == [0, 0, 1]
    assert eval_str([b""], texts).tolist() == [1, 0, 0]
    v = np.array([0, 5], dtype=np.int64)
    assert eval_i64(np.zeros(0, np.int64), False, v, [0, 1]).tolist() == [0, 0]
    assert eval_i64(np.zeros(0, np.int64), True, v, [0, 1]).tolist() == [0, 1]


def test_builder_and_abi():
    e = y.col(0).isin([3, None, -1])
    assert e.c.op == _abi.EX_IN and e.c.list_len == 3 and not e.c.b
    assert [e.c.list[i].type for i in range(3)] == \
        [_abi.VT_INT64, _abi.VT_NULL, _abi.VT_INT64]
    assert e.c.list[2].data.i64 == -1
    e = y.isin(y.col(1), [b"x\x00y", b"", "é"])
    assert [e.c.list[i].length for i in range(3)] == [3, 0, 2]
    assert C.string_at(e.c.list[0].data.u64, 3) == b"x\x00y"
    assert C.string_at(e.c.list[2].data.u64, 2) == "é".encode()
    e = y.isin(y.col(0), np.array([1, 2**64 - 1], dtype=np.uint64))
    assert e.c.list[1].type == _abi.VT_UINT64 and e.c.list[1].data.u64 == 2**64 - 1
    assert y.isin(y.col(0), [True]).c.list[0].type == _abi.VT_BOOLEAN
    assert y.isin(y.col(0), [5], unsigned=True).c.list[0].type == _abi.VT_UINT64
    # list / list_len are second names of the lit_str / lit_len words: the
    # struct is as large as it was, and zero in every node without a literal
    f = _abi.YtExpr
    assert (f.list.offset, f.list_len.offset) == (f.lit_str.offset,
                                                  f.lit_len.offset) == (40, 48)
    assert C.sizeof(f) == 56
    for other in (y.col(0), y.lit(1), y.col(0) + 1):
        assert not other.c.list and other.c.list_len == 0


def test_the_oracle_is_never_handed_an_in_plan():
    chunk = y.Chunk([y.encode_int64(np.arange(10, dtype=np.int64))], 10)
    for plan in (y.Plan(filter=y.col(0).isin([1, 2]), aggs=[y.agg_sum1()]),
                 y.Plan(filter=(y.col(0) > 1).and_(y.col(0).isin([1]).not_()),
                        aggs=[y.agg_sum1()]),
                 y.Plan(keys=[y.col(0).isin([1])], aggs=[y.agg_sum1()]),
                 y.Plan(aggs=[y.agg_sum(y.col(0).isin([1]))]),
                 y.Plan(projects=[y.col(0).isin([1])]),
                 y.Plan(keys=[y.col(0)], aggs=[y.agg_sum1()],
                        having=y.col(1).isin([1]))):
        with pytest.raises(NotImplementedError):
            y.oracle_execute(plan, chunk)
        with pytest.raises(NotImplementedError):
            y.oracle_partial(plan, chunk, 2)
