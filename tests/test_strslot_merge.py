"""The StrSlot identity protocol of the three string-key merges (dense
GROUP BY, general GROUP BY, two-phase state merge), pinned against a Python
dict on a key set built to reach every accept and demote rule of the slot
comment in csrc/common.h:

  * a few hundred keys of 8 bytes or less: accepted on ident + in-slot prefix;
  * keys of exactly 16 and exactly 17 bytes that differ only in their last
    byte: the longest key the prefix decides, and the shortest it cannot;
  * 50 keys of 27..40 bytes sharing their first 16 bytes and (in groups)
    their length: the prefix never decides, every duplicate goes through the
    owner byte comparison;
  * the empty string and the null key.

Every key occurs in every key segment, so each one is a cross-segment (and,
in the two-phase case, a cross-state) duplicate. Values are int64 and doubles
that are whole numbers below 2^20: every partial sum is an integer below
2^53, exact under any atomic order, so the comparison is equality.

Not covered here: a genuine hash48|len collision between two different
strings (same upper 48 FNV-1a bits and same length) cannot be constructed
cheaply; that demote-and-walk-on branch is covered by review only.
"""
import ctypes as C

import numpy as np
import pytest

import ytsaurus_amd as y
from ytsaurus_amd import _abi
from ytsaurus_amd._abi import (VT_DOUBLE, VT_INT64, VT_STRING,
                               SCAN_PATH_STR_DENSE, SCAN_PATH_STR_GENERAL)

SEG = 2500          # 6000 rows -> key segments of 2500, 2500 and a ragged 1000
HALF_SEG = 1250     # 3000 rows -> 1250, 1250 and a ragged 500
BLOCK = 1000        # every key occurs once at the head of each 1000-row block


def scan_path():
    return _abi.gpu_lib().yt_gpu_debug_last_scan_path()


def key_set():
    keys = [b"s%03d" % i for i in range(300)]                   # 4 bytes
    keys += [b"k%07d" % (i * 7919) for i in range(40)]          # 8 bytes
    keys += [b"a", b"ab", b"abc"]
    stem = b"sixteen-bytes-ke"                                  # 16 bytes
    assert len(stem) == 16
    keys += [stem[:15] + c for c in (b"0", b"1", b"2", b"3")]   # exactly 16
    keys += [stem + c for c in (b"0", b"1", b"2", b"3")]        # exactly 17
    for i in range(50):                                         # 27..40 bytes
        ln = 27 + i % 14
        tail = b"%02d" % i
        keys.append(stem + b"-" * (ln - 16 - len(tail)) + tail)
    keys.append(b"")
    keys.append(None)
    assert len(set(keys)) == len(keys)
    return keys


def build_rows(keys, n, seed):
    """n rows in blocks of BLOCK: each block opens with every key once (in a
    shuffled order) and is filled up with random picks."""
    rng = np.random.default_rng(seed)
    assert len(keys) <= BLOCK and n % BLOCK == 0
    idx = []
    for _ in range(n // BLOCK):
        idx += list(rng.permutation(len(keys)))
        idx += list(rng.integers(0, len(keys), BLOCK - len(keys)))
    idx = np.array(idx)
    vi = rng.integers(-10**6, 10**6, n, dtype=np.int64)
    vin = (rng.random(n) < 0.05).astype(np.uint8)
    vd = rng.integers(0, 1 << 20, n).astype(np.float64)
    vdn = (rng.random(n) < 0.05).astype(np.uint8)
    return {"keys": [keys[i] for i in idx], "kidx": idx.astype(np.int64),
            "vi": vi, "vin": vin, "vd": vd, "vdn": vdn}


CHUNK_TYPES = [VT_STRING, VT_INT64, VT_DOUBLE, VT_INT64]


def chunk_of(rows, lo=0, hi=None, seg=SEG):
    """columns: 0 key, 1 int64, 2 double, 3 key index (a function of the
    key); every column cut into the same segments"""
    hi = len(rows["keys"]) if hi is None else hi
    return y.Chunk(
        [y.encode_string(rows["keys"][lo:hi], max_segment_values=seg),
         y.encode_int64(rows["vi"][lo:hi], rows["vin"][lo:hi],
                        max_segment_values=seg),
         y.encode_double(rows["vd"][lo:hi], rows["vdn"][lo:hi],
                         max_segment_values=seg),
         y.encode_int64(rows["kidx"][lo:hi], max_segment_values=seg)],
        hi - lo)


_CACHE = {}


def data(name):
    """shared inputs, built once and never modified:
    'mixed'    6000 rows over key_set()
    'distinct' 6000 rows over 3000 distinct keys (for the overflow retry)"""
    if name not in _CACHE:
        if name == "mixed":
            rows = build_rows(key_set(), 6000, 20261)
        else:
            keys = [b"d%04d" % i for i in range(2990)]
            keys += [b"distinct-long-key-%022d" % i for i in range(10)]
            rng = np.random.default_rng(20262)
            # each key exactly twice, once in each half; the second half is
            # the first rotated by 500 rows, which puts the two occurrences
            # into different 2500-row segments
            perm = rng.permutation(3000)
            idx = np.concatenate([perm, np.roll(perm, -500)])
            n = 6000
            rows = {"keys": [keys[i] for i in idx], "kidx": idx.astype(np.int64),
                    "vi": rng.integers(-10**6, 10**6, n, dtype=np.int64),
                    "vin": np.zeros(n, dtype=np.uint8),
                    "vd": rng.integers(0, 1 << 20, n).astype(np.float64),
                    "vdn": np.zeros(n, dtype=np.uint8)}
        _CACHE[name] = (rows, chunk_of(rows))
    return _CACHE[name]


def reference(rows, val, nul, keep=None):
    """{key: [sum over non-null or None, non-null count, row count]}"""
    ref = {}
    for i, k in enumerate(rows["keys"]):
        if keep is not None and not keep[i]:
            continue
        r = ref.setdefault(k, [None, 0, 0])
        r[2] += 1
        if not rows[nul][i]:
            r[0] = (r[0] or 0) + rows[val][i].item()
            r[1] += 1
    return ref


def rkey(r):
    return (r[0] is None, r[0] or b"")


def assert_equal(got, want):
    got = sorted(got, key=rkey)
    want = sorted(want, key=rkey)
    print("groups: got %d want %d" % (len(got), len(want)))
    assert [r[0] for r in got] == [r[0] for r in want]
    bad = [(g, w) for g, w in zip(got, want) if tuple(g) != tuple(w)]
    print("differing rows: %d %r" % (len(bad), bad[:3]))
    assert not bad


def sum_rows(ref):
    return [(k, r[0], r[2]) for k, r in ref.items()]


# ---- dense path ----

def dense_plan():
    return y.Plan(keys=[y.col(0)], aggs=[y.agg_sum(y.col(2)), y.agg_sum1()])


@pytest.mark.gpu
@pytest.mark.parametrize("name,hint", [("mixed", 1024), ("distinct", 1)])
def test_dense_merge(cuda, name, hint):
    """hint 1 starts the table at 2048 slots for 3000 distinct keys: the
    merge overflows and is retried on a larger table"""
    rows, chunk = data(name)
    assert chunk.columns[0]._cenc.segment_count == 3
    got, st = y.gpu_execute(dense_plan(), chunk.c_device(cuda),
                            max_groups_hint=hint, out_capacity=8192)
    assert scan_path() == SCAN_PATH_STR_DENSE
    want = reference(rows, "vd", "vdn")
    assert_equal(got, sum_rows(want))
    assert st.grouped_row_count == len(want) and st.incomplete_output == 0


# ---- general path ----

@pytest.mark.gpu
@pytest.mark.parametrize("name,hint", [("mixed", 1024), ("distinct", 1)])
def test_general_merge(cuda, name, hint):
    rows, chunk = data(name)
    plan = y.Plan(filter=y.col(1) > -800_000, keys=[y.col(0)],
                  aggs=[y.agg_min(y.col(1)), y.agg_max(y.col(2)),
                        y.agg_avg(y.col(2)), y.agg_first(y.col(3))])
    got, _ = y.gpu_execute(plan, chunk.c_device(cuda), max_groups_hint=hint,
                           out_capacity=8192)
    assert scan_path() == SCAN_PATH_STR_GENERAL
    # a null col1 makes the filter null: the row is dropped
    keep = (rows["vin"] == 0) & (rows["vi"] > -800_000)
    ref = reference(rows, "vd", "vdn", keep)
    by_key = {}
    for i in np.flatnonzero(keep):
        by_key.setdefault(rows["keys"][i], []).append(i)
    want = []
    for k, (s, nn, cnt) in ref.items():
        sel = by_key[k]
        vi = [rows["vi"][i].item() for i in sel]
        vd = [rows["vd"][i].item() for i in sel if not rows["vdn"][i]]
        want.append((k, min(vi), max(vd) if vd else None,
                     s / nn if nn else None, rows["kidx"][sel[0]].item()))
    assert_equal(got, want)


# ---- two-phase: partial states of two halves, merged ----

def merge_str(plan, states_ptr, counts, pool_ptr, pbytes, col_types, hint,
              group_row_limit=0):
    """yt_gpu_merge_states_str with every option (api.gpu_merge_str passes
    no group_row_limit); col_types are the types of the chunk's columns"""
    opts = _abi.YtExecOptions(max_groups_hint=hint,
                              group_row_limit=group_row_limit)
    nseg = len(counts)
    sc = (C.c_int64 * nseg)(*counts)
    sb = (C.c_int64 * nseg)(*pbytes)
    ct = (C.c_uint8 * 8)(*(list(col_types) + [0] * (8 - len(col_types))))
    rs = y.make_rowset(sum(counts) + 16, 3,
                       pool_bytes=max(sum(pbytes), 1024))
    st = _abi.YtStatistics()
    err = C.create_string_buffer(512)
    rc = _abi.gpu_lib().yt_gpu_merge_states_str(
        C.byref(plan.c), C.c_void_p(states_ptr), sc, nseg,
        C.c_void_p(pool_ptr), sb, ct, C.byref(opts), C.byref(rs),
        C.byref(st), err, 512)
    assert rc == 0, err.value
    return y.rows_from_rowset(rs), st


def two_phase(cuda, rows, val_col, hint, group_row_limit=0):
    plan = y.Plan(keys=[y.col(0)], aggs=[y.agg_sum(y.col(val_col)),
                                         y.agg_sum1()])
    n = len(rows["keys"])
    cap, pool_cap = n + 32, 64 * n
    states_t = cuda.zeros((cap, 4), dtype=cuda.int64, device="cuda")
    pool_t = cuda.zeros(pool_cap, dtype=cuda.uint8, device="cuda")
    counts, pbytes = [], []
    for lo in (0, n // 2):
        half = chunk_of(rows, lo, lo + n // 2, seg=HALF_SEG)
        assert half.columns[0]._cenc.segment_count == 3
        c, b, _ = y.gpu_partial_str(
            plan, half.c_device(cuda), 1,
            states_t.data_ptr() + 32 * sum(counts), cap - sum(counts),
            pool_t.data_ptr() + sum(pbytes), pool_cap - sum(pbytes),
            max_groups_hint=hint)
        counts += c
        pbytes += b
    return merge_str(plan, states_t.data_ptr(), counts, pool_t.data_ptr(),
                     pbytes, CHUNK_TYPES, hint, group_row_limit)


@pytest.mark.gpu
@pytest.mark.parametrize("val_col", [1, 2], ids=["int", "double"])
@pytest.mark.parametrize("name,hint", [("mixed", 1024), ("distinct", 1)])
def test_two_phase_merge(cuda, name, hint, val_col):
    rows, _ = data(name)
    got, st = two_phase(cuda, rows, val_col, hint)
    want = reference(rows, *(("vi", "vin") if val_col == 1 else ("vd", "vdn")))
    assert_equal(got, sum_rows(want))
    assert st.grouped_row_count == len(want) and st.incomplete_output == 0


# ---- group_row_limit ----

@pytest.mark.gpu
def test_group_row_limit(cuda):
    """as test_string_group_general.test_group_row_limit_matches_
    specialised_path: the limit marks the output incomplete, the identity
    merge still completes and counts every group"""
    rows, chunk = data("mixed")
    ngroups = len(set(rows["keys"]))
    _, st = y.gpu_execute(dense_plan(), chunk.c_device(cuda),
                          max_groups_hint=1024, group_row_limit=50)
    assert scan_path() == SCAN_PATH_STR_DENSE
    print("dense:", st.incomplete_output, st.grouped_row_count)
    assert st.incomplete_output == 1 and st.grouped_row_count == ngroups
    _, st = two_phase(cuda, rows, 2, 1024, group_row_limit=50)
    print("state merge:", st.incomplete_output, st.grouped_row_count)
    assert st.incomplete_output == 1 and st.grouped_row_count == ngroups
    _, st = two_phase(cuda, rows, 2, 1024)
    assert st.incomplete_output == 0
