"""Phase A of the partitioned GROUP BY at its tile edges.

k_scan_partition decodes a tile of T rows once into registers, ranks every
row in its bucket, gathers the tile's records bucket-major in LDS and copies
each bucket's run out as contiguous stores. A record region must hold one
whole tile whatever the key skew, so T is 4096 rows until bucket_stride
reaches 8192 and 8-byte packed records then tile 8192; both constants are
read from yt_gpu_debug_partition_tile_rows, so the shapes follow them.

Shapes, each in the four record / bucket modes of test_partition_modes
(dp 12+31 bits direct packed, hp 40+20 hash packed, d16 12+62 direct
16-byte, h16 40+40 hash 16-byte):

  segs     segments of T-1, T, T+1, 2T+3 and 1 rows in one column, each with
           its own min_value and width: masked tails, a tile of one row, and
           a segment whose sibling needs more tiles than it does
  runs1    one tile, 1024 rows, every bucket hit exactly once: runs of 1
  two      one full tile on two buckets: long runs; the hot bucket is sized
           from the bucket_stride formula to stay under the capacity guard,
           so no hash retry (H) may show in the path bits
  f1pct    a range filter that keeps about 1 % of the rows
  ftile    a range filter that rejects every row of ONE tile of four
  nulls    null keys, INT64_MIN keys and null values mixed inside one tile:
           both side slots and the null-value stream. The keys sit at the top
           of the zigzag range, [2^64 - 2^w, 2^64 - 1], whose last value is
           INT64_MIN, so the span stays w bits and every mode is reached
  nulls_min  the same with keys from zigzag 0 up to INT64_MIN: the span is
           64 bits, 16-byte hash records
  large    the smallest input whose packed records tile 8192 rows (22.3 M
           rows, direct packed, a partial last segment): every thread holds
           its full 16 rows. 1 % null values, 0.5 % null keys, a range
           filter on a third column that keeps 90 %, and 5000 rows of one
           key at the head of the first tile, a run longer than a 4096-row
           tile can produce. Written by the product encoder and compared as
           arrays, to stay within seconds.

Every GPU case asserts rows equal to the independent reference of
test_partition_modes exactly, the scan-path bits equal to predict_bits, and
rows_read / rows_written / grouped_row_count. The CPU twin runs the same
inputs through the oracle against that reference and checks the literal
bits of each mode against predict_bits, so the generators are proven
without a GPU.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ytsaurus_amd as y
from ytsaurus_amd import _abi

from test_partition_modes import (
    D, H, K, KX, M64, MK, MV, N, P, Case, DenseColumn, check_case, last_path,
    I64_MIN, np_reference_as_dict, predict_bits, reference_groupby_np,
    rowset_arrays, zz_dec)

KNB = 1024

MODES = {            # name: (key bits, value bits, path bits)
    "dp": (12, 31, P | D | K),
    "hp": (40, 20, P | K),
    "d16": (12, 62, P | D | KX),
    "h16": (40, 40, P),
}


@functools.lru_cache(maxsize=None)
def tile_rows(large=False):
    return int(_abi.gpu_lib().yt_gpu_debug_partition_tile_rows(int(large)))


def bucket_stride(rows):
    """run_partitioned's record capacity of one (bucket, XCD sub) region"""
    s = rows // (KNB * 8) + (rows // (KNB * 8)) // 2 + 4096
    return (s + 7) & ~7


def mix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def hash_bucket(zz):
    """phase A's hash-mode bucket of zigzag-domain keys"""
    key = zz_dec(zz).view(np.uint64)
    return ((mix64(key) >> np.uint64(40)) & np.uint64(KNB - 1)).astype(np.int64)


class RaggedColumn:
    """DenseColumn's segments at arbitrary row counts: each piece is written
    by DenseColumn as one segment, the pieces share one blob."""

    value_type = _abi.VT_INT64
    meta_range = DenseColumn.meta_range

    def __init__(self, zz, nulls, sizes):
        zz = np.ascontiguousarray(zz, dtype=np.uint64)
        assert sum(sizes) == len(zz)
        nulls = (np.zeros(len(zz), dtype=bool) if nulls is None
                 else np.asarray(nulls, dtype=bool))
        self.has_nulls = bool(nulls.any())
        live = zz[~nulls]
        self.exact = (int(live.min()), int(live.max())) if len(live) else None
        pieces, a = [], 0
        for n in sizes:
            pieces.append(DenseColumn(zz[a:a + n], nulls[a:a + n], n))
            a += n
        assert all(len(p.seg_meta) == 1 for p in pieces)
        self.seg_meta = [p.seg_meta[0] for p in pieces]
        blobs = [bytes(p._buf) for p in pieces]
        self._buf = (C.c_uint64 * (sum(map(len, blobs)) // 8)).from_buffer_copy(
            b"".join(blobs))
        base = C.addressof(self._buf)
        self._segs = (_abi.YtSegment * len(pieces))()
        at = 0
        for i, ((mn, w, rows), b) in enumerate(zip(self.seg_meta, blobs)):
            self._segs[i] = _abi.YtSegment(
                type=_abi.SEG_DIRECT_DENSE, row_count=rows, min_value=mn,
                data=base + at, data_size=len(b))
            at += len(b)
        self._cenc = _abi.YtEncodedColumn(
            segment_count=len(pieces), segments=self._segs, blob=base,
            blob_size=at)
        self.segments = [self._segs[i] for i in range(len(pieces))]


class TileCase(Case):
    """A Case whose segments have the row counts `sizes`, with the
    reference computed by the numpy form."""

    def __init__(self, cid, make, bits, sizes, **kw):
        super().__init__(cid, make, bits, **kw)
        self.sizes = list(sizes)

    def columns(self):
        return [RaggedColumn(z, nu, self.sizes) for z, nu in self.data()]

    @functools.lru_cache(maxsize=None)
    def reference(self):
        return np_reference_as_dict(reference_groupby_np(
            self.decoded(), 0, list(self.sums), self.flt))


# ------------------------------------------------------------------ #
# generators (zigzag domain)                                          #

def seg_values(rng, sizes, m, w, pool):
    """per segment its own base (m, m+3, m+6, ...) and width (w for the
    first, w-1 after it), both ends of its range in its first two rows; the
    column's span is the first segment's, 2^w - 1"""
    out = []
    for s, n in enumerate(sizes):
        lo = m + 3 * s
        ws = w if s == 0 else w - 1
        hi = min(lo + (1 << ws) - 1, M64 - 1)
        raw = rng.integers(0, M64, size=pool, dtype=np.uint64, endpoint=True)
        vals = np.array([lo + int(r) % (hi - lo + 1) for r in raw],
                        dtype=np.uint64)
        v = vals[rng.integers(0, pool, n)]
        v[0] = lo
        if n > 1:
            v[1] = hi
        out.append(v)
    assert sizes[0] > 1
    return np.concatenate(out)


def seg_nulls(rng, sizes, frac):
    m = rng.random(sum(sizes)) < frac
    a = 0
    for n in sizes:
        m[a:a + 2] = False
        a += n
    return m


def make_plain(sizes, wk, wv, knulls=0.0, vnulls=0.0, fcol=None):
    def make(rng):
        k = seg_values(rng, sizes, MK, wk, 300)
        v = seg_values(rng, sizes, MV, wv, 64)
        kn = seg_nulls(rng, sizes, knulls) if knulls else None
        vn = seg_nulls(rng, sizes, vnulls) if vnulls else None
        cols = [(k, kn), (v, vn)]
        if fcol is not None:
            cols.append((fcol(rng, sum(sizes)), None))
        return cols
    return make


def make_runs1(wk, wv, direct):
    """1024 rows, one per bucket"""
    def make(rng):
        if direct:
            dshift = wk - 10
            low = rng.integers(0, 1 << dshift, KNB)
            low[0], low[KNB - 1] = 0, (1 << dshift) - 1
            k = MK + (np.arange(KNB) << dshift) + low
        else:
            ends = np.array([MK, MK + (1 << wk) - 1], dtype=np.uint64)
            eb = hash_bucket(ends)
            assert eb[0] != eb[1]
            cand = (MK + 1 + rng.integers(0, (1 << wk) - 2, 64 * KNB)).astype(
                np.uint64)
            cb = hash_bucket(cand)
            first = np.full(KNB, -1, dtype=np.int64)
            first[cb[::-1]] = np.arange(len(cand))[::-1]
            assert (first >= 0).all()
            k = cand[first]
            k[eb] = ends
            assert sorted(hash_bucket(k).tolist()) == list(range(KNB))
        k = rng.permutation(np.asarray(k, dtype=np.uint64))
        v = seg_values(rng, [KNB], MV, wv, 64)
        return [(k, None), (v, None)]
    return make


def two_bucket_counts(t):
    """(hot, cold) rows of a full tile on two buckets, the hot one as large
    as the tile and the region capacity allow"""
    hot = min(t - 16, bucket_stride(t) - 1)
    return hot, t - hot


def make_two(t, wk, wv, direct):
    def make(rng):
        hot, cold = two_bucket_counts(t)
        if direct:
            dshift = wk - 10
            a = MK + rng.integers(0, 1 << dshift, hot)
            b = MK + ((KNB - 1) << dshift) + rng.integers(0, 1 << dshift, cold)
            a[0], b[0] = MK, MK + (1 << wk) - 1
        else:
            a = np.full(hot, MK)
            b = np.full(cold, MK + (1 << wk) - 1)
            assert len(set(hash_bucket(np.array([a[0], b[0]],
                                                dtype=np.uint64)).tolist())) == 2
        k = rng.permutation(np.concatenate([a, b]).astype(np.uint64))
        v = seg_values(rng, [t], MV, wv, 64)
        return [(k, None), (v, None)]
    return make


def filter_col(t):
    """decoded 0..9999 uniformly, except rows T..2T-1 (one tile): 20000"""
    def col(rng, n):
        f = rng.integers(0, 10_000, n)
        f[t:2 * t] = 20_000
        return (2 * f).astype(np.uint64)      # zigzag of a non-negative value
    return col


def make_nulls(t, wk, wv):
    """keys in the top 2^wk zigzag values, 2 % of them INT64_MIN (zigzag
    2^64 - 1), 10 % null keys, 10 % null values"""
    def make(rng):
        lo = M64 - ((1 << wk) - 1)
        raw = rng.integers(0, M64, size=300, dtype=np.uint64, endpoint=True)
        vals = np.array([lo + int(r) % (1 << wk) for r in raw], dtype=np.uint64)
        k = vals[rng.integers(0, 300, t)]
        k[rng.random(t) < 0.02] = M64
        k[0], k[1] = lo, M64
        v = seg_values(rng, [t], MV, wv, 64)
        return [(k, seg_nulls(rng, [t], 0.1)), (v, seg_nulls(rng, [t], 0.1))]
    return make


def make_nulls_min(t):
    def make(rng):
        k = seg_values(rng, [t], 0, 40, 300)
        k[rng.random(t) < 0.02] = M64          # zigzag of INT64_MIN
        k[0] = 0
        v = seg_values(rng, [t], MV, 40, 64)
        return [(k, seg_nulls(rng, [t], 0.1)), (v, seg_nulls(rng, [t], 0.1))]
    return make


def _rng_filter(lo, hi):
    return lambda: (y.col(2) >= lo).and_(y.col(2) <= hi)


def _cases():
    out = []
    t = tile_rows()
    for mode, (wk, wv, bits) in MODES.items():
        direct = bool(bits & D)
        sizes = [t - 1, t, t + 1, 2 * t + 3, 1]
        out.append(TileCase("segs_" + mode, make_plain(sizes, wk, wv), bits,
                            sizes))
        out.append(TileCase("runs1_" + mode, make_runs1(wk, wv, direct), bits,
                            [KNB]))
        out.append(TileCase("two_" + mode, make_two(t, wk, wv, direct), bits,
                            [t]))
        fsizes = [2 * t, 2 * t]
        fmake = make_plain(fsizes, wk, wv, fcol=filter_col(t))
        out.append(TileCase("f1pct_" + mode, fmake, bits, fsizes,
                            flt=(2, 0, 99), flt_expr=_rng_filter(0, 99)))
        out.append(TileCase("ftile_" + mode, fmake, bits, fsizes,
                            flt=(2, 0, 9_999), flt_expr=_rng_filter(0, 9_999)))
        out.append(TileCase("nulls_" + mode, make_nulls(t, wk, wv),
                            bits | N, [t]))
    out.append(TileCase("nulls_min", make_nulls_min(t), P | N, [t]))
    return out


SHAPES = ("segs", "runs1", "two", "f1pct", "ftile", "nulls")
IDS = ["%s_%s" % (sh, mode) for mode in MODES for sh in SHAPES] + ["nulls_min"]


@functools.lru_cache(maxsize=None)
def cases():
    """built on first use: the tile constants come from the built library"""
    out = {c.id: c for c in _cases()}
    assert list(out) == IDS
    return out


@functools.lru_cache(maxsize=None)
def large_rows():
    """the first row count whose regions hold a large tile, and 1000 rows
    more so that the last segment ends inside a tile"""
    q = next(q for q in range(1, 1 << 12)
             if bucket_stride(q * KNB * 8) >= tile_rows(True))
    return q * KNB * 8 + 1000


# ------------------------------------------------------------------ #
# CPU tier                                                            #

def test_tile_constants():
    """bucket_stride's fixed slack covers one whole small tile, and large_rows()
    is the first row count whose regions hold a large one"""
    LARGE_ROWS = large_rows()
    assert 2 * KNB <= tile_rows() <= bucket_stride(0)
    assert tile_rows(True) == 2 * tile_rows()
    assert bucket_stride(LARGE_ROWS) >= tile_rows(True)
    assert bucket_stride(LARGE_ROWS - KNB * 8) < tile_rows(True)
    assert 20_000_000 < LARGE_ROWS < 25_000_000


@pytest.mark.parametrize("cid", IDS)
def test_inputs_and_oracle(cid):
    """the generated columns sit in the mode they were built for, the shape
    is what its name says, and the oracle agrees with the reference"""
    case = cases()[cid]
    cols = case.columns()
    assert predict_bits(cols[0], cols[1]) == case.bits
    assert [m[2] for m in cols[0].seg_meta] == case.sizes
    shape, _, mode = case.id.partition("_")
    zk, kn = case.data()[0]
    if shape == "segs":
        assert len({m[0] for m in cols[0].seg_meta}) == len(case.sizes)
        assert len({m[1] for m in cols[0].seg_meta}) >= 3
    if shape in ("runs1", "two"):
        wk, _, bits = MODES[mode]
        b = (((zk - np.uint64(MK)) >> np.uint64(wk - 10)).astype(np.int64)
             if bits & D else hash_bucket(zk))
        cnt = np.bincount(b, minlength=KNB)
        if shape == "runs1":
            assert (cnt == 1).all()
        else:
            t = case.sizes[0]
            assert sorted(cnt[cnt > 0].tolist()) == sorted(two_bucket_counts(t))
            assert cnt.max() <= bucket_stride(t) and cnt.max() > t // 2 - 8
    if shape in ("f1pct", "ftile"):
        f = zz_dec(case.data()[2][0])
        keep = (f >= case.flt[1]) & (f <= case.flt[2])
        t = case.sizes[0] // 2
        assert not keep[t:2 * t].any()
        if shape == "ftile":
            assert keep[:t].all() and keep[2 * t:].all()
        else:
            assert 0.005 < keep.mean() < 0.015
    if shape == "nulls":
        vn = case.data()[1][1]
        assert kn.any() and vn.any() and (kn & vn).any() and (~kn & vn).any()
        imin = ~kn & (zk == np.uint64(M64))
        assert (imin & vn).any() and (imin & ~vn).any()
        ref = case.reference()
        assert None in ref and I64_MIN in ref
        if mode != "min":
            wk = MODES[mode][0]
            assert cols[0].exact == (M64 - (1 << wk) + 1, M64)
    got, st = y.oracle_execute(case.plan(), case.chunk())
    want = case.rows()
    assert y.sort_rows(got) == y.sort_rows(want)
    assert st.rows_read == sum(case.sizes)
    assert st.rows_written == len(want)


LARGE_RUN = 5000       # rows of one key at the head of the first tile
LARGE_FLT = (2, 0, 9 << 16)   # of 0 .. 10 << 16: keeps 90 %


def large_input(n):
    """-> [(keys, nulls), (values, nulls), (filter column, None)], decoded.
    Keys uniform over 2^13 zigzag values (direct packed, dshift 3: a tile
    puts 8 records on a bucket on average), 0.5 % null; values below 2^31,
    1 % null; filter column uniform below 10 * 2^16. The first LARGE_RUN rows hold
    key 7, never null, and pass the filter."""
    rng = np.random.default_rng(n)
    k = rng.integers(-(1 << 12), 1 << 12, n, dtype=np.int16).astype(np.int64)
    kn = rng.integers(0, 200, n, dtype=np.uint8) == 0
    v = rng.integers(0, 1 << 31, n, dtype=np.int32).astype(np.int64)
    vn = rng.integers(0, 100, n, dtype=np.uint8) == 0
    f = rng.integers(0, 10 << 16, n, dtype=np.int32).astype(np.int64)
    k[:LARGE_RUN], kn[:LARGE_RUN], f[:LARGE_RUN] = 7, False, 0
    return [(k, kn), (v, vn), (f, None)]


def bincount_reference(cols):
    """-> (keys ascending, sums, counts, (null-key sum, null-key count));
    float64 weights are exact while every sum stays below 2^53"""
    (k, kn), (v, vn), (f, _) = cols
    keep = (f >= LARGE_FLT[1]) & (f <= LARGE_FLT[2])
    live = keep & ~kn
    lo = int(k.min())
    idx = k[live] - lo
    cnt = np.bincount(idx)
    assert int(cnt.max()) << 31 < 1 << 53
    ssum = np.bincount(idx, weights=np.where(vn[live], 0, v[live])).astype(np.int64)
    keys = np.flatnonzero(cnt) + lo
    side = keep & kn
    return (keys, ssum[keys - lo], cnt[keys - lo],
            (int(v[side & ~vn].sum()), int(side.sum())))


def large_plan():
    return y.Plan(filter=_rng_filter(*LARGE_FLT[1:])(), keys=[y.col(0)],
                  aggs=[y.agg_sum(y.col(1)), y.agg_sum1()])


def large_chunk(cols):
    encs = [y.encode_int64(a) if nu is None
            else y.encode_int64(a, nu.astype(np.uint8)) for a, nu in cols]
    return encs, y.Chunk(encs, len(cols[0][0]))


def test_large_generator_and_reference():
    """the large case's generator through the oracle, and its bincount
    reference against reference_groupby_np, on 2^17 rows"""
    n = 1 << 17
    cols = large_input(n)
    keys, ssum, cnt, (nsum, ncnt) = bincount_reference(cols)
    ukeys, rsum, rnn, rcnt, nullgrp = reference_groupby_np(
        cols, 0, [1], LARGE_FLT)
    assert (rnn[0] > 0).all()
    assert (keys == ukeys).all() and (ssum == rsum[0]).all()
    assert (cnt == rcnt).all()
    assert nullgrp == ([nsum], [nullgrp[1][0]], ncnt) and nullgrp[1][0] > 0
    assert cnt[keys == 7][0] > LARGE_RUN
    got, st = y.oracle_execute(large_plan(), large_chunk(cols)[1])
    want = list(zip(keys.tolist(), ssum.tolist(), cnt.tolist()))
    want.append((None, nsum, ncnt))
    assert y.sort_rows(got) == y.sort_rows(want)
    assert st.rows_read == n


# ------------------------------------------------------------------ #
# GPU tier                                                            #

@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_tiles(cid, cuda):
    case = cases()[cid]
    check_case(case, cuda)
    cols = case.columns()
    assert last_path() == predict_bits(cols[0], cols[1])
    assert not last_path() & H
    if case.id.startswith("nulls"):
        ref = case.reference()
        assert None in ref and I64_MIN in ref


@pytest.mark.gpu
def test_large_tiles(cuda):
    """8192-row tiles, every thread's 16 rows live"""
    n = large_rows()
    cols = large_input(n)
    keys, ssum, cnt, (nsum, ncnt) = bincount_reference(cols)
    assert cnt[keys == 7][0] > LARGE_RUN > tile_rows() and ncnt > 0
    encs, chunk = large_chunk(cols)
    for enc in encs:
        assert all(s.type == _abi.SEG_DIRECT_DENSE for s in enc.segments)
    assert encs[0].segments[-1].row_count % tile_rows(True) != 0
    dev = chunk.c_device(cuda)
    g = len(keys) + 1
    rs, st = y.gpu_execute(large_plan(), dev, max_groups_hint=1 << 14,
                           rowset=y.make_rowset(g + 16, 3), raw_rowset=True)
    assert last_path() == P | D | K | N
    assert rs.row_count == g and rs.column_count == 3
    types, data = rowset_arrays(rs, 3)
    assert (types[:, 1:] == _abi.VT_INT64).all()
    nullkey = types[:, 0] == _abi.VT_NULL
    assert nullkey.sum() == 1 and (types[~nullkey, 0] == _abi.VT_INT64).all()
    assert tuple(data[nullkey][0, 1:].tolist()) == (nsum, ncnt)
    data = data[~nullkey]
    order = np.argsort(data[:, 0], kind="stable")
    assert (data[order, 0] == keys).all()
    assert (data[order, 1] == ssum).all()
    assert (data[order, 2] == cnt).all()
    assert (st.rows_read, st.rows_written, st.grouped_row_count) == (n, g, g)
    assert st.incomplete_output == 0 and st.kernel_scan_launches == 1
