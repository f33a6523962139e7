"""Phase A's plain decode, and the copy-out at awkward tile totals.

k_scan_partition has a plain instantiation for the commonest shape: 8-byte
packed records, a direct-span key, a value column, no filter, no nulls, key
segments of at most 32 bits and no INT64_MIN key in the column. It cuts each
field from a window of two or three dwords of the staged words, without a
clamp, so the last row's window may read one dword past them.
yt_gpu_debug_partition_variant() tells which instantiation the last launch
used: 0 16-byte records, 1 packed, 3 packed and plain.

The width sweeps of test_partition_decode (vw01..vw51, kw01..kw22) run the
plain decode by themselves. The shapes here are what they cannot see, T =
yt_gpu_debug_partition_tile_rows:

  disp_*     dispatch: one direct packed input (plain), and the same with one
             null key, one null value, a filter column, a 23-bit key span
             (hash) and a 62-bit value span (16-byte records): not plain
  min_in     keys in the top 2^12 zigzag values, INT64_MIN (zigzag 2^64 - 1)
             among them: not plain, the side slot exact
  min_out    the neighbouring column that ends at zigzag 2^64 - 2: plain
  edge_kKK_vVV  key widths 1, 21, 22, 31, 32 x value widths 1, 31, 32, 33, 42
             and the widest that still packs beside the key (direct packed
             and plain up to 22 key bits; a key SPAN of 31 or 32 bits is hash
             packed, the general decode). A segment of T rows, one of T - 1
             and, where the value's or the key's width is odd, one whose last
             field ends ONE bit before the end of its last staged word (n w =
             63 mod 64); the column's two ends in each segment's last two
             rows, so the last field has all its bits set and the window
             behind it reads past the staged words
  wkey_k23_vVV  key segments WRITTEN at 23 bits over a 22-bit span (WideColumn)
             beside value widths 1, 31, 32, 33, 41: plain, at the widest key
             field that can reach it. Direct mode needs a header span of at
             most 23 bits (the exact key scan runs for no wider one), so a
             key field of 24..32 bits, which the kernel allows, is not
             reachable through run_partitioned and no test can run it
  full       22 + 42 written bits per row at the 8192-row tile: the staged
             words fill the 64 KiB scratch exactly and the last row's window
             reads into the histograms. The spans are 21 + 41 bits, which the
             exact scans find, so the input is direct packed; the segments
             are written one bit wider than they need (WideColumn). The one
             case above a few tiles (22.3 M rows), compared as arrays
  runs_<mode>  the copy-out loop (one record per lane and pass, every
             instantiation) under YTQL_GRID=8: a segment of T rows on ONE
             bucket (a run of T records), one of 1024 rows with one per
             bucket, and 22 tiles on all other buckets, the last of T - 3
             rows, an odd total; the four modes of test_partition_tiles

Every GPU case asserts exact rows, path bits and counters (check_case) and
the variant. The CPU twin runs each generator through the oracle against the
reference and asserts the shape its name claims.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ytsaurus_amd as y
from ytsaurus_amd import _abi

from test_partition_modes import (
    D, H, I64_MIN, K, KX, M64, MK, MV, N, P, DenseColumn, _pack_words,
    check_case, last_path, predict_bits, rowset_arrays, zz_dec)
from test_partition_tiles import (
    KNB, MODES, TileCase, bucket_stride, filter_col, hash_bucket, large_rows,
    make_plain, seg_values, tile_rows, RaggedColumn)

PACKED, PLAIN = 1, 3        # yt_gpu_debug_partition_variant()


def variant():
    return int(_abi.gpu_lib().yt_gpu_debug_partition_variant())


def want_variant(case):
    """run_partitioned's choice, from the case's columns and plan"""
    cols = case.columns()
    bits = predict_bits(cols[0], cols[1])
    if not bits & K:
        return 0
    key = cols[0]
    top = key.exact[1] if bits & KX else key.meta_range()[1]
    lo, hi = key.meta_range()
    plain = (bits & D and case.flt is None and not key.has_nulls
             and not cols[1].has_nulls and top < M64 and hi < M64
             and hi - lo < 1 << 32)
    return PLAIN if plain else PACKED


# ------------------------------------------------------------------ #
# generators (zigzag domain)                                          #

DISP_SIZES = lambda t: [2 * t + 3]


def make_disp(t, kind):
    """the same 12 + 31-bit data for every kind but the last two, whose
    spans differ by construction"""
    wk, wv = {"hash": (23, 31), "rec16": (12, 62)}.get(kind, (12, 31))

    def make(_):
        rng = np.random.default_rng(20261021)
        fcol = filter_col(t) if kind == "filter" else None
        cols = make_plain(DISP_SIZES(t), wk, wv, fcol=fcol)(rng)
        n = len(cols[0][0])
        one = np.zeros(n, dtype=bool)
        one[n // 2] = True
        if kind == "knull":
            cols[0] = (cols[0][0], one)
        if kind == "vnull":
            cols[1] = (cols[1][0], one)
        return cols
    return make


DISP = {          # kind: (variant, path bits)
    "plain": (PLAIN, P | D | K),
    "knull": (PACKED, P | D | K),
    "vnull": (PACKED, P | D | K | N),
    "filter": (PACKED, P | D | K),
    "hash": (PACKED, P | K | KX),
    "rec16": (0, P | D | KX),
}


def make_top(n, wk, wv, top):
    """keys in [top - 2^wk + 1, top], both ends in rows 0 and 1 and 2 % of
    the rows on top"""
    def make(rng):
        lo = top - ((1 << wk) - 1)
        raw = rng.integers(0, M64, size=300, dtype=np.uint64, endpoint=True)
        vals = np.array([lo + int(r) % (1 << wk) for r in raw], dtype=np.uint64)
        k = vals[rng.integers(0, 300, n)]
        k[rng.random(n) < 0.02] = top
        k[0], k[1] = lo, top
        return [(k, None), (seg_values(rng, [n], MV, wv, 64), None)]
    return make


EDGE_KW = (1, 21, 22, 31, 32)


def edge_widths():
    out = []
    for kw in EDGE_KW:
        cap = (63 if kw <= 22 else 64) - kw      # direct packed / hash packed
        for vw in sorted({min(v, cap) for v in (1, 31, 32, 33, 42, cap)}):
            out.append((kw, vw))
    return out


def edge_values(rng, sizes, m, w, pool):
    """every segment over the whole [m, m + 2^w - 1], its ends in its last
    two rows"""
    out = []
    for n in sizes:
        raw = rng.integers(0, M64, size=pool, dtype=np.uint64, endpoint=True)
        vals = np.array([m + int(r) % (1 << w) for r in raw], dtype=np.uint64)
        v = vals[rng.integers(0, pool, n)]
        v[n - 2], v[n - 1] = m, m + (1 << w) - 1
        out.append(v)
    return np.concatenate(out)


def make_edge(sizes, kw, vw):
    def make(rng):
        return [(edge_values(rng, sizes, MK, kw, 300), None),
                (edge_values(rng, sizes, MV, vw, 64), None)]
    return make


def short_field(kw, vw):
    """the written width whose last field a segment can end one bit before a
    word's end: the value's if odd, else the key's if odd, else None"""
    return vw if vw % 2 else kw if kw % 2 else None


def edge_sizes(t, kw, vw):
    """T, T - 1 and, for an odd width w, the largest n <= T - 2 with
    n w = 63 (mod 64)"""
    w = short_field(kw, vw)
    if w is None:
        return [t, t - 1]
    return [t, t - 1, next(n for n in range(t - 2, 0, -1) if n * w % 64 == 63)]


WKEY_W, WKEY_SPAN = 23, 22         # written key width, key span bits
WKEY_VW = (1, 31, 32, 33, 41)      # 22 + 41 = 63: the widest direct packed


class WideKeyCase(TileCase):
    """a TileCase whose key segments are written at WKEY_W bits"""

    def columns(self):
        (zk, _), (zv, _) = self.data()
        return [WideColumn(zk, WKEY_W, sizes=self.sizes),
                RaggedColumn(zv, None, self.sizes)]


RUN_HOT = 512            # the bucket of the one-run tile
RUN_TILES = 22           # tiles of the last segment


def run_sizes(t):
    return [t, KNB, RUN_TILES * t - 3]


def run_bucket(zk, wk, direct):
    if direct:
        return ((zk - np.uint64(MK)) >> np.uint64(wk - 10)).astype(np.int64)
    return hash_bucket(zk)


def make_runs(t, wk, wv, direct):
    def make(rng):
        ends = np.array([MK, MK + (1 << wk) - 1], dtype=np.uint64)
        cand = (MK + 1 + rng.integers(0, (1 << wk) - 2, 64 * KNB)).astype(
            np.uint64)
        cb = run_bucket(cand, wk, direct)
        first = np.full(KNB, -1, dtype=np.int64)
        first[cb[::-1]] = np.arange(len(cand))[::-1]
        assert (first >= 0).all()
        one_each = cand[first]                       # one key of every bucket
        eb = run_bucket(ends, wk, direct)
        assert eb[0] != eb[1] and RUN_HOT not in eb.tolist()
        one_each[eb] = ends
        hot = cand[cb == RUN_HOT][:4]
        cold = cand[cb != RUN_HOT][:3000]
        sizes = run_sizes(t)
        last = cold[rng.integers(0, len(cold), sizes[2])]
        last[:2] = ends     # the headers' range is the exact one: dshift = wk - 10
        k = np.concatenate([hot[rng.integers(0, len(hot), sizes[0])],
                            rng.permutation(one_each), last])
        return [(k.astype(np.uint64), None),
                (seg_values(rng, sizes, MV, wv, 64), None)]
    return make


def _cases():
    t = tile_rows()
    out = []
    for kind, (_, bits) in DISP.items():
        kw = {}
        if kind == "filter":
            kw = dict(flt=(2, 0, 4_999),
                      flt_expr=lambda: (y.col(2) >= 0).and_(y.col(2) <= 4_999))
        out.append(TileCase("disp_" + kind, make_disp(t, kind), bits,
                            DISP_SIZES(t), **kw))
    n = 2 * t + 3
    out.append(TileCase("min_in", make_top(n, 12, 31, M64), P | D | K, [n]))
    out.append(TileCase("min_out", make_top(n, 12, 31, M64 - 1), P | D | K, [n]))
    for kw_, vw in edge_widths():
        sizes = edge_sizes(t, kw_, vw)
        out.append(TileCase("edge_k%02d_v%02d" % (kw_, vw),
                            make_edge(sizes, kw_, vw), None, sizes))
    for vw in WKEY_VW:
        sizes = edge_sizes(t, WKEY_W, vw)
        out.append(WideKeyCase("wkey_k%02d_v%02d" % (WKEY_W, vw),
                               make_edge(sizes, WKEY_SPAN, vw), None, sizes))
    for mode, (wk, wv, bits) in MODES.items():
        out.append(TileCase("runs_" + mode,
                            make_runs(t, wk, wv, bool(bits & D)), bits,
                            run_sizes(t)))
    return out


DISP_IDS = ["disp_" + k for k in DISP]
MIN_IDS = ["min_in", "min_out"]
EDGE_IDS = ["edge_k%02d_v%02d" % kv for kv in edge_widths()]
WKEY_IDS = ["wkey_k%02d_v%02d" % (WKEY_W, vw) for vw in WKEY_VW]
RUN_IDS = ["runs_" + m for m in MODES]
IDS = DISP_IDS + MIN_IDS + EDGE_IDS + WKEY_IDS + RUN_IDS


@functools.lru_cache(maxsize=None)
def cases():
    """built on first use: the tile constant comes from the built library"""
    out = {c.id: c for c in _cases()}
    assert list(out) == IDS
    return out


def case_bits(case):
    cols = case.columns()
    return case.bits if case.bits is not None else predict_bits(cols[0], cols[1])


# ---- the full-scratch input: segments written wider than their span ---- #

FULL_KW, FULL_VW = 22, 42          # written widths: 64 bits per row
FULL_KSPAN, FULL_VSPAN = 21, 41    # exact span bits


def pack_fast(vals, w):
    """_pack_words for w < 64 without the per-bit expansion: 64 values fill
    w words exactly, so value j of every 64 goes to one word (and the next)"""
    n = len(vals)
    g = -(-n // 64)
    v = np.zeros(g * 64, dtype=np.uint64)
    v[:n] = vals
    v = v.reshape(g, 64)
    words = np.zeros((g, w + 1), dtype=np.uint64)
    for j in range(64):
        wi, sh = (j * w) >> 6, (j * w) & 63
        words[:, wi] |= v[:, j] << np.uint64(sh)
        if sh + w > 64:
            words[:, wi + 1] |= v[:, j] >> np.uint64(64 - sh)
    return words[:, :w].reshape(-1)[:(n * w + 63) // 64]


class WideColumn:
    """DenseColumn without nulls whose segments are all written at `width`
    bits, wider than their values need"""

    value_type = _abi.VT_INT64
    has_nulls = False
    meta_range = DenseColumn.meta_range

    def __init__(self, zz, width, max_seg=128 * 1024, sizes=None):
        zz = np.ascontiguousarray(zz, dtype=np.uint64)
        self.exact = (int(zz.min()), int(zz.max()))
        self.seg_meta, words, offs, at = [], [], [], 0
        if sizes is None:
            sizes = [min(max_seg, len(zz) - a) for a in range(0, len(zz), max_seg)]
        assert sum(sizes) == len(zz)
        for a, n in zip(np.cumsum([0] + list(sizes[:-1])), sizes):
            v = zz[a:a + n]
            mn = int(v.min())
            assert int(v.max()) - mn < 1 << width
            bm = np.zeros((len(v) + 63) // 64, dtype=np.uint64)
            seg = np.concatenate([
                np.array([len(v) | (width << 56)], dtype=np.uint64),
                pack_fast(v - np.uint64(mn), width), bm])
            self.seg_meta.append((mn, width, len(v)))
            offs.append(at)
            words.append(seg)
            at += len(seg) * 8
        blob = np.concatenate(words)
        self._buf = (C.c_uint64 * len(blob)).from_buffer_copy(blob.tobytes())
        base = C.addressof(self._buf)
        self._segs = (_abi.YtSegment * len(words))()
        for i, (mn, w, rows) in enumerate(self.seg_meta):
            self._segs[i] = _abi.YtSegment(
                type=_abi.SEG_DIRECT_DENSE, row_count=rows, min_value=mn,
                data=base + offs[i], data_size=len(words[i]) * 8)
        self._cenc = _abi.YtEncodedColumn(
            segment_count=len(words), segments=self._segs, blob=base,
            blob_size=at)
        self.segments = [self._segs[i] for i in range(len(words))]


def full_input(n):
    """-> zigzag keys over 2^21 values and values over 2^41, the ends of both
    in rows 0 and 1 of the column"""
    rng = np.random.default_rng(n)
    k = (MK + rng.integers(0, 1 << FULL_KSPAN, n)).astype(np.uint64)
    v = (MV + rng.integers(0, 1 << FULL_VSPAN, n)).astype(np.uint64)
    k[0], k[1] = MK, MK + (1 << FULL_KSPAN) - 1
    v[0], v[1] = MV, MV + (1 << FULL_VSPAN) - 1
    return k, v


def full_reference(k, v):
    """-> (keys ascending, sums, counts); float64 weights are exact while
    every sum stays below 2^53"""
    idx = (k - np.uint64(MK)).astype(np.int64)
    cnt = np.bincount(idx, minlength=1 << FULL_KSPAN)
    assert int(cnt.max()) << FULL_VSPAN < 1 << 53
    ssum = np.bincount(idx, weights=zz_dec(v).astype(np.float64),
                       minlength=1 << FULL_KSPAN).astype(np.int64)
    at = np.flatnonzero(cnt)
    keys = zz_dec((at + MK).astype(np.uint64))
    order = np.argsort(keys, kind="stable")
    return keys[order], ssum[at][order], cnt[at][order]


def full_plan():
    return y.Plan(keys=[y.col(0)], aggs=[y.agg_sum(y.col(1)), y.agg_sum1()])


def full_columns(k, v):
    return [WideColumn(k, FULL_KW), WideColumn(v, FULL_VW)]


# ------------------------------------------------------------------ #
# CPU tier                                                            #

def check_oracle(case):
    got, st = y.oracle_execute(case.plan(), case.chunk())
    want = case.rows()
    assert y.sort_rows(got) == y.sort_rows(want)
    assert st.rows_read == sum(case.sizes)
    assert st.rows_written == len(want)


@pytest.mark.parametrize("cid", DISP_IDS + MIN_IDS)
def test_dispatch_inputs_and_oracle(cid):
    case = cases()[cid]
    cols = case.columns()
    assert predict_bits(cols[0], cols[1]) == case.bits
    if cid in DISP_IDS:
        kind = cid[5:]
        assert want_variant(case) == DISP[kind][0]
        base = cases()["disp_plain"].data()
        if kind in ("knull", "vnull", "filter"):       # the same data
            for c in (0, 1):
                assert (case.data()[c][0] == base[c][0]).all()
        nulls = [0 if nu is None else int(nu.sum()) for _, nu in case.data()]
        assert nulls[:2] == [int(kind == "knull"), int(kind == "vnull")]
        kb = (cols[0].exact[1] - cols[0].exact[0]).bit_length()
        vb = (cols[1].exact[1] - cols[1].exact[0]).bit_length()
        assert (kb, vb) == {"hash": (23, 31), "rec16": (12, 62)}.get(
            kind, (12, 31))
        if kind == "filter":
            f = zz_dec(case.data()[2][0])
            assert 0.2 < ((f >= 0) & (f <= 4_999)).mean() < 0.6
    else:
        top = M64 if cid == "min_in" else M64 - 1
        assert cols[0].exact == (top - 4095, top)
        assert cols[0].meta_range() == cols[0].exact
        assert (I64_MIN in case.reference()) == (cid == "min_in")
        assert want_variant(case) == (PACKED if cid == "min_in" else PLAIN)
        if cid == "min_in":
            assert case.reference()[I64_MIN][1] > 50
    check_oracle(case)


@pytest.mark.parametrize("cid", EDGE_IDS + WKEY_IDS)
def test_edge_inputs_and_oracle(cid):
    case = cases()[cid]
    kw, vw = int(cid[6:8]), int(cid[10:12])     # written widths
    wide = cid in WKEY_IDS
    kspan = WKEY_SPAN if wide else kw
    t = tile_rows()
    sizes = case.sizes
    assert sizes[:2] == [t, t - 1] and len(sizes) == (3 if kw % 2 or vw % 2 else 2)
    cols = case.columns()
    bits = predict_bits(cols[0], cols[1])
    assert bits & K and bool(bits & D) == (kspan <= 22) and not bits & N
    assert want_variant(case) == (PLAIN if kspan <= 22 else PACKED)
    if wide:      # the headers say 23 bits, the exact key scan finds 22
        lo, hi = cols[0].meta_range()
        assert (hi - lo).bit_length() == kw == 23 and bits & KX
        assert (cols[0].exact[1] - cols[0].exact[0]).bit_length() == kspan
    for c, w, span, m in ((0, kw, kspan, MK), (1, vw, vw, MV)):
        assert cols[c].seg_meta == [(m, w, n) for n in sizes]
        z = case.data()[c][0]
        for end in np.cumsum(sizes):    # the ends in a segment's last two rows
            assert (int(z[end - 2]), int(z[end - 1])) == (m, m + (1 << span) - 1)
    # the T-row segment's last field ends with its last word; the third
    # segment's last value (or key) field one bit before it
    assert (t * kw) % 64 == 0 and (t * vw) % 64 == 0
    if len(sizes) == 3:
        assert sizes[2] <= t - 2 and sizes[2] * short_field(kw, vw) % 64 == 63
    check_oracle(case)


def test_edge_width_list():
    assert len(EDGE_IDS) == len(set(EDGE_IDS)) == 23
    assert {kw for kw, _ in edge_widths()} == set(EDGE_KW)
    for kw in EDGE_KW:
        vws = [v for k, v in edge_widths() if k == kw]
        assert 1 in vws and max(vws) == (63 if kw <= 22 else 64) - kw
    assert (1, 33) in edge_widths() and (21, 42) in edge_widths()


@pytest.mark.parametrize("cid", RUN_IDS)
def test_run_inputs_and_oracle(cid):
    case = cases()[cid]
    wk, wv, bits = MODES[cid[5:]]
    cols = case.columns()
    assert predict_bits(cols[0], cols[1]) == bits
    assert cols[0].exact == (MK, MK + (1 << wk) - 1)
    if bits & D:        # the buckets below are the kernel's: dshift = wk - 10
        assert cols[0].meta_range() == cols[0].exact
    assert want_variant(case) == {"dp": PLAIN, "hp": PACKED, "d16": 0,
                                  "h16": 0}[cid[5:]]
    t = tile_rows()
    sizes = case.sizes
    assert sizes == [t, KNB, RUN_TILES * t - 3] and sum(sizes) // t + 1 == 24
    assert (sizes[2] % t) % 2 == 1
    b = run_bucket(case.data()[0][0], wk, bool(bits & D))
    assert (b[:t] == RUN_HOT).all()
    assert (np.bincount(b[t:t + KNB], minlength=KNB) == 1).all()
    assert not (b[t + KNB:] == RUN_HOT).any()
    # grid 8: tile = segment * tiles_per_seg + tile in segment, sub = tile & 7
    per_seg = RUN_TILES
    tile = np.concatenate([s * per_seg + np.arange(n) // t
                           for s, n in enumerate(sizes)])
    per = np.bincount(b * 8 + (tile & 7), minlength=KNB * 8)
    assert per.max() <= bucket_stride(sum(sizes))
    check_oracle(case)


@pytest.mark.parametrize("w", [1, 13, 22, 42, 63])
def test_pack_fast_equals_pack_words(w):
    rng = np.random.default_rng(w)
    for n in (1, 63, 64, 65, 1000):
        v = rng.integers(0, 1 << w, n, dtype=np.uint64)
        assert (pack_fast(v, w) == _pack_words(v, w)).all()


def test_full_generator_and_reference():
    """the full-scratch generator at 2^17 rows: written widths, spans, the
    path it is built for, and the oracle against the bincount reference"""
    n = 1 << 17
    k, v = full_input(n)
    cols = full_columns(k, v)
    assert {m[1] for m in cols[0].seg_meta} == {FULL_KW}
    assert {m[1] for m in cols[1].seg_meta} == {FULL_VW}
    assert (cols[0].exact[1] - cols[0].exact[0]).bit_length() == FULL_KSPAN
    assert (cols[1].exact[1] - cols[1].exact[0]).bit_length() == FULL_VSPAN
    bits = predict_bits(cols[0], cols[1])
    assert bits & (P | D | K | KX) == P | D | K | KX and not bits & N
    # a large tile's staged words are the whole 64 KiB scratch
    assert tile_rows(True) * (FULL_KW + FULL_VW) == 8 * tile_rows(True) * 8
    keys, ssum, cnt = full_reference(k, v)
    got, st = y.oracle_execute(full_plan(), y.Chunk(cols, n))
    want = list(zip(keys.tolist(), ssum.tolist(), cnt.tolist()))
    assert y.sort_rows(got) == y.sort_rows(want)
    assert st.rows_read == n


# ------------------------------------------------------------------ #
# GPU tier                                                            #

def run_gpu(cid, cuda):
    case = cases()[cid]
    if case.bits is None:
        case.bits = case_bits(case)
    check_case(case, cuda)
    assert not last_path() & H
    assert variant() == want_variant(case)
    return case


@pytest.mark.gpu
@pytest.mark.parametrize("cid", DISP_IDS)
def test_dispatch(cid, cuda):
    run_gpu(cid, cuda)
    assert variant() == DISP[cid[5:]][0]


@pytest.mark.gpu
@pytest.mark.parametrize("cid", MIN_IDS)
def test_int64_min_boundary(cid, cuda):
    case = run_gpu(cid, cuda)
    assert variant() == (PACKED if cid == "min_in" else PLAIN)
    assert (I64_MIN in case.reference()) == (cid == "min_in")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", EDGE_IDS)
def test_window_edges(cid, cuda):
    run_gpu(cid, cuda)
    assert variant() == (PLAIN if int(cid[6:8]) <= 22 else PACKED)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", WKEY_IDS)
def test_wide_key_fields(cid, cuda):
    """23-bit key fields under the plain decode"""
    run_gpu(cid, cuda)
    assert variant() == PLAIN and last_path() & KX


@pytest.mark.gpu
@pytest.mark.parametrize("cid", RUN_IDS)
def test_copy_out_runs(cid, cuda, monkeypatch):
    monkeypatch.setenv("YTQL_GRID", "8")
    run_gpu(cid, cuda)


@pytest.mark.gpu
def test_full_scratch(cuda):
    """8192-row tiles of 64 written bits per row under the plain decode"""
    n = large_rows()
    k, v = full_input(n)
    keys, ssum, cnt = full_reference(k, v)
    cols = full_columns(k, v)
    want_bits = predict_bits(cols[0], cols[1])
    chunk = y.Chunk(cols, n)
    dev = chunk.c_device(cuda)
    g = len(keys)
    rs, st = y.gpu_execute(full_plan(), dev, max_groups_hint=1 << 21,
                           rowset=y.make_rowset(g + 16, 3), raw_rowset=True)
    assert last_path() == want_bits and want_bits & D and want_bits & K
    assert variant() == PLAIN
    assert rs.row_count == g and rs.column_count == 3
    types, data = rowset_arrays(rs, 3)
    assert (types == _abi.VT_INT64).all()
    order = np.argsort(data[:, 0], kind="stable")
    assert (data[order, 0] == keys).all()
    assert (data[order, 1] == ssum).all()
    assert (data[order, 2] == cnt).all()
    assert (st.rows_read, st.rows_written, st.grouped_row_count) == (n, g, g)
    assert st.incomplete_output == 0 and st.kernel_scan_launches == 1
