"""Phase A of the partitioned GROUP BY: the decode at every width, the null
bitmaps, the filter column, and the per-tile reservations.

k_scan_partition reserves each bucket's run with returning global adds that
are issued before the scratch fill and taken after it, on cursors laid out
[sub][bucket]; a workgroup that takes several tiles adds to the same cursors
again, and a capacity guard may trip on a later tile, after that tile's
scratch was filled. The shapes here, T = yt_gpu_debug_partition_tile_rows:

  vw01..vw64   value widths 1..64 beside a 12-bit key: direct packed up to
               51 bits, packed without the spare bit at 52, 16-byte records
               above; segments of T+1, 17, 15, 16, 1, 2T+3 and T-1 rows, so
               a 16-row group ends inside a segment, at its edge, and in a
               one-row segment. Every segment has its own min_value, and the
               widths differ by segment: the column's span in the first,
               narrower ones after it, width 1 among them
  kw01..kw40   key widths 1..40 beside a 20-bit value, the same segments:
               direct-span up to 22 bits, hash from 23
  bm_<mode>    one segment of T+1 rows; null keys and null values in patterns
               aligned to the 16-row groups: a whole group, row 0 only,
               row 15 only, alternating rows, and the last, one-row group
  flt<w>_<mode>  a third column of width 1, 13, 33, 64 under a range filter
               that keeps about half the rows (modes dp and h16)
  many_<kind>_<mode>  24 tiles under YTQL_GRID=8: every workgroup takes three
               tiles and all eight subs are used. uni: keys on all 1024
               buckets; odd: only odd buckets (and the bucket of the span's
               low end); vn: 10 % null values, the null stream's reservations
  guard_later  16 tiles of 4096 rows under YTQL_GRID=8, about 300 keys of one
               direct-span bucket: a workgroup's second tile trips the stride
               guard with its scratch filled; the hash rung finishes
               (P D K H, 2 launches, as E1 of test_partition_modes)

Every GPU case asserts rows equal to the independent reference of
test_partition_modes exactly, the path bits, and rows_read / rows_written /
grouped_row_count (check_case). The CPU twin runs the same inputs through the
oracle against that reference and asserts that the generator made the shape
its name says.
"""
import functools

import numpy as np
import pytest

import ytsaurus_amd as y

from test_partition_modes import (
    D, H, I64_MAX, K, M64, MK, MV, N, P, check_case, predict_bits, zz_dec)
from test_partition_tiles import (
    KNB, MODES, TileCase, bucket_stride, hash_bucket, seg_nulls, seg_values,
    tile_rows)


def sweep_sizes(t):
    return [t + 1, 17, 15, 16, 1, 2 * t + 3, t - 1]


def seg_widths(w):
    """the column's span in the first segment, narrower ones after it"""
    return [w, max(w - 1, 1), 1, max(w // 2, 1), 1, max(w - 2, 1),
            max(w - 1, 1)]


def ragged_values(rng, sizes, m, w, pool, balanced=False):
    """segment s at width seg_widths(w)[s] (0 for a one-row segment), its
    base 3 s above m where the column's span [m, m + 2^w - 1] has the room;
    both ends of a segment's range in its first two rows. balanced: the
    pool's values in turn, not at random, so that a narrow key column (two
    keys at width 1) puts the same share of every tile on each key and no
    record region fills"""
    top = m + (1 << w) - 1
    assert top <= M64
    out, metas = [], []
    for s, (n, ws) in enumerate(zip(sizes, seg_widths(w))):
        lo = m + min(3 * s, (1 << w) - (1 << ws)) if s else m
        hi = lo + (1 << ws) - 1
        assert m <= lo and hi <= top
        raw = rng.integers(0, M64, size=pool, dtype=np.uint64, endpoint=True)
        vals = np.array([lo + int(r) % (hi - lo + 1) for r in raw],
                        dtype=np.uint64)
        if balanced:
            vals = np.unique(vals)
            v = vals[np.arange(n) % len(vals)]
        else:
            v = vals[rng.integers(0, pool, n)]
        v[0] = lo
        if n > 1:
            v[1] = hi
        out.append(v)
        metas.append((lo, ws if n > 1 else 0, n))
    return np.concatenate(out), metas


def make_sweep(sizes, wk, wv, wf=None):
    def make(rng):
        k, _ = ragged_values(rng, sizes, MK, wk, 300, balanced=True)
        v, _ = ragged_values(rng, sizes, 0 if wv == 64 else MV, wv, 64)
        cols = [(k, None), (v, None)]
        if wf is not None:
            f, _ = ragged_values(rng, sizes, 0 if wf == 64 else 40, wf, 500)
            cols.append((f, None))
        return cols
    return make


# a group's pattern by its index: none, whole group, row 0, row 15, alternating
def group_pattern(n, phase):
    m = np.zeros(n, dtype=bool)
    for g in range(1, (n + 15) // 16):      # group 0 holds the span's two ends
        a, p = 16 * g, (g + phase) % 5
        if p == 1:
            m[a:a + 16] = True
        elif p == 2:
            m[a] = True
        elif p == 3:
            m[min(a + 15, n - 1)] = True
        elif p == 4:
            m[a:a + 16:2] = True
    m[16 * ((n - 1) // 16):] = True         # the last group
    return m


def make_bitmaps(t, wk, wv):
    def make(rng):
        n = t + 1
        k = seg_values(rng, [n], MK, wk, 300)
        v = seg_values(rng, [n], MV, wv, 64)
        return [(k, group_pattern(n, 0)), (v, group_pattern(n, 2))]
    return make


def region_counts(case, direct, wk):
    """records per (bucket, sub) region when every tile has a workgroup of
    its own: tile = segment * tiles_per_seg + tile in segment, sub = tile & 7"""
    t = tile_rows()
    per_seg = (max(case.sizes) + t - 1) // t
    tile = np.concatenate([s * per_seg + np.arange(n) // t
                           for s, n in enumerate(case.sizes)])
    b = bucket_of(case.data()[0][0], wk, direct)
    return np.bincount(b * 8 + (tile & 7), minlength=KNB * 8)


def bucket_of(zk, wk, direct):
    if direct:
        return ((zk - np.uint64(MK)) >> np.uint64(max(wk - 10, 0))).astype(
            np.int64)
    return hash_bucket(zk)


def make_many(n, wk, wv, direct, kind):
    """keys on every bucket (uni, vn) or on the odd ones (odd), the span's
    two ends in rows 0 and 1"""
    def make(rng):
        ends = np.array([MK, MK + (1 << wk) - 1], dtype=np.uint64)
        cand = (MK + 1 + rng.integers(0, (1 << wk) - 2, 64 * KNB)).astype(
            np.uint64)
        cb = bucket_of(cand, wk, direct)
        if kind == "odd":
            cand, cb = cand[cb % 2 == 1], cb[cb % 2 == 1]
        first = np.full(KNB, -1, dtype=np.int64)
        first[cb[::-1]] = np.arange(len(cand))[::-1]
        seed = cand[first[first >= 0]]      # one key of every wanted bucket
        pool = np.concatenate([seed, cand[:2000]])
        k = pool[rng.integers(0, len(pool), n)]
        k[:len(seed) + 2] = np.concatenate([ends, seed])
        v = seg_values(rng, [n], MV, wv, 64)
        vn = seg_nulls(rng, [n], 0.1) if kind == "vn" else None
        return [(k, None), (v, vn)]
    return make


GUARD_ROWS, GUARD_WK, GUARD_HOT = 16 * 4096, 20, 512


def make_guard(rng):
    n = GUARD_ROWS
    hot = (GUARD_HOT << 10) + rng.permutation(1024)[:300]
    k = hot[rng.integers(0, 300, n)].astype(np.uint64)
    k[0], k[1] = 0, (1 << GUARD_WK) - 1
    v = seg_values(rng, [n], 777, 31, 64)
    return [(k, None), (v, None)]


def _half_filter():
    return (y.col(2) >= 0).and_(y.col(2) <= I64_MAX)


MANY_TILES = 24
FLT_WIDTHS = (1, 13, 33, 64)


def _cases():
    t = tile_rows()
    sizes = sweep_sizes(t)
    out = []
    for wv in range(1, 65):
        out.append(TileCase("vw%02d" % wv, make_sweep(sizes, 12, wv), None,
                            sizes))
    for wk in range(1, 41):
        out.append(TileCase("kw%02d" % wk, make_sweep(sizes, wk, 20), None,
                            sizes))
    for mode, (wk, wv, bits) in MODES.items():
        out.append(TileCase("bm_" + mode, make_bitmaps(t, wk, wv), bits | N,
                            [t + 1]))
    for wf in FLT_WIDTHS:
        for mode in ("dp", "h16"):
            wk, wv, bits = MODES[mode]
            out.append(TileCase("flt%02d_%s" % (wf, mode),
                                make_sweep(sizes, wk, wv, wf), bits, sizes,
                                flt=(2, 0, I64_MAX), flt_expr=_half_filter))
    for kind in ("uni", "odd", "vn"):
        for mode, (wk, wv, bits) in MODES.items():
            n = MANY_TILES * t
            out.append(TileCase(
                "many_%s_%s" % (kind, mode),
                make_many(n, wk, wv, bool(bits & D), kind),
                bits | (N if kind == "vn" else 0), [n]))
    out.append(TileCase("guard_later", make_guard, P | D | K | H,
                        [GUARD_ROWS], launches=2, model=False))
    return out


WIDTH_IDS = (["vw%02d" % w for w in range(1, 65)]
             + ["kw%02d" % w for w in range(1, 41)])
BM_IDS = ["bm_" + m for m in MODES]
FLT_IDS = ["flt%02d_%s" % (w, m) for w in FLT_WIDTHS for m in ("dp", "h16")]
MANY_IDS = ["many_%s_%s" % (k, m) for k in ("uni", "odd", "vn") for m in MODES]
IDS = WIDTH_IDS + BM_IDS + FLT_IDS + MANY_IDS + ["guard_later"]


@functools.lru_cache(maxsize=None)
def cases():
    """built on first use: the tile constant comes from the built library"""
    out = {c.id: c for c in _cases()}
    assert list(out) == IDS
    return out


def want_bits(case):
    cols = case.columns()
    return case.bits if case.bits is not None else predict_bits(cols[0], cols[1])


# ------------------------------------------------------------------ #
# CPU tier                                                            #

def check_oracle(case):
    got, st = y.oracle_execute(case.plan(), case.chunk())
    want = case.rows()
    assert y.sort_rows(got) == y.sort_rows(want)
    assert st.rows_read == sum(case.sizes)
    assert st.rows_written == len(want)


@pytest.mark.parametrize("cid", WIDTH_IDS + FLT_IDS)
def test_sweep_inputs_and_oracle(cid):
    case = cases()[cid]
    cols = case.columns()
    t = tile_rows()
    assert case.sizes == [t + 1, 17, 15, 16, 1, 2 * t + 3, t - 1]
    if cid.startswith("flt"):
        wk, wv, bits = MODES[cid[6:]]
        swept = [(2, int(cid[3:5]))]
        assert predict_bits(cols[0], cols[1]) == bits
        f = zz_dec(case.data()[2][0])
        assert 0.4 < (f >= 0).mean() < 0.6
    else:
        w = int(cid[2:])
        wk, wv = (12, w) if cid[0] == "v" else (w, 20)
        swept = [(0, wk), (1, wv)]
        bits = predict_bits(cols[0], cols[1])
        assert bits & P
        assert bool(bits & D) == (wk <= 22 and (wk + wv <= 63 or wk + wv > 64))
        assert bool(bits & K) == (wk + wv <= 64)
        # no region fills: the guard stays quiet, no hash retry
        per = region_counts(case, bool(bits & D), wk)
        assert per.max() <= bucket_stride(sum(case.sizes))
    for c, w in swept:
        meta = cols[c].seg_meta
        assert [m[2] for m in meta] == case.sizes
        want_w = [ws if n > 1 else 0 for ws, n in zip(seg_widths(w), case.sizes)]
        assert [m[1] for m in meta] == want_w
        lo, hi = cols[c].meta_range()
        assert (hi - lo).bit_length() == w and cols[c].exact == (lo, hi)
        if w >= 6:
            assert len({m[0] for m in meta}) == len(meta)
        if w > 1:
            assert 1 in want_w and len(set(want_w)) >= 3
    check_oracle(case)


@pytest.mark.parametrize("cid", BM_IDS)
def test_bitmap_inputs_and_oracle(cid):
    case = cases()[cid]
    cols = case.columns()
    assert predict_bits(cols[0], cols[1]) == case.bits
    n = case.sizes[0]
    assert n == tile_rows() + 1
    for c in (0, 1):
        nu = case.data()[c][1]
        g = nu[:16 * (n // 16)].reshape(-1, 16)
        assert g.all(axis=1).any()                               # a whole group
        assert (g[:, 0] & (g.sum(axis=1) == 1)).any()            # row 0 only
        assert (g[:, 15] & (g.sum(axis=1) == 1)).any()           # row 15 only
        alt = np.arange(16) % 2 == 0
        assert (g == alt).all(axis=1).any()                      # alternating
        assert n % 16 == 1 and nu[n - 1]                         # the one-row group
        assert not nu[:2].any()
    kn, vn = case.data()[0][1], case.data()[1][1]
    assert (kn & vn).any() and (kn & ~vn).any() and (~kn & vn).any()
    check_oracle(case)


@pytest.mark.parametrize("cid", MANY_IDS)
def test_many_inputs_and_oracle(cid):
    case = cases()[cid]
    _, kind, mode = cid.split("_")
    wk, wv, bits = MODES[mode]
    cols = case.columns()
    assert predict_bits(cols[0], cols[1]) == case.bits
    t = tile_rows()
    assert case.sizes == [MANY_TILES * t] and bucket_stride(case.sizes[0]) < 2 * t
    zk = case.data()[0][0]
    b = bucket_of(zk, wk, bool(bits & D))
    # the first tile alone reaches every wanted bucket
    cnt = np.bincount(b[:t], minlength=KNB)
    if kind == "odd":
        assert (cnt[1::2] > 0).all()
        assert set(np.flatnonzero(cnt[0::2]) * 2) <= set(b[:2].tolist())
    else:
        assert (cnt > 0).all()
    if kind == "vn":
        assert 0.05 < case.data()[1][1].mean() < 0.15
    # no region fills: the guard stays quiet, no hash retry
    tile = np.arange(len(zk)) // t
    per = np.bincount(b * 8 + (tile & 7), minlength=KNB * 8)
    assert per.max() <= bucket_stride(case.sizes[0])
    check_oracle(case)


def test_guard_inputs_and_oracle():
    case = cases()["guard_later"]
    zk = case.data()[0][0]
    n = len(zk)
    assert n == GUARD_ROWS and tile_rows() == 4096
    stride = bucket_stride(n)
    assert zk[0] == 0 and zk[1] == (1 << GUARD_WK) - 1
    assert 250 < len(np.unique(zk)) <= 302
    tile = np.arange(n) // 4096
    sub = tile & 7
    db = (zk >> np.uint64(GUARD_WK - 10)).astype(np.int64)
    assert set(db.tolist()) == {0, GUARD_HOT, KNB - 1}
    hot = np.bincount(sub[db == GUARD_HOT], minlength=8)
    # a sub's first tile fits its region, its second one does not
    first = np.bincount(sub[(db == GUARD_HOT) & (tile < 8)], minlength=8)
    assert (first <= stride).all() and (hot > stride).all()
    per = np.bincount(hash_bucket(zk) * 8 + sub, minlength=KNB * 8)
    assert per.max() <= stride
    cols = case.columns()
    assert predict_bits(cols[0], cols[1]) == P | D | K
    check_oracle(case)


# ------------------------------------------------------------------ #
# GPU tier                                                            #

def run_gpu(cid, cuda):
    case = cases()[cid]
    if case.bits is None:
        case.bits = want_bits(case)
    _, st = check_case(case, cuda)
    return case, st


@pytest.mark.gpu
@pytest.mark.parametrize("cid", WIDTH_IDS)
def test_width_sweep(cid, cuda):
    run_gpu(cid, cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", BM_IDS)
def test_null_bitmaps(cid, cuda):
    case, _ = run_gpu(cid, cuda)
    assert None in case.reference()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", FLT_IDS)
def test_filter_widths(cid, cuda):
    run_gpu(cid, cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", MANY_IDS)
def test_many_tiles_per_workgroup(cid, cuda, monkeypatch):
    monkeypatch.setenv("YTQL_GRID", "8")
    _, st = run_gpu(cid, cuda)
    assert st.kernel_scan_launches == 1


@pytest.mark.gpu
def test_guard_on_a_later_tile(cuda, monkeypatch):
    """P D K H and two launches: the direct-span rung tripped its guard"""
    monkeypatch.setenv("YTQL_GRID", "8")
    run_gpu("guard_later", cuda)
