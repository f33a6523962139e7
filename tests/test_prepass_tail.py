"""The pre-pass and the host tail around the partitioned GROUP BY's two
kernels: the exact range scan (k_scan_zzrange, which streams the packed words
and takes every value from registers), the 32-byte group records that phase B
writes when the whole query runs in one call, and their sliced copy with the
row emit running behind it.

Every case has one int64 key, sum(v) and / or sum(1), and asserts exact rows
against the independent reference of test_partition_modes.py, exact
yt_gpu_debug_last_scan_path() bits and exact counters. As there, every
generator also has an unmarked CPU test that runs it through the oracle
against the reference and checks the path bits it was built for with
predict_bits, so the inputs are proven without a GPU.

Exact range scan. The scan's result decides the record format, so a wrong one
shows twice: a maximum too wide changes the asserted bits, one too narrow (or
a minimum too high) also corrupts the packed records and with them the rows.

  key flip    packed key width w in {2, 7, 21, 22}: segment 1 lacks the
              column minimum, its meta bound overshoots (w + 1 bits), KX runs
              and brings the span back to w bits. At w = 1 a segment that
              lacks the minimum is one value wide (width 0, no overshoot) and
              at w = 23 an overshoot gives 24 meta bits, where KX does not
              run; those two keep meta = exact with bv chosen so that KX runs
              and one more bit would change the bits.
  value flip  value width w in {24, 32, 33, 40, 41, 63}: the same through VX,
              with bk = 63 - w and 64 - w (64 and 65 bits by meta); w = 64
              cannot overshoot (the bound is clamped) and runs meta = exact
              with bk = 0 and 1.
  position    w = 21 (key, KX) and w = 33 (value, VX): the column's only
              maximum, or only minimum, sits in one row: row 0, the last
              row, a row whose bits straddle a 64-bit word, a row in the
              final partial word. Segment lengths 1, 63, 64, 65, 2003 and
              5000 in one column. The CPU tier shows that a scan blind to
              that row would give other bits.
  nulls       null rows carry all-ones packed bits (RaggedColumn writes them
              so), which exceed every real value: a scan that ignores the
              bitmap reports one bit more. One column is null in every row.

Slim records and the sliced tail: ngroups in {65,535, 65,536, 65,537,
200,003} on either side of emit_rows' worker threshold, with and without the
two side groups (an INT64_MIN key and null keys), with and without the sum,
one group whose values are all null; rowset capacity exact and one short;
output_row_limit below ngroups.

Other paths: gpu_partial + gpu_merge on 65,537 groups (the partial path
consumes OutGroups), and the fallback ladder of test_partition_modes.py (E1:
hash retry; E2: both rungs overflow and k_compact's OutGroups emit).
"""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import ytsaurus_amd as y
from ytsaurus_amd import _abi

from test_partition_modes import (
    DenseColumn, zz_column, null_mask, reference_groupby_np, reference_rows,
    predict_bits, last_path)
from test_partition_modes import (
    Case, E1, E2, check_case, np_reference_as_dict, rowset_arrays, two_cols,
    zz_dec, _pack_words, P, D, K, N, KX, VX, M64, MK, MV, N_ROWS, SEG)


def ids(cases):
    return [c.id for c in cases]


# ------------------------------------------------------------------ #
# a DirectDense writer with chosen segment lengths and null bits      #

class RaggedColumn(DenseColumn):
    """DenseColumn with a list of segment lengths in place of one maximum,
    and the packed bits of null rows all ones (DenseColumn writes zeros; the
    reader must not look at them either way)."""

    def __init__(self, zz, nulls, lens):
        zz = np.ascontiguousarray(zz, dtype=np.uint64)
        n = len(zz)
        assert sum(lens) == n
        nulls = (np.zeros(n, dtype=bool) if nulls is None
                 else np.asarray(nulls, dtype=bool))
        self.has_nulls = bool(nulls.any())
        live = zz[~nulls]
        self.exact = (int(live.min()), int(live.max())) if len(live) else None
        self.seg_meta = []
        words, offs = [], []
        at = a = 0
        for ln in lens:
            v, nu = zz[a:a + ln], nulls[a:a + ln]
            a += ln
            if (~nu).any():
                mn = int(v[~nu].min())
                w = (int(v[~nu].max()) - mn).bit_length()
                ones = np.uint64(M64 if w == 64 else (1 << w) - 1)
                rel = np.where(nu, ones, v - np.uint64(mn))
            else:
                mn, w = M64, 1
                rel = np.ones(len(v), dtype=np.uint64)
            bm = np.packbits(nu.astype(np.uint8), bitorder="little")
            bm = np.concatenate([bm, np.zeros((-len(bm)) % 8, np.uint8)])
            seg = np.concatenate([
                np.array([len(v) | (w << 56)], dtype=np.uint64),
                _pack_words(rel, w), bm.view("<u8")])
            self.seg_meta.append((mn, w, len(v)))
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


def even_lens(n, seg):
    return [min(seg, n - a) for a in range(0, n, seg)]


class RCase(Case):
    """a Case whose columns RaggedColumn writes (lens: segment lengths)"""

    def __init__(self, cid, make, bits, lens=None, **kw):
        Case.__init__(self, cid, make, bits, **kw)
        self.lens = lens

    def columns(self):
        return [RaggedColumn(z, nu, self.lens or even_lens(len(z), self.seg))
                for z, nu in self.data()]


def test_ragged_writer_decodes_through_oracle():
    """lengths 1 .. 5000 in one column, null rows written as all-ones"""
    rng = np.random.default_rng(3)
    lens = [1, 63, 64, 65, 2003, 5000]
    n = sum(lens)
    for w in (1, 21, 33, 64):
        zz = zz_column(rng, n, 0 if w == 64 else MK, w, seg=0)
        nulls = rng.random(n) < 0.2
        col = RaggedColumn(zz, nulls, lens)
        colc = _abi.YtColumn(value_type=col.value_type,
                             segment_count=col._cenc.segment_count,
                             segments=col._cenc.segments)
        vals = np.zeros(n, dtype=np.int64)
        nu = np.zeros(n, dtype=np.uint8)
        rc = _abi.oracle_lib().yto_decode_column(
            C.byref(colc), n, vals.ctypes.data_as(C.POINTER(C.c_int64)),
            nu.ctypes.data_as(C.POINTER(C.c_uint8)))
        assert rc == 0
        assert (nu.astype(bool) == nulls).all()
        assert (vals[~nulls] == zz_dec(zz)[~nulls]).all()
        assert [m[2] for m in col.seg_meta] == lens


# ------------------------------------------------------------------ #
# exact range scan: flip cases                                        #

KEY_FLIP = [
    # w = 1: meta = exact, 1 + 63 = 64 (one bit more: 65, not packed)
    Case("kf_w01", two_cols(MK, 1, MV, 63), P | K | KX | VX),
    # meta w + 1 with bv = 63 - w: 64 by meta, 63 after the scan
    Case("kf_w02", two_cols(MK, 2, MV, 61, klacks=(1,)), P | D | K | KX),
    Case("kf_w07", two_cols(MK, 7, MV, 56, klacks=(1,)), P | D | K | KX),
    Case("kf_w21", two_cols(MK, 21, MV, 42, klacks=(1,)), P | D | K | KX),
    # 23 meta bits: KX runs whatever bv is; 22 + 41 = 63 after the scan
    Case("kf_w22", two_cols(MK, 22, MV, 41, klacks=(1,)), P | D | K | KX),
    # w = 23: meta = exact, 23 + 41 = 64 (one bit more: 65, not packed)
    Case("kf_w23", two_cols(MK, 23, MV, 41), P | K | KX | VX),
]


def _val_flip():
    out = []
    # 32 is the scan's last width with 32-bit values, 33 its first with 64
    for w in (24, 32, 33, 40, 41, 63):
        for bk in (63 - w, 64 - w):
            bits = P | K | VX           # 63 or 64 bits after the scan
            if 1 <= bk <= 23:
                bits |= KX              # bk + bv >= 64 by meta
            if bk <= 22 and max(bk, 1) + w <= 63:
                bits |= D
            out.append(Case("vf_w%02d_k%02d" % (w, bk),
                            two_cols(MK, bk, MV, w, vlacks=(2,)), bits))
    out.append(Case("vf_w64_k00", two_cols(MK, 0, 0, 64), P | K | VX))
    out.append(Case("vf_w64_k01", two_cols(MK, 1, 0, 64), P | D | KX | VX))
    return out


VAL_FLIP = _val_flip()


def test_flip_cases_overshoot():
    """meta span = exact span + 1 bit, except where the docstring says why
    not; widths as named"""
    for case in KEY_FLIP + VAL_FLIP:
        k, v = case.columns()
        col = k if case.id.startswith("kf") else v
        w = int(case.id[4:6])
        ex = (col.exact[1] - col.exact[0]).bit_length()
        lo, hi = col.meta_range()
        assert ex == w, case.id
        assert {m[1] for m in col.seg_meta} == {w}, case.id
        same = case.id in ("kf_w01", "kf_w23", "vf_w64_k00", "vf_w64_k01")
        assert (hi - lo).bit_length() == (w if same else w + 1), case.id


# ------------------------------------------------------------------ #
# exact range scan: position cases                                    #

POS_LENS = [1, 63, 64, 65, 2003, 5000]
POS_N = sum(POS_LENS)
POS_START = dict(zip(POS_LENS, np.cumsum([0] + POS_LENS[:-1]).tolist()))


def pos_row(where, w):
    """(segment length, row in segment) of the one extreme row"""
    if where == "first":
        return 5000, 0
    if where == "last":
        return 5000, 4999
    if where == "straddle":
        # past the first 256 words, bits on both sides of a word boundary
        r = next(r for r in range(1500, 5000) if (r * w) % 64 + w > 64)
        return 5000, r
    # the first row with bits in the last, partial word of its segment that
    # is not the segment's last row (w = 21: row 4998 of 5000; w = 33: row
    # 2001 of 2003)
    for seglen in (2003, 5000):
        assert (seglen * w) % 64 != 0
        last_word = (seglen * w - 1) >> 6
        r = next(r for r in range(seglen)
                 if ((r + 1) * w - 1) >> 6 == last_word)
        if r != seglen - 1:
            return seglen, r
    raise AssertionError(w)


def pos_other(rng, lo, w, pool):
    """the column beside the scanned one: both ends of [lo, lo + 2^w - 1] in
    rows 0 and 1 of every segment that has two rows, so meta = exact"""
    x = zz_column(rng, POS_N, lo, w, seg=0, pool=pool)
    for ln in POS_LENS[1:]:
        x[POS_START[ln]], x[POS_START[ln] + 1] = lo, lo + (1 << w) - 1
    return x


def pos_cols(w, which, where, scanned):
    """the scanned column's values lie in the second quarter of
    [m, m + 2^w - 1] (which = max) or in its third quarter (min), except ONE
    row that holds m + 2^w - 1 (max) or m (min), and rows 10 and 11 of that
    row's segment, which hold the span's other end. Meta = exact = w bits;
    without the one row the exact span has w - 1 bits or fewer."""
    def make(rng):
        m = MK
        lo_mid, hi_mid = m + (1 << (w - 2)), m + (1 << (w - 1)) - 1
        x = (lo_mid + rng.integers(0, hi_mid - lo_mid + 1, POS_N)
             ).astype(np.uint64)
        if which == "max":
            other_end, ext = m, m + (1 << w) - 1
        else:
            x += np.uint64(1 << (w - 2))
            other_end, ext = m + (1 << w) - 1, m
        seglen, r = pos_row(where, w)
        assert r not in (10, 11)
        x[POS_START[seglen] + 10] = other_end
        x[POS_START[seglen] + 11] = other_end
        x[POS_START[seglen] + r] = ext
        if scanned == "key":
            # 21 + 43 = 64: KX and VX run, packed, no direct-span
            return [(x, None), (pos_other(rng, MV, 43, 64), None)]
        # 32 + 33 = 65: VX runs, 16-byte records
        return [(pos_other(rng, MK, 32, 300), None), (x, None)]
    return make


def _pos_cases():
    out = []
    for which in ("max", "min"):
        for where in ("first", "last", "straddle", "partial"):
            # key at 21 bits beside 43: 64, packed, no direct-span
            out.append(RCase("pos_k21_%s_%s" % (which, where),
                             pos_cols(21, which, where, "key"),
                             P | K | KX | VX, lens=POS_LENS))
            # value at 33 bits beside 32: 65, 16-byte records
            out.append(RCase("pos_v33_%s_%s" % (which, where),
                             pos_cols(33, which, where, "val"),
                             P | VX, lens=POS_LENS))
    return out


POS_CASES = _pos_cases()


@pytest.mark.parametrize("case", POS_CASES, ids=ids(POS_CASES))
def test_position_cases_hinge_on_one_row(case):
    """the extreme is in exactly one row, where the name says, and a scan
    that missed that row would choose other bits"""
    cols = case.columns()
    scanned = 0 if "_k21_" in case.id else 1
    w = 21 if scanned == 0 else 33
    col = cols[scanned]
    zz = case.data()[scanned][0]
    which, where = case.id.split("_")[2:4]
    ext = col.exact[1] if which == "max" else col.exact[0]
    at = np.flatnonzero(zz == np.uint64(ext))
    seglen, r = pos_row(where, w)
    assert at.tolist() == [POS_START[seglen] + r]
    assert (col.exact[1] - col.exact[0]).bit_length() == w
    assert col.seg_meta[POS_LENS.index(seglen)][1] == w
    assert col.seg_meta[0][1:] == (0, 1)          # one row: width 0
    if where == "straddle":
        assert (r * w) // 64 != ((r + 1) * w - 1) // 64 and (r * w) // 64 > 256
    if where == "partial":
        assert r != seglen - 1
    rest = np.delete(zz, at)
    col.exact = (int(rest.min()), int(rest.max()))
    blind = predict_bits(cols[0], cols[1])
    assert blind != case.bits


# ------------------------------------------------------------------ #
# exact range scan: null cases                                        #

def null_ones_cols(w, scanned):
    """even segments hold [m, m + 2^(w-1)], odd ones [m + 2^(w-1) - 1,
    m + 2^w - 1]: all of width w, exact span w bits, meta w + 1. 30 % of the
    rows are null, written as all-ones: in an odd segment that decodes to
    m + 2^(w-1) - 1 + 2^w - 1, a (w + 1)-bit span."""
    def make(rng):
        n, half = N_ROWS, 1 << (w - 1)
        x = np.empty(n, dtype=np.uint64)
        for s, a in enumerate(range(0, n, SEG)):
            b = min(a + SEG, n)
            lo = MK if s % 2 == 0 else MK + half - 1
            x[a:b] = (lo + rng.integers(0, half + 1, b - a)).astype(np.uint64)
            x[a], x[a + 1] = lo, lo + half
        xn = null_mask(rng, n, 0.3)
        if scanned == "key":
            return [(x, xn), (zz_column(rng, n, MV, 42), None)]   # 22 + 42
        return [(zz_column(rng, n, MK, 31, pool=300), None), (x, xn)]  # 31 + 34
    return make


def all_null_value(rng):
    """a 64-bit key span beside a value column that is null in every row:
    VX runs (64 + 0) over a column with nothing to find"""
    cols = two_cols(0, 64, MV, 20, ktop=M64, vnulls=1.0)(rng)
    return cols


NULL_CASES = [
    RCase("nul_k21", null_ones_cols(21, "key"), P | D | K | KX),
    RCase("nul_v33", null_ones_cols(33, "val"), P | K | VX | N),
    RCase("nul_all", all_null_value, P | VX | N),
]


def test_null_cases_all_ones_exceed_the_span():
    """read without the bitmap, the null rows of nul_k21 / nul_v33 widen the
    span by one bit and the bits change; nul_all has no value at all"""
    for case, scanned, w in ((NULL_CASES[0], 0, 21), (NULL_CASES[1], 1, 33)):
        cols = case.columns()
        col = cols[scanned]
        assert {m[1] for m in col.seg_meta} == {w}
        assert (col.exact[1] - col.exact[0]).bit_length() == w
        widest = max(mn + (1 << wd) - 1 for mn, wd, _ in col.seg_meta)
        col.exact = (col.exact[0], widest)      # what all-ones decode to
        assert predict_bits(cols[0], cols[1]) != case.bits
    k, v = NULL_CASES[2].columns()
    assert v.exact is None and v.has_nulls
    assert (k.meta_range()[1] - k.meta_range()[0]).bit_length() == 64


SCAN_CASES = KEY_FLIP + VAL_FLIP + POS_CASES + NULL_CASES


@pytest.mark.parametrize("case", SCAN_CASES, ids=ids(SCAN_CASES))
def test_scan_cases_oracle_and_cell(case):
    got, st = y.oracle_execute(case.plan(), case.chunk())
    want = case.rows()
    assert y.sort_rows(got) == y.sort_rows(want)
    assert st.rows_read == len(case.data()[0][0])
    assert st.rows_written == len(want)
    cols = case.columns()
    assert predict_bits(cols[0], cols[1]) == case.bits, case.id


@pytest.mark.gpu
@pytest.mark.parametrize("case", SCAN_CASES, ids=ids(SCAN_CASES))
def test_exact_range_scan(case, cuda):
    check_case(case, cuda)


# ------------------------------------------------------------------ #
# slim records and the sliced tail                                    #

NGROUPS = [65_535, 65_536, 65_537, 200_003]
I64_MIN = -(1 << 63)


class TailInput:
    """ngroups distinct keys, each in one to a few rows (1.5 rows per key);
    group `null_sum_key` has only null values. sides: three rows with the
    key INT64_MIN (zigzag 2^64 - 1: the partitioned path's sentinel, a side
    slot) and 1 % null keys (the other side slot)."""

    def __init__(self, ngroups, sides):
        self.ngroups, self.sides = ngroups, sides
        self.id = "g%d_%s" % (ngroups, "sides" if sides else "plain")

    def __repr__(self):
        return self.id

    @functools.lru_cache(maxsize=None)
    def data(self):
        rng = np.random.default_rng(zlib.crc32(self.id.encode()))
        g = self.ngroups
        n = g + g // 2
        keys = (MK + np.arange(g)).astype(np.uint64)
        k = rng.permutation(np.concatenate(
            [keys, keys[rng.integers(0, g, n - g)]]))
        v = zz_column(rng, n, MV, 31, seg=0)
        vn = rng.random(n) < 0.05
        vn[k == keys[7]] = True
        kn = None
        if self.sides:
            kn = rng.random(n) < 0.01
            # the plain groups must all survive the null keys
            first = np.unique(k, return_index=True)[1]
            kn[first] = False
            k = np.concatenate([k, np.full(3, M64, dtype=np.uint64)])
            kn = np.concatenate([kn, np.zeros(3, dtype=bool)])
            v = np.concatenate([v, v[:3]])
            vn = np.concatenate([vn, np.array([False, True, False])])
        return [(k, kn), (v, vn)]

    @functools.lru_cache(maxsize=None)
    def columns(self):
        return [DenseColumn(z, nu) for z, nu in self.data()]

    def chunk(self):
        return y.Chunk(list(self.columns()), len(self.data()[0][0]))

    def decoded(self):
        return [(zz_dec(z), nu) for z, nu in self.data()]

    @functools.lru_cache(maxsize=None)
    def reference(self):
        """(keys ascending, sums, non-null counts, counts, null group)"""
        ukeys, ssum, snn, cnt, nullgrp = reference_groupby_np(
            self.decoded(), 0, [1])
        return ukeys, ssum[0], snn[0], cnt, nullgrp

    def total(self):
        return len(self.reference()[0]) + (self.reference()[4] is not None)

    def null_sum_key(self):
        return int(zz_dec([MK + 7])[0])

    def bits(self, with_sum):
        if self.sides:      # 64-bit key span: hash, 16-byte beside a sum
            return (P | N) if with_sum else (P | K)
        return (P | D | K | N) if with_sum else (P | D | K)


TAIL_INPUTS = [TailInput(g, s) for g in NGROUPS for s in (False, True)]


def tail_plan(with_sum):
    aggs = ([y.agg_sum(y.col(1))] if with_sum else []) + [y.agg_sum1()]
    return y.Plan(keys=[y.col(0)], aggs=aggs)


@pytest.mark.parametrize("inp", TAIL_INPUTS, ids=ids(TAIL_INPUTS))
def test_tail_inputs_oracle_and_cell(inp):
    ukeys, ssum, snn, cnt, nullgrp = inp.reference()
    assert len(ukeys) == inp.ngroups + (1 if inp.sides else 0)
    assert (nullgrp is not None) == inp.sides
    if inp.sides:
        assert ukeys[0] == I64_MIN and cnt[0] == 3
    at = int(np.searchsorted(ukeys, inp.null_sum_key()))
    assert ukeys[at] == inp.null_sum_key() and snn[at] == 0 and cnt[at] >= 1
    k, v = inp.columns()
    assert predict_bits(k, v) == inp.bits(True)
    assert predict_bits(k, None) == inp.bits(False)
    got, st = y.oracle_execute(tail_plan(True), inp.chunk())
    ref = np_reference_as_dict(reference_groupby_np(inp.decoded(), 0, [1]))
    assert y.sort_rows(got) == y.sort_rows(reference_rows(ref, 1, True))
    assert st.rows_written == inp.total()


def check_tail_rows(inp, with_sum, rs, complete=True):
    """rows of the raw rowset against the reference, keyed by group key"""
    ukeys, ssum, snn, cnt, nullgrp = inp.reference()
    ncols = 3 if with_sum else 2
    assert rs.column_count == ncols
    types, data = rowset_arrays(rs, ncols)
    isnull = types[:, 0] == _abi.VT_NULL
    assert (types[~isnull, 0] == _abi.VT_INT64).all()
    assert (types[:, ncols - 1] == _abi.VT_INT64).all()
    keys = data[~isnull, 0]
    order = np.argsort(keys, kind="stable")
    keys = keys[order]
    if complete:
        assert len(keys) == len(ukeys) and (keys == ukeys).all()
        assert int(isnull.sum()) == (nullgrp is not None)
    at = np.searchsorted(ukeys, keys)
    assert (at < len(ukeys)).all() and (ukeys[at] == keys).all()
    assert len(np.unique(keys)) == len(keys)
    assert (data[~isnull, ncols - 1][order] == cnt[at]).all()
    if with_sum:
        st, sd = types[~isnull, 1][order], data[~isnull, 1][order]
        has = snn[at] > 0
        assert (st[has] == _abi.VT_INT64).all() and (sd[has] == ssum[at][has]).all()
        assert (st[~has] == _abi.VT_NULL).all()
        assert not has[keys == inp.null_sum_key()].any()
    for row_t, row_d in zip(types[isnull], data[isnull]):
        sums, nns, c = nullgrp
        assert row_d[ncols - 1] == c
        if with_sum:
            want = np.uint64(sums[0]).astype(np.int64) if nns[0] else None
            assert (row_d[1] if row_t[1] == _abi.VT_INT64 else None) == want


@pytest.mark.gpu
@pytest.mark.parametrize("with_sum", [True, False], ids=["sum_cnt", "cnt"])
@pytest.mark.parametrize("inp", TAIL_INPUTS, ids=ids(TAIL_INPUTS))
def test_slim_records_and_sliced_tail(inp, with_sum, cuda):
    chunk = inp.chunk()         # owns the device tensors behind `dev`
    dev = chunk.c_device(cuda)
    plan = tail_plan(with_sum)
    n = len(inp.data()[0][0])
    total = inp.total()
    ncols = 3 if with_sum else 2
    hint = 1 << 18

    # capacity exactly groups + sides
    rs, st = y.gpu_execute(plan, dev, max_groups_hint=hint,
                           rowset=y.make_rowset(total, ncols), raw_rowset=True)
    assert last_path() == inp.bits(with_sum)
    assert rs.row_count == total
    assert (st.rows_read, st.rows_written, st.grouped_row_count) == (
        n, total, total)
    assert st.incomplete_output == 0
    check_tail_rows(inp, with_sum, rs)

    # one row short
    with pytest.raises(RuntimeError) as e:
        y.gpu_execute(plan, dev, max_groups_hint=hint,
                      rowset=y.make_rowset(total - 1, ncols), raw_rowset=True)
    assert "ytql error %d" % _abi.YT_ERR_CAPACITY in str(e.value)

    # output_row_limit below ngroups: the serial path, flagged incomplete
    limit = inp.ngroups - 5
    rs, st = y.gpu_execute(plan, dev, max_groups_hint=hint,
                           rowset=y.make_rowset(total, ncols), raw_rowset=True,
                           output_row_limit=limit)
    assert rs.row_count == limit
    assert (st.rows_written, st.grouped_row_count) == (limit, total)
    assert st.incomplete_output == 1
    check_tail_rows(inp, with_sum, rs, complete=False)


# ------------------------------------------------------------------ #
# other paths                                                         #

@pytest.mark.gpu
def test_partial_and_merge_keep_outgroups(cuda):
    """gpu_partial feeds the partitioned path's groups to the partition
    kernels as OutGroups: 65,537 groups through partial + merge"""
    inp = TAIL_INPUTS[NGROUPS.index(65_537) * 2]
    assert not inp.sides
    chunk = inp.chunk()
    dev = chunk.c_device(cuda)
    plan = tail_plan(True)
    cap = inp.ngroups + 1024
    states_t = cuda.zeros((cap, 4), dtype=cuda.int64, device="cuda")
    counts, _ = y.gpu_partial(plan, dev, 1, states_t.data_ptr(), cap,
                              max_groups_hint=1 << 18)
    assert last_path() == inp.bits(True)
    assert sum(counts) == inp.ngroups
    rs, st = y.gpu_merge(plan, states_t.data_ptr(), sum(counts),
                         max_groups_hint=1 << 18,
                         rowset=y.make_rowset(cap, 3), raw_rowset=True)
    assert rs.row_count == inp.ngroups
    check_tail_rows(inp, True, rs)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [E1, E2], ids=ids([E1, E2]))
def test_fallback_ladder_still_emits(case, cuda):
    """E1: the direct-span rung trips its guard and the hash retry's slim
    records emit; E2: both rungs overflow, k_scan_fast finishes and
    k_compact's OutGroups emit"""
    check_case(case, cuda)
