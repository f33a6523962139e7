"""Phase B of the partitioned GROUP BY at its loop and flush edges.

k_bucket_agg_direct streams each of a bucket's eight sub-regions in full
passes of eight 16-byte loads per lane (P = yt_gpu_debug_bucket_pass_records()
packed 8-byte records; the hash kernel's full pass is P / 2 records), then in
turns of one load per lane, then the odd last record. Both phase-B kernels
flush through one routine: ranks from ballot and popcount, one reservation
per workgroup, stores by rank.

Inputs are segments of exactly yt_gpu_debug_partition_tile_rows(0) rows, so
segment i is tile i, the grid equals the tile count and tile i lands in
sub-region i & 7: a generator chooses how many records each (bucket, sub)
region receives. Rows 0 and 1 of every segment hold the two ends of the key
span (direct buckets 0 and 1023), as everywhere in test_partition_modes.

Shapes, in the modes of test_partition_tiles (dp, hp, d16, h16) where the
mode applies:

  counts   16 segments; the eight sub-regions of ONE bucket receive 0, 1, 2,
           3, p-1, p, p+1 and 2p+1 records, p the records of a full pass in
           that mode (P for dp, P / 2 for the others): an empty region, the
           odd last record, regions shorter than a pass, a pass boundary, a
           stream that runs from a region into an empty one and out again.
           Tiles i and i+8 share a sub-region; the other rows spread over
           other buckets. For dp 2p+1 = 8193 records do not fit a region at
           any input of this size: bucket_stride is rows/8192 * 1.5 + 4096,
           so a region of 8193 needs 22 M rows. Its eighth region holds
           bucket_stride - 1 = 4111 records instead: a full pass, turns
           behind it, and an odd last record, which is what 2p+1 is there
           for.
  edges    direct: keys only in slot 0 and slot SL-1 of buckets 0, 1, 511,
           1023; the other 1020 workgroups must reserve nothing
  span     direct packed at bk = 10 (SL = 1), 11 and 22 (SL = 4096, the
           largest table, beside which the flush's scan words must fit)
  dense    direct packed: every slot of two adjacent buckets non-empty, at
           bk = 13 (SL = 8) and at bk = 22 (SL = 4096: all four waves, every
           chunk full)
  nullcnt  one bucket: a key with only null values, one with both, one with
           none, with sum + sum(1), sum(1) alone and sum alone
  limit    302 groups over five buckets, group_row_limit one below, at and
           one above; dp and hp
  cap      dense at bk = 22 against max_groups_hint = 1: 8194 groups, 4098
           fit

Every GPU case asserts rows equal to the independent reference of
test_partition_modes exactly, the path bits equal to predict_bits, and
rows_read / rows_written / grouped_row_count. The CPU twin runs the same
inputs through the oracle against that reference and checks the region
counts the generators promise. tools/probe_bucket.hip is compiled, not run.
"""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import ytsaurus_amd as y
from ytsaurus_amd import _abi

from test_partition_modes import (
    AGGS, D, H, K, KX, MK, MV, N, P, SHAPES, check_case, last_path,
    predict_bits)
from test_partition_tiles import (
    KNB, MODES, TileCase, bucket_stride, hash_bucket, seg_values, tile_rows)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def pass_records(mode="dp"):
    p = int(_abi.gpu_lib().yt_gpu_debug_bucket_pass_records())
    return p if mode == "dp" else p // 2


# ------------------------------------------------------------------ #
# generators (zigzag domain)                                          #

def bucket_of(zz, wk, direct):
    zz = np.asarray(zz, dtype=np.uint64)
    if direct:
        return ((zz - np.uint64(MK)) >> np.uint64(max(wk - 10, 0))).astype(np.int64)
    return hash_bucket(zz)


def keys_in_bucket(rng, wk, direct, b, count):
    """`count` distinct keys of bucket b, none of them an end of the span"""
    if direct:
        sl = 1 << (wk - 10)
        slots = np.sort(rng.choice(sl, count, replace=False))
        return (MK + (b << (wk - 10)) + slots).astype(np.uint64)
    out = np.zeros(0, dtype=np.uint64)
    while len(out) < count:
        cand = (MK + 1 + rng.integers(0, (1 << wk) - 2, 1 << 18)).astype(np.uint64)
        out = np.unique(np.concatenate([out, cand[hash_bucket(cand) == b]]))
    return out[:count]


def keys_elsewhere(rng, wk, direct, avoid, count):
    """`count` keys outside the buckets `avoid`, spread over the span"""
    cand = (MK + 1 + rng.integers(0, (1 << wk) - 2, 4 * count + 64)).astype(np.uint64)
    cand = np.unique(cand[~np.isin(bucket_of(cand, wk, direct), avoid)])
    assert len(cand) >= count
    return rng.permutation(cand)[:count]


def with_ends(k, sizes, wk):
    """rows 0 and 1 of every segment: the two ends of the key span"""
    a = 0
    for n in sizes:
        k[a], k[a + 1] = MK, MK + (1 << wk) - 1
        a += n
    return k


TARGET = 5          # the bucket under test; 0 and 1023 hold the span's ends


def count_plan(mode):
    """records of bucket TARGET per sub-region"""
    p = pass_records(mode)
    t = tile_rows()
    last = 2 * p + 1
    if last > bucket_stride(16 * t) - 1:
        last = bucket_stride(16 * t) - 1
    return [0, 1, 2, 3, p - 1, p, p + 1, last]


def make_counts(mode):
    wk, wv, bits = MODES[mode]
    direct = bool(bits & D)

    def make(rng):
        t = tile_rows()
        sizes = [t] * 16
        mine = keys_in_bucket(rng, wk, direct, TARGET, 4 if direct else 5)
        other = keys_elsewhere(rng, wk, direct, [TARGET], 300)
        k = other[rng.integers(0, len(other), 16 * t)]
        for sub, c in enumerate(count_plan(mode)):
            first = min(c, t - 2)
            for tile, n in ((sub, first), (sub + 8, c - first)):
                assert n <= t - 2
                at = tile * t + 2 + rng.permutation(t - 2)[:n]
                k[at] = mine[rng.integers(0, len(mine), n)]
        k = with_ends(k, sizes, wk)
        v = seg_values(rng, sizes, MV, wv, 64)
        return [(k, None), (v, None)]
    return make


def make_edges(wk, wv):
    def make(rng):
        t = tile_rows()
        sl = 1 << (wk - 10)
        ks = np.array([MK + (b << (wk - 10)) + s
                       for b in (0, 1, 511, 1023) for s in (0, sl - 1)],
                      dtype=np.uint64)
        k = with_ends(ks[rng.integers(0, len(ks), t)], [t], wk)
        k[2:2 + len(ks)] = ks
        return [(k, None), (seg_values(rng, [t], MV, wv, 64), None)]
    return make


def make_span(bk, ngroups):
    def make(rng):
        t = tile_rows()
        ks = (MK + rng.choice(1 << bk, ngroups, replace=False)).astype(np.uint64)
        k = with_ends(ks[rng.integers(0, len(ks), t)], [t], bk)
        k[2:2 + len(ks)] = ks
        return [(k, None), (seg_values(rng, [t], MV, 20, 64), None)]
    return make


def dense_sizes(bk):
    """tiles that hold three rows of every key of two buckets"""
    return [tile_rows()] * ((6 << (bk - 10)) // tile_rows() + 1)


def make_dense(bk):
    """every slot of buckets 511 and 512, three rows or more each"""
    def make(rng):
        sizes = dense_sizes(bk)
        n = sum(sizes)
        ks = (MK + (511 << (bk - 10)) + np.arange(2 << (bk - 10))).astype(np.uint64)
        body = n - 2 * len(sizes)
        k = np.zeros(n, dtype=np.uint64)
        rest = np.ones(n, dtype=bool)
        rest[np.cumsum([0] + sizes[:-1])] = False
        rest[np.cumsum([0] + sizes[:-1]) + 1] = False
        k[rest] = rng.permutation(np.concatenate(
            [ks, ks, ks, ks[rng.integers(0, len(ks), body - 3 * len(ks))]]))
        k = with_ends(k, sizes, bk)
        return [(k, None), (seg_values(rng, sizes, MV, 20, 64), None)]
    return make


def make_nullcnt(mode):
    """rows 2..5: ka with a null value, kb with a value, kb with a null
    value, kc with a value; after them the three keys at random, ka's values
    all null, kb's half, kc's never"""
    wk, wv, bits = MODES[mode]
    direct = bool(bits & D)

    def make(rng):
        t = tile_rows()
        ka, kb, kc = keys_in_bucket(rng, wk, direct, TARGET, 3)
        k = np.array([ka, kb, kc], dtype=np.uint64)[rng.integers(0, 3, t)]
        k[2:6] = [ka, kb, kb, kc]
        k = with_ends(k, [t], wk)
        vn = (k == ka) | ((k == kb) & (rng.random(t) < 0.5))
        vn[3], vn[4] = False, True
        return [(k, None), (seg_values(rng, [t], MV, wv, 64), vn)]
    return make


LIMIT_WK = {"dp": 17, "hp": 40}
LIMIT_BUCKETS = (3, 4, 700)


def make_limit(mode):
    wk = LIMIT_WK[mode]
    direct = mode == "dp"

    def make(rng):
        t = tile_rows()
        ks = np.concatenate([keys_in_bucket(rng, wk, direct, b, 100)
                             for b in LIMIT_BUCKETS])
        k = with_ends(ks[rng.integers(0, len(ks), t)], [t], wk)
        k[2:2 + len(ks)] = ks
        return [(k, None), (seg_values(rng, [t], MV, 20, 64), None)]
    return make


def _cases():
    out = []
    t = tile_rows()
    for mode, (wk, wv, bits) in MODES.items():
        out.append(TileCase("counts_" + mode, make_counts(mode), bits, [t] * 16))
        for an, (sums, sum1) in AGGS.items():
            b = (bits | N) if sums else SHAPES[mode][3]
            out.append(TileCase("nullcnt_%s_%s" % (mode, an), make_nullcnt(mode),
                                b, [t], sums=sums, sum1=sum1))
    out.append(TileCase("edges_dp", make_edges(12, 31), P | D | K, [t]))
    out.append(TileCase("edges_d16", make_edges(12, 62), P | D | KX, [t]))
    for bk in (10, 11, 22):
        out.append(TileCase("span_%d" % bk, make_span(bk, 300), P | D | K, [t]))
    for bk in (13, 22):
        out.append(TileCase("dense_%d" % bk, make_dense(bk), P | D | K,
                            dense_sizes(bk)))
    out.append(TileCase("limit_dp", make_limit("dp"), P | D | K, [t]))
    out.append(TileCase("limit_hp", make_limit("hp"), P | K, [t]))
    return out


IDS = []
for _mode in MODES:
    IDS.append("counts_" + _mode)
    IDS += ["nullcnt_%s_%s" % (_mode, _an) for _an in AGGS]
IDS += ["edges_dp", "edges_d16", "span_10", "span_11", "span_22",
        "dense_13", "dense_22", "limit_dp", "limit_hp"]
LIMIT_GROUPS = 302


@functools.lru_cache(maxsize=None)
def cases():
    """built on first use: the constants come from the built library"""
    out = {c.id: c for c in _cases()}
    assert sorted(out) == sorted(IDS)
    return out


def case_cols(case):
    cols = case.columns()
    return cols[0], (cols[1] if case.sums else None)


# ------------------------------------------------------------------ #
# CPU tier                                                            #

def test_pass_constant():
    """a full pass is eight 16-byte loads of 256 lanes, and a region of this
    file's inputs holds P + 1 records but not 2 P + 1"""
    p = pass_records()
    assert p == 256 * 8 * 2
    stride = bucket_stride(16 * tile_rows())
    assert p + 1 < stride - 1 < 2 * p + 1
    assert 2 * (p // 2) + 1 <= stride - 1
    assert (stride - 1) // 2 > p // 2 and (stride - 1) % 2 == 1


@pytest.mark.parametrize("cid", IDS)
def test_inputs_and_oracle(cid):
    case = cases()[cid]
    key, val = case_cols(case)
    assert predict_bits(key, val) == case.bits
    assert [m[2] for m in key.seg_meta] == case.sizes
    shape, _, rest = case.id.partition("_")
    zk = case.data()[0][0]
    ref = case.reference()
    if shape == "counts":
        wk, _, bits = MODES[rest]
        t = tile_rows()
        b = bucket_of(zk, wk, bool(bits & D))
        per_tile = [(b[i * t:(i + 1) * t] == TARGET).sum() for i in range(16)]
        got = [per_tile[s] + per_tile[s + 8] for s in range(8)]
        assert got == count_plan(rest)
        assert got[7] > pass_records(rest) + 1 and got[7] % 2 == 1
        for sub in range(8):       # no region above its capacity
            rows = np.concatenate([b[sub * t:(sub + 1) * t],
                                   b[(sub + 8) * t:(sub + 9) * t]])
            assert np.bincount(rows, minlength=KNB).max() <= bucket_stride(16 * t)
    if shape == "edges":
        assert len(ref) == 8
        assert sorted(set(bucket_of(zk, 12, True).tolist())) == [0, 1, 511, 1023]
    if shape == "span":
        assert len(ref) in (301, 302)
    if shape == "dense":
        bk = int(rest)
        sl = 1 << (bk - 10)
        assert len(ref) == 2 * sl + 2
        b = bucket_of(zk, bk, True)
        assert sorted(set(b.tolist())) == [0, 511, 512, 1023]
    if shape == "nullcnt":
        mode = rest.partition("_")[0]
        wk, _, bits = MODES[mode]
        assert set(bucket_of(zk[2:], wk, bool(bits & D)).tolist()) == {TARGET}
        if case.sums:
            nosum = [k for k, (s, c) in ref.items() if s[0] is None]
            assert len(ref) == 5 and len(nosum) == 1
            vn = case.data()[1][1]
            kb = zk[3]
            assert vn[zk == kb].any() and not vn[zk == kb].all()
    if shape == "limit":
        assert len(ref) == LIMIT_GROUPS
        b = bucket_of(zk[2:], LIMIT_WK[rest], rest == "dp")
        assert sorted(set(b.tolist())) == sorted(LIMIT_BUCKETS)
    got, st = y.oracle_execute(case.plan(), case.chunk())
    want = case.rows()
    assert y.sort_rows(got) == y.sort_rows(want)
    assert st.rows_read == sum(case.sizes)
    assert st.rows_written == len(want)


def test_probe_compiles(tmp_path):
    """tools/probe_bucket.hip builds for gfx950; nothing is run"""
    hipcc = shutil.which("hipcc")
    if hipcc is None:
        pytest.skip("no hipcc")
    r = subprocess.run(
        [hipcc, "--offload-arch=gfx950", "-c",
         os.path.join(REPO, "tools", "probe_bucket.hip"),
         "-o", str(tmp_path / "probe_bucket.o")],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


# ------------------------------------------------------------------ #
# GPU tier                                                            #

PLAIN = [i for i in IDS if not i.startswith("limit")]


@pytest.mark.gpu
@pytest.mark.parametrize("cid", PLAIN)
def test_phase_b(cid, cuda):
    case = cases()[cid]
    got, _ = check_case(case, cuda)
    key, val = case_cols(case)
    assert last_path() == predict_bits(key, val)
    assert not last_path() & H
    if cid.startswith("nullcnt") and case.sums:
        assert sum(1 for r in got if r[1] is None) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["dp", "hp"])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_group_row_limit(mode, delta, cuda):
    """the limit falls inside one workgroup's reservation: flagged incomplete
    exactly when the groups exceed it, and every returned row is a row of
    the reference, once"""
    case = cases()["limit_" + mode]
    want = case.rows()
    assert len(want) == LIMIT_GROUPS
    limit = LIMIT_GROUPS + delta
    chunk = case.chunk()        # owns the device tensors behind `dev`
    dev = chunk.c_device(cuda)
    got, st = y.gpu_execute(case.plan(), dev, max_groups_hint=case.hint,
                            group_row_limit=limit)
    assert last_path() == case.bits
    assert st.incomplete_output == (1 if LIMIT_GROUPS > limit else 0)
    assert len(set(got)) == len(got)
    assert all(r in set(want) for r in got)
    if LIMIT_GROUPS > limit:
        assert len(got) >= limit
    else:
        assert y.sort_rows(got) == y.sort_rows(want)
        assert st.rows_written == st.grouped_row_count == len(want)


@pytest.mark.gpu
def test_output_capacity(cuda):
    """8194 groups against max_groups_hint = 1 (4098 fit, the cap falls
    inside a full workgroup's run): the exact result, or an error that names
    the knob; never a short rowset passed off as complete"""
    case = cases()["dense_22"]
    want = case.rows()
    assert len(want) == 8194
    chunk = case.chunk()        # owns the device tensors behind `dev`
    dev = chunk.c_device(cuda)
    try:
        got, st = y.gpu_execute(case.plan(), dev, max_groups_hint=1)
    except RuntimeError as e:
        assert "max_groups_hint" in str(e)
        return
    assert st.incomplete_output == 0
    assert y.sort_rows(got) == y.sort_rows(want)
    assert st.rows_written == st.grouped_row_count == len(want)
