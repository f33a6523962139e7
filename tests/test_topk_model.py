"""ORDER BY ... LIMIT on the GPU against an exact model, cell by cell.

run_scan_topk (evaluator.cpp) selects the (offset + limit) least rows with
histogram passes over an order-isomorphic u64 mapping of the first order key,
gathers the candidates and sorts them on the host. Which kernels run (the fast
pair or the generic pair), how many passes the refinement takes and how it
ends depend on the data; yt_gpu_debug_last_topk() reports all of that, and
every case here asserts the cell it was built for before it trusts its result.

Reference: a numpy model in this file (model_order), independent of the CPU
oracle: filter, sort by the TopCollector comparer (null < any value, int64
signed, uint64 / boolean unsigned, double by value; descending inverts,
nulls last), take [offset, offset + limit). The model is itself checked
against oracle_execute on small chunks without a GPU (test_model_vs_oracle),
and the host refinement loop is replayed in numpy (replay) and checked
against the pass counts the spike recipe was designed for
(test_replay_spike_recipe).

Every chunk carries id = arange(n) as its second column and every plan
projects it, so nothing is computed and every check is exact:
  * the ordered key sequence equals the model's;
  * len(rows) == rows_written == min(limit, max(0, passing - offset));
  * ids are unique, each returned (key, id) is the source row at that id and
    that row passes the filter;
  * for every key value of the output but the first and the last distinct
    one, the ids are ALL source ids with that key (membership is arbitrary
    only in the two edge tie groups).
Multi-key plans order by (key, id): the result is fully determined and whole
rows are compared.

The spike recipe (2^20 rows, 8 DirectDense segments): a 63-bit background, a
cluster of 300 000 keys in [C, C + 2^22), 160 000 copies of C + 777 and both
int64 extremes. Ascending, with lt = count(a < spike), le = count(a <= spike):
K = 100 ends after 1 pass, K = count(a < C) after 2, K = count(a < C) + 1
after 5, K = lt after 6, K = lt + 1 after 6 on the single-valued bucket of
160 000 rows, K = le + 1 after 6.
"""
import functools

import numpy as np
import pytest

import ytsaurus_amd as y
from ytsaurus_amd import _abi

CAPB = 1 << 17                  # run_scan_topk's tie cap
SPIKE_N = 1 << 20
SPIKE_C = 120_000_000_000_000   # about 1.2e14
SPIKE = SPIKE_C + 777
U64 = (1 << 64) - 1

VDT = np.dtype([("id", "<u2"), ("type", "u1"), ("flags", "u1"),
                ("length", "<u4"), ("bits", "<u8")])
VT = {"i64": _abi.VT_INT64, "u64": _abi.VT_UINT64, "bool": _abi.VT_BOOLEAN,
      "f64": _abi.VT_DOUBLE}


# ---------------------------------------------------------------- data

class Data:
    """One key column (+ nulls) and id = arange(n)."""

    def __init__(self, kind, key, nulls=None, max_seg=0):
        self.kind = kind
        self.n = len(key)
        self.key = np.ascontiguousarray(key)
        self.nulls = (np.zeros(self.n, dtype=bool) if nulls is None
                      else np.asarray(nulls, dtype=bool))
        nl = self.nulls.astype(np.uint8) if nulls is not None else None
        if kind == "i64":
            kc = y.encode_int64(self.key, nl, max_segment_values=max_seg)
        elif kind == "u64":
            kc = y.encode_int64(self.key.view(np.int64), nl,
                                max_segment_values=max_seg, unsigned=True)
        elif kind == "bool":
            kc = y.encode_bool(self.key.astype(np.uint8), nl,
                               max_segment_values=max_seg)
        else:
            kc = y.encode_double(self.key, nl, max_segment_values=max_seg)
        self.ids = np.arange(self.n, dtype=np.int64)
        self.chunk = y.Chunk(
            [kc, y.encode_int64(self.ids, max_segment_values=max_seg)], self.n)
        self.all = np.ones(self.n, dtype=bool)
        self._dev = None
        self._orders = {}

    def seg_types(self):
        return [s.type for s in self.chunk.columns[0].segments]

    def dev(self, cuda):
        if self._dev is None:
            self._dev = self.chunk.c_device(cuda)
        return self._dev

    def key_bits(self):
        if self.kind == "bool":
            return self.key.astype(np.uint64)
        return self.key.view(np.uint64)

    def order(self, desc, passing=None, id_desc=None, tag="all"):
        k = (bool(desc), id_desc, tag)
        if k not in self._orders:
            self._orders[k] = model_order(
                self.key, self.nulls,
                self.all if passing is None else passing, desc, id_desc)
        return self._orders[k]


# ---------------------------------------------------------------- model

def model_order(key, nulls, passing, desc, id_desc=None):
    """ids of the passing rows in TopCollector order. Rows with equal keys
    are ordered by id (descending when id_desc): for a single-key plan that
    order is arbitrary, for a (key, id) plan it is the second order key."""
    ids = np.flatnonzero(passing)
    isn = nulls[ids]
    nl, nn = ids[isn], ids[~isn]
    k = key[nn]
    if k.dtype == np.bool_:
        k = k.astype(np.uint8)
    assert not (k.dtype.kind == "f" and np.isnan(k).any())
    # numpy's own order of the dtype: signed, unsigned, by value. A
    # descending first key is the ascending sort with the second key turned
    # round, read backwards
    sec = nn if bool(id_desc) == bool(desc) else -nn
    o = nn[np.lexsort((sec, k))]
    if desc:
        o = o[::-1]
    if id_desc:
        nl = nl[::-1]
    return np.concatenate([o, nl] if desc else [nl, o])


def expect_count(passing, offset, limit):
    return min(limit, max(0, int(passing.sum()) - offset))


def decode(kind, bits):
    if kind == "i64":
        return bits.view(np.int64)
    if kind == "f64":
        return bits.view(np.float64)
    if kind == "bool":
        return (bits != 0).astype(np.uint8)
    return bits


def mapped(kind, key, desc):
    """the u64 mapping of topk_map / topk_map_int, restated"""
    if kind == "i64":
        m = key.view(np.uint64) ^ np.uint64(1 << 63)
    elif kind == "f64":
        b = key.view(np.uint64)
        m = np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))
    else:
        m = key.astype(np.uint64)
    return ~m if desc else m


def replay(m, null_cnt, K, desc):
    """run_scan_topk's host refinement over the mapped non-null passing keys
    m: dict(passes, only_nulls, all_nonnull, big_tie)."""
    r = dict(passes=1, only_nulls=False, all_nonnull=False, big_tie=False)
    nonnull = len(m)
    if desc:
        k_nonnull = min(K, nonnull)
    else:
        k_nonnull = K - min(null_cnt, K)
    if k_nonnull <= 0:
        r["only_nulls"] = True
        return r
    if k_nonnull >= nonnull:
        r["all_nonnull"] = True
        return r
    lo, hi, shift, S = 0, U64, 53, 0
    mmin, mmax = int(m.min()), int(m.max())
    level0 = True
    while True:
        m = m[(m >= np.uint64(lo)) & (m <= np.uint64(hi))]
        bins = np.bincount(((m - np.uint64(lo)) >> np.uint64(shift))
                           .astype(np.int64), minlength=2048)
        cum = np.cumsum(bins)
        t = int(np.argmax(S + cum >= k_nonnull))
        assert S + cum[t] >= k_nonnull
        S += int(cum[t] - bins[t])
        T = int(bins[t])
        nlo = lo + (t << shift)
        nhi = min(nlo + (1 << shift) - 1, hi)
        if level0:
            nlo, nhi = max(nlo, mmin), min(nhi, mmax)
        lo, hi = nlo, nhi
        if T <= CAPB or shift == 0 or lo >= hi:
            break
        shift = 0
        while ((hi - lo) >> shift) >= 2048:
            shift += 1
        level0 = False
        r["passes"] += 1
    r["big_tie"] = T > CAPB
    return r


def predict(d, passing, desc, K):
    sel = passing & ~d.nulls
    return replay(mapped(d.kind, d.key[sel], desc),
                  int((passing & d.nulls).sum()), K, desc)


# ---------------------------------------------------------------- datasets

def _spike_keys():
    rng = np.random.default_rng(20260)
    n = SPIKE_N
    a = rng.integers(-2**62, 2**62, n, dtype=np.int64)
    perm = rng.permutation(n)
    a[perm[:300_000]] = SPIKE_C + rng.integers(0, 1 << 22, 300_000)
    a[perm[300_000:460_000]] = SPIKE
    a[perm[460_000]] = -2**63
    a[perm[460_001]] = 2**63 - 1
    return rng, a


@functools.lru_cache(maxsize=None)
def spike(variant="plain"):
    """the spike recipe; 'nulls': 5 % nulls; 'seg3': nulls in segment 3
    only"""
    rng, a = _spike_keys()
    nulls = None
    if variant == "nulls":
        nulls = rng.random(SPIKE_N) < 0.05
    elif variant == "seg3":
        nulls = np.zeros(SPIKE_N, dtype=bool)
        nulls[3 * CAPB:4 * CAPB] = rng.random(CAPB) < 0.05
    d = Data("i64", a, nulls)
    # encoder drift must not quietly move the recipe off the fast kernels
    assert d.seg_types() == [_abi.SEG_DIRECT_DENSE] * 8
    return d


def spike_ks(d, desc, passing=None):
    a = d.key[(d.all if passing is None else passing) & ~d.nulls]
    if desc:
        return dict(cntC=int((a >= SPIKE_C + (1 << 22)).sum()),
                    lt=int((a > SPIKE).sum()), le=int((a >= SPIKE).sum()))
    return dict(cntC=int((a < SPIKE_C).sum()),
                lt=int((a < SPIKE).sum()), le=int((a <= SPIKE).sum()))


A_KS = {
    "1": lambda c, n: 1,
    "100": lambda c, n: 100,
    "cntC": lambda c, n: c["cntC"],
    "cntC+1": lambda c, n: c["cntC"] + 1,
    "lt": lambda c, n: c["lt"],
    "lt+1": lambda c, n: c["lt"] + 1,
    "lt+1000": lambda c, n: c["lt"] + 1000,
    "le": lambda c, n: c["le"],
    "le+1": lambda c, n: c["le"] + 1,
    "n-1": lambda c, n: n - 1,
    "n": lambda c, n: n,
    "n+5": lambda c, n: n + 5,
}
A_DEEP = ("cntC+1", "lt", "lt+1", "lt+1000", "le", "le+1")
# descending, the step into the cluster from above takes 4 passes
A_DEEP_DESC = A_DEEP[1:]


@functools.lru_cache(maxsize=None)
def u64_data():
    rng = np.random.default_rng(20261)
    n = 1 << 18
    a = rng.integers(0, 2**64, n, dtype=np.uint64)
    sp = rng.permutation(n)[:12]
    a[sp] = np.repeat(np.array([0, 2**63 - 1, 2**63, 2**64 - 1],
                               dtype=np.uint64), 3)
    d = Data("u64", a)
    assert d.seg_types() == [_abi.SEG_DIRECT_DENSE] * 2
    return d


ND = (1 << 17) + 3


@functools.lru_cache(maxsize=None)
def small(name):
    rng = np.random.default_rng(20262)
    n = ND
    if name == "ragged":
        a = rng.integers(-4000, 4000, n, dtype=np.int64)
        return Data("i64", a, rng.random(n) < 0.03, max_seg=5000)
    if name == "dict":
        vals = rng.integers(-2**60, 2**60, 37, dtype=np.int64)
        d = Data("i64", vals[rng.integers(0, 37, n)])
        # (the last segment holds 3 rows)
        assert d.seg_types()[0] in (_abi.SEG_DICTIONARY_DENSE,
                                    _abi.SEG_DICTIONARY_RLE), d.seg_types()
        return d
    if name == "rle":
        a = np.sort(rng.integers(0, 300, n, dtype=np.int64) * 10**9)
        d = Data("i64", a)
        assert d.seg_types()[0] in (_abi.SEG_DIRECT_RLE,
                                    _abi.SEG_DICTIONARY_RLE), d.seg_types()
        return d
    if name == "expr":
        return Data("i64", rng.integers(-10**6, 10**6, n, dtype=np.int64))
    if name == "bool":
        return Data("bool", rng.random(n) < 0.5, rng.random(n) < 0.05)
    if name == "card20":
        return Data("i64", rng.integers(0, 20, n, dtype=np.int64),
                    rng.random(n) < 0.05)
    assert name == "double"
    a = rng.standard_normal(n) * 1e3
    big = np.finfo(np.float64).max
    special = [np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 2.2e-308 / 4,
               -2.2e-308 / 4, big, -big]
    pos = rng.permutation(n)[:len(special) * 3]
    a[pos] = np.repeat(np.array(special), 3)
    return Data("f64", a, rng.random(n) < 0.03)


# ---------------------------------------------------------------- running

def id_filter(kind):
    """filters over the id column, with their numpy restatement"""
    if kind == "all":                     # passes every row; forces generic
        return y.col(1) >= 0, lambda d: d.all
    if kind == "none":
        return y.col(1) < 0, lambda d: ~d.all
    raise ValueError(kind)


def run(cuda, d, order_by, limit, offset=0, filt=None, projects=None, **kw):
    plan = y.Plan(filter=filt,
                  projects=projects or [y.col(0), y.col(1)],
                  order_by=order_by, limit=limit, offset=offset)
    rs, st = y.gpu_execute(plan, d.dev(cuda), raw_rowset=True,
                           out_capacity=max(min(limit, d.n), 1), **kw)
    nr, nc = rs.row_count, rs.column_count
    assert nc == 2
    v = np.frombuffer(rs._buf, dtype=VDT, count=nr * nc).reshape(nr, nc)
    return v["type"].copy(), v["bits"].copy(), st, y.gpu_debug_last_topk()


def check_single(d, types, bits, st, desc, offset, limit, passing=None,
                 key=None, order_tag="all"):
    """the single-key checks of the module docstring. key: the order key
    per row where it is not the stored column (expression keys);
    order_tag names `passing` for the cache of model orders."""
    passing = d.all if passing is None else passing
    key = d.key if key is None else key
    if key is d.key:
        order = d.order(desc, passing, tag=order_tag)
    else:
        order = model_order(key, d.nulls, passing, desc)
    exp_ids = order[offset:offset + limit]
    exp_n = expect_count(passing, offset, limit)
    assert len(exp_ids) == exp_n
    assert types.shape[0] == exp_n
    assert st.rows_written == exp_n
    if exp_n == 0:
        return
    kind = d.kind
    # ordered key sequence
    gnull = types[:, 0] == _abi.VT_NULL
    assert np.array_equal(gnull, d.nulls[exp_ids])
    assert (types[~gnull, 0] == VT[kind]).all()
    gv = decode(kind, bits[:, 0])
    kk = key.astype(np.uint8) if key.dtype == np.bool_ else key
    assert np.array_equal(gv[~gnull], kk[exp_ids][~gnull])
    # ids: unique, and each row is the source row at its id
    assert (types[:, 1] == _abi.VT_INT64).all()
    gid = bits[:, 1].view(np.int64)
    assert ((gid >= 0) & (gid < d.n)).all()
    assert len(np.unique(gid)) == exp_n
    assert passing[gid].all()
    assert np.array_equal(d.nulls[gid], gnull)
    kb = kk.astype(np.uint64) if kind == "bool" else kk.view(np.uint64)
    assert np.array_equal(kb[gid][~gnull], bits[~gnull, 0])
    # complete membership of every tie group but the two edge ones
    interior = ~gnull
    if not gnull[0]:
        interior &= gv != gv[0]
    if not gnull[-1]:
        interior &= gv != gv[-1]
    if interior.any():
        vals = np.unique(gv[interior])
        src = np.flatnonzero(passing & ~d.nulls & np.isin(kk, vals))
        assert np.array_equal(np.sort(gid[interior]), src)


def check_diag(topk, want, fast):
    assert topk["fast"] == fast
    for f in ("passes", "only_nulls", "all_nonnull", "big_tie"):
        assert topk[f] == want[f], (f, topk, want)


def window(K):
    off = max(K - 50, 0)
    return off, K - off


def run_window(cuda, d, desc, K, path, offset=None, limit=None):
    """one spike-recipe style case: run, check the cell, check the rows"""
    if offset is None:
        offset, limit = window(K)
    filt = id_filter("all")[0] if path == "generic" else None
    types, bits, st, topk = run(cuda, d, [(0, desc)], limit, offset, filt)
    want = predict(d, d.all, desc, offset + limit)
    check_diag(topk, want, path == "fast")
    check_single(d, types, bits, st, desc, offset, limit)
    return topk


PATHS = ("fast", "generic")
DIRS = (False, True)


# ---------------------------------------------------------------- CPU tests

def _small_cpu(kind, with_nulls, rng, n):
    if kind == "i64":
        a = rng.integers(-50, 50, n, dtype=np.int64)
        a[:4] = [-2**63, 2**63 - 1, 0, -1]
    elif kind == "u64":
        a = rng.integers(0, 32, n, dtype=np.uint64) * np.uint64(2**59)
        a[:4] = np.array([0, 2**63 - 1, 2**63, 2**64 - 1], dtype=np.uint64)
    elif kind == "bool":
        a = rng.random(n) < 0.5
    else:
        a = np.round(rng.standard_normal(n), 1)
        a[:6] = [np.inf, -np.inf, 0.0, -0.0, 5e-324, -1.7976931348623157e308]
    return Data(kind, a, (rng.random(n) < 0.1) if with_nulls else None)


@pytest.mark.parametrize("kind", ["i64", "u64", "bool", "f64"])
@pytest.mark.parametrize("with_nulls", [False, True])
def test_model_vs_oracle(kind, with_nulls):
    """a wrong model fails here, without a GPU"""
    rng = np.random.default_rng(77)
    n = 4999
    d = _small_cpu(kind, with_nulls, rng, n)
    filt, passing = y.col(1) % 7 != 3, d.ids % 7 != 3
    for desc in DIRS:
        for offset, limit in ((0, 40), (13, 700), (4000, 2000), (0, 1)):
            for f, p in ((None, d.all), (filt, passing)):
                plan = y.Plan(filter=f, projects=[y.col(0), y.col(1)],
                              order_by=[(0, desc)], limit=limit,
                              offset=offset)
                rows, st = y.oracle_execute(plan, d.chunk)
                e = model_order(d.key, d.nulls, p, desc)[offset:offset + limit]
                assert len(rows) == expect_count(p, offset, limit) == len(e)
                assert st.rows_written == len(e)
                want = [None if d.nulls[i] else d.key[i].item() for i in e]
                assert [r[0] for r in rows] == want
                # two keys: (key, id) decides every row
                for id_desc in DIRS:
                    plan = y.Plan(filter=f, projects=[y.col(0), y.col(1)],
                                  order_by=[(0, desc), (1, id_desc)],
                                  limit=limit, offset=offset)
                    rows, _ = y.oracle_execute(plan, d.chunk)
                    e = model_order(d.key, d.nulls, p, desc,
                                    id_desc)[offset:offset + limit]
                    want = [(None if d.nulls[i] else d.key[i].item(), int(i))
                            for i in e]
                    assert rows == want


def test_replay_spike_recipe():
    """the recipe reaches the cells it was designed for (module docstring):
    the replay of the host loop gives the designed pass counts"""
    d = spike()
    n = d.n
    c = spike_ks(d, False)
    m = mapped("i64", d.key, False)
    got = {k: replay(m, 0, f(c, n), False) for k, f in A_KS.items()}
    want = {"100": (1, False), "n-1": (1, False), "cntC": (2, False),
            "cntC+1": (5, False), "lt": (6, False), "lt+1": (6, True),
            "le+1": (6, False)}
    for k, (passes, big) in want.items():
        assert (got[k]["passes"], got[k]["big_tie"]) == (passes, big), k
        assert not got[k]["all_nonnull"] and not got[k]["only_nulls"]
    assert got["n"]["all_nonnull"] and got["n"]["passes"] == 1
    assert got["n+5"]["all_nonnull"]
    assert got["lt+1000"]["big_tie"] and got["le"]["big_tie"]
    # the mirrored counts are as deep descending
    cd = spike_ks(d, True)
    md = mapped("i64", d.key, True)
    for k in A_DEEP:
        assert got[k]["passes"] >= 5
    for k in A_DEEP_DESC:
        assert replay(md, 0, A_KS[k](cd, n), True)["passes"] >= 5, k
    assert replay(md, 0, cd["cntC"] + 1, True)["passes"] == 4
    # the tie-cap cases owe more than CAPB rows of the spike
    assert c["le"] - c["lt"] > CAPB + 9000
    for dn in ("nulls", "seg3"):
        spike(dn)


def test_replay_null_regimes():
    m = mapped("i64", np.arange(1000, dtype=np.int64), False)
    assert replay(m, 50, 50, False)["only_nulls"]
    assert replay(m, 50, 49, False)["only_nulls"]
    assert not replay(m, 50, 51, False)["only_nulls"]
    assert replay(m, 50, 1050, False)["all_nonnull"]
    assert not replay(m, 50, 1049, False)["all_nonnull"]
    md = mapped("i64", np.arange(1000, dtype=np.int64), True)
    assert not replay(md, 50, 999, True)["all_nonnull"]
    for K in (1000, 1001, 1050):
        assert replay(md, 50, K, True)["all_nonnull"]


def test_small_data_encodings():
    """the generic triggers of case D are what they claim, without a GPU"""
    assert len(small("ragged").seg_types()) > 20
    for name in ("dict", "rle", "expr", "bool", "double", "card20"):
        small(name)
    u64_data()


# ---------------------------------------------------------------- A

@pytest.mark.gpu
@pytest.mark.parametrize("kname", list(A_KS))
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("desc", DIRS, ids=["asc", "desc"])
def test_a_boundary_placement(cuda, desc, path, kname):
    d = spike()
    K = A_KS[kname](spike_ks(d, desc), d.n)
    topk = run_window(cuda, d, desc, K, path)
    if kname in (A_DEEP_DESC if desc else A_DEEP):
        assert topk["passes"] >= 5
    if kname in ("100", "n-1", "n"):
        assert topk["passes"] == 1
    if not desc:
        assert topk["big_tie"] == (kname in ("lt+1", "lt+1000", "le"))
        assert topk["all_nonnull"] == (kname in ("n", "n+5"))


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("desc", DIRS, ids=["asc", "desc"])
def test_a_small_offsets(cuda, desc, path):
    d = spike()
    c = spike_ks(d, desc)
    for offset, limit in ((3, 20), (c["lt"] - 5, 10), (c["le"] - 5, 10)):
        run_window(cuda, d, desc, None, path, offset, limit)


# ---------------------------------------------------------------- B

def b_ks(d, desc):
    nn = int((~d.nulls).sum())
    nc = d.n - nn
    if desc:
        return {"nonnull-1": nn - 1, "nonnull": nn, "nonnull+1": nn + 1,
                "n": d.n}
    return {"null_cnt-1": nc - 1, "null_cnt": nc, "null_cnt+1": nc + 1,
            "null_cnt+lt+1": nc + spike_ks(d, False)["lt"] + 1}


@pytest.mark.gpu
@pytest.mark.parametrize("ki", range(4))
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("desc", DIRS, ids=["asc", "desc"])
def test_b_nulls(cuda, desc, path, ki):
    d = spike("nulls")
    kname, K = list(b_ks(d, desc).items())[ki]
    topk = run_window(cuda, d, desc, K, path)
    # the host arithmetic, stated once more
    if not desc:
        assert topk["only_nulls"] == (kname in ("null_cnt-1", "null_cnt"))
        assert topk["big_tie"] == (kname == "null_cnt+lt+1")
        assert not topk["all_nonnull"]
    else:
        assert topk["all_nonnull"] == (kname != "nonnull-1")
        assert not topk["only_nulls"]


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_b_offset_inside_nulls(cuda, path):
    d = spike("nulls")
    nc = int(d.nulls.sum())
    # ascending: the window starts in the nulls and ends in the values;
    # descending: it starts in the values and ends in the trailing nulls,
    # or lies in them altogether
    run_window(cuda, d, False, None, path, nc - 20, 50)
    run_window(cuda, d, False, None, path, nc - 60, 50)
    run_window(cuda, d, True, None, path, d.n - nc - 20, 50)
    run_window(cuda, d, True, None, path, d.n - nc + 10, 50)


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_b_nulls_in_one_segment(cuda, path):
    d = spike("seg3")
    nc = int(d.nulls.sum())
    assert nc > 1000
    for desc, K in ((False, 100), (False, nc), (False, nc + 100),
                    (True, 100), (True, d.n - nc + 7), (True, d.n)):
        run_window(cuda, d, desc, K, path)


# ---------------------------------------------------------------- C

@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("desc", DIRS, ids=["asc", "desc"])
def test_c_uint64(cuda, desc, path):
    d = u64_data()
    assert (d.key >= np.uint64(2**63)).sum() > 1000
    for K in (1, 3, 4, 100, d.n // 2, d.n - 1, d.n):
        run_window(cuda, d, desc, K, path)
    # the extremes come back as uint64 values, in unsigned order
    types, bits, _, _ = run(cuda, d, [(0, desc)], 3)
    assert (types[:, 0] == _abi.VT_UINT64).all()
    assert bits[:, 0].tolist() == [U64 if desc else 0] * 3


# ---------------------------------------------------------------- D

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ragged", "dict", "rle", "bool", "double"])
@pytest.mark.parametrize("desc", DIRS, ids=["asc", "desc"])
def test_d_generic_triggers(cuda, desc, name):
    d = small(name)
    nn = int((~d.nulls).sum())
    for offset, limit in ((0, 1000), (nn - 30, 80), (d.n // 2, 50),
                          (d.n - 10, 50)):
        types, bits, st, topk = run(cuda, d, [(0, desc)], limit, offset)
        check_diag(topk, predict(d, d.all, desc, offset + limit), False)
        check_single(d, types, bits, st, desc, offset, limit)


@pytest.mark.gpu
@pytest.mark.parametrize("desc", DIRS, ids=["asc", "desc"])
def test_d_expression_key(cuda, desc):
    d = small("expr")
    key = d.key * 3 - d.ids
    for offset, limit in ((0, 500), (d.n - 10, 50)):
        types, bits, st, topk = run(
            cuda, d, [(0, desc)], limit, offset,
            projects=[y.col(0) * 3 - y.col(1), y.col(1)])
        assert not topk["fast"]
        check_single(d, types, bits, st, desc, offset, limit, key=key)


@pytest.mark.gpu
def test_d_nan(cuda):
    d0 = small("double")
    a = d0.key.copy()
    row = int(np.flatnonzero(~d0.nulls)[5])
    a[row] = np.nan
    d = Data("f64", a, d0.nulls)
    # a NaN in a row the filter drops is never compared
    passing = d.ids != row
    for desc in DIRS:
        types, bits, st, _ = run(cuda, d, [(0, desc)], 300, 4,
                                 filt=y.col(1) != row)
        check_single(d, types, bits, st, desc, 4, 300, passing=passing,
                     order_tag="nonan")
    for filt in (None, y.col(1) >= 0):
        with pytest.raises(RuntimeError, match="NaN"):
            run(cuda, d, [(0, False)], 300, filt=filt)


# ---------------------------------------------------------------- E

@pytest.mark.gpu
@pytest.mark.parametrize("offset,limit", [(0, 200_000), (199_950, 50)])
def test_e_tie_cap_constant(cuda, offset, limit):
    """more than CAPB rows owed from one key value: the tie buffer has to
    hold them all (it returned 131 072 rows with YT_OK)"""
    d = e_constant()
    for desc in DIRS:
        types, bits, st, topk = run(cuda, d, [(0, desc)], limit, offset)
        assert topk["big_tie"]
        check_single(d, types, bits, st, desc, offset, limit)
        assert types.shape[0] == limit


@functools.lru_cache(maxsize=None)
def e_constant():
    return Data("i64", np.full(300_000, 7, dtype=np.int64))


@functools.lru_cache(maxsize=None)
def e_bool():
    rng = np.random.default_rng(20263)
    return Data("bool", rng.random(300_000) < 0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("desc", DIRS, ids=["asc", "desc"])
def test_e_tie_cap_bool(cuda, desc):
    d = e_bool()
    first = int((d.key == desc).sum())      # false first ascending
    assert d.n - first > 140_000
    K = first + 140_000
    offset, limit = window(K)
    types, bits, st, topk = run(cuda, d, [(0, desc)], limit, offset)
    assert topk["big_tie"] and not topk["fast"]
    check_single(d, types, bits, st, desc, offset, limit)
    assert types.shape[0] == 50


@pytest.mark.gpu
@pytest.mark.parametrize("kname", ["lt+140000", "le"])
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("desc", DIRS, ids=["asc", "desc"])
def test_e_tie_cap_spike(cuda, desc, path, kname):
    d = spike()
    c = spike_ks(d, desc)
    K = c["lt"] + 140_000 if kname == "lt+140000" else c["le"]
    topk = run_window(cuda, d, desc, K, path)
    assert topk["big_tie"] and topk["passes"] >= 5


# ---------------------------------------------------------------- F

@pytest.mark.gpu
def test_f_degenerate(cuda):
    one = Data("i64", np.array([42], dtype=np.int64))
    for desc in DIRS:
        types, bits, st, _ = run(cuda, one, [(0, desc)], 10)
        check_single(one, types, bits, st, desc, 0, 10)
        assert bits[:, 0].tolist() == [42]
    d = spike()
    for desc in DIRS:
        # a filter that passes nothing
        filt, p = id_filter("none")
        types, bits, st, _ = run(cuda, d, [(0, desc)], 10, filt=filt)
        check_single(d, types, bits, st, desc, 0, 10, passing=p(d),
                     order_tag="none")
        assert types.shape[0] == 0
        # offset at and past the passing rows: empty, no error
        for path in PATHS:
            for offset in (d.n, d.n + 1000):
                filt = id_filter("all")[0] if path == "generic" else None
                types, bits, st, _ = run(cuda, d, [(0, desc)], 10, offset,
                                         filt)
                assert types.shape[0] == 0 and st.rows_written == 0
            # limit = 1
            run_window(cuda, d, desc, None, path, 0, 1)
            run_window(cuda, d, desc, None, path, 777, 1)
    types, bits, _, _ = run(cuda, d, [(0, False)], 1)
    assert bits[:, 0].view(np.int64).tolist() == [-2**63]
    types, bits, _, _ = run(cuda, d, [(0, True)], 1)
    assert bits[:, 0].view(np.int64).tolist() == [2**63 - 1]


@pytest.mark.gpu
@pytest.mark.parametrize("desc", DIRS, ids=["asc", "desc"])
def test_f_input_row_limit_fast(cuda, desc):
    """InputRowLimit cuts segment 3 in two: the selection sees the prefix"""
    full = spike("nulls")
    nrows = 3 * CAPB + 12_345
    passing = full.ids < nrows
    for offset, limit in ((0, 100), (nrows // 3, 50), (nrows - 20, 50)):
        types, bits, st, topk = run(cuda, full, [(0, desc)], limit, offset,
                                    input_row_limit=nrows)
        assert topk["fast"]
        assert st.incomplete_input == 1
        assert st.rows_read == nrows
        want = predict(full, passing, desc, offset + limit)
        check_diag(topk, want, True)
        check_single(full, types, bits, st, desc, offset, limit,
                     passing=passing, order_tag="prefix")


@pytest.mark.gpu
def test_f_output_row_limit(cuda):
    d = spike()
    for desc in DIRS:
        types, bits, st, _ = run(cuda, d, [(0, desc)], 100, 5,
                                 output_row_limit=40)
        assert st.incomplete_output == 1
        assert st.incomplete_input == 0
        # the first 40 rows of the slice
        check_single(d, types, bits, st, desc, 5, 40)
        types, bits, st, _ = run(cuda, d, [(0, desc)], 40, 5,
                                 output_row_limit=40)
        assert st.incomplete_output == 0 and types.shape[0] == 40


# ---------------------------------------------------------------- G

def _pool():
    return int(_abi.gpu_lib().yt_gpu_debug_pool_blocks_in_use())


@pytest.mark.gpu
def test_g_refusals(cuda):
    d = spike()
    c = spike_ks(d, False)
    base = _pool()
    with pytest.raises(RuntimeError, match="capped at 16M"):
        run(cuda, small("expr"), [(0, False)], (1 << 24) + 1)
    assert _pool() == base
    # K = 2^24 itself is served
    e = small("expr")
    types, bits, st, _ = run(cuda, e, [(0, False)], 50, (1 << 24) - 50)
    assert types.shape[0] == 0
    assert _pool() == base
    # two keys, the boundary inside the spike of 160 000 equal keys
    for path in PATHS:
        filt = id_filter("all")[0] if path == "generic" else None
        with pytest.raises(RuntimeError, match="tie set too large"):
            run(cuda, d, [(0, False), (1, True)], 50, c["lt"] + 1000, filt)
        assert y.gpu_debug_last_topk()["big_tie"]
        assert _pool() == base
    # two keys, ascending, the boundary inside more nulls than K + CAPB
    rng = np.random.default_rng(20264)
    n = 1 << 18
    nd = Data("i64", rng.integers(-10**9, 10**9, n, dtype=np.int64),
              rng.random(n) < 0.6)
    nc = int(nd.nulls.sum())
    assert nc > 100 + CAPB
    base = _pool()
    with pytest.raises(RuntimeError, match="null order-key set too large"):
        run(cuda, nd, [(0, False), (1, True)], 50, 50)
    assert _pool() == base
    # a single key over the same chunk is served: any nulls will do
    types, bits, st, topk = run(cuda, nd, [(0, False)], 50, 50)
    assert topk["only_nulls"]
    check_single(nd, types, bits, st, False, 50, 50)
    assert _pool() == base


# ---------------------------------------------------------------- H

def check_multi(d, types, bits, st, desc, id_desc, offset, limit):
    e = d.order(desc, id_desc=id_desc)[offset:offset + limit]
    assert types.shape[0] == len(e) == st.rows_written
    assert np.array_equal(bits[:, 1].view(np.int64), e)
    assert (types[:, 1] == _abi.VT_INT64).all()
    gnull = types[:, 0] == _abi.VT_NULL
    assert np.array_equal(gnull, d.nulls[e])
    assert (types[~gnull, 0] == VT[d.kind]).all()
    assert np.array_equal(bits[~gnull, 0], d.key_bits()[e][~gnull])


@pytest.mark.gpu
@pytest.mark.parametrize("desc", DIRS, ids=["asc", "desc"])
def test_h_multikey_card20(cuda, desc):
    d = small("card20")
    nc = int(d.nulls.sum())
    offs = [(7, 500), (0, 1), (d.n - 40, 100)]
    # the boundary inside the nulls, and just past them
    offs += [(nc - 30, 20), (nc - 10, 30)] if not desc else \
        [(d.n - nc - 10, 30), (d.n - nc + 5, 30)]
    for offset, limit in offs:
        for id_desc in DIRS:
            types, bits, st, topk = run(cuda, d, [(0, desc), (1, id_desc)],
                                        limit, offset)
            assert not topk["big_tie"]
            check_multi(d, types, bits, st, desc, id_desc, offset, limit)


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("desc", DIRS, ids=["asc", "desc"])
def test_h_multikey_spike(cuda, desc, path):
    d = spike("nulls")
    c = spike_ks(d, desc)
    nc = int(d.nulls.sum())
    lead = 0 if desc else nc            # nulls first ascending
    filt = id_filter("all")[0] if path == "generic" else None
    # the boundary just before and well after the spike, never inside it
    for K in (100, lead + c["lt"] - 10, lead + c["le"] + 500):
        offset, limit = window(K)
        types, bits, st, topk = run(cuda, d, [(0, desc), (1, True)], limit,
                                    offset, filt)
        assert topk["fast"] == (path == "fast")
        assert not topk["big_tie"]
        check_multi(d, types, bits, st, desc, True, offset, limit)


# ---------------------------------------------------------------- I

NG = 1 << 16


def _group_rows(cuda, chunk, plan, hint=8192):
    got, st = y.gpu_execute(plan, chunk.c_device(cuda), max_groups_hint=hint)
    assert st.rows_written == len(got)
    assert y.gpu_debug_last_topk()["passes"] == 0     # not the k-selection
    return got


@functools.lru_cache(maxsize=None)
def group_ints():
    rng = np.random.default_rng(20265)
    k = rng.integers(0, 3000, NG, dtype=np.int64)
    u = rng.integers(0, 2**60, NG, dtype=np.uint64)
    v = rng.integers(0, 10**6, NG, dtype=np.int64)
    chunk = y.Chunk([y.encode_int64(k),
                     y.encode_int64(u.view(np.int64), unsigned=True),
                     y.encode_int64(v)], NG)
    groups = {}
    for ki, ui, vi in zip(k.tolist(), u.tolist(), v.tolist()):
        g = groups.setdefault(ki, [0, 0, 0])
        g[0] = (g[0] + ui) & U64
        g[1] += vi
        g[2] += 1
    return chunk, groups


@pytest.mark.gpu
def test_i_group_order_uint64_sum(cuda):
    chunk, groups = group_ints()
    sums = sorted(g[0] for g in groups.values())
    assert len(set(sums)) == len(sums)
    assert sums[0] < 2**63 < sums[-1]            # the order crosses 2^63
    for desc in DIRS:
        plan = y.Plan(keys=[y.col(0)], aggs=[y.agg_sum(y.col(1))],
                      order_by=[(1, desc)], limit=len(groups), offset=3)
        want = sorted(((k, g[0]) for k, g in groups.items()),
                      key=lambda r: r[1], reverse=desc)[3:]
        assert _group_rows(cuda, chunk, plan) == want
    # an offset past the group count
    plan = y.Plan(keys=[y.col(0)], aggs=[y.agg_sum(y.col(1))],
                  order_by=[(1, False)], limit=10, offset=len(groups))
    assert _group_rows(cuda, chunk, plan) == []
    plan = y.Plan(keys=[y.col(0)], aggs=[y.agg_sum(y.col(1))],
                  order_by=[(1, False)], limit=10, offset=len(groups) - 4)
    assert len(_group_rows(cuda, chunk, plan)) == 4


@pytest.mark.gpu
def test_i_group_order_avg_desc(cuda):
    chunk, groups = group_ints()
    # sums below 2^53: the average is one correctly rounded division
    avg = {k: g[1] / g[2] for k, g in groups.items()}
    assert len(set(avg.values())) == len(avg)
    plan = y.Plan(keys=[y.col(0)], aggs=[y.agg_avg(y.col(2))],
                  order_by=[(1, True)], limit=200, offset=1)
    want = sorted(avg.items(), key=lambda r: r[1], reverse=True)[1:201]
    assert _group_rows(cuda, chunk, plan) == want


@pytest.mark.gpu
def test_i_group_order_count_then_key(cuda):
    chunk, groups = group_ints()
    plan = y.Plan(keys=[y.col(0)], aggs=[y.agg_sum1(), y.agg_sum(y.col(2))],
                  order_by=[(1, True), (0, False)], limit=len(groups))
    want = sorted(((k, g[2], g[1]) for k, g in groups.items()),
                  key=lambda r: (-r[1], r[0]))
    assert len({r[1] for r in want}) < len(want) // 10    # heavy ties
    assert _group_rows(cuda, chunk, plan) == want


@functools.lru_cache(maxsize=None)
def group_strings(with_null=False):
    rng = np.random.default_rng(20266)
    keyset = ["a", "aa", "ab", "b", "aaa"] + \
        ["g%04d" % i for i in range(2995)]
    idx = rng.integers(0, len(keyset), NG)
    keys = [keyset[int(i)] for i in idx]
    if with_null:
        keys[1234] = None
    v = rng.integers(0, 10**6, NG, dtype=np.int64)
    chunk = y.Chunk([y.encode_string(keys), y.encode_int64(v)], NG)
    groups = {}
    for ki, vi in zip(keys, v.tolist()):
        if ki is None:
            continue
        g = groups.setdefault(ki.encode(), [0, 0])
        g[0] += vi
        g[1] += 1
    return chunk, groups


@pytest.mark.gpu
def test_i_group_order_string_key(cuda):
    chunk, groups = group_strings()
    assert len(groups) == 3000
    rows = sorted((k, g[0], g[1]) for k, g in groups.items())
    # memcmp, then length: a prefix sorts before its extensions
    assert [r[0] for r in rows[:5]] == [b"a", b"aa", b"aaa", b"ab", b"b"]
    for desc in DIRS:
        want = rows[::-1] if desc else rows
        for offset, limit in ((0, 10), (len(rows) - 10, 50), (len(rows), 5)):
            plan = y.Plan(keys=[y.col(0)],
                          aggs=[y.agg_sum(y.col(1)), y.agg_sum1()],
                          order_by=[(0, desc)], limit=limit, offset=offset)
            assert _group_rows(cuda, chunk, plan) == \
                want[offset:offset + limit]


@pytest.mark.gpu
def test_i_group_order_null_string_key_forbidden(cuda):
    chunk, _ = group_strings(with_null=True)
    plan = y.Plan(keys=[y.col(0)], aggs=[y.agg_sum1()],
                  order_by=[(0, True)], limit=10)
    with pytest.raises(RuntimeError, match="forbidden in group key"):
        y.gpu_execute(plan, chunk.c_device(cuda), max_groups_hint=8192)
