#!/usr/bin/env python
"""Multi-key GROUP BY with a STRING key against its two baselines, measured once.

One chunk: bench.py's strgroup key column (dictionary-encoded "k%09d", every
1Mi rows draw from their own window of keys), an int64 column that holds the
number inside each row's string (its rank: the precomputed-id baseline), an
int64 column of 16 values and an int64 value column. Three plans:

    str2   GROUP BY (key, small)   sum(col1), sum(1)   string ids
    int2   GROUP BY (rank, small)  sum(col1), sum(1)   integer two-key plan
    str1   GROUP BY key WHERE small >= 0               the single-string-key
                                                       general kernel set

str2 and int2 return the same groups, which is checked on the row count, the
sum of the counts and the sum of the sums. Prints per-query wall times of the
plans, run alternately, the entries the id pass covered against the rows,
and - from a last query of each kind under YTQL_TIMING - the library's own
entry-pass / phase lines (stderr).

    python tools/strkey_measure.py [--rows 2e8] [--keys 100000] [--plans str2,int2,str1]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402

VALUE = np.dtype([("id", "u2"), ("type", "u1"), ("flags", "u1"),
                  ("length", "u4"), ("bits", "u8")])


def key_ids(b, m, window, seed, i):
    rng = np.random.default_rng([seed, 777, i])
    widx = (b + np.arange(m)) // (bench.SLICE // 2)
    return widx * window + rng.integers(0, window, m)


def encode_str(y, ids):
    m = len(ids)
    dig = (ids[:, None] // 10 ** np.arange(8, -1, -1)) % 10
    arr = np.empty((m, 10), dtype=np.uint8)
    arr[:, 0] = ord("k")
    arr[:, 1:] = dig + ord("0")
    return y.encode_string_raw(arr.tobytes(), np.arange(m, dtype=np.uint64) * 10,
                               np.full(m, 10, dtype=np.uint32),
                               np.zeros(m, dtype=np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=2e8)
    ap.add_argument("--keys", type=int, default=100_000)
    ap.add_argument("--plans", default="str2,int2,str1")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    n = int(args.rows)
    kinds = args.plans.split(",")

    import torch
    import ytsaurus_amd as y
    from concurrent.futures import ThreadPoolExecutor
    assert torch.cuda.is_available(), "needs a GPU"

    nwin = (n + bench.SLICE // 2 - 1) // (bench.SLICE // 2)
    window = max(1024, (args.keys + nwin - 1) // nwin)
    key_space = nwin * window
    slices = [(s, min(s + bench.SLICE, n)) for s in range(0, n, bench.SLICE)]
    threads = min(16, os.cpu_count() or 8)

    def work(item):
        i, (b, e) = item
        ids = key_ids(b, e - b, window, bench.SEED, i)
        rng = np.random.default_rng([bench.SEED, 781, i])
        return (encode_str(y, ids),
                y.encode_int64(ids.astype(np.int64), cum_rows_base=b),
                y.encode_int64(rng.integers(0, 16, e - b, dtype=np.int64),
                               cum_rows_base=b),
                y.encode_int64(rng.integers(0, 1000, e - b, dtype=np.int64),
                               cum_rows_base=b))

    t0 = time.monotonic()
    with ThreadPoolExecutor(max_workers=threads) as ex:
        parts = list(ex.map(work, enumerate(slices)))
    chunk, _ = bench.build_device_chunk([[p[c] for p in parts] for c in range(4)],
                                        n, torch)
    torch.cuda.synchronize()
    groups = key_space * 16
    print("data: %d rows, %d keys (%d windows of %d), %.1fs"
          % (n, key_space, nwin, window, time.monotonic() - t0), flush=True)

    aggs = [y.agg_sum(y.col(3)), y.agg_sum1()]
    plans = {"str2": y.Plan(keys=[y.col(0), y.col(2)], aggs=aggs),
             "int2": y.Plan(keys=[y.col(1), y.col(2)], aggs=aggs),
             "str1": y.Plan(filter=y.col(2) >= 0, keys=[y.col(0)], aggs=aggs)}
    rs = y.make_rowset(groups + 4096, 4, pool_bytes=10 * (groups + 4096))
    lib = y._abi.gpu_lib()

    def run(kind):
        t = time.monotonic()
        _, st = y.gpu_execute(plans[kind], chunk, max_groups_hint=groups,
                              rowset=rs, raw_rowset=True)
        return (time.monotonic() - t) * 1e3, st

    sums = {}
    for kind in kinds:
        run(kind)
        ncols = rs.column_count
        v = np.frombuffer(rs._buf, dtype=VALUE,
                          count=rs.row_count * ncols).reshape(rs.row_count, ncols)
        sums[kind] = (int(rs.row_count), int(v[:, ncols - 1]["bits"].sum()),
                      int(v[:, ncols - 2]["bits"].sum()))
        print("%s: scan path 0x%x, %d groups, %d rows counted, sum %d"
              % ((kind, lib.yt_gpu_debug_last_scan_path()) + sums[kind]), flush=True)
        if kind == "str2":
            print("string ids: %d entries, %d distinct for %d rows"
                  % (y.gpu_debug_last_strkey() + (n,)), flush=True)
    if "str2" in sums and "int2" in sums:
        assert sums["str2"] == sums["int2"], "the two plans disagree"
    for kind in sums:
        assert sums[kind][1] == n, "rows lost"

    for r in range(args.rounds):
        for kind in kinds:
            for _ in range(args.warmup):
                run(kind)
            ms, scan = [], []
            for _ in range(args.steps):
                w, st = run(kind)
                ms.append(w)
                scan.append(st.kernel_scan_ms)
            print("round %d %s: wall ms/query %s  median %.2f  scan kernel "
                  "median %.2f" % (r, kind, " ".join("%.2f" % v for v in ms),
                                   float(np.median(ms)), float(np.median(scan))),
                  flush=True)

    os.environ["YTQL_TIMING"] = "1"
    for kind in kinds:
        print("YTQL_TIMING, %s:" % kind, file=sys.stderr, flush=True)
        run(kind)


if __name__ == "__main__":
    main()
