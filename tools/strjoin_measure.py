#!/usr/bin/env python
"""String-key join against the same join on an integer key, measured once.

The join workload's shape (bench.py --workload join): a fact chunk joined to
a dimension of --keys unique keys, GROUP BY the fact's integer key with
sum(foreign value) and sum(1). The fact chunk holds the key twice, as an
int64 column and as the dictionary-encoded string "k%09d" of the same number
(bench.py's strgroup generator: every 1Mi rows draw from their own window of
keys, so a 128Ki-row segment holds a few thousand dictionary entries). The
dimension holds both forms too. The two plans differ in the join item alone
and return the same rows, which is asserted.

Prints per-query wall times of the two plans, run alternately, the entries
probed against the rows, and - from a last query of each kind under
YTQL_TIMING - the library's own build / entry-pass / phase lines (stderr).

    python tools/strjoin_measure.py [--rows 2e8] [--keys 1000000] [--rounds 3]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402


def key_ids(b, m, window, seed, i):
    rng = np.random.default_rng([seed, 777, i])
    widx = (b + np.arange(m)) // (bench.SLICE // 2)
    return widx * window + rng.integers(0, window, m)


def key_bytes(ids):
    dig = (ids[:, None] // 10 ** np.arange(8, -1, -1)) % 10
    arr = np.empty((len(ids), 10), dtype=np.uint8)
    arr[:, 0] = ord("k")
    arr[:, 1:] = dig + ord("0")
    return arr.tobytes()


def encode_str(y, ids):
    m = len(ids)
    return y.encode_string_raw(key_bytes(ids), np.arange(m, dtype=np.uint64) * 10,
                               np.full(m, 10, dtype=np.uint32),
                               np.zeros(m, dtype=np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=2e8)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    n = int(args.rows)

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
        rng = np.random.default_rng([bench.SEED, 779, i])
        return (encode_str(y, ids),
                y.encode_int64(ids.astype(np.int64), cum_rows_base=b),
                y.encode_int64(rng.integers(0, 1000, e - b, dtype=np.int64),
                               cum_rows_base=b))

    t0 = time.monotonic()
    with ThreadPoolExecutor(max_workers=threads) as ex:
        parts = list(ex.map(work, enumerate(slices)))
    fact, _ = bench.build_device_chunk([[p[c] for p in parts] for c in range(3)],
                                       n, torch)
    rng = np.random.default_rng([bench.SEED, 999])
    fids = rng.permutation(key_space)
    fval = rng.integers(0, 2 ** bench.VAL_BITS, key_space, dtype=np.int64)
    dim = y.Chunk([encode_str(y, fids), y.encode_int64(fids.astype(np.int64)),
                   y.encode_int64(fval)], key_space)
    ddim = dim.c_device(torch)
    torch.cuda.synchronize()
    print("data: %d rows, %d keys (%d windows of %d), %.1fs"
          % (n, key_space, nwin, window, time.monotonic() - t0), flush=True)

    def plan(kind):
        col = 0 if kind == "str" else 1
        return y.Plan(keys=[y.col(1)], aggs=[y.agg_sum(y.col(3)), y.agg_sum1()],
                      join=y.Join(dim, col, col, [2]))

    plans = {k: plan(k) for k in ("str", "int")}
    rs = y.make_rowset(key_space + 4096, 3)

    def run(kind):
        t = time.monotonic()
        _, st = y.gpu_execute(plans[kind], fact, max_groups_hint=key_space,
                              rowset=rs, raw_rowset=True, join_foreign=ddim)
        return (time.monotonic() - t) * 1e3, st

    rows = {}
    for kind in ("str", "int"):
        got, _ = y.gpu_execute(plans[kind], fact, max_groups_hint=key_space,
                               rowset=rs, join_foreign=ddim)
        rows[kind] = y.sort_rows(got)
        if kind == "str":
            print("string join: inserted %d foreign rows, probed %d entries "
                  "for %d rows" % (y.gpu_debug_last_strjoin() + (n,)), flush=True)
    assert rows["str"] == rows["int"], "the two joins disagree"
    print("rows equal: %d groups" % len(rows["str"]), flush=True)

    for r in range(args.rounds):
        for kind in ("str", "int"):
            for _ in range(args.warmup):
                run(kind)
            ms, scan = [], []
            for _ in range(args.steps):
                w, st = run(kind)
                ms.append(w)
                scan.append(st.kernel_scan_ms)
            print("round %d %s key: wall ms/query %s  median %.2f  scan kernel "
                  "median %.2f" % (r, kind, " ".join("%.2f" % v for v in ms),
                                   float(np.median(ms)), float(np.median(scan))),
                  flush=True)

    os.environ["YTQL_TIMING"] = "1"
    for kind in ("str", "int"):
        print("YTQL_TIMING, %s key:" % kind, file=sys.stderr, flush=True)
        run(kind)


if __name__ == "__main__":
    main()
