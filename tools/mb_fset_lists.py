"""Microbenchmark: what a batched DB::get pays to learn, per table, which keys
to look up — mask rows brought home against per-table key lists.

The README's filter-set shape (bench.ProbeLegs: 10 M 16-B keys, half of them
members, 8 SST-sized filters with their key ranges, one-byte rows).  In one
process, HIP events over --reps repetitions after warm-up:
  (a) probe_dev(row_bytes=1) + D2H of the n rows to pinned memory
  (b) probe_lists_dev + D2H of starts, then of the `total` entries
and the two probes alone.  --absent probes only the batch's fresh half (n / 2
keys no table holds: the entries are the filters' false positives), the
sparse answer of a miss-dominated batch.  Not in either figure: the scan of
the n rows on a CPU thread that (a) still needs to get the lists (b) already is.
Prints one JSON line.  Usage: python tools/mb_fset_lists.py [--reps 20] [--n 10000000] [--absent]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "storage-engine_amd"))
import bench  # noqa: E402  (the shared probe setup: ProbeLegs)
import lsmbloom  # noqa: E402


def timed(fn, reps):
    """Median and minimum ms of fn() over reps, each between two events."""
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--tables", type=int, default=8, help="at most 8: one-byte rows")
    ap.add_argument("--absent", action="store_true", help="probe only the fresh half of the batch")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, F = args.n, args.tables
    ctx = lsmbloom.Context(0)
    P = bench.ProbeLegs(ctx, dev, n, F)
    fs, q = P.fs, P.q
    if args.absent:  # ProbeLegs: the first half are members, the rest fresh keys
        q = q[n // 2:]
        n = q.shape[0]
    rows = torch.zeros(n, dtype=torch.uint8, device=dev)
    rows_h = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    starts = torch.zeros(65, dtype=torch.int64, device=dev)
    starts_h = torch.empty(65, dtype=torch.int64, pin_memory=True)
    # sized by a counting call, as a caller that keeps its buffers would
    fs.probe_lists_dev(q, n, starts, None, key_len=16)
    torch.cuda.synchronize()
    total = int(starts.cpu()[64])
    index = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)
    index_h = torch.empty(max(total, 1), dtype=torch.int32, pin_memory=True)

    def mask_probe():
        fs.probe_dev(q, n, rows, key_len=16, row_bytes=1)

    def lists_probe():
        fs.probe_lists_dev(q, n, starts, index, key_len=16)

    def path_a():
        mask_probe()
        rows_h.copy_(rows, non_blocking=True)

    def path_b():
        lists_probe()
        starts_h.copy_(starts, non_blocking=True)
        torch.cuda.current_stream().synchronize()  # the caller reads total before it copies the entries
        t = int(starts_h[64])
        index_h[:t].copy_(index[:t], non_blocking=True)

    res = {"n": n, "tables": F, "absent": args.absent, "total_entries": total, "reps": args.reps,
           "bytes_home_a": n, "bytes_home_b": 65 * 8 + 4 * total}
    for name, fn in (("mask_probe", mask_probe), ("lists_probe", lists_probe), ("a_rows_home", path_a),
                     ("b_lists_home", path_b)):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        med, lo = timed(fn, args.reps)
        res[name + "_ms"] = round(med, 4)
        res[name + "_min_ms"] = round(lo, 4)
    # the two answers agree: the lists are the rows' transpose
    m = rows_h.numpy()
    st = starts_h.numpy().view(np.uint64)
    ix = index_h.numpy().view(np.uint32)
    ok = int(st[64]) == total
    for s in range(64):
        ok = ok and np.array_equal(ix[int(st[s]):int(st[s + 1])], np.nonzero((m >> (s & 7)) & 1)[0] if s < 8 else [])
    res["lists_equal_rows"] = bool(ok)
    print(json.dumps(res), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
