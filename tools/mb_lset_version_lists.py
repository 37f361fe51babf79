"""Microbenchmark: the per-table key lists of a whole Version — 8 overlapping
L0 tables plus one sorted, disjoint row of T tables — from one
lsmb_lset_probe_version_lists_dev against the only device route to the same
lists without it: a FilterSet holding the same 8 tables answering
probe_lists_dev, then LevelSet.probe_lists_dev over the row, back to back on
one stream (two XXH3 per key, a second resident copy of the L0 filters).

Shapes and protocol are those of tools/mb_lset_version.py: n device-resident
16-byte keys (default 10 M), half of them members of the row's tables; L0 "sst"
= 8 filters new(1000, 0.01), "mixed" = new(1000), new(5000), new(20000) at
0.01, all spanning the key space; each shape with the keys as fixed 16-byte
keys and again through the variable-length source.  In one process, HIP events
(torch.cuda.Event) around each route, --warmup calls of both first, then --reps
repetitions alternating one call / two calls; median, minimum and maximum of
each.  Before anything is timed the two routes' starts and entries are compared
over all n keys.  Prints one JSON line per shape.
Usage: python tools/mb_lset_version_lists.py [--n 10000000] [--tables 512,4096] [--reps 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "storage-engine_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsmbloom  # noqa: E402
from lsmbloom import FilterSet, LevelSet  # noqa: E402
from mb_lset_version import L0_SIZES, PER, device_filter, stats, timed, with_table_word  # noqa: E402


def run_shape(ctx, dev, T, n, reps, warmup):
    mem = torch.empty((T * PER, 16), dtype=torch.uint8, device=dev)
    ctx.gen_key16_dev(0x5EED0700, 0, T * PER, mem)
    torch.cuda.synchronize()
    with_table_word(mem, torch.arange(T * PER, device=dev) // PER)
    row = [device_filter(ctx, mem[t * PER:(t + 1) * PER], PER) for t in range(T)]
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    half = n // 2
    q = torch.empty((n, 16), dtype=torch.uint8, device=dev)
    q[:half] = mem[torch.randint(0, T * PER, (half,), device=dev, generator=g)]
    torch.cuda.synchronize()
    ctx.gen_key16_dev(0x5EED0800, 0, n - half, q[half:])
    torch.cuda.synchronize()
    with_table_word(q[half:], torch.randint(0, T, (n - half,), device=dev, generator=g))
    q = q[torch.randperm(n, device=dev, generator=g)].contiguous()
    offs = torch.arange(n + 1, dtype=torch.int64, device=dev) * 16
    st = torch.cuda.Stream(dev)  # every probe and both timing events go on this stream
    ok = True
    for l0_name, sizes in L0_SIZES.items():
        ls, fs = LevelSet(ctx), FilterSet(ctx)
        for t, f in enumerate(row):
            ls.add_filter(0, t, f, int(t).to_bytes(4, "big") + b"\x00" * 12, int(t).to_bytes(4, "big") + b"\xff" * 12)
        for j, count in enumerate(sizes):  # members: a random sample of the row's keys
            pick = mem[torch.randint(0, T * PER, (count,), device=dev, generator=g)].contiguous()
            f = device_filter(ctx, pick, count)
            assert fs.add_filter(f, b"", b"\xff" * 16) == j
            ls.add_filter(lsmbloom.LSMB_LSET_ROW_L0, 10_000_000 + j, f, b"", b"\xff" * 16)
        ls.seal()
        T0, V = ls.l0_tables(), ls.version_tables()
        assert T0 == len(sizes) and V == T0 + T
        work_one = torch.empty(ls.version_lists_work_bytes(n), dtype=torch.uint8, device=dev)
        work_two = torch.empty(ls.lists_work_bytes(n), dtype=torch.uint8, device=dev)
        s_one = torch.empty(V + 1, dtype=torch.int64, device=dev)
        s_l0 = torch.empty(65, dtype=torch.int64, device=dev)
        s_row = torch.empty(T + 1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        for src in ("fixed16", "varlen"):
            kw = {"key_len": 16} if src == "fixed16" else {"offsets": offs}
            kw["stream"] = st.cuda_stream
            # capacities from counting calls (the lists do not depend on the key source)
            ls.probe_version_lists_dev(q, n, s_one, None, work_one, **kw)
            st.synchronize()
            e0, total = int(s_one[T0].item()), int(s_one[V].item())
            i_one = torch.full((total,), -1, dtype=torch.int32, device=dev)
            i_l0 = torch.full((e0,), -1, dtype=torch.int32, device=dev)
            i_row = torch.full((total - e0,), -1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()

            def one_call():
                ls.probe_version_lists_dev(q, n, s_one, i_one, work_one, **kw)

            def two_calls():
                fs.probe_lists_dev(q, n, s_l0, i_l0, **kw)
                ls.probe_lists_dev(q, n, s_row, i_row, work_two, **kw)

            one_call()
            two_calls()
            torch.cuda.synchronize()
            agree = (bool(torch.equal(s_one[:T0 + 1], s_l0[:T0 + 1])) and bool(torch.equal(s_one[T0:], s_row + e0))
                     and int(s_l0[64].item()) == e0 and bool(torch.equal(i_one[:e0], i_l0))
                     and bool(torch.equal(i_one[e0:], i_row)))
            for _ in range(warmup):
                one_call()
                two_calls()
            torch.cuda.synchronize()
            a, b = [], []
            for _ in range(reps):  # alternating
                a.append(timed(one_call, st))
                b.append(timed(two_calls, st))
            sa, sb = stats(a), stats(b)
            res = {"l0": l0_name, "l0_tables": T0, "row_tables": T, "n": n, "keys": src, "reps": reps,
                   "one_call": dict(sa, gkeys_s=round(n / sa["median_ms"] / 1e6, 3)),
                   "two_calls": dict(sb, gkeys_s=round(n / sb["median_ms"] / 1e6, 3)),
                   "ratio": round(sb["median_ms"] / sa["median_ms"], 3),
                   "one_call_median_le_two_calls_median": sa["median_ms"] <= sb["median_ms"],
                   "answers_agree": agree, "l0_entries": e0, "entries": total,
                   "work_bytes": {"one_call": int(work_one.numel()), "two_calls_lset": int(work_two.numel())},
                   "clock": "HIP events (torch.cuda.Event)"}
            print(json.dumps(res), flush=True)
            ok = ok and agree
        fs.close()
        ls.close()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--tables", default="512,4096")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = lsmbloom.Context(0)
    ok = True
    for T in (int(x) for x in args.tables.split(",")):
        ok = run_shape(ctx, dev, T, args.n, args.reps, args.warmup) and ok
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
