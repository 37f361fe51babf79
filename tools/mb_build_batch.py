"""Microbenchmark: T SSTable filters (`new(1000, 0.01)`, 1 000 16-byte keys
each) built at once, the batched build against the two routes the library had
before it and still has, and the way of the built filters into a level set.

(a) build, keys resident on the device:
      batch      one lsmb_build_batch_dev
      dev_loop   T lsmb_build_fixed_dev_new calls on one stream (per-build
                 timing events off: the loop at its best)
      host_loop  T lsmb_build_fixed calls on host copies of the keys (1 000
                 keys are below lsmb_host_max_keys: the library's host loop)
(b) into a level set (open .. seal timed, closes outside):
      built      lsmb_build_batch_dev + lsmb_lset_add_batch_dev + seal
      host       T lsmb_build_block on the host (build + serialize), one
                 lsmb_lset_add_batch, seal
(c) geometry A/B of the batched build, HIP events, each round after an untimed
    call and in rotating order: the wave class (the default) against every
    table sent to the workgroup class (LSMB_BB_WAVE_MAX_BITS=0) of 1 024 lanes
    and of 256 lanes (LSMB_BB_GROUP_LANES=256).
One more shape, `mixed`: 512 tables of 100 / 1 000 / 5 000 / 20 000 keys in
filters sized new(keys, 0.01): both classes, split tables, device builds on
the host route above lsmb_host_max_keys.

Every call goes straight to the C ABI through ctypes with its arguments
prepared beforehand.  Clock: time.perf_counter around the calls and the
synchronisation of their stream (a launch returns before its kernel ends, and
the dev_loop is bound by its launches, not by its kernels); the batch alone is
also timed with HIP events.  --warmup rounds of every route first, then --reps
rounds alternating the routes; median, minimum and maximum.  Before anything
is timed, every route's words are equal and both level sets answer a probe
batch identically.  Prints one JSON line per shape and markdown tables.
Usage: python tools/mb_build_batch.py [--tables 64,512,4096] [--reps 10] [--warmup 3]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "storage-engine_amd"))
import lsmbloom  # noqa: E402
from lsmbloom import LevelSet, u8p, u32p, u64p  # noqa: E402

vp = ctypes.c_void_p


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(min(ms)), 4),
            "max_ms": round(float(max(ms)), 4)}


def fmt(s):
    return "%.3f ms [%.3f-%.3f]" % (s["median_ms"], s["min_ms"], s["max_ms"])


def p(a, t):
    return a.ctypes.data_as(t)


def run_shape(ctx, dev, name, counts, reps, warmup):
    L = lsmbloom.lib()
    T = len(counts)
    shapes = [lsmbloom.params(max(c, 1), 0.01) for c in counts]
    nb = np.array([s[0] for s in shapes], np.uint32)
    kk = np.array([s[1] for s in shapes], np.uint32)
    seg = np.zeros(T + 1, np.uint64)
    np.cumsum(counts, out=seg[1:])
    n = int(seg[-1])
    woff = lsmbloom.build_batch_layout(nb)
    total = int(woff[-1])
    st = torch.cuda.Stream(dev)
    sp = vp(st.cuda_stream)
    keys = torch.empty((n, 16), dtype=torch.uint8, device=dev)
    ctx.gen_key16_dev(0x5EED0B00, 0, n, keys)
    torch.cuda.synchronize()
    # disjoint ranges for the level set: the first four bytes name the table
    tw = torch.repeat_interleave(torch.arange(T, device=dev), torch.from_numpy(np.asarray(counts)).to(dev))
    for b in range(4):
        keys[:, b] = ((tw >> (8 * (3 - b))) & 0xFF).to(torch.uint8)
    torch.cuda.synchronize()
    hkeys = keys.cpu().numpy()
    words = {r: torch.full((total,), -1, dtype=torch.int64, device=dev)
             for r in ("batch", "dev_loop", "group1024", "group256")}
    hwords = np.zeros(total, np.uint64)
    kp = keys.data_ptr()
    per_dev = [(vp(kp + 16 * int(seg[t])), int(counts[t]), int(nb[t]), int(kk[t]),
                vp(words["dev_loop"].data_ptr() + 8 * int(woff[t]))) for t in range(T)]
    hk0, hw0 = hkeys.ctypes.data, hwords.ctypes.data
    per_host = [(ctypes.cast(hk0 + 16 * int(seg[t]), u8p), int(counts[t]), int(nb[t]), int(kk[t]),
                 ctypes.cast(hw0 + 8 * int(woff[t]), u64p)) for t in range(T)]
    segp, nbp, kkp = p(seg, u64p), p(nb, u32p), p(kk, u32p)

    def batch(dst="batch"):
        rc = L.lsmb_build_batch_dev(ctx.h, vp(kp), None, 16, n, T, segp, nbp, kkp, vp(words[dst].data_ptr()), total, sp)
        assert rc == 0, L.lsmb_last_error()

    def group_only(lanes):
        os.environ["LSMB_BB_WAVE_MAX_BITS"] = "0"
        os.environ["LSMB_BB_GROUP_LANES"] = str(lanes)
        try:
            batch("group%d" % lanes)
        finally:
            del os.environ["LSMB_BB_WAVE_MAX_BITS"]
            del os.environ["LSMB_BB_GROUP_LANES"]

    geoms = [("wave", batch), ("group1024", lambda: group_only(1024)), ("group256", lambda: group_only(256))]

    def dev_loop():
        for k, c, b, h, w in per_dev:
            rc = L.lsmb_build_fixed_dev_new(ctx.h, k, 16, c, b, h, w, sp)
            assert rc == 0, rc

    def host_loop():
        hwords[:] = 0
        for k, c, b, h, w in per_host:
            rc = L.lsmb_build_fixed(ctx.h, k, 16, c, b, h, w)
            assert rc == 0, rc

    def wall(fn, sync=True):
        t0 = time.perf_counter()
        fn()
        if sync:
            st.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b)

    ctx.set_timing(False)
    # (b) the two routes into a level set
    rows = np.zeros(T, np.uint32)
    ids = np.arange(T, dtype=np.uint32)
    rk = b"".join(int(t).to_bytes(4, "big") + b"\x00" * 12 + int(t).to_bytes(4, "big") + b"\xff" * 12 for t in range(T))
    rkeys = np.frombuffer(rk, np.uint8).copy()
    koff = np.arange(0, 32 * T + 1, 16, dtype=np.uint64)
    boff = np.zeros(T + 1, np.uint64)
    np.cumsum([lsmbloom.serialized_size(int(b)) for b in nb], out=boff[1:])
    blocks = np.zeros(int(boff[-1]), np.uint8)
    b0 = blocks.ctypes.data
    per_block = [(ctypes.cast(hk0 + 16 * int(seg[t]), u8p), int(counts[t]), int(nb[t]), int(kk[t]),
                  ctypes.cast(b0 + int(boff[t]), u8p), int(boff[t + 1] - boff[t])) for t in range(T)]
    lwords = torch.full((total,), -1, dtype=torch.int64, device=dev)

    def set_built(h):
        rc = L.lsmb_build_batch_dev(ctx.h, vp(kp), None, 16, n, T, segp, nbp, kkp, vp(lwords.data_ptr()), total, sp)
        assert rc == 0, L.lsmb_last_error()
        rc = L.lsmb_lset_add_batch_dev(h, T, p(rows, u32p), p(ids, u32p), vp(lwords.data_ptr()), p(woff, u64p), nbp, kkp,
                                       p(rkeys, u8p), p(koff, u64p), sp)
        assert rc == 0, L.lsmb_last_error()

    def set_host(h):
        for k, c, b, hh, blk, blen in per_block:
            rc = L.lsmb_build_block(ctx.h, k, None, 16, c, b, hh, blk, blen)
            assert rc == 0, rc
        rc = L.lsmb_lset_add_batch(h, T, p(rows, u32p), p(ids, u32p), p(blocks, u8p), p(boff, u64p), None,
                                   p(rkeys, u8p), p(koff, u64p), None)
        assert rc == 0, L.lsmb_last_error()

    def timed_set(fill):
        h = vp()
        t0 = time.perf_counter()
        assert L.lsmb_lset_open(ctx.h, ctypes.byref(h)) == 0
        fill(h)
        assert L.lsmb_lset_seal(h) == 0
        return (time.perf_counter() - t0) * 1e3, h

    def answers(h, q):
        ls = LevelSet.__new__(LevelSet)
        ls.ctx, ls.h = ctx, h
        try:
            return ls.probe(q, key_len=16)
        finally:
            ls.h = None

    # equality first: every route's words, both sets' answers
    for fn in [g[1] for g in geoms] + [dev_loop]:
        fn()
    st.synchronize()
    host_loop()
    ref = words["batch"].cpu().numpy().view(np.uint64)
    equal = True
    for t in range(T):
        a, nw = int(woff[t]), (int(nb[t]) + 63) // 64
        for other in [words[r].cpu().numpy().view(np.uint64) for r in ("dev_loop", "group1024", "group256")] + [hwords]:
            equal = equal and bool(np.array_equal(ref[a:a + nw], other[a:a + nw]))
    q = hkeys[np.random.default_rng(7).integers(0, n, 20000)]
    _, h1 = timed_set(set_built)
    _, h2 = timed_set(set_host)
    a1, a2 = answers(h1, q), answers(h2, q)
    agree = bool(np.array_equal(a1, a2)) and bool((a1[0] == np.ascontiguousarray(q[:, :4]).view(">u4").ravel()).all())
    L.lsmb_lset_close(h1)
    L.lsmb_lset_close(h2)
    assert equal and agree, (equal, agree)

    tm = {r: [] for r in ("batch", "batch_events", "dev_loop", "host_loop", "set_built", "set_host", "ab_wave",
                          "ab_group1024", "ab_group256")}
    for it in range(warmup + reps):
        got = {"batch": wall(batch), "batch_events": events(batch), "dev_loop": wall(dev_loop),
               "host_loop": wall(host_loop, sync=False)}
        wall(batch)  # the A/B starts from a busy device
        for j in range(3):
            gname, fn = geoms[(it + j) % 3]
            got["ab_" + gname] = events(fn)
        for r, fill in (("set_built", set_built), ("set_host", set_host)):
            ms, h = timed_set(fill)
            L.lsmb_lset_close(h)
            got[r] = ms
        if it >= warmup:
            for r, ms in got.items():
                tm[r].append(ms)
    ctx.set_timing(True)
    res = {"shape": name, "tables": T, "keys": n, "filter_words": total, "reps": reps, "warmup": warmup,
           "times": {r: stats(v) for r, v in tm.items()}, "words_equal": equal, "answers_agree": agree,
           "batch_slowest_below_dev_loop_fastest": bool(max(tm["batch"]) < min(tm["dev_loop"])),
           "clock": "perf_counter around the calls and the stream's synchronise; batch_events: HIP events"}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", default="64,512,4096")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-mixed", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = lsmbloom.Context(0)
    todo = [("T=%s" % x, [1000] * int(x)) for x in args.tables.split(",") if x]
    if not args.no_mixed:
        todo.append(("mixed", [(100, 1000, 5000, 20000)[t % 4] for t in range(512)]))
    res = [run_shape(ctx, dev, name, counts, args.reps, args.warmup) for name, counts in todo]
    ctx.close()

    def ratio(new, old):
        return "%.2f×" % (old["median_ms"] / new["median_ms"])

    print("\n| shape | `build_batch_dev` | HIP events | T × `build_fixed_dev_new` | ratio | T × host build | ratio | "
          "slowest batch < fastest loop |\n|---|---|---|---|---|---|---|---|")
    for r in res:
        t = r["times"]
        print("| %s | %s | %s | %s | %s | %s | %s | %s |" % (
            r["shape"], fmt(t["batch"]), fmt(t["batch_events"]), fmt(t["dev_loop"]), ratio(t["batch"], t["dev_loop"]),
            fmt(t["host_loop"]), ratio(t["batch"], t["host_loop"]),
            "yes" if r["batch_slowest_below_dev_loop_fastest"] else "NO"))
    print("\n| shape | build + `add_built` + `seal` | host builds + `add_batch` + `seal` | ratio |\n|---|---|---|---|")
    for r in res:
        t = r["times"]
        print("| %s | %s | %s | %s |" % (r["shape"], fmt(t["set_built"]), fmt(t["set_host"]),
                                        ratio(t["set_built"], t["set_host"])))
    print("\n| shape | wave class (default) | all tables: 1 024-lane workgroups | ratio | all tables: 256-lane workgroups | "
          "ratio |\n|---|---|---|---|---|---|")
    for r in res:
        t = r["times"]
        print("| %s | %s | %s | %s | %s | %s |" % (r["shape"], fmt(t["ab_wave"]), fmt(t["ab_group1024"]),
                                                  ratio(t["ab_wave"], t["ab_group1024"]), fmt(t["ab_group256"]),
                                                  ratio(t["ab_wave"], t["ab_group256"])))
    return 0 if all(r["words_equal"] and r["answers_agree"] for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
