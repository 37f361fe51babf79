"""Microbenchmark: a derive that repacks sparse arena chunks on the device
(lsmb_lset_derive_packed) and the segmented copy kernel behind it, each
against the routes the library had before.  Tables are SSTable filters
(`new(1000, 0.01)`, 1 200 bytes of words each), one row.

(a) kernel: one lsmb_copy_segs_dev over T slots of 1 216 B (HIP events around the
    launch) against T torch slice copies of the same bytes on the same stream,
    the per-table hipMemcpyAsync route (wall clock around the loop and its
    stream synchronisation); the two clocks differ, the work is the same bytes.
(b) edit: lsmb_lset_derive_packed(ALL, drop 4 tables) + one add + seal against
    the plain lsmb_lset_derive + add + seal, and against the only earlier route
    to a dense set: a reload of the T - 3 tables with one lsmb_lset_add_batch.
(c) chain: E edits from a set of T tables with repack None / 0.5 / "all".  A
    compaction edit (drop the 4 oldest tables, add 1) is followed by three
    flush edits (drop none, add 1), so the set stays at T tables over the whole
    chain; every edit is derive + add + seal, then the parent is closed.
    Reports the final chunk_bytes and occupancy, and the median edit time.

Every timed call goes straight to the C ABI through ctypes with its arguments
prepared beforehand.  (b), (c): time.perf_counter around synchronous calls;
closes are outside the timed region.  --warmup rounds of every route first,
then --reps rounds alternating the routes; median, minimum and maximum.
Before timing, every route's bytes or probe answers are checked equal.  Prints
one JSON line per shape and markdown tables.
Usage: python tools/mb_lset_repack.py [--tables 64,512,4096] [--reps 10] [--warmup 3]
                                      [--chain-tables 512] [--edits 1000]
"""
import argparse
import ctypes
import json
import os
import struct
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "storage-engine_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsmbloom  # noqa: E402
from lsmbloom import u32p  # noqa: E402
from mb_lset_load import PER, Batch, borrowed, fmt, p, stats, timed_load  # noqa: E402

vp = ctypes.c_void_p
ALL = lsmbloom.LSMB_LSET_REPACK_ALL
SLOT = 1216


def tables(ctx, dev, n):
    """n serialized SSTable filters built on the device, and their key ranges
    (every key of table t starts with t, big-endian); the member keys too."""
    nb, k = lsmbloom.params(PER, 0.01)
    nw = lsmbloom.num_words(nb)
    mem = torch.empty((n * PER, 16), dtype=torch.uint8, device=dev)
    ctx.gen_key16_dev(0x5EED0A00, 0, n * PER, mem)
    torch.cuda.synchronize()
    tw = (torch.arange(n * PER, device=dev) // PER).to(torch.int64)
    for b in range(4):
        mem[:, b] = ((tw >> (8 * (3 - b))) & 0xFF).to(torch.uint8)
    words = torch.zeros((n, nw), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    for t in range(n):
        ctx.build_fixed_dev(mem[t * PER:(t + 1) * PER], 16, PER, nb, k, words[t])
    torch.cuda.synchronize()
    hw = words.cpu().numpy().view(np.uint64)
    hdr = struct.pack("<III", k, nb, nw)
    blocks = [hdr + hw[t].tobytes() for t in range(n)]
    ranges = [(int(t).to_bytes(4, "big") + b"\x00" * 12, int(t).to_bytes(4, "big") + b"\xff" * 12) for t in range(n)]
    return blocks, ranges, mem


def run_kernel(ctx, dev, T, reps, warmup):
    src = torch.randint(0, 256, (T * SLOT,), dtype=torch.uint8, device=dev)
    dst = torch.zeros(T * SLOT, dtype=torch.uint8, device=dev)
    segs = torch.tensor([[src.data_ptr() + t * SLOT, dst.data_ptr() + t * SLOT, SLOT] for t in range(T)],
                        dtype=torch.int64, device=dev)
    pairs = [(dst[t * SLOT:(t + 1) * SLOT], src[t * SLOT:(t + 1) * SLOT]) for t in range(T)]
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize()

    def kernel():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        ctx.copy_segs_dev(segs, T, stream=st.cuda_stream)
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b)

    def loop():
        with torch.cuda.stream(st):
            t0 = time.perf_counter()
            for d, s in pairs:
                d.copy_(s, non_blocking=True)
            st.synchronize()
            return (time.perf_counter() - t0) * 1e3

    kernel()
    by_kernel = dst.clone()
    dst.zero_()
    torch.cuda.synchronize()
    loop()
    equal = bool(torch.equal(by_kernel, src) and torch.equal(dst, src))
    tk = {"copy_segs": [], "memcpy_loop": []}
    for it in range(warmup + reps):
        a, b = kernel(), loop()
        if it >= warmup:
            tk["copy_segs"].append(a)
            tk["memcpy_loop"].append(b)
    return {n: stats(v) for n, v in tk.items()}, equal


def run_edit(ctx, dev, T, reps, warmup):
    L = lsmbloom.lib()
    blocks, ranges, mem = tables(ctx, dev, T + 1)
    full = Batch(list(range(T)), blocks[:T], ranges[:T])
    drop = [T // 5, 2 * T // 5, 3 * T // 5, 4 * T // 5]
    keep = [t for t in range(T) if t not in drop]
    after = Batch(keep + [T], [blocks[t] for t in keep + [T]], [ranges[t] for t in keep + [T]])
    out1 = Batch([T], [blocks[T]], [ranges[T]])
    drop_a = np.array(drop, dtype=np.uint32)
    q = mem[torch.randperm((T + 1) * PER, device=dev)[:20000]].cpu().numpy()
    _, parent = timed_load(L, ctx, lambda h: full.add_batch(L, h, False))

    def edit(ppm):
        h = vp()
        t0 = time.perf_counter()
        if ppm is None:
            rc = L.lsmb_lset_derive(parent, p(drop_a, u32p), 4, None, ctypes.byref(h))
        else:
            rc = L.lsmb_lset_derive_packed(parent, p(drop_a, u32p), 4, ppm, None, None, ctypes.byref(h), None)
        assert rc == 0, (rc, L.lsmb_last_error())
        out1.add_batch(L, h, False)
        assert L.lsmb_lset_seal(h) == 0
        return (time.perf_counter() - t0) * 1e3, h

    routes = {"derive_packed": lambda: edit(ALL), "derive": lambda: edit(None),
              "reload_batch": lambda: timed_load(L, ctx, lambda h: after.add_batch(L, h, False))}
    answers, st = {}, {}
    for name, run in routes.items():
        _, h = run()
        answers[name] = borrowed(ctx, h, lambda ls: ls.probe(q, key_len=16))
        st[name] = borrowed(ctx, h, lambda ls: ls.stats())
        L.lsmb_lset_close(h)
    tab = np.ascontiguousarray(q[:, :4]).view(">u4").ravel()  # every key is a member of the table its first word names
    gone = np.isin(tab, drop)
    agree = all(np.array_equal(answers["reload_batch"], a) for a in answers.values())
    agree = agree and bool((answers["derive_packed"][0][~gone] == tab[~gone]).all())
    te = {n: [] for n in routes}
    for it in range(warmup + reps):
        for name, run in routes.items():  # alternating
            ms, h = run()
            L.lsmb_lset_close(h)
            if it >= warmup:
                te[name].append(ms)
    L.lsmb_lset_close(parent)
    return {n: stats(v) for n, v in te.items()}, st, bool(agree)


def run_chain(ctx, dev, T, E):
    L = lsmbloom.lib()
    blocks, ranges, mem = tables(ctx, dev, T + E)
    full = Batch(list(range(T)), blocks[:T], ranges[:T])
    ones = [Batch([T + e], [blocks[T + e]], [ranges[T + e]]) for e in range(E)]
    q = mem[torch.randperm((T + E) * PER, device=dev)[:20000]].cpu().numpy()
    res, answers = {}, {}
    for name, ppm in (("none", None), ("0.5", 500000), ("all", ALL)):
        _, cur = timed_load(L, ctx, lambda h: full.add_batch(L, h, False))
        oldest, ms = 0, []
        for e in range(E):
            if e % 4 == 0:  # a compaction: the four oldest tables go
                drop_a = np.arange(oldest, oldest + 4, dtype=np.uint32)
                oldest += 4
            else:           # a flush
                drop_a = np.zeros(0, dtype=np.uint32)
            h = vp()
            t0 = time.perf_counter()
            if ppm is None:
                rc = L.lsmb_lset_derive(cur, p(drop_a, u32p) if drop_a.size else None, drop_a.size, None, ctypes.byref(h))
            else:
                rc = L.lsmb_lset_derive_packed(cur, p(drop_a, u32p) if drop_a.size else None, drop_a.size, ppm, None,
                                               None, ctypes.byref(h), None)
            assert rc == 0, (rc, L.lsmb_last_error())
            ones[e].add_batch(L, h, False)
            assert L.lsmb_lset_seal(h) == 0
            ms.append((time.perf_counter() - t0) * 1e3)
            L.lsmb_lset_close(cur)
            cur = h
        s = borrowed(ctx, cur, lambda ls: ls.stats())
        answers[name] = borrowed(ctx, cur, lambda ls: ls.probe(q, key_len=16))
        L.lsmb_lset_close(cur)
        res[name] = {"edit": stats(ms), "tables": s["tables"], "chunk_bytes": s["chunk_bytes"],
                     "occupancy": round(s["occupancy"], 6)}
    agree = all(np.array_equal(answers["none"], a) for a in answers.values())
    return res, bool(agree)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", default="64,512,4096")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chain-tables", type=int, default=512)
    ap.add_argument("--edits", type=int, default=1000)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = lsmbloom.Context(0)
    res = []
    for T in (int(x) for x in args.tables.split(",")):
        kern, equal = run_kernel(ctx, dev, T, args.reps, args.warmup)
        edit, st, agree = run_edit(ctx, dev, T, args.reps, args.warmup)
        r = {"tables": T, "slot_bytes": SLOT, "reps": args.reps, "warmup": args.warmup, "kernel": kern, "edit": edit,
             "edit_stats": st, "copies_equal": equal, "answers_agree": agree,
             "clock": "HIP events (copy_segs); perf_counter around synchronous calls (memcpy_loop, edit)"}
        print(json.dumps(r), flush=True)
        res.append(r)
    chain, chain_agree = (run_chain(ctx, dev, args.chain_tables, args.edits) if args.edits else ({}, True))
    if chain:
        print(json.dumps({"chain_tables": args.chain_tables, "edits": args.edits, "chain": chain,
                          "answers_agree": chain_agree}), flush=True)
    ctx.close()

    def ratio(a, b):
        return "%.2f×" % (b["median_ms"] / a["median_ms"])

    print("\n| T | `k_copy_segs` (HIP events) | T slice copies (wall clock) | ratio | slowest kernel < fastest loop |"
          "\n|---|---|---|---|---|")
    for r in res:
        k = r["kernel"]
        print("| %d | %s | %s | %s | %s |" % (r["tables"], fmt(k["copy_segs"]), fmt(k["memcpy_loop"]),
                                             ratio(k["copy_segs"], k["memcpy_loop"]),
                                             "yes" if k["copy_segs"]["max_ms"] < k["memcpy_loop"]["min_ms"] else "NO"))
    print("\n| T | `derive_packed(ALL)` + add + `seal` | `derive` + add + `seal` | ratio | reload, `add_batch` | ratio |"
          "\n|---|---|---|---|---|---|")
    for r in res:
        e = r["edit"]
        print("| %d | %s | %s | %s | %s | %s |" % (r["tables"], fmt(e["derive_packed"]), fmt(e["derive"]),
                                                  ratio(e["derive_packed"], e["derive"]), fmt(e["reload_batch"]),
                                                  ratio(e["derive_packed"], e["reload_batch"])))
    if chain:
        print("\n| `repack` | tables | `chunk_bytes` | occupancy | edit |\n|---|---|---|---|---|")
        for name, c in chain.items():
            print("| %s | %d | %d | %.4f | %s |" % (name, c["tables"], c["chunk_bytes"], c["occupancy"], fmt(c["edit"])))
    return 0 if all(r["copies_equal"] and r["answers_agree"] for r in res) and chain_agree else 1


if __name__ == "__main__":
    sys.exit(main())
