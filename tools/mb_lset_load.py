"""Microbenchmark: the life cycle of a level set of T SSTable filters
(`new(1000, 0.01)`, one row), each new route against the route the library
had before it and still has.

(a) load: one lsmb_lset_add_batch (without and with CRCs, the CRCs checked on
    the device copies by one k_crc32_seg launch) against T lsmb_lset_add
    calls, one synchronous copy each.  Timed: open, the adds, seal.
(b) version edit: lsmb_lset_derive (drop 4 tables) + one add + seal against a
    full reload of the T - 3 tables the new Version holds, by the per-table
    loop and by one batch.
(c) CRC: k_crc32_seg over the T blocks' words in device memory (HIP events
    around one lsmb_crc32_seg_dev) against T lsmb_crc32 calls on the host
    (wall clock); the two clocks differ, the work is the same bytes.

Every call goes straight to the C ABI through ctypes with its arguments
prepared beforehand, so no Python packing is inside a timed region.  (a) and
(b): time.perf_counter around synchronous calls; closes are outside the timed
region.  --warmup rounds of every route first, then --reps rounds
alternating the routes; median, minimum and maximum.  Before timing, every
route's set answers a probe batch identically and the device CRCs equal
zlib's.  Prints one JSON line per shape and a markdown table.
Usage: python tools/mb_lset_load.py [--tables 64,512,4096] [--reps 10] [--warmup 3]
"""
import argparse
import ctypes
import json
import os
import struct
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "storage-engine_amd"))
import lsmbloom  # noqa: E402
from lsmbloom import LevelSet, u8p, u32p, u64p  # noqa: E402

PER = 1000  # keys per table
vp = ctypes.c_void_p


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(min(ms)), 4),
            "max_ms": round(float(max(ms)), 4)}


def fmt(s):
    return "%.3f ms [%.3f-%.3f]" % (s["median_ms"], s["min_ms"], s["max_ms"])


def p(a, t):
    return a.ctypes.data_as(t)


class Batch:
    """T tables prepared for both routes: the batch arrays and per-table pointers."""

    def __init__(self, ids, blocks, ranges):
        self.n = len(ids)
        self.rows = np.zeros(self.n, np.uint32)
        self.ids = np.ascontiguousarray(ids, dtype=np.uint32)
        self.boff = np.zeros(self.n + 1, np.uint64)
        np.cumsum([len(b) for b in blocks], out=self.boff[1:])
        self.blocks = np.frombuffer(b"".join(blocks), dtype=np.uint8).copy()
        flat = [k for r in ranges for k in r]
        self.koff = np.zeros(2 * self.n + 1, np.uint64)
        np.cumsum([len(k) for k in flat], out=self.koff[1:])
        self.keys = np.frombuffer(b"".join(flat), dtype=np.uint8).copy()
        self.crcs = np.array([zlib.crc32(b) for b in blocks], dtype=np.uint32)
        self.status = np.zeros(self.n, np.int32)
        b0, k0 = self.blocks.ctypes.data, self.keys.ctypes.data
        self.per_table = [(int(self.ids[t]), ctypes.cast(b0 + int(self.boff[t]), u8p), int(self.boff[t + 1] - self.boff[t]),
                           ctypes.cast(k0 + int(self.koff[2 * t]), u8p), int(self.koff[2 * t + 1] - self.koff[2 * t]),
                           ctypes.cast(k0 + int(self.koff[2 * t + 1]), u8p),
                           int(self.koff[2 * t + 2] - self.koff[2 * t + 1])) for t in range(self.n)]

    def add_loop(self, L, h):
        for tid, b, nb, lo, nlo, hi, nhi in self.per_table:
            rc = L.lsmb_lset_add(h, 0, tid, b, nb, lo, nlo, hi, nhi)
            assert rc == 0, rc

    def add_batch(self, L, h, crc):
        rc = L.lsmb_lset_add_batch(h, self.n, p(self.rows, u32p), p(self.ids, u32p), p(self.blocks, u8p),
                                   p(self.boff, u64p), p(self.crcs, u32p) if crc else None, p(self.keys, u8p),
                                   p(self.koff, u64p), p(self.status, ctypes.POINTER(ctypes.c_int32)))
        assert rc == 0, (rc, L.lsmb_last_error())


def timed_load(L, ctx, fill):
    """ms of open + fill + seal; returns (ms, handle)."""
    h = vp()
    t0 = time.perf_counter()
    assert L.lsmb_lset_open(ctx.h, ctypes.byref(h)) == 0
    fill(h)
    assert L.lsmb_lset_seal(h) == 0
    return (time.perf_counter() - t0) * 1e3, h


def borrowed(ctx, h, fn):
    """fn(LevelSet over handle h); the handle stays the caller's."""
    ls = LevelSet.__new__(LevelSet)
    ls.ctx, ls.h = ctx, h
    try:
        return fn(ls)
    finally:
        ls.h = None


def run_shape(ctx, dev, T, reps, warmup):
    L = lsmbloom.lib()
    nb, k = lsmbloom.params(PER, 0.01)
    nw = lsmbloom.num_words(nb)
    # T + 1 filters built on the device (the last one is the compaction's output of (b))
    mem = torch.empty(((T + 1) * PER, 16), dtype=torch.uint8, device=dev)
    ctx.gen_key16_dev(0x5EED0900, 0, (T + 1) * PER, mem)
    torch.cuda.synchronize()
    tw = (torch.arange((T + 1) * PER, device=dev) // PER).to(torch.int64)
    for b in range(4):
        mem[:, b] = ((tw >> (8 * (3 - b))) & 0xFF).to(torch.uint8)
    words = torch.zeros((T + 1, nw), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    for t in range(T + 1):
        ctx.build_fixed_dev(mem[t * PER:(t + 1) * PER], 16, PER, nb, k, words[t])
    torch.cuda.synchronize()
    hw = words.cpu().numpy().view(np.uint64)
    hdr = struct.pack("<III", k, nb, nw)
    blocks = [hdr + hw[t].tobytes() for t in range(T + 1)]
    ranges = [(int(t).to_bytes(4, "big") + b"\x00" * 12, int(t).to_bytes(4, "big") + b"\xff" * 12) for t in range(T + 1)]
    full = Batch(list(range(T)), blocks[:T], ranges[:T])
    drop = [T // 5, 2 * T // 5, 3 * T // 5, 4 * T // 5]
    keep = [t for t in range(T) if t not in drop]
    after = Batch(keep + [T], [blocks[t] for t in keep + [T]], [ranges[t] for t in keep + [T]])
    out1 = Batch([T], [blocks[T]], [ranges[T]])
    drop_a = np.array(drop, dtype=np.uint32)
    # probe batch for the equality checks: members of every table
    q = mem[torch.randperm((T + 1) * PER, device=dev)[:20000]].cpu().numpy()

    routes_a = {"loop": lambda h: full.add_loop(L, h), "batch": lambda h: full.add_batch(L, h, False),
                "batch_crc": lambda h: full.add_batch(L, h, True)}

    def derive_edit(parent):
        h = vp()
        t0 = time.perf_counter()
        assert L.lsmb_lset_derive(parent, p(drop_a, u32p), 4, None, ctypes.byref(h)) == 0
        out1.add_batch(L, h, False)
        assert L.lsmb_lset_seal(h) == 0
        return (time.perf_counter() - t0) * 1e3, h

    routes_b = {"reload_loop": lambda h: after.add_loop(L, h), "reload_batch": lambda h: after.add_batch(L, h, False)}

    # answers agree, route by route
    answers = {}
    for name, fill in routes_a.items():
        _, h = timed_load(L, ctx, fill)
        answers[name] = borrowed(ctx, h, lambda ls: ls.probe(q, key_len=16))
        if name != "loop":
            L.lsmb_lset_close(h)
        else:
            parent = h
    agree = all(np.array_equal(answers["loop"], a) for a in answers.values())
    tab = np.ascontiguousarray(q[:, :4]).view(">u4").ravel()  # every key is a member of the table its first word names
    agree = agree and bool((answers["loop"][0][tab < T] == tab[tab < T]).all())
    _, hd = derive_edit(parent)
    ad = borrowed(ctx, hd, lambda ls: ls.probe(q, key_len=16))
    st_d = borrowed(ctx, hd, lambda ls: ls.stats())
    L.lsmb_lset_close(hd)
    for name, fill in routes_b.items():
        _, h = timed_load(L, ctx, fill)
        agree = agree and np.array_equal(ad, borrowed(ctx, h, lambda ls: ls.probe(q, key_len=16)))
        L.lsmb_lset_close(h)

    ta = {n: [] for n in routes_a}
    tb = {n: [] for n in list(routes_b) + ["derive"]}
    for it in range(warmup + reps):
        for name, fill in routes_a.items():  # alternating
            ms, h = timed_load(L, ctx, fill)
            L.lsmb_lset_close(h)
            if it >= warmup:
                ta[name].append(ms)
        ms, h = derive_edit(parent)
        L.lsmb_lset_close(h)
        if it >= warmup:
            tb["derive"].append(ms)
        for name, fill in routes_b.items():
            ms, h = timed_load(L, ctx, fill)
            L.lsmb_lset_close(h)
            if it >= warmup:
                tb[name].append(ms)
    L.lsmb_lset_close(parent)

    # (c) the segmented kernel alone over the T blocks' words, 16-byte-aligned slots
    slot = (nw * 8 + 15) // 16 * 16
    dwords = torch.zeros(T * slot, dtype=torch.uint8, device=dev)
    dwords.view(T, slot)[:, :nw * 8] = torch.from_numpy(hw[:T].view(np.uint8).reshape(T, nw * 8)).to(dev)
    segs = torch.tensor([[dwords.data_ptr() + t * slot, nw * 8] for t in range(T)], dtype=torch.int64, device=dev)
    dout = torch.zeros(T, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    wbytes = [hw[t].tobytes() for t in range(T)]
    wptr = [(np.frombuffer(w, dtype=np.uint8), len(w)) for w in wbytes]
    wptr = [(p(a, u8p), n) for a, n in wptr]

    def dev_crc():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        ctx.crc32_seg_dev(segs, T, dout, stream=st.cuda_stream)
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b)

    def host_crc():
        t0 = time.perf_counter()
        for ptr, n in wptr:
            L.lsmb_crc32(0, ptr, n)
        return (time.perf_counter() - t0) * 1e3

    dev_crc()
    crc_ok = bool(np.array_equal(dout.cpu().numpy().view(np.uint32),
                                 np.array([zlib.crc32(w) for w in wbytes], dtype=np.uint32)))
    tc = {"seg_kernel": [], "host": []}
    for it in range(warmup + reps):
        d, hh = dev_crc(), host_crc()
        if it >= warmup:
            tc["seg_kernel"].append(d)
            tc["host"].append(hh)

    res = {"tables": T, "num_bits": nb, "k": k, "block_bytes": 12 + 8 * nw, "reps": reps, "warmup": warmup,
           "load": {n: stats(v) for n, v in ta.items()}, "edit": {n: stats(v) for n, v in tb.items()},
           "crc": {n: stats(v) for n, v in tc.items()}, "derived_stats": st_d, "answers_agree": bool(agree),
           "crcs_equal_zlib": crc_ok,
           "clock": "perf_counter around synchronous calls (load, edit, host crc); HIP events (seg_kernel)"}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", default="64,512,4096")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = lsmbloom.Context(0)
    res = [run_shape(ctx, dev, int(x), args.reps, args.warmup) for x in args.tables.split(",")]
    ctx.close()

    def ratio(a, b):
        return "%.2f×" % (b["median_ms"] / a["median_ms"])

    print("\n| T | `add` loop | `add_batch` | ratio | `add_batch` + CRCs | ratio |\n|---|---|---|---|---|---|")
    for r in res:
        l = r["load"]
        print("| %d | %s | %s | %s | %s | %s |" % (r["tables"], fmt(l["loop"]), fmt(l["batch"]), ratio(l["batch"], l["loop"]),
                                                  fmt(l["batch_crc"]), ratio(l["batch_crc"], l["loop"])))
    print("\n| T | `derive` + add + `seal` | reload, `add` loop | ratio | reload, `add_batch` | ratio |\n|---|---|---|---|---|---|")
    for r in res:
        e = r["edit"]
        print("| %d | %s | %s | %s | %s | %s |" % (r["tables"], fmt(e["derive"]), fmt(e["reload_loop"]),
                                                  ratio(e["derive"], e["reload_loop"]), fmt(e["reload_batch"]),
                                                  ratio(e["derive"], e["reload_batch"])))
    print("\n| T | `k_crc32_seg` (HIP events) | T host `lsmb_crc32` (wall clock) | ratio |\n|---|---|---|---|")
    for r in res:
        c = r["crc"]
        print("| %d | %s | %s | %s |" % (r["tables"], fmt(c["seg_kernel"]), fmt(c["host"]), ratio(c["seg_kernel"], c["host"])))
    return 0 if all(r["answers_agree"] and r["crcs_equal_zlib"] for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
