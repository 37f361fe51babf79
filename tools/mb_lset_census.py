"""Microbenchmark: the fill census of a resident Version (lsmb_lset_census) and
the segmented popcount kernel behind it, next to the CRC kernel that reads the
same bytes.  Tables are SSTable filters (`new(1000, 0.01)`: 9 568 bits, 1 200
bytes of words each, random words), one row.

(a) census: lsmb_lset_census of a sealed set of T tables, the whole call (the
    host's plan, the upload of the items, the launch, the copy back, the wait,
    the fold): HIP events on the call's stream around it, and the wall clock.
(b) kernels: one lsmb_popcount_segs_dev over the census' items laid out in a
    buffer of the benchmark's own (T slots of 1 216 B), HIP events around the
    launch, and one lsmb_crc32_seg_dev over the same segments (byte lengths in
    place of bit counts) in the same process, alternating.
(c) --big-mib M: a set of 512 such tables and one of M MiB; the kernels run
    over its 64 KiB items, which the CRC kernel takes too.

GB/s = the words' bytes over the median time, against the 6.29 TB/s copy rate
of DESIGN.md section 5.1.  --warmup rounds first, then --reps rounds; median,
minimum and maximum.  Before timing, the census is checked against numpy's
count of the words.  Prints one JSON line per shape and a markdown table.
Usage: python tools/mb_lset_census.py [--tables 512,4096,65536] [--big-mib 64] [--reps 10] [--warmup 3]
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
from lsmbloom import LevelSet, u64p  # noqa: E402
from mb_lset_load import PER, fmt, p, stats  # noqa: E402

vp = ctypes.c_void_p
COPY_GBS = 6290.0
ITEM = 64 << 10    # the census' item cut (csrc/popcount_seg.hpp)
POP8 = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.uint64)


def count(words, nbits):
    """Set bits below nbits of LE words given as bytes (nbits a multiple of 8 here)."""
    assert nbits % 8 == 0
    return int(POP8[words[:nbits // 8]].sum())


def make_set(ctx, T, big_bits):
    """A sealed set of T SST-sized tables of random words (and one of big_bits
    bits, id T, when big_bits), its tables' (bytes, bits) in version order."""
    nb, k = lsmbloom.params(PER, 0.01)
    nw = lsmbloom.num_words(nb)
    rng = np.random.default_rng(0x5EEDCE25)
    raw = rng.integers(0, 256, (T, nw * 8), dtype=np.uint8)
    hdr = struct.pack("<III", k, nb, nw)
    blocks = [hdr + raw[t].tobytes() for t in range(T)]
    tabs = [(raw[t], nb) for t in range(T)]
    if big_bits:
        big = rng.integers(0, 256, big_bits // 8, dtype=np.uint8)
        blocks.append(struct.pack("<III", k, big_bits, big_bits // 64) + big.tobytes())
        tabs.append((big, big_bits))
    ranges = [(int(t).to_bytes(4, "big") + b"\x00" * 12, int(t).to_bytes(4, "big") + b"\xff" * 12)
              for t in range(len(blocks))]
    ls = LevelSet(ctx)
    ls.add_many([0] * len(blocks), list(range(len(blocks))), blocks, ranges)
    ls.seal()
    return ls, tabs


def run_shape(ctx, dev, T, big_bits, reps, warmup):
    L = lsmbloom.lib()
    ls, tabs = make_set(ctx, T, big_bits)
    V = len(tabs)
    exp = np.array([count(w, nb) for w, nb in tabs], dtype=np.uint64)
    got = ls.census()[3]
    equal = bool(np.array_equal(got, exp))
    nbytes = sum((nb + 63) // 64 * 8 for _, nb in tabs)
    st = torch.cuda.Stream(dev)
    sb = np.zeros(V, np.uint64)

    def census():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        t0 = time.perf_counter()
        rc = L.lsmb_lset_census(ls.h, p(sb, u64p), vp(st.cuda_stream))
        wall = (time.perf_counter() - t0) * 1e3
        b.record(st)
        b.synchronize()
        assert rc == 0, (rc, L.lsmb_last_error())
        return a.elapsed_time(b), wall

    # the same segments in a buffer of the benchmark's own: 16-byte slots back to back, cut as the census cuts
    slots, at = [], 0
    for w, nb in tabs:
        slots.append(at)
        at += (w.size + 15) // 16 * 16
    host = np.zeros(at + 16, np.uint8)
    for (w, nb), a in zip(tabs, slots):
        host[a:a + w.size] = w
    buf = torch.from_numpy(host).to(dev)
    pop, crc, item_tab = [], [], []
    for t, ((w, nb), a) in enumerate(zip(tabs, slots)):
        for off in range(0, w.size, ITEM):
            n = min(ITEM, w.size - off)
            pop.append([buf.data_ptr() + a + off, min(ITEM * 8, nb - off * 8)])
            crc.append([buf.data_ptr() + a + off, n])
            item_tab.append(t)
    nit = len(pop)
    d_pop = torch.tensor(pop, dtype=torch.int64, device=dev)
    d_crc = torch.tensor(crc, dtype=torch.int64, device=dev)
    o_pop = torch.zeros(nit, dtype=torch.int64, device=dev)
    o_crc = torch.zeros(nit, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def kernel(fn, segs, out):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn(segs, nit, out, stream=st.cuda_stream)
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b)

    kernel(ctx.popcount_segs_dev, d_pop, o_pop)
    folded = np.zeros(V, np.uint64)
    np.add.at(folded, np.array(item_tab), o_pop.cpu().numpy().view(np.uint64))
    equal = equal and bool(np.array_equal(folded, exp))
    tk = {"census_events": [], "census_wall": [], "popcount_segs": [], "crc32_seg": []}
    for it in range(warmup + reps):
        ev, wall = census()
        a = kernel(ctx.popcount_segs_dev, d_pop, o_pop)
        b = kernel(ctx.crc32_seg_dev, d_crc, o_crc)
        if it >= warmup:
            tk["census_events"].append(ev)
            tk["census_wall"].append(wall)
            tk["popcount_segs"].append(a)
            tk["crc32_seg"].append(b)
    ls.close()
    res = {n: stats(v) for n, v in tk.items()}
    for n in res:
        res[n]["gb_s"] = round(nbytes / (res[n]["median_ms"] * 1e-3) / 1e9, 2)
    return {"tables": V, "big_bits": big_bits, "items": nit, "filter_bytes": nbytes, "reps": reps, "warmup": warmup,
            "counts_equal": equal, "times": res,
            "clock": "HIP events (census_events, popcount_segs, crc32_seg); perf_counter around the call (census_wall)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", default="512,4096,65536")
    ap.add_argument("--big-mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = lsmbloom.Context(0)
    shapes = [(int(x), 0) for x in args.tables.split(",") if x]
    if args.big_mib:
        shapes.append((512, args.big_mib << 23))
    res = []
    for T, big in shapes:
        r = run_shape(ctx, dev, T, big, args.reps, args.warmup)
        print(json.dumps(r), flush=True)
        res.append(r)
    ctx.close()

    def cell(s):
        return "%s, %.1f GB/s (%.1f %%)" % (fmt(s), s["gb_s"], 100.0 * s["gb_s"] / COPY_GBS)

    print("\n| tables | items | bytes | `lsmb_lset_census` (HIP events) | (wall clock) | `k_popcount_segs` | `k_crc32_seg` |"
          "\n|---|---|---|---|---|---|---|")
    for r in res:
        t = r["times"]
        print("| %d%s | %d | %d | %s | %s | %s | %s |" % (
            r["tables"], " (one of %d MiB)" % (r["big_bits"] >> 23) if r["big_bits"] else "", r["items"],
            r["filter_bytes"], fmt(t["census_events"]), fmt(t["census_wall"]), cell(t["popcount_segs"]),
            cell(t["crc32_seg"])))
    return 0 if all(r["counts_equal"] for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
