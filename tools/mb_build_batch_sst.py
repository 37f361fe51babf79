"""Microbenchmark: T SSTable filters built at once straight from the tables'
data blocks (lsmb_build_batch_sst_dev) against the same filters from packed
keys already on the device (lsmb_build_batch_dev: the existing route's kernel
floor — it reads 12 bytes per key where the blocks route reads the values too).

Tables: 1 000 twelve-byte keys with 100-byte values in 4 KiB blocks cut by
BlockBuilder::add's rule (src/sstable/block/builder.rs:41-47: 34 entries per
block, 30 blocks per table), filters new(1000, 0.01); one more shape, `mixed`:
512 tables of 100 / 1 000 / 5 000 / 20 000 keys in filters sized new(keys,
0.01): both classes and split tables.

Clock: HIP events on the calls' stream around one call (its work-list copy and
its launches; nothing on the host is waited for inside).  An untimed first
batch of each route, then --reps rounds alternating the two; median [min-max].
Block bytes per second are set against the 6.29 TB/s copy rate of DESIGN.md
section 9.  Before anything is timed the two routes' words are equal and every
block's reported entry count is the generator's.  --host-parse N also times a
literal per-entry Python parse of N tables' blocks (the host route this
replaces, at its slowest: say so when quoting it).  Then the bounds A/B: the
block bytes one work item walks per class (LSMB_SST_WAVE_BYTES /
LSMB_SST_GROUP_BYTES), in rotating order.  Prints one JSON line per shape and
markdown tables.
Usage: python tools/mb_build_batch_sst.py [--tables 64,512,4096] [--reps 10] [--host-parse 8]
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
import lsmbloom  # noqa: E402
from lsmbloom import u32p, u64p  # noqa: E402

vp = ctypes.c_void_p
KLEN, VLEN, BLOCK = 12, 100, 4096
ENTRY = 4 + KLEN + VLEN
PER_BLOCK = (BLOCK - 2) // (ENTRY + 2)  # entries until estimated_size() + entry_size > block_size: 34
assert (PER_BLOCK - 1) * (ENTRY + 2) + 2 + ENTRY <= BLOCK < PER_BLOCK * (ENTRY + 2) + 2 + ENTRY
COPY_TBS = 6.29
# (wave item bytes, group item bytes) of the bounds A/B; the first pair is the library's default
AB_BOUNDS = [(256 << 10, 1 << 20), (64 << 10, 1 << 20), (1 << 20, 1 << 20), (256 << 10, 4 << 20), (256 << 10, 16 << 20)]


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(min(ms)), 4),
            "max_ms": round(float(max(ms)), 4)}


def fmt(s):
    return "%.3f ms [%.3f-%.3f]" % (s["median_ms"], s["min_ms"], s["max_ms"])


def p(a, t):
    return a.ctypes.data_as(t)


def blocks_of(keys, value):
    """keys uint8 [m, KLEN] with m <= PER_BLOCK per block, all blocks of one
    shape [nblk, m, KLEN] -> uint8 [nblk, block bytes]: the entries, their
    offsets, the count."""
    nblk, m, _ = keys.shape
    out = np.empty((nblk, m * ENTRY + 2 * m + 2), np.uint8)
    ent = out[:, :m * ENTRY].reshape(nblk, m, ENTRY)
    ent[:, :, 0:4] = np.frombuffer(struct.pack("<HH", KLEN, VLEN), np.uint8)
    ent[:, :, 4:4 + KLEN] = keys
    ent[:, :, 4 + KLEN:] = value
    tail = np.arange(m, dtype="<u2") * ENTRY
    out[:, m * ENTRY:m * ENTRY + 2 * m] = tail.view(np.uint8)
    out[:, -2:] = np.frombuffer(struct.pack("<H", m), np.uint8)
    return out


def make_tables(counts, seed):
    """-> (block bytes uint8, blk_off, blk_len, bseg, packed keys uint8 [n, KLEN])."""
    rng = np.random.default_rng(seed)
    n = int(sum(counts))
    keys = rng.integers(0, 256, (n, KLEN), dtype=np.uint8)
    value = np.arange(VLEN, dtype=np.uint8)
    parts, lens, bseg = [], [], [0]
    at = 0
    for c in counts:
        full, rem = divmod(int(c), PER_BLOCK)
        k = keys[at:at + c]
        if full:
            b = blocks_of(k[:full * PER_BLOCK].reshape(full, PER_BLOCK, KLEN), value)
            parts.append(b.reshape(-1))
            lens += [b.shape[1]] * full
        if rem:
            b = blocks_of(k[full * PER_BLOCK:].reshape(1, rem, KLEN), value)
            parts.append(b.reshape(-1))
            lens.append(b.shape[1])
        bseg.append(len(lens))
        at += c
    blk_len = np.array(lens, np.uint32)
    blk_off = np.zeros(len(lens), np.uint64)
    np.cumsum(blk_len[:-1], out=blk_off[1:])
    return np.concatenate(parts), blk_off, blk_len, np.array(bseg, np.uint64), keys


def python_parse(buf, blk_off, blk_len):
    """The literal per-entry host parse: every key of every block as bytes."""
    raw = buf.tobytes()  # (the caller passes just the parsed tables' bytes)
    keys = []
    for off, ln in zip(blk_off.tolist(), blk_len.tolist()):
        blk = raw[off:off + ln]
        (cnt,) = struct.unpack_from("<H", blk, ln - 2)
        data_end = ln - 2 - 2 * cnt
        for i in range(cnt):
            (o,) = struct.unpack_from("<H", blk, data_end + 2 * i)
            klen, _ = struct.unpack_from("<HH", blk, o)
            keys.append(blk[o + 4:o + 4 + klen])
    return keys


def run_shape(ctx, dev, name, counts, reps, host_parse):
    L = lsmbloom.lib()
    T = len(counts)
    shapes = [lsmbloom.params(max(c, 1), 0.01) for c in counts]
    nb = np.array([s[0] for s in shapes], np.uint32)
    kk = np.array([s[1] for s in shapes], np.uint32)
    buf, blk_off, blk_len, bseg, keys = make_tables(counts, 0x5EED0C00 + T)
    n, nblk = keys.shape[0], blk_off.size
    seg = np.zeros(T + 1, np.uint64)
    np.cumsum(counts, out=seg[1:])
    total = int(lsmbloom.build_batch_layout(nb)[-1])
    st = torch.cuda.Stream(dev)
    sp = vp(st.cuda_stream)
    d_bytes = torch.from_numpy(buf).to(dev)
    d_keys = torch.from_numpy(np.concatenate([keys.reshape(-1), np.zeros(16, np.uint8)])).to(dev)
    words = {r: torch.full((total,), -1, dtype=torch.int64, device=dev) for r in ("sst", "keys")}
    d_ent = torch.zeros(nblk, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def sst():
        rc = L.lsmb_build_batch_sst_dev(ctx.h, vp(d_bytes.data_ptr()), buf.size, nblk, p(blk_off, u64p), p(blk_len, u32p), T,
                                        p(bseg, u64p), p(nb, u32p), p(kk, u32p), vp(words["sst"].data_ptr()), total,
                                        vp(d_ent.data_ptr()), sp)
        assert rc == 0, L.lsmb_last_error()

    def packed():
        rc = L.lsmb_build_batch_dev(ctx.h, vp(d_keys.data_ptr()), None, KLEN, n, T, p(seg, u64p), p(nb, u32p), p(kk, u32p),
                                    vp(words["keys"].data_ptr()), total, sp)
        assert rc == 0, L.lsmb_last_error()

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b)

    # the untimed first batch of each route, and equality before anything is timed
    sst()
    packed()
    st.synchronize()
    equal = bool(torch.equal(words["sst"], words["keys"]))
    ent = d_ent.cpu().numpy()
    per = np.concatenate([[PER_BLOCK] * (c // PER_BLOCK) + ([c % PER_BLOCK] if c % PER_BLOCK else []) for c in counts])
    counted = bool(np.array_equal(ent, per))
    assert equal and counted, (equal, counted)
    tm = {"sst": [], "keys": []}
    for it in range(reps):
        for r, fn in (("sst", sst), ("keys", packed)) if it % 2 == 0 else (("keys", packed), ("sst", sst)):
            tm[r].append(events(fn))
    # the bounds A/B: the block bytes one item walks (wave class, group class), the default first
    def bounded(wave, group):
        def fn():
            os.environ["LSMB_SST_WAVE_BYTES"], os.environ["LSMB_SST_GROUP_BYTES"] = str(wave), str(group)
            try:
                sst()
            finally:
                del os.environ["LSMB_SST_WAVE_BYTES"], os.environ["LSMB_SST_GROUP_BYTES"]
        return fn

    ab = [("%dK/%dK" % (w >> 10, g >> 10), bounded(w, g)) for w, g in AB_BOUNDS]
    ab_tm = {a[0]: [] for a in ab}
    for aname, fn in ab:  # untimed, and the words do not depend on the bounds
        fn()
        st.synchronize()
        assert bool(torch.equal(words["sst"], words["keys"])), aname
    for it in range(reps):
        for j in range(len(ab)):
            aname, fn = ab[(it + j) % len(ab)]
            ab_tm[aname].append(events(fn))
    res = {"shape": name, "tables": T, "keys": n, "bounds_ab": {a: stats(v) for a, v in ab_tm.items()},
           "blocks": int(nblk), "block_bytes": int(buf.size),
           "key_bytes": int(n * KLEN), "reps": reps, "times": {r: stats(v) for r, v in tm.items()},
           "words_equal": equal, "entries_exact": counted, "clock": "HIP events around one call"}
    res["block_tb_per_s"] = round(buf.size / (res["times"]["sst"]["median_ms"] * 1e-3) / 1e12, 3)
    if host_parse:
        m = min(host_parse, T)
        hi = int(bseg[m])
        t0 = time.perf_counter()
        got = python_parse(buf[:int(blk_off[hi - 1]) + int(blk_len[hi - 1])], blk_off[:hi], blk_len[:hi])
        res["python_parse_ms_per_table"] = round((time.perf_counter() - t0) * 1e3 / m, 3)
        res["python_parse_tables"] = m
        assert len(got) == int(seg[m])
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", default="64,512,4096")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-parse", type=int, default=0)
    ap.add_argument("--no-mixed", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = lsmbloom.Context(0)
    ctx.set_timing(False)
    todo = [("T=%s" % x, [1000] * int(x)) for x in args.tables.split(",") if x]
    if not args.no_mixed:
        todo.append(("mixed", [(100, 1000, 5000, 20000)[t % 4] for t in range(512)]))
    res = [run_shape(ctx, dev, name, counts, args.reps, args.host_parse) for name, counts in todo]
    ctx.close()
    print("\n| shape | keys | block bytes | `build_batch_sst_dev` | block bytes / s | of %.2f TB/s | `build_batch_dev`, "
          "packed keys | blocks / packed |\n|---|---|---|---|---|---|---|---|" % COPY_TBS)
    for r in res:
        t = r["times"]
        print("| %s | %d | %.1f MB | %s | %.2f TB/s | %.0f %% | %s | %.2f× |" % (
            r["shape"], r["keys"], r["block_bytes"] / 1e6, fmt(t["sst"]), r["block_tb_per_s"],
            100 * r["block_tb_per_s"] / COPY_TBS, fmt(t["keys"]), t["sst"]["median_ms"] / t["keys"]["median_ms"]))
    names = list(res[0]["bounds_ab"]) if res else []
    print("\n| shape | " + " | ".join("item bytes %s" % a for a in names) + " |\n|---|" + "---|" * len(names))
    for r in res:
        print("| %s | %s |" % (r["shape"], " | ".join(fmt(r["bounds_ab"][a]) for a in names)))
    for r in res:
        if "python_parse_ms_per_table" in r:
            print("%s: literal Python parse of the blocks, %.3f ms per table over %d tables (host, one thread)"
                  % (r["shape"], r["python_parse_ms_per_table"], r["python_parse_tables"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
