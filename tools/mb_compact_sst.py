"""Microbenchmark: the surviving keys of a compaction's merged data blocks
resolved on the device (lsmb_compact_sst_mark_dev / lsmb_compact_sst_gather_dev)
and the output table's filter built from them (lsmb_build_var_dev_new), against
the union build of the same bytes (lsmb_build_batch_sst_dev: one table of every
input block), which is the only device route without them.

Input: a synthetic compaction of 4 L0-like sources (--l0 keys each, a random
subset of the key space, 10 % tombstones) plus one large older source (--older
keys: the whole space, so that every L0 entry shadows one of its entries), keys
of 16 .. 32 bytes, 100-byte values, 4 KiB blocks cut by BlockBuilder::add's rule
(src/sstable/block/builder.rs:41-47).

Clock: HIP events on the calls' stream around one call (its descriptor copy and
its launches; nothing on the host is waited for inside).  The mark's passes are
timed by difference with the library's measurement switch LSMB_CS_STAGES (1: the
index pass alone, 2: index and mark, unset: with the scan and the totals).  An
untimed first round of every route, then --reps rounds in rotating order; median
[min-max].  Before anything is timed the totals equal a numpy model of the merge
and the gathered run's filter equals the filter of the model's keys.  The union
build's filter is sized for every input entry, capped at
lsmb_build_batch_max_bits().  Prints one JSON line and a markdown table.
Usage: python tools/mb_compact_sst.py [--older 400000] [--l0 16000] [--reps 10]
"""
import argparse
import ctypes
import json
import os
import struct
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "storage-engine_amd"))
import lsmbloom  # noqa: E402
from lsmbloom import u32p, u64p  # noqa: E402

vp = ctypes.c_void_p
VLEN, BLOCK = 100, 4096
COPY_TBS = 6.29


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(min(ms)), 4),
            "max_ms": round(float(max(ms)), 4)}


def fmt(s):
    return "%.3f ms [%.3f-%.3f]" % (s["median_ms"], s["min_ms"], s["max_ms"])


def p(a, t):
    return a.ctypes.data_as(t)


def key_of(i):
    """Key i of the space: 16 .. 32 bytes, ascending in i."""
    return b"%016d" % i + b"k" * (i * 7 % 17)


def source_blocks(ids, tomb):
    """The entries (key_of(i), 100 bytes or nothing) of ascending ids cut into
    4 KiB blocks -> [block bytes]."""
    value = bytes(range(VLEN))
    blocks, cur, offs, data = [], [], [], 0
    for i, t in zip(ids.tolist(), tomb.tolist()):
        k = key_of(i)
        v = b"" if t else value
        size = 4 + len(k) + len(v)
        if cur and data + 2 * len(offs) + 2 + size > BLOCK:
            blocks.append(b"".join(cur) + struct.pack("<%dH" % (len(offs) + 1), *offs, len(offs)))
            cur, offs, data = [], [], 0
        offs.append(data)
        cur.append(struct.pack("<HH", len(k), len(v)) + k + v)
        data += size
    if cur:
        blocks.append(b"".join(cur) + struct.pack("<%dH" % (len(offs) + 1), *offs, len(offs)))
    return blocks


def make_input(n_older, n_l0, seed):
    """-> (bytes uint8, blk_off, blk_len, sseg, per source (ids, tombstone flags))."""
    rng = np.random.default_rng(seed)
    srcs = []
    for _ in range(4):
        ids = np.sort(rng.choice(n_older, size=min(n_l0, n_older), replace=False))
        srcs.append((ids, rng.random(ids.size) < 0.10))
    srcs.append((np.arange(n_older), np.zeros(n_older, bool)))
    blocks, sseg = [], [0]
    for ids, tomb in srcs:
        blocks += source_blocks(ids, tomb)
        sseg.append(len(blocks))
    blk_len = np.array([len(b) for b in blocks], np.uint32)
    blk_off = np.zeros(len(blocks), np.uint64)
    np.cumsum(blk_len[:-1], out=blk_off[1:])
    return np.frombuffer(b"".join(blocks), np.uint8), blk_off, blk_len, np.array(sseg, np.uint64), srcs


def model(srcs, n_space, drop):
    """The merge by ids: -> (survivor ids in (source, entry) order, entries seen)."""
    newest = np.full(n_space, -1, np.int64)
    for s in range(len(srcs) - 1, -1, -1):
        newest[srcs[s][0]] = s
    out = []
    for s, (ids, tomb) in enumerate(srcs):
        keep = newest[ids] == s
        if drop:
            keep &= ~tomb
        out.append(ids[keep])
    return np.concatenate(out), int(sum(ids.size for ids, _ in srcs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--older", type=int, default=400000)
    ap.add_argument("--l0", type=int, default=16000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--drop", type=int, default=1)
    args = ap.parse_args()
    L = lsmbloom.lib()
    dev = torch.device("cuda:0")
    ctx = lsmbloom.Context(0)
    ctx.set_timing(False)
    buf, blk_off, blk_len, sseg, srcs = make_input(args.older, args.l0, 0x5EEDC0DE)
    nblk, nsrc = blk_off.size, sseg.size - 1
    surv_ids, entries = model(srcs, args.older, args.drop)
    surv, kbytes = surv_ids.size, int(sum(len(key_of(i)) for i in surv_ids.tolist()))
    nb, k = lsmbloom.params(max(surv, 1), 0.01)
    nb_u, k_u = lsmbloom.params(entries, 0.01)
    nb_u = min(nb_u, lsmbloom.build_batch_max_bits())
    st = torch.cuda.Stream(dev)
    sp = vp(st.cuda_stream)
    d_bytes = torch.from_numpy(buf.copy()).to(dev)
    wb = lsmbloom.compact_sst_work_bytes(blk_len)
    work = torch.zeros(wb, dtype=torch.uint8, device=dev)
    totals = torch.zeros(4, dtype=torch.int64, device=dev)
    key_data = torch.zeros(kbytes + 16, dtype=torch.uint8, device=dev)
    key_offs = torch.zeros(surv + 1, dtype=torch.int64, device=dev)
    words = torch.zeros(lsmbloom.num_words(nb), dtype=torch.int64, device=dev)
    union_tot = int(lsmbloom.build_batch_layout([nb_u])[-1])
    union_words = torch.zeros(union_tot, dtype=torch.int64, device=dev)
    bseg = np.array([0, nblk], np.uint64)
    nbu, kku = np.array([nb_u], np.uint32), np.array([k_u], np.uint32)
    torch.cuda.synchronize()

    def mark(stages=None):
        def fn():
            if stages:
                os.environ["LSMB_CS_STAGES"] = str(stages)
            try:
                rc = L.lsmb_compact_sst_mark_dev(ctx.h, vp(d_bytes.data_ptr()), buf.size, nblk, p(blk_off, u64p),
                                                 p(blk_len, u32p), nsrc, p(sseg, u64p), args.drop, vp(work.data_ptr()), wb,
                                                 None, vp(totals.data_ptr()), sp)
            finally:
                os.environ.pop("LSMB_CS_STAGES", None)
            assert rc == 0, L.lsmb_last_error()
        return fn

    def gather():
        rc = L.lsmb_compact_sst_gather_dev(ctx.h, vp(d_bytes.data_ptr()), buf.size, nblk, p(blk_off, u64p), p(blk_len, u32p),
                                           nsrc, p(sseg, u64p), vp(work.data_ptr()), vp(key_data.data_ptr()), kbytes,
                                           vp(key_offs.data_ptr()), surv + 1, sp)
        assert rc == 0, L.lsmb_last_error()

    def build():
        rc = L.lsmb_build_var_dev_new(ctx.h, vp(key_data.data_ptr()), vp(key_offs.data_ptr()), surv, nb, k,
                                      vp(words.data_ptr()), sp)
        assert rc == 0, L.lsmb_last_error()

    def union():
        rc = L.lsmb_build_batch_sst_dev(ctx.h, vp(d_bytes.data_ptr()), buf.size, nblk, p(blk_off, u64p), p(blk_len, u32p), 1,
                                        p(bseg, u64p), p(nbu, u32p), p(kku, u32p), vp(union_words.data_ptr()), union_tot,
                                        None, sp)
        assert rc == 0, L.lsmb_last_error()

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b)

    routes = [("index", mark(1)), ("index+mark", mark(2)), ("mark call", mark()), ("gather", gather), ("build", build),
              ("union build", union)]
    # the untimed first round, and the results before anything is timed
    for name, fn in routes[2:]:
        fn()
    st.synchronize()
    tot = [int(x) for x in totals.cpu().numpy().view(np.uint64)]
    assert tot == [surv, kbytes, entries, 0], (tot, surv, kbytes, entries)
    keys = [key_of(i) for i in surv_ids.tolist()]
    exp_offs = np.zeros(surv + 1, np.int64)
    np.cumsum([len(x) for x in keys], out=exp_offs[1:])
    assert np.array_equal(key_offs.cpu().numpy(), exp_offs), "offsets"
    assert key_data[:kbytes].cpu().numpy().tobytes() == b"".join(keys), "key bytes"
    ref = torch.zeros_like(words)
    d_ref_keys = torch.from_numpy(np.frombuffer(b"".join(keys) + bytes(16), np.uint8).copy()).to(dev)
    d_ref_offs = torch.from_numpy(exp_offs).to(dev)
    ctx.build_var_dev_new(d_ref_keys, d_ref_offs, surv, nb, k, ref, stream=st.cuda_stream)
    st.synchronize()
    assert bool(torch.equal(ref, words)), "the filter of the gathered run"
    routes[0][1](), routes[1][1]()
    st.synchronize()
    tm = {name: [] for name, _ in routes}
    for it in range(args.reps):
        for j in range(len(routes)):
            name, fn = routes[(it + j) % len(routes)]
            if name in ("gather", "build"):
                continue
            tm[name].append(events(fn))
    # gather and build need a whole mark in front of them (the staged passes leave no scans)
    mark()()
    for it in range(args.reps):
        for name, fn in (routes[3], routes[4]) if it % 2 == 0 else (routes[4], routes[3]):
            tm[name].append(events(fn))
    t = {name: stats(v) for name, v in tm.items()}
    med = {name: s["median_ms"] for name, s in t.items()}
    route_ms = med["mark call"] + med["gather"] + med["build"]
    res = {"older": args.older, "l0": args.l0, "drop_tombstones": args.drop, "blocks": int(nblk), "block_bytes": int(buf.size),
           "entries": entries, "survivors": surv, "survivor_key_bytes": kbytes, "filter_bits": nb, "union_filter_bits": nb_u,
           "reps": args.reps, "times": t, "clock": "HIP events around one call",
           "by_difference_ms": {"index": med["index"], "mark": round(med["index+mark"] - med["index"], 4),
                                "scan+totals": round(med["mark call"] - med["index+mark"], 4)},
           "route_ms": round(route_ms, 4),
           "block_gb_per_s": {"mark call": round(buf.size / (med["mark call"] * 1e-3) / 1e9, 1),
                              "mark+gather+build": round(buf.size / (route_ms * 1e-3) / 1e9, 1),
                              "union build": round(buf.size / (med["union build"] * 1e-3) / 1e9, 1)}}
    print(json.dumps(res), flush=True)
    ctx.close()
    print("\n| step | time | block bytes / s |\n|---|---|---|")
    for name in ("index", "index+mark", "mark call", "gather", "build", "union build"):
        print("| %s | %s | %.1f GB/s |" % (name, fmt(t[name]), buf.size / (med[name] * 1e-3) / 1e9))
    print("| mark call + gather + build | %.3f ms | %.1f GB/s |" % (route_ms, res["block_gb_per_s"]["mark+gather+build"]))
    print("\n%d blocks, %.1f MB, %d entries, %d survivors; copy rate of DESIGN.md section 9: %.2f TB/s"
          % (nblk, buf.size / 1e6, entries, surv, COPY_TBS))
    return 0


if __name__ == "__main__":
    sys.exit(main())
