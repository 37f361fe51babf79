"""Microbenchmark: round 1 of the walk probe's per-table lists
(lsmb_lset_probe_walk_lists_dev, from NULL: each key's first candidate in
DB::get's order, at most one list entry per key) against the Version lists
probe (lsmb_lset_probe_version_lists_dev: every candidate of every key) on the
same keys of the same sealed set in the same process.  The Version lists probe
is the baseline: it is what a table-by-table multi-get had before the walk
probe, and the walk does a subset of its work (no row search below a key's
first hit, one answer row to transpose instead of a mask row and a row per
level).

Shapes and protocol are those of tools/mb_lset_version_lists.py: n
device-resident 16-byte keys (default 10 M), half of them members of the row's
tables; 8 L0 tables spanning the key space, "sst" = 8 filters new(1000, 0.01),
"mixed" = new(1000), new(5000), new(20000) at 0.01; one row of T tables; each
shape with the keys as fixed 16-byte keys and again through the
variable-length source.  HIP events (torch.cuda.Event) around each call on one
stream, --warmup calls of both first, then --reps repetitions alternating walk
/ Version lists; median, minimum and maximum of each.  Before anything is timed
the walk's steps and lists are held against the first candidate per key
reduced (on the device, with torch) from the Version lists.  Prints one JSON
line per shape, with the list entries of each call.
Usage: python tools/mb_lset_walk.py [--n 10000000] [--tables 512,4096] [--reps 10]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "storage-engine_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsmbloom  # noqa: E402
from lsmbloom import LevelSet  # noqa: E402
from mb_lset_version import L0_SIZES, PER, device_filter, stats, timed, with_table_word  # noqa: E402


def entry_ordinals(starts, V):
    """starts int64[V + 1] (device) -> the ordinal of every list entry, int64[total]."""
    return torch.repeat_interleave(torch.arange(V, device=starts.device), starts[1:] - starts[:-1])


def step_of(v, T0):
    """Version ordinal -> walk step, one row: L0 newest first, then the row."""
    return torch.where(v < T0, T0 - 1 - v, torch.full_like(v, T0))


def first_candidates_agree(n, T0, V, s_all, i_all, s_walk, i_walk, step):
    """The walk's steps and lists against the Version lists reduced to each key's smallest step."""
    big = 1 << 40
    best = torch.full((n,), big, dtype=torch.int64, device=s_all.device)
    best.scatter_reduce_(0, i_all.to(torch.int64), step_of(entry_ordinals(s_all, V), T0), reduce="amin")
    exp_step = torch.where(best == big, torch.full_like(best, -1), best)  # LSMB_LSET_NONE read as int32 is -1
    walk_idx = i_walk.to(torch.int64)
    return (bool(torch.equal(step.to(torch.int64), exp_step)) and int(s_walk[V].item()) == int((best != big).sum().item())
            and bool(torch.equal(step_of(entry_ordinals(s_walk, V), T0), exp_step[walk_idx])))


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
        ls = LevelSet(ctx)
        for t, f in enumerate(row):
            ls.add_filter(0, t, f, int(t).to_bytes(4, "big") + b"\x00" * 12, int(t).to_bytes(4, "big") + b"\xff" * 12)
        for j, count in enumerate(sizes):  # members: a random sample of the row's keys
            pick = mem[torch.randint(0, T * PER, (count,), device=dev, generator=g)].contiguous()
            ls.add_filter(lsmbloom.LSMB_LSET_ROW_L0, 10_000_000 + j, device_filter(ctx, pick, count), b"", b"\xff" * 16)
        ls.seal()
        T0, V = ls.l0_tables(), ls.version_tables()
        assert T0 == len(sizes) and V == T0 + T and ls.walk_steps() == T0 + 1
        work_walk = torch.empty(ls.walk_lists_work_bytes(n), dtype=torch.uint8, device=dev)
        work_all = torch.empty(ls.version_lists_work_bytes(n), dtype=torch.uint8, device=dev)
        s_walk = torch.empty(V + 1, dtype=torch.int64, device=dev)
        s_all = torch.empty(V + 1, dtype=torch.int64, device=dev)
        step = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        for src in ("fixed16", "varlen"):
            kw = {"key_len": 16} if src == "fixed16" else {"offsets": offs}
            kw["stream"] = st.cuda_stream
            # capacities from counting calls (the lists do not depend on the key source)
            ls.probe_walk_lists_dev(q, n, s_walk, None, work_walk, **kw)
            ls.probe_version_lists_dev(q, n, s_all, None, work_all, **kw)
            st.synchronize()
            e_walk, e_all = int(s_walk[V].item()), int(s_all[V].item())
            i_walk = torch.full((e_walk,), -1, dtype=torch.int32, device=dev)
            i_all = torch.full((e_all,), -1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()

            def walk():
                ls.probe_walk_lists_dev(q, n, s_walk, i_walk, work_walk, step=step, **kw)

            def version_lists():
                ls.probe_version_lists_dev(q, n, s_all, i_all, work_all, **kw)

            walk()
            version_lists()
            torch.cuda.synchronize()
            agree = first_candidates_agree(n, T0, V, s_all, i_all, s_walk, i_walk, step)
            for _ in range(warmup):
                walk()
                version_lists()
            torch.cuda.synchronize()
            a, b = [], []
            for _ in range(reps):  # alternating
                a.append(timed(walk, st))
                b.append(timed(version_lists, st))
            sa, sb = stats(a), stats(b)
            res = {"l0": l0_name, "l0_tables": T0, "row_tables": T, "n": n, "keys": src, "reps": reps,
                   "walk": dict(sa, gkeys_s=round(n / sa["median_ms"] / 1e6, 3)),
                   "version_lists": dict(sb, gkeys_s=round(n / sb["median_ms"] / 1e6, 3)),
                   "ratio": round(sb["median_ms"] / sa["median_ms"], 3),
                   "walk_median_le_version_lists_median": sa["median_ms"] <= sb["median_ms"],
                   "answers_agree": agree, "entries": {"walk": e_walk, "version_lists": e_all},
                   "work_bytes": {"walk": int(work_walk.numel()), "version_lists": int(work_all.numel())},
                   "clock": "HIP events (torch.cuda.Event)"}
            print(json.dumps(res), flush=True)
            ok = ok and agree
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
