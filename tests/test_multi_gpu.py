"""Multi-GPU paths on the GPU box.

The box has one MI355X, so every multi-shard test here runs its shards on
device 0: the same kernels, the same merge, with the "peer" reads served
locally.  The 8-GPU runs are the driver's (bench.py --gpus 8).

* lsmb_multi (one process, several GPUs): sharded device build + OR
  reduce-scatter by peer loads + all-gather; sharded host-keys build straight
  into the serialized block.  Every word vs the single-process oracle build.
* torch.distributed ranks (one process per GPU): two ranks on cuda:0 build
  partials with the HIP kernels and merge over gloo through
  lsmbloom.dist.or_allreduce_(..., ctx=...), i.e. the device OR kernel
  (lsmb_or_reduce_dev) — the path the RCCL bench takes, with gloo moving the
  bytes because RCCL refuses two ranks on one device.
* bench.py --gpus 2 launching its own ranks (the driver's form).
* One context used from two streams (the partition workspace guard), and a
  filter-set add on one context while another context's builds are queued.
"""
import json
import os
import socket
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

import keygen
import lsmbloom

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ctx():
    c = lsmbloom.Context(0)
    yield c
    c.close()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("G,n,filter_n", [(2, 2_000_000, 50_000_000),   # partition
                                          (2, 2_000_000, 10**9),        # 2 sweeps: merge overlapped per range
                                          (3, 600_001, 10**9),          # 2 sweeps, ragged shards
                                          (3, 1_000_001, 1_000_000),    # tiled, ragged shards
                                          (4, 40_000, 40_000),          # lds, odd word count
                                          (2, 3, 10_000_000)])          # atomic, shards of 1-2 keys
def test_multi_build_fixed_dev_equals_oracle(torch, oracle, G, n, filter_n):
    nb, k = lsmbloom.params(filter_n, 0.01)
    nw = lsmbloom.num_words(nb)
    dev = torch.device("cuda:0")
    m = lsmbloom.Multi([0] * G)
    try:
        assert m.size() == G
        keys, words = [], []
        host = keygen.key16(0x5EED0001, 0, n)
        for g in range(G):
            lo, hi = n * g // G, n * (g + 1) // G
            keys.append(torch.from_numpy(np.ascontiguousarray(host[lo:hi])).to(dev))
            words.append(torch.zeros(nw, dtype=torch.int64, device=dev))
        m.build_fixed_dev(keys, 16, nb, k, words)
        ref = oracle.build_fixed_mt(host, 16, nb, k, 8)
        for g in range(G):
            assert np.array_equal(_u64(words[g]), ref), "shard %d's merged filter differs" % g
        tot, bld, mrg = m.last_ms()
        assert tot >= bld >= 0 and mrg >= 0
    finally:
        m.close()


def test_multi_build_fixed_dev_or_accumulates(torch, oracle):
    # pre-existing bits in any shard's words survive the merge (OR-accumulate)
    nb, k = lsmbloom.params(3_000_000, 0.01)
    nw = lsmbloom.num_words(nb)
    dev = torch.device("cuda:0")
    pre = oracle.build_fixed(keygen.key16(7, 0, 1000), 16, nb, k)
    host = keygen.key16(0x5EED0001, 0, 300_000)
    m = lsmbloom.Multi([0, 0])
    try:
        keys = [torch.from_numpy(np.ascontiguousarray(host[:100_000])).to(dev),
                torch.from_numpy(np.ascontiguousarray(host[100_000:])).to(dev)]
        words = [torch.from_numpy(pre.view(np.int64).copy()).to(dev), torch.zeros(nw, dtype=torch.int64, device=dev)]
        m.build_fixed_dev(keys, 16, nb, k, words)
        ref = oracle.build_fixed(host, 16, nb, k, words=pre.copy())
        assert np.array_equal(_u64(words[0]), ref) and np.array_equal(_u64(words[1]), ref)
    finally:
        m.close()


@pytest.mark.parametrize("filter_n,n", [(1_000_000_000, 2_000_000),   # C5's filter: 2 sweeps
                                         (200_000_000, 2_000_000),     # 1.9e9 bits: one sweep of 2^21-bit bins
                                         (1_000_000, 1_000_000)])        # one sweep (tiled)
def test_sweep_builds_cover_the_filter(torch, ctx, oracle, filter_n, n):
    """lsmb_build_fixed_dev_sweep: sweep s sets only the bits of its word range
    (lsmb_sweep_words) and every sweep together == the whole build — the
    property the N > 1 bench leans on to OR-allreduce range s while s+1 builds."""
    nb, k = lsmbloom.params(filter_n, 0.01)
    nw = lsmbloom.num_words(nb)
    dev = torch.device("cuda:0")
    host = keygen.key16(0x5EED0001, 0, n)
    keys = torch.from_numpy(np.ascontiguousarray(host)).to(dev)
    ref = oracle.build_fixed_mt(host, 16, nb, k, 8)
    nsw = lsmbloom.build_sweeps(nb, n, k)
    assert nsw == (2 if filter_n == 1_000_000_000 else 1)
    acc = torch.zeros(nw, dtype=torch.int64, device=dev)
    one = torch.zeros(nw, dtype=torch.int64, device=dev)
    for s in range(nsw):
        lo, hi = lsmbloom.sweep_words(nb, n, s, k)
        one.zero_()
        ctx.build_fixed_dev_sweep(keys, 16, n, nb, k, one, s)
        ctx.build_fixed_dev_sweep(keys, 16, n, nb, k, acc, s)
        got = _u64(one)
        assert np.array_equal(got[lo:hi], ref[lo:hi]), "sweep %d's range differs" % s
        assert not got[:lo].any() and not got[hi:].any(), "sweep %d wrote outside its range" % s
    assert np.array_equal(_u64(acc), ref)
    with pytest.raises(ValueError):
        ctx.build_fixed_dev_sweep(keys, 16, n, nb, k, acc, nsw)


def test_multi_distinct_devices(torch, oracle):
    """lsmb_multi across DISTINCT GPUs: xGMI peer loads in the OR
    gather, hipMemcpyPeerAsync in the all-gather, cross-device event waits.
    Every other multi test repeats device 0; this one runs wherever the box
    has two or more GPUs and is skipped on the one-GPU lease."""
    ndev = torch.cuda.device_count()
    if ndev < 2:
        pytest.skip("one visible GPU: cross-device parity is checked on multi-GPU leases only")
    G = min(ndev, 4)
    n = 3_000_000
    for filter_n in (50_000_000, 10**9):  # one sweep; two sweeps with per-range merges
        nb, k = lsmbloom.params(filter_n, 0.01)
        nw = lsmbloom.num_words(nb)
        host = keygen.key16(0x5EED0001, 0, n)
        m = lsmbloom.Multi(list(range(G)))
        try:
            keys, words = [], []
            for g in range(G):
                lo, hi = n * g // G, n * (g + 1) // G
                keys.append(torch.from_numpy(np.ascontiguousarray(host[lo:hi])).to("cuda:%d" % g))
                words.append(torch.zeros(nw, dtype=torch.int64, device="cuda:%d" % g))
            m.build_fixed_dev(keys, 16, nb, k, words)
            ref = oracle.build_fixed_mt(host, 16, nb, k, 16)
            for g in range(G):
                assert np.array_equal(_u64(words[g]), ref), "device %d's merged filter differs" % g
            blk = m.build_block(host, nb, k, key_len=16)
            assert bytes(blk) == bytes(oracle.serialize(ref, nb, k))
        finally:
            m.close()


@pytest.mark.parametrize("G", [1, 2, 3])
def test_multi_build_block_fixed_and_varlen(oracle, G):
    m = lsmbloom.Multi([0] * G)
    try:
        n = 3_000_000
        nb, k = lsmbloom.params(n, 0.01)
        keys = keygen.key16(0x5EED0001, 0, n)
        blk = m.build_block(keys, nb, k, key_len=16)
        ref = oracle.serialize(oracle.build_fixed_mt(keys, 16, nb, k, 8), nb, k)
        assert bytes(blk) == bytes(ref)
        data, offs = keygen.varlen(400_000)
        nb2, k2 = lsmbloom.params(400_000, 0.01)
        blk2 = m.build_block(data, nb2, k2, offsets=offs)
        assert bytes(blk2) == bytes(oracle.serialize(oracle.build_var(data, offs, nb2, k2), nb2, k2))
        # degenerate runs: no keys, and every key empty (one insert of b"")
        assert bytes(m.build_block(np.zeros(0, np.uint8), nb, k, key_len=16)) == \
            bytes(oracle.serialize(np.zeros(lsmbloom.num_words(nb), np.uint64), nb, k))
        empty_ref = oracle.serialize(oracle.build_var(b"", np.zeros(2, np.uint64), nb2, k2), nb2, k2)
        assert bytes(m.build_block(np.zeros(0, np.uint8), nb2, k2, offsets=np.zeros(5, np.uint64))) == \
            bytes(empty_ref)
    finally:
        m.close()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _digest(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<u8").tobytes()).hexdigest()


def _dist_worker(rank, world, port, n, filter_n, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, os.path.join(ROOT, "storage-engine_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist

    import lsmbloom
    from lsmbloom import dist as ldist
    lsmbloom.set_host_max_keys(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dev = torch.device("cuda:0")
        ctx = lsmbloom.Context(0)
        nb, k = lsmbloom.params(filter_n, 0.01)
        lo, hi = n * rank // world, n * (rank + 1) // world
        keys = torch.empty((hi - lo, 16), dtype=torch.uint8, device=dev)
        ctx.gen_key16_dev(0x5EED0001, lo, hi - lo, keys)
        words = torch.zeros(lsmbloom.num_words(nb), dtype=torch.int64, device=dev)
        ctx.build_fixed_dev(keys, 16, hi - lo, nb, k, words)
        part = words.clone()
        mine, start = ldist.or_reduce_scatter_(part, ctx=ctx)
        ldist.or_allreduce_(words, ctx=ctx)
        torch.cuda.synchronize()
        # digests, not arrays: C5's filter is 512 MiB per rank
        q.put((rank, _digest(words.cpu().numpy().view(np.uint64)), _digest(mine.cpu().numpy().view(np.uint64)),
               start, mine.numel()))
        ctx.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world,n,filter_n", [(2, 3_000_000, 30_000_000), (3, 500_001, 500_001),
                                              (4, 4_000_000, 1_000_000_000)])  # C5's 2^32-1-bit filter
def test_dist_or_allreduce_device_path(oracle, world, n, filter_n):
    import torch.multiprocessing as mp
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    procs = [mpc.Process(target=_dist_worker, args=(r, world, port, n, filter_n, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    nb, k = lsmbloom.params(filter_n, 0.01)
    ref = oracle.build_fixed_mt(keygen.key16(0x5EED0001, 0, n), 16, nb, k, 16)
    for rank, words, mine, start, per in res:
        assert words == _digest(ref), "rank %d merged filter differs" % rank
        sl = np.zeros(per, np.uint64)
        end = min(start + per, ref.size)
        sl[: end - start] = ref[start:end]
        assert mine == _digest(sl), "rank %d reduce-scatter slice differs" % rank


def _ipc_worker(rank, world, port, n, filter_n, per_sweep, q, ordered="device", seeds=(0x5EED0001,)):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, os.path.join(ROOT, "storage-engine_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import time

    import torch
    import torch.distributed as dist

    import lsmbloom
    from lsmbloom import dist as ldist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dev = torch.device("cuda:0")
        ctx = lsmbloom.Context(0)
        nb, k = lsmbloom.params(filter_n, 0.01)
        lo, hi = n * rank // world, n * (rank + 1) // world
        keys = torch.empty((hi - lo, 16), dtype=torch.uint8, device=dev)
        words = torch.empty(lsmbloom.num_words(nb), dtype=torch.int64, device=dev)
        words.fill_(-1)  # garbage: the fresh build writes every word
        m = ldist.IpcMerge(words, ctx, ordered=ordered)
        nsw = lsmbloom.build_sweeps(nb, hi - lo, k)
        # host-side ordering inside a merge (device-ordered: none after the
        # first, range-checking call of each range)
        calls = {"sync": 0, "barrier": 0}
        real_sync, real_barrier = torch.cuda.Stream.synchronize, dist.barrier

        def count_sync(self):
            calls["sync"] += 1
            return real_sync(self)

        def count_barrier(*a, **kw):
            calls["barrier"] += 1
            return real_barrier(*a, **kw)
        digests = []
        for i, seed in enumerate(seeds):
            ctx.gen_key16_dev(seed, lo, hi - lo, keys)
            torch.cuda.synchronize()
            if rank == world - 1:
                time.sleep(0.3)  # the last rank builds late: the others' merge must wait for it on the GPU
            if i == 1:
                torch.cuda.Stream.synchronize, dist.barrier = count_sync, count_barrier
            if per_sweep:  # the bench's overlapped form: sweep s's range merged after sweep s
                for s in range(nsw):
                    ctx.build_fixed_dev_sweep_new(keys, 16, hi - lo, nb, k, words, s)
                    a, b = lsmbloom.sweep_words(nb, hi - lo, s, k)
                    m.allreduce(a, b)
            else:
                ctx.build_fixed_dev_new(keys, 16, hi - lo, nb, k, words)
                m.allreduce()
            torch.cuda.Stream.synchronize, dist.barrier = real_sync, real_barrier
            torch.cuda.synchronize()
            digests.append(_digest(words.cpu().numpy().view(np.uint64)))
        timeouts = m.timeouts()
        q.put((rank, nsw, digests, calls, timeouts))
        m.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world,n,filter_n,per_sweep,ordered,nseeds",
                         [(2, 3_000_000, 30_000_000, False, "device", 2),
                          (3, 500_001, 500_001, False, "device", 2),    # ragged slices
                          (4, 8_000_000, 1_000_000_000, True, "device", 1),  # C5's filter, 2 ranges
                          (2, 3_000_000, 30_000_000, False, "host", 2)])
def test_ipc_or_allreduce_cross_process(oracle, world, n, filter_n, per_sweep, ordered, nseeds):
    """the N > 1 merge without RCCL — `world` processes
    on cuda:0, each exporting its words (lsmb_ipc_export), mapping the others'
    (lsmb_ipc_import) and merging by peer loads (lsmb_or_gather_dev), the path
    `bench.py --backend ipc` times.  RCCL refuses two ranks on one GPU; IPC
    does not, so the cross-process product merge runs here.  Every rank's
    merged words == the single-process oracle build (digest).
    VERDICT r04 item 5: ordered="device" orders the merge's phases with flags
    on the GPUs (lsmb_flag_*): the last rank builds late and the others' merges
    must wait for it there; a second build + merge on the same words repeats
    it, and inside that merge the host neither synchronises a stream nor
    enters a barrier; no flag wait times out."""
    import torch.multiprocessing as mp
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    seeds = (0x5EED0001, 0x5EED0003)[:nseeds]
    procs = [mpc.Process(target=_ipc_worker, args=(r, world, port, n, filter_n, per_sweep, q, ordered, seeds))
             for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    nb, k = lsmbloom.params(filter_n, 0.01)
    refs = [_digest(oracle.build_fixed_mt(keygen.key16(sd, 0, n), 16, nb, k, 16)) for sd in seeds]
    for rank, nsw, digests, calls, timeouts in res:
        assert nsw == 2 or not per_sweep  # 2 M keys per rank: C5's filter builds in 2 sweeps
        assert digests == refs, "rank %d merged filter differs" % rank
        assert timeouts == 0
        if ordered == "device" and nseeds > 1:
            assert calls == {"sync": 0, "barrier": 0}, calls


@pytest.mark.timeout(300)
@pytest.mark.parametrize("backend", ["gloo", "ipc"])
def test_bench_pipelined_steps(backend):
    """The pipelined step form (--step-form pipelined): a step does not wait for
    its last range's merge, the next step's sweep 0 (range 0 only) runs under
    it and sweep s waits only for range s's previous merge.  After the timed
    steps the merged filter must still equal the single-GPU build, word for
    word, with either merge."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", backend,
           "--global-keys", "8000000", "--filter-keys", "1000000000", "--steps", "4", "--warmup", "2",
           "--step-form", "pipelined", "--full", "--no-cpu-baseline", "--no-e2e", "--no-varlen", "--no-exact10",
           "--no-probe"]
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][0])
    assert "the last one while the next step's first sweep builds" in out["step_split"]["timed_step"]
    assert out["step_split"]["overlap_calibration"]["timed_form"] == "pipelined"
    assert out["multi_gpu_merged_equals_single_gpu_build"] is True and out["value"] > 0


@pytest.mark.timeout(300)
@pytest.mark.parametrize("filter_keys,backend", [(None, "gloo"), (1_000_000_000, "gloo"), (1_000_000_000, "ipc"),
                                                 (1_000_000_000, "auto-gloo")])
def test_bench_launches_its_own_ranks(filter_keys, backend):
    """`python bench.py --gpus 2` (no torchrun) starts two ranks itself; here
    over gloo, both on cuda:0.  The line must say n_gpus 2, carry the split
    build / OR-allreduce timing, and the rank-0 word-for-word self-check."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", backend,
           "--global-keys", "8000000", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-e2e",
           "--no-varlen", "--no-exact10", "--probe-keys", "200000"]
    if filter_keys:  # C5's 2^32-1-bit filter: 2 sweeps, per-range allreduce overlapped
        cmd += ["--filter-keys", str(filter_keys), "--no-probe"]
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(line) == 1, r.stdout
    out = json.loads(line[0])
    assert out["n_gpus"] == 2 and out["config"]["global_keys"] == 8_000_000
    assert out["scaling"] == "strong" and out["config"]["keys_per_gpu"] == 4_000_000
    assert out["multi_gpu_merged_equals_single_gpu_build"] is True
    assert out["step_split"]["or_allreduce_ms"] > 0 and out["step_split"]["build_ms"] > 0
    if filter_keys:  # overlapped vs serial steps timed first; the faster form is the timed one
        cal = out["step_split"]["overlap_calibration"]
        merges = out["step_split"]["merges_available"]
        assert set(merges) == ({"gloo", "ipc"} if backend == "auto-gloo" else {backend})
        for m in merges:
            for md in ("overlapped", "pipelined", "serial"):
                assert cal["%s_%s_ms_per_step" % (m, md)] > 0
        assert cal["timed_merge"] == out["step_split"]["merge"] in merges
        assert out["step_split"]["timed_step"].startswith("2 build sweeps") == (cal["timed_form"] != "serial")
        if backend == "auto-gloo":  # both merges ran, agreed word for word, the faster was timed
            assert out["step_split"]["merges_agree"] is True
        if "ipc" in merges:
            assert out["step_split"]["flag_timeouts"] == 0 and out["step_split"]["merge_poisoned"] is False
        assert out["config"]["ranks_per_gpu"] == (2 if torch_count() < 2 else 1)
    assert "invalid" not in out and out["value"] > 0
    assert filter_keys or out["legs"]["c3_probe"]["member_rows_all_hit"] is True


def torch_count():
    import torch
    return torch.cuda.device_count()


@pytest.mark.timeout(300)
def test_bench_under_torch_distributed_run():
    """The driver's N > 1 launch: `python -m torch.distributed.run --nnodes=1
    --nproc-per-node 2 --master-addr 127.0.0.1 --master-port P bench.py --gpus
    2 ...`, the ranks from the launcher's environment (RANK / LOCAL_RANK /
    WORLD_SIZE), not self-started.  Both ranks share this box's one GPU, so the
    merge is the IPC one (the default `auto` needs one GPU per rank: checked
    below to refuse with exit 2 and no line); rank 0 alone prints the line."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    base = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
            "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2",
            "--global-keys", "8000000", "--filter-keys", "1000000000", "--steps", "3", "--warmup", "2",
            "--full", "--no-cpu-baseline", "--no-e2e", "--no-varlen", "--no-exact10", "--no-probe"]
    env = dict(os.environ)
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(v, None)
    r = subprocess.run(base + ["--backend", "ipc"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["step_split"]["merge"] == "ipc"
    assert out["multi_gpu_merged_equals_single_gpu_build"] is True and out["value"] > 0
    assert out["config"]["ranks_per_gpu"] == (2 if torch_count() < 2 else 1)
    if torch_count() < 2:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            base[base.index("--master-port") + 1] = str(s.getsockname()[1])
        r = subprocess.run(base, capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode != 0 and not [x for x in r.stdout.splitlines() if x.startswith("{")], r.stdout[-2000:]


@pytest.mark.timeout(300)
def test_bench_fault_nulls_the_value():
    """at N > 1 a merged filter that fails its own word
    check (here a bit flipped on rank 0 after the self-check step,
    --inject-merge-fault) must not publish a throughput: value null, the
    reasons in `invalid`, and a non-zero exit after the line."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo",
           "--global-keys", "2000000", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-e2e",
           "--no-varlen", "--no-exact10", "--no-probe", "--inject-merge-fault"]
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 3, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][0])
    assert out["value"] is None and out["multi_gpu_merged_equals_single_gpu_build"] is False
    assert any("multi_gpu_merged_equals_single_gpu_build" in x for x in out["invalid"])


@pytest.mark.timeout(300)
def test_bench_auto_drops_a_poisoned_ipc_merge():
    """--backend auto's agreement step with an IPC merge that fails safe: the
    last rank's merge status starts poisoned (--inject-ipc-poison), so every
    rank's IPC merge ends all-ones instead of exact.  The merges then disagree,
    IPC is dropped before any timing, the other merge (gloo here, RCCL on a
    multi-GPU node) is the one timed, and the line stands: its merged filter
    passes the word check."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "auto-gloo",
           "--global-keys", "2000000", "--filter-keys", "1000000000", "--steps", "2", "--warmup", "1",
           "--full", "--no-cpu-baseline", "--no-e2e", "--no-varlen", "--no-exact10", "--no-probe",
           "--inject-ipc-poison"]
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][0])
    ss = out["step_split"]
    assert ss["merges_agree"] is False and "ipc" not in ss["merges_available"] and ss["merge"] == "gloo"
    assert ss["merge_poisoned"] is True  # reported, though not the timed merge
    assert out["multi_gpu_merged_equals_single_gpu_build"] is True
    assert "invalid" not in out and out["value"] > 0


def test_bench_auto_refuses_ranks_sharing_a_gpu():
    """--backend auto (the default) with more ranks than visible GPUs
    exits 2, as nccl does, instead of timing N ranks on fewer GPUs."""
    if torch_count() >= 2:
        pytest.skip("two GPUs visible: auto runs one rank per GPU")
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 2 and "visible" in r.stderr, r.stderr[-2000:]


def test_bench_refuses_world_mismatch():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 2 and "WORLD_SIZE" in r.stderr


def test_one_context_two_streams(torch, oracle):
    """the partition workspace is shared by every build on a
    context; a build issued on another stream must wait for the previous one
    (build_dev's ws_done event) instead of overwriting its regions."""
    ctx = lsmbloom.Context(0)
    try:
        dev = torch.device("cuda:0")
        n = 1_500_000
        nb, k = lsmbloom.params(40_000_000, 0.01)
        assert lsmbloom.build_strategy(nb, n) == "partition"
        ka = torch.empty((n, 16), dtype=torch.uint8, device=dev)
        kb = torch.empty_like(ka)
        ctx.gen_key16_dev(11, 0, n, ka)
        ctx.gen_key16_dev(22, 0, n, kb)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        wa = torch.zeros(lsmbloom.num_words(nb), dtype=torch.int64, device=dev)
        wb = torch.zeros_like(wa)
        torch.cuda.synchronize()
        for _ in range(3):  # alternate streams back to back, no host sync between
            ctx.build_fixed_dev(ka, 16, n, nb, k, wa, stream=s1.cuda_stream)
            ctx.build_fixed_dev(kb, 16, n, nb, k, wb, stream=s2.cuda_stream)
        torch.cuda.synchronize()
        ctx.sync()
        assert np.array_equal(_u64(wa), oracle.build_fixed_mt(keygen.key16(11, 0, n), 16, nb, k, 8))
        assert np.array_equal(_u64(wb), oracle.build_fixed_mt(keygen.key16(22, 0, n), 16, nb, k, 8))
    finally:
        ctx.close()


def test_fset_and_builds_on_two_contexts_concurrently(torch, oracle):
    """flush / compaction builds on one context while the
    read path adds, removes and probes filters on another, from two host
    threads at once (src/compaction/scheduler.rs:37).  The filter set waits
    for its own probes only (per-set events; no device-wide synchronisation,
    which tests/test_capi_host.py checks in the source); here every result of
    both threads must be exact.  Whether the two contexts' work overlaps in
    time also depends on how the runtime maps streams to the 4 hardware
    queues, so no timing is asserted."""
    dev = torch.device("cuda:0")
    a, b = lsmbloom.Context(0), lsmbloom.Context(0)
    errors = []
    try:
        n = 4_000_000
        nb, k = lsmbloom.params(n, 0.01)
        keys = torch.empty((n, 16), dtype=torch.uint8, device=dev)
        a.gen_key16_dev(3, 0, n, keys, stream=a_stream(a))
        ref_build = oracle.build_fixed_mt(keygen.key16(3, 0, n), 16, nb, k, 8)

        def builder():
            try:
                words = torch.zeros(lsmbloom.num_words(nb), dtype=torch.int64, device=dev)
                for _ in range(20):
                    words.zero_()
                    a.build_fixed_dev(keys, 16, n, nb, k, words, stream=a_stream(a))
                a.sync()
                torch.cuda.synchronize()
                if not np.array_equal(_u64(words), ref_build):
                    errors.append("build differs")
            except Exception as e:  # noqa: BLE001
                errors.append(repr(e))

        th = threading.Thread(target=builder)
        th.start()
        fs = lsmbloom.FilterSet(b)
        filters = []
        for t in range(6):
            f = lsmbloom.BloomFilter.new(1000, 0.01)
            for i in range(100):
                f.insert(b"t%d_key_%05d" % (t, i))
            filters.append(f)
        for rep in range(10):
            slots = [fs.add_filter(f, b"t%d_key_00000" % t, b"t%d_key_00099" % t) for t, f in enumerate(filters)]
            q = [b"t%d_key_%05d" % (t, i) for t in range(6) for i in (0, 50, 99)] + [b"zzz", b"t0_key_00500"]
            got = fs.probe_keys(q)
            for j, key in enumerate(q):
                exp = 0
                for t, f in enumerate(filters):
                    lo, hi = b"t%d_key_00000" % t, b"t%d_key_00099" % t
                    if lo <= key <= hi and f.may_contain(key):
                        exp |= 1 << slots[t]
                assert int(got[j]) == exp, (rep, key)
            for sl in slots:
                fs.remove(sl)
        fs.close()
        th.join(timeout=120)
        assert not th.is_alive()
        assert not errors, errors
    finally:
        a.close()
        b.close()


def a_stream(c):
    """The context's own stream (NULL selects it)."""
    return 0


def _silent_rank_worker(rank, port, n, filter_n, q, late=False):
    """World 2 on cuda:0: both ranks build their shard; rank 1 then agrees on
    the word range and never runs its merge kernels (a rank that died after
    the range check), rank 0 merges device-ordered with a short timeout.
    late=True: rank 1 is alive but stalls past the timeout, then merges: its
    waits must see rank 0's poison (published across processes) and its own
    merge must end all-ones and raise too."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, os.path.join(ROOT, "storage-engine_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist

    import lsmbloom
    from lsmbloom import dist as ldist
    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        dev = torch.device("cuda:0")
        ctx = lsmbloom.Context(0)
        nb, k = lsmbloom.params(filter_n, 0.01)
        lo, hi = n * rank // 2, n * (rank + 1) // 2
        keys = torch.empty((hi - lo, 16), dtype=torch.uint8, device=dev)
        ctx.gen_key16_dev(0x5EED0001, lo, hi - lo, keys)
        words = torch.empty(lsmbloom.num_words(nb), dtype=torch.int64, device=dev)
        m = ldist.IpcMerge(words, ctx, ordered="device", timeout_ms=300)
        ctx.build_fixed_dev_new(keys, 16, hi - lo, nb, k, words)
        torch.cuda.synchronize()
        raised = None
        if rank == 0 or late:
            if rank == 1:
                m._check_range(0, words.numel())  # the range collective, then the stall
                time.sleep(1.5)
            t0 = time.time()
            try:
                m.allreduce(check=True)
            except ldist.MergePoisoned as e:
                raised = str(e)
            elapsed = time.time() - t0
            poisoned, tmo = m.status()
            q.put((rank, _digest(words.cpu().numpy().view(np.uint64)),
                   bool((words == -1).all().item()), raised, poisoned, tmo, elapsed))
        else:
            m._check_range(0, words.numel())  # the range collective, then silence
            q.put((rank, None, None, None, None, None, None))
        dist.barrier()
        m.close(check=False)
        ctx.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_ipc_merge_with_a_silent_rank_fails_safe(oracle):
    """rank 1 never merges.  Rank 0's device-ordered waits
    time out (300 ms), the merge poisons itself, writes no partial OR and
    leaves every word all-ones — a bit-superset of the oracle's merged filter,
    so no false negative — and allreduce(check=True) raises MergePoisoned."""
    import torch.multiprocessing as mp
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    n, filter_n = 2_000_000, 20_000_000
    procs = [mpc.Process(target=_silent_rank_worker, args=(r, port, n, filter_n, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=200) for _ in range(2)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    _, digest, all_ones, raised, poisoned, tmo, elapsed = res[0]
    assert raised and "poisoned" in raised
    assert poisoned and tmo >= 1
    assert all_ones
    nb, k = lsmbloom.params(filter_n, 0.01)
    ref = oracle.build_fixed_mt(keygen.key16(0x5EED0001, 0, n), 16, nb, k, 8)
    assert ref.any() and digest != _digest(ref)  # all-ones: every oracle bit set, and more
    assert elapsed < 30  # a poisoned merge does not wait out every phase


@pytest.mark.timeout(240)
def test_ipc_merge_with_a_late_rank_fails_safe():
    """The stalled (not dead) peer on the GPU: rank 1 merges 1.5 s late, past
    rank 0's 300 ms timeout.  Rank 0 gives up and poisons; rank 1's first wait
    then finds rank 0's flags already set but reads its poison word through the
    IPC mapping, so it poisons itself without reading rank 0's (possibly
    rewritten) words: both ranks end all-ones, with no timeout on rank 1, and
    both raise MergePoisoned."""
    import torch.multiprocessing as mp
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    procs = [mpc.Process(target=_silent_rank_worker, args=(r, port, 2_000_000, 20_000_000, q, True)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=200) for _ in range(2)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, digest, all_ones, raised, poisoned, tmo, elapsed in res:
        assert raised and "poisoned" in raised, rank
        assert poisoned and all_ones, rank
    assert res[0][5] >= 1  # rank 0 timed out waiting for rank 1
    assert res[1][5] == 0 and res[1][6] < 5  # rank 1 saw the poison at once


def test_merge_status_kernels(torch, ctx):
    """The fail-safe's kernels alone on one GPU: a wait that times out poisons
    the status words and counts; a wait whose flags are met but that sees a
    poison word poisons without a timeout; a poisoned or_gather / copy_slices
    writes all-ones and reads no source; the final fill writes all-ones only
    when poisoned."""
    dev = torch.device("cuda:0")
    flags = torch.zeros(8, dtype=torch.int32, device=dev)   # [0..2] epochs, [3] poison, [4] timeouts
    other = torch.zeros(8, dtype=torch.int32, device=dev)   # a peer's flag array
    st = flags.data_ptr() + 12
    torch.cuda.synchronize()
    # flags met, nobody poisoned: status stays clean, no timeout
    other[0] = 1
    flags[0] = 1
    torch.cuda.synchronize()
    ctx.flag_wait_dev([flags.data_ptr(), other.data_ptr()], 1, st, 1000,
                      poison_ptrs=[flags.data_ptr() + 12, other.data_ptr() + 12])
    assert ctx.merge_status(st) == (0, 0)
    # the fill leaves healthy words alone
    w = torch.arange(1000, dtype=torch.int64, device=dev)
    ctx.poison_fill_dev(w.data_ptr(), 1000, st)
    torch.cuda.synchronize()
    assert torch.equal(w, torch.arange(1000, dtype=torch.int64, device=dev))
    # flags met but the peer is poisoned: poisoned, no timeout, fast
    other[3] = 1
    torch.cuda.synchronize()
    t0 = time.time()
    ctx.flag_wait_dev([flags.data_ptr(), other.data_ptr()], 1, st, 5000,
                      poison_ptrs=[flags.data_ptr() + 12, other.data_ptr() + 12])
    assert ctx.merge_status(st) == (1, 0) and time.time() - t0 < 2.0
    # a flag short of the epoch times out (200 ms): counted
    clean = torch.zeros(8, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    t0 = time.time()
    ctx.flag_wait_dev([clean.data_ptr(), other.data_ptr()], 2, clean.data_ptr() + 12, 200)
    p, t = ctx.merge_status(clean.data_ptr() + 12)
    assert (p, t) == (1, 1) and time.time() - t0 >= 0.15
    # poisoned kernels: all-ones, sources untouched
    src = [torch.randint(0, 2 ** 62, (3001,), dtype=torch.int64, device=dev) for _ in range(3)]
    keep = [x.clone() for x in src]
    dst = torch.zeros(3001, dtype=torch.int64, device=dev)
    ctx.or_gather_dev(dst.data_ptr(), [x.data_ptr() for x in src], 3001, status_ptr=st)
    out = torch.zeros(3001, dtype=torch.int64, device=dev)
    ctx.copy_slices_dev(out.data_ptr(), [src[0].data_ptr(), 0, src[2].data_ptr()], 1001, 3001, status_ptr=st)
    ctx.poison_fill_dev(w.data_ptr(), 999, st)
    torch.cuda.synchronize()
    assert bool((dst == -1).all())
    assert bool((out[:1001] == -1).all()) and bool((out[1001:2002] == 0).all()) and bool((out[2002:] == -1).all())
    assert bool((w[:999] == -1).all()) and int(w[999]) == 999
    assert all(torch.equal(a, b) for a, b in zip(src, keep))
    # a clean status leaves the kernels exact
    fresh = torch.zeros(8, dtype=torch.int32, device=dev)
    ctx.or_gather_dev(dst.data_ptr(), [x.data_ptr() for x in src], 3001, status_ptr=fresh.data_ptr() + 12)
    torch.cuda.synchronize()
    assert torch.equal(dst, src[0] | src[1] | src[2])


@pytest.mark.parametrize("nsrc", [1, 2, 3, 5, 8, 9, 12, 16])
@pytest.mark.parametrize("nwords,offset", [(1 << 20, 0), (100_003, 1), (7, 0)])
def test_or_gather_and_copy_slices_dev(torch, ctx, nsrc, nwords, offset):
    """The merge kernels alone (lsmb_or_gather_dev: N sources at compile time
    for N <= 8, a runtime loop above; lsmb_copy_slices_dev: every slice of a
    range from its own source in one kernel, a NULL source leaving its slice
    alone), against numpy; 16-B aligned and 8-B-only (offset) pointers, ragged
    last slices, and the in-place case (the destination is source 0)."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(nsrc * 1000 + nwords)
    src = [torch.randint(-2 ** 62, 2 ** 62, (nwords + offset,), generator=g, dtype=torch.int64).to(dev)
           for _ in range(nsrc)]
    ref = _u64(src[0][offset:]).copy()
    for s in src[1:]:
        ref |= _u64(s[offset:])
    dst = torch.zeros(nwords + offset, dtype=torch.int64, device=dev)
    ctx.or_gather_dev(dst.data_ptr() + 8 * offset, [s.data_ptr() + 8 * offset for s in src], nwords)
    torch.cuda.synchronize()
    assert np.array_equal(_u64(dst[offset:]), ref)
    keep = src[0].clone()  # in place: source 0 is the destination
    ctx.or_gather_dev(src[0].data_ptr() + 8 * offset, [s.data_ptr() + 8 * offset for s in src], nwords)
    torch.cuda.synchronize()
    assert np.array_equal(_u64(src[0][offset:]), ref)
    src[0].copy_(keep)
    # copy_slices: slice r from source r, slice `skip` left alone
    per = (nwords + nsrc - 1) // nsrc
    per += per & 1
    skip = nsrc // 2
    out = torch.full((nwords + offset,), -1, dtype=torch.int64, device=dev)
    ptrs = [s.data_ptr() + 8 * offset if r != skip else 0 for r, s in enumerate(src)]
    ctx.copy_slices_dev(out.data_ptr() + 8 * offset, ptrs, per, nwords)
    torch.cuda.synchronize()
    got = _u64(out[offset:])
    for r in range(nsrc):
        a, b = min(nwords, r * per), min(nwords, (r + 1) * per)
        want = np.full(b - a, np.uint64(2 ** 64 - 1)) if r == skip else _u64(src[r][offset:])[a:b]
        assert np.array_equal(got[a:b], want), r
