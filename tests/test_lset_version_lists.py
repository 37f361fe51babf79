"""Per-table candidate key lists of a whole Version (lsmb_lset_probe_version_lists*):
the Version probe's answer transposed, L0 included, from one hash per key.
With T0 L0 tables and G row tables, Version ordinal v < T0 is the L0 table at
position v, v >= T0 the rows' ordinal v - T0, and

    index[starts[v] : starts[v+1]] = the ascending indices i of the keys with
    min_v <= key i <= max_v && may_contain(filter v, key i)

The expectation is the CPU oracle's answer (reference() of
tests/test_lset_version.py) and the set's own probe_version (held against the
oracle there), transposed by lset_support's version_lists_from; the pass-edge test takes
it from a bisect over the ranges.  Every comparison covers all V + 1 starts and
all entries.
"""
import bisect
import ctypes
import os
import subprocess

import numpy as np
import pytest

import keygen
import lsmbloom
from lsmbloom import LevelSet
from lset_support import (POISON, add_tables, always_maybe, build_table, check_lists, cpp_bin, dev_lists, dev_vlists,
                          expected_ids, expected_mask, l0_tables, lists_from_ids, low_bits, queries, reference, row_tables,
                          version_lists_from)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "lset_vlists_plan_test.cpp")
NONE = lsmbloom.LSMB_LSET_NONE
L0 = lsmbloom.LSMB_LSET_ROW_L0
EINVAL = lsmbloom.LSMB_EINVAL
vp = ctypes.c_void_p


def own_lists(ls, mask, ids):
    return version_lists_from(mask, ids, ls.l0_tables(), ls.table_order()[0])


# ---------------------------------------------------------------- without a GPU

def test_version_lists_from_on_a_hand_written_example():
    # two L0 tables; one row whose table ids 50, 40 are ordinals 0, 1
    mask = np.array([1, 3, 2, 0], dtype=np.uint64)
    ids = np.array([[40, NONE, 50, 40]], dtype=np.uint32)
    starts, index = version_lists_from(mask, ids, 2, [50, 40])
    assert starts.tolist() == [0, 2, 4, 5, 7] and index.tolist() == [0, 1, 1, 2, 2, 0, 3]
    assert starts.dtype == np.uint64 and index.dtype == np.uint32
    # no L0 table: lists_from_ids; no row: the L0 lists and the total
    s, i = version_lists_from(np.zeros(4, np.uint64), ids, 0, [50, 40])
    assert s.tolist() == [0, 1, 3] and i.tolist() == [2, 0, 3]
    s, i = version_lists_from(mask, np.zeros((0, 4), np.uint32), 2, [])
    assert s.tolist() == [0, 2, 4] and i.tolist() == [0, 1, 1, 2]
    s, i = version_lists_from(np.zeros(0, np.uint64), np.zeros((0, 0), np.uint32), 0, [])
    assert s.tolist() == [0] and i.size == 0


def test_version_lists_entry_points_reject_a_null_set():
    L = lsmbloom.lib()
    starts = np.full(4, 7, np.uint64)
    index = np.full(4, 9, np.uint32)
    data = np.zeros(16, np.uint8)
    p8, ps, pi = data.ctypes.data_as(lsmbloom.u8p), starts.ctypes.data_as(lsmbloom.u64p), index.ctypes.data_as(lsmbloom.u32p)
    assert L.lsmb_lset_version_tables(None) == 0
    assert L.lsmb_lset_version_lists_work_bytes(None, 1000) == 0
    assert L.lsmb_lset_version_order(None, pi, ps) == EINVAL
    assert L.lsmb_lset_version_order(None, None, None) == EINVAL
    assert L.lsmb_lset_probe_version_lists(None, p8, None, 4, 4, ps, pi, 4) == EINVAL
    assert L.lsmb_lset_probe_version_lists_dev(None, vp(1), None, 4, 4, vp(1), vp(1), 4, vp(16), 1 << 20, None) == EINVAL
    assert (starts == 7).all() and (index == 9).all()
    assert L.lsmb_abi_version() == 6


def test_version_lists_entry_points_are_in_the_signature_table():
    c = ctypes
    S = lsmbloom.SIGNATURES
    assert S["lsmb_lset_version_tables"] == (c.c_uint64, [vp])
    assert S["lsmb_lset_version_order"] == (c.c_int, [vp, lsmbloom.u32p, lsmbloom.u64p])
    assert S["lsmb_lset_version_lists_work_bytes"] == (c.c_uint64, [vp, c.c_uint64])
    assert S["lsmb_lset_probe_version_lists_dev"] == (
        c.c_int, [vp, vp, vp, c.c_uint32, c.c_uint64, vp, vp, c.c_uint64, vp, c.c_uint64, vp])
    assert S["lsmb_lset_probe_version_lists"] == (
        c.c_int, [vp, lsmbloom.u8p, lsmbloom.u64p, c.c_uint32, c.c_uint64, lsmbloom.u64p, lsmbloom.u32p, c.c_uint64])
    for name in ("lsmb_lset_version_tables", "lsmb_lset_version_order", "lsmb_lset_version_lists_work_bytes",
                 "lsmb_lset_probe_version_lists_dev", "lsmb_lset_probe_version_lists"):
        assert hasattr(lsmbloom.lib(), name)
    for name in ("version_tables", "version_order", "version_lists_work_bytes", "probe_version_lists",
                 "probe_version_lists_keys", "probe_version_lists_dev"):
        assert callable(getattr(LevelSet, name))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan_ubsan"])
def test_lset_vlists_plan_and_reference_host(tmp_path, flags):
    """The mask row width, the workspace layout and lset_vlists_ref
    (csrc/lset_vlists_plan.hpp) by tests/cpp/lset_vlists_plan_test.cpp: a
    stand-alone host program, once plain and once under ASan and UBSan."""
    exe = str(tmp_path / "lset_vlists_plan_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, PLAN_SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout


def test_cpp_mirror_version_lists_argument_checks():
    r = subprocess.run([cpp_bin("lset_version_lists_test")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


# ------------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def ctx():
    c = lsmbloom.Context(0)
    yield c
    c.close()


def host_vlists(ls, kind, q):
    if kind == "var":
        return ls.probe_version_lists_keys(q)
    data = np.frombuffer(b"".join(q), dtype=np.uint8)
    return ls.probe_version_lists(data, key_len=16 if kind == "fixed16" else 12)


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["sst", "mixed"])
@pytest.mark.parametrize("t0", [1, 8, 33, 64])
def test_version_lists_match_the_oracle_and_the_version_probe(ctx, oracle, t0, geom):
    tabs, _ = l0_tables(geom)
    rows = row_tables()
    placed = [(r, t) for r, row in enumerate(rows) for t in row]
    for j, t in enumerate(tabs[:t0]):
        placed.insert(2 * j, (L0, t))
    ls = LevelSet(ctx)
    ls.add_many([r for r, _ in placed], [t[0] for _, t in placed],
                [oracle.serialize(t[1], t[2], t[3]) for _, t in placed], [(t[4], t[5]) for _, t in placed])
    ls.seal()
    G = sum(len(r) for r in rows)
    assert ls.l0_tables() == t0 and ls.rows() == 3 and ls.version_tables() == t0 + G
    vids, part = ls.version_order()
    order_ids, base = ls.table_order()
    assert vids.dtype == np.uint32 and part.dtype == np.uint64
    assert vids.tolist() == ls.l0_order().tolist() + order_ids.tolist()
    assert part.tolist() == [0] + [t0 + int(b) for b in base]
    for kind in ("fixed16", "fixed12", "var"):
        q = queries(kind)
        mask, ids = reference(geom, kind)
        for n in (1, 257, 5000):
            got = host_vlists(ls, kind, q[:n])
            check_lists(got, version_lists_from(low_bits(mask[:n], t0), ids[:, :n], t0, order_ids), ("oracle", kind, n))
            if kind == "var":
                gm, gi = ls.probe_version_keys(q[:n])
            else:
                gm, gi = ls.probe_version(np.frombuffer(b"".join(q[:n]), dtype=np.uint8),
                                          key_len=16 if kind == "fixed16" else 12)
            check_lists(got, version_lists_from(gm, gi, t0, order_ids), ("probe", kind, n))
            assert int(got[0][t0]) == sum(bin(int(m)).count("1") for m in gm)  # starts[T0] = the L0 entries
    ls.close()


@pytest.fixture(scope="module")
def small_set(ctx, oracle):
    """T0 = 3 overlapping L0 tables and two rows of 4 and 3 tables over 16-byte
    keys (quantile ranges of 4000 keys each), 70 001 query keys (members and
    absent keys, shuffled) and probe_version()'s answers for them, computed once."""
    ls = LevelSet(ctx)
    for r, (seed, cuts) in enumerate([(0x5EED0700, 4), (0x5EED0701, 3)]):
        srt = sorted(bytes(x) for x in keygen.key16(seed, 0, 4000))
        tabs = []
        for c in range(cuts):
            part = srt[c * len(srt) // cuts:(c + 1) * len(srt) // cuts]
            tabs.append(build_table(oracle, 100 * r + c + 1, part, (len(part), 0.01)))
        add_tables(ls, oracle, r, tabs[::-1])
        if r == 0:
            for j, (a, b) in enumerate([(0, 2500), (1000, 3500), (2000, 4000)]):
                add_tables(ls, oracle, L0, [build_table(oracle, 900 + j, srt[a:b:2], ((b - a) // 2, 0.01))])
    ls.seal()
    assert ls.l0_tables() == 3 and ls.total_tables() == 7 and ls.version_tables() == 10
    q = np.concatenate([keygen.key16(0x5EED0700, 0, 4000), keygen.key16(0x5EED0701, 0, 4000),
                        keygen.key16(0x5EED0702, 0, 62001)])
    q = np.ascontiguousarray(q[np.random.default_rng(32).permutation(len(q))])
    assert q.shape == (70001, 16)
    mask, ids = ls.probe_version(q, key_len=16)
    assert (mask != 0).sum() > 2000 and (mask == 0).sum() > 8000 and (ids != NONE).sum() > 8000
    mask.setflags(write=False)
    ids.setflags(write=False)
    yield ls, q, mask, ids
    ls.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 70001])
def test_version_lists_batch_sizes_with_device_keys(small_set, n):
    """The wave (64), the L0 compaction's tile (1024 keys) and the rows' split
    tile (2048 elements) at their edges, and more than one tile of each."""
    import torch

    ls, q, mask, ids = small_set
    dq = torch.from_numpy(q[:n]).to("cuda:0")
    exp = own_lists(ls, mask[:n], ids[:, :n])
    check_lists(dev_vlists(ls, dq, n), exp, n)
    if n in (65, 2049):  # the host entry point and the any-length key source agree
        check_lists(ls.probe_version_lists(q[:n], key_len=16), exp, n)
        q7 = np.ascontiguousarray(q[:n, :7])
        check_lists(ls.probe_version_lists(q7, key_len=7), own_lists(ls, *ls.probe_version(q7, key_len=7)), n)


@pytest.mark.gpu
def test_version_lists_grid_stride(ctx, oracle):
    """600 000 aligned 16-byte keys and 300 000 var-len keys: past one resident
    grid of 1024-lane workgroups (2 and 1 per CU on 256 CUs) of the ordinal
    instantiations."""
    import torch

    n = 600_000
    keys = keygen.key16(0x5EED0700, 0, n)
    srt = sorted(bytes(x) for x in keys[:4000])
    rng = np.random.default_rng(66)
    ls = LevelSet(ctx)
    for j in range(8):  # overlapping quantile ranges, members from inside
        a = int(rng.integers(0, 3000))
        part = srt[a:a + int(rng.integers(200, 1000))]
        t = build_table(oracle, 50 + j, part[::2], (1000, 0.01))
        ls.add(L0, t[0], oracle.serialize(t[1], t[2], t[3]), part[0], part[-1])
    for c in range(16):
        add_tables(ls, oracle, 0, [build_table(oracle, 900 + c, srt[c * 250:(c + 1) * 250], (250, 0.01))])
    ls.seal()
    assert ls.version_tables() == 24
    gm, gi = ls.probe_version(keys, key_len=16)
    assert (gm[:4000] != 0).sum() > 300 and (gi[0, :4000] != NONE).all()
    dq = torch.from_numpy(keys).to("cuda:0")
    check_lists(dev_vlists(ls, dq, n), own_lists(ls, gm, gi), "fixed16")
    # var-len: the first 8 .. 16 bytes of the first 300 000 keys
    nv = 300_000
    lens = 8 + (np.arange(nv) * 7) % 9
    lens[:4000] = 16  # the members stay whole
    data = keys[:nv][np.arange(16)[None, :] < lens[:, None]]
    offs = np.zeros(nv + 1, np.uint64)
    np.cumsum(lens, out=offs[1:])
    vm, vi = ls.probe_version(data, offs)
    assert (vi[0, :4000] != NONE).all() and (vi[0, 4000:] == NONE).sum() > 100_000
    d_data = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to("cuda:0")
    d_offs = torch.from_numpy(offs.view(np.int64)).to("cuda:0")
    check_lists(dev_vlists(ls, d_data, nv, offsets=d_offs, key_len=0), own_lists(ls, vm, vi), "var")
    ls.close()


@pytest.mark.gpu
def test_version_lists_capacity(small_set):
    import torch

    ls, q, mask, ids = small_set
    n = 5000
    T0, V = ls.l0_tables(), ls.version_tables()
    dq = torch.from_numpy(q[:n]).to("cuda:0")
    es, ei = own_lists(ls, mask[:n], ids[:, :n])
    counted, _ = dev_vlists(ls, dq, n, cap=0)  # cap == 0, null index: a counting call
    assert np.array_equal(counted, es)
    E0, total = int(counted[T0]), int(counted[V])
    assert 1 < E0 < total - 1 and total == ei.size
    for cap in (1, E0 - 1, E0, E0 + 1, total - 1, total, total + 7):
        starts, index = dev_vlists(ls, dq, n, cap=cap)
        assert np.array_equal(starts, es), cap
        w = min(total, cap)
        assert index.shape == (cap,) and np.array_equal(index[:w], ei[:w]), cap
        assert (index[w:] == POISON).all(), cap  # nothing past min(total, cap) is touched
    # the host form: a counting call, then the first entries only
    s2, i2 = ls.probe_version_lists(q[:n], key_len=16, cap=0)
    assert np.array_equal(s2, es) and i2.size == 0
    s2, i2 = ls.probe_version_lists(q[:n], key_len=16, cap=E0 + 1)
    assert np.array_equal(s2, es) and np.array_equal(i2, ei[:E0 + 1])
    # a capacity with a null index is refused
    L = lsmbloom.lib()
    starts = torch.full((V + 1,), -1, dtype=torch.int64, device="cuda:0")
    work = torch.empty(ls.version_lists_work_bytes(n), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert L.lsmb_lset_probe_version_lists_dev(ls.h, vp(dq.data_ptr()), None, 16, n, vp(starts.data_ptr()), None, 5,
                                               vp(work.data_ptr()), work.numel(), None) == EINVAL
    torch.cuda.synchronize()
    assert (starts.cpu().numpy() == -1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("t0,total,nrows", [(5, 257, 2), (64, 256, 1)])
def test_version_lists_radix_pass_edges_behind_l0(ctx, t0, total, nrows):
    """One and two radix passes of the rows' split (256 tables is the edge)
    with the lists based behind an L0 part; always-maybe filters, so the
    ranges alone decide and the expectation is a bisect."""
    rng = np.random.default_rng(2000 + total)
    f = always_maybe()
    ls = LevelSet(ctx)
    tids = rng.permutation(total).astype(np.uint32) + 100
    for t in rng.permutation(total):
        r = next(r for r in range(nrows) if t < total * (r + 1) // nrows)
        ls.add_filter(r, int(tids[t]), f, b"t%07d0" % t, b"t%07d5" % t)
    l0_rg = []
    for j in range(t0):  # overlapping spans of whole tables, some ending inside one
        a = int(rng.integers(0, total - 1))
        b = min(total - 1, a + int(rng.integers(0, 40)))
        l0_rg.append((b"t%07d0" % a, b"t%07d%d" % (b, int(rng.integers(0, 10)))))
        ls.add_filter(L0, 10_000 + j, f, *l0_rg[-1])
    ls.seal()
    assert ls.version_tables() == t0 + total and np.array_equal(ls.table_order()[0], tids)
    n = 5000
    tq = rng.integers(0, total + 2, n)
    tq[:min(total, n)] = rng.permutation(total)[:n]
    keys = [b"t%07d%d" % (t, d) for t, d in zip(tq, rng.integers(0, 10, n))]
    los = [b"t%07d0" % t for t in range(total)]
    exp_ord = np.full((nrows, n), NONE, dtype=np.uint32)
    exp_mask = np.zeros(n, dtype=np.uint64)
    for i, key in enumerate(keys):
        j = bisect.bisect_right(los, key) - 1
        if j >= 0 and key <= b"t%07d5" % j:
            exp_ord[next(r for r in range(nrows) if j < total * (r + 1) // nrows), i] = j
        for v, (lo, hi) in enumerate(l0_rg):
            if lo <= key <= hi:
                exp_mask[i] |= np.uint64(1 << v)
    exp = version_lists_from(exp_mask, exp_ord, t0, np.arange(total, dtype=np.uint32))
    assert n // 6 < int(exp[0][-1]) - int(exp[0][t0]) < n and int(exp[0][t0]) > 0
    got = ls.probe_version_lists_keys(keys)
    check_lists(got, exp, total)
    check_lists(got, own_lists(ls, *ls.probe_version_keys(keys)), total)
    ls.close()


@pytest.mark.gpu
def test_version_lists_skew(ctx):
    f = always_maybe()
    ls = LevelSet(ctx)
    for j in range(64):
        ls.add_filter(L0, j, f, b"a", b"z\xff")
    ls.add_filter(0, 100, f, b"b", b"d")
    ls.add_filter(0, 101, f, b"f", b"h")
    ls.seal()
    n = 5000
    keys = [b"g%05d" % i for i in range(n)]
    starts, index = ls.probe_version_lists_keys(keys)
    every = np.arange(n, dtype=np.uint32)
    assert starts.tolist() == [n * j for j in range(65)] + [64 * n, 65 * n]
    assert int(starts[64]) == 64 * n
    assert np.array_equal(index, np.tile(every, 65))
    # keys outside every range: below, above
    for keys in ([b"A%05d" % i for i in range(n)] + [b"", b"Z"], [b"z\xff\x00%d" % i for i in range(n)] + [b"\xff" * 20]):
        starts, index = ls.probe_version_lists_keys(keys)
        assert starts.tolist() == [0] * 67 and index.size == 0
    ls.close()


@pytest.mark.gpu
def test_version_lists_degenerate_sets(ctx, oracle, small_set):
    import torch

    base, q, mask, ids = small_set
    dev = "cuda:0"
    n = 3000
    dq = torch.from_numpy(q[:n]).to(dev)
    tabs, _ = l0_tables("sst")
    rows = row_tables()
    qv = queries("var")[:1500]
    # T0 = 0: the bytes of probe_lists_dev, and its workspace
    ls = LevelSet(ctx)
    add_tables(ls, oracle, 0, rows[1])
    add_tables(ls, oracle, 1, rows[2])
    ls.seal()
    assert ls.version_tables() == ls.total_tables() == 8
    assert ls.version_lists_work_bytes(n) == ls.lists_work_bytes(n) > 0
    assert ls.version_order()[0].tolist() == ls.table_order()[0].tolist()
    assert ls.version_order()[1].tolist() == [0] + ls.table_order()[1].tolist()
    data, offs = keygen.pack(qv)
    d_data = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    a = dev_vlists(ls, d_data, len(qv), offsets=d_offs, key_len=0)
    b = dev_lists(ls, d_data, len(qv), offsets=d_offs, key_len=0)
    assert a[1].size > 100 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    ha, hb = ls.probe_version_lists_keys(qv), ls.probe_lists_keys(qv)
    assert ha[0].tobytes() == hb[0].tobytes() and ha[1].tobytes() == hb[1].tobytes()
    ls.close()
    # R = 0: the L0 lists alone
    ls = LevelSet(ctx)
    for t in tabs[:9]:
        add_tables(ls, oracle, L0, [t])
    ls.seal()
    assert ls.rows() == 0 and ls.version_tables() == 9 and ls.version_order()[1].tolist() == [0, 9]
    em, _ = expected_mask(oracle, tabs[:9], qv)
    exp = version_lists_from(em, np.zeros((0, len(qv)), np.uint32), 9, [])
    assert exp[1].size > 100
    check_lists(ls.probe_version_lists_keys(qv), exp, "R = 0, host")
    check_lists(dev_vlists(ls, d_data, len(qv), offsets=d_offs, key_len=0), exp, "R = 0, device")
    ls.close()
    # R > 0 with every row table dropped by derive: the L0 lists alone
    child = base.derive([int(t) for t in base.table_order()[0]])
    child.seal()
    assert child.rows() == 2 and child.total_tables() == 0 and child.version_tables() == 3
    assert child.version_order()[1].tolist() == [0, 3, 3, 3]
    assert 0 < child.version_lists_work_bytes(n) < base.version_lists_work_bytes(n)
    exp = version_lists_from(mask[:n], np.zeros((0, n), np.uint32), 3, [])
    check_lists(dev_vlists(child, dq, n), exp, "rows emptied, device")
    check_lists(child.probe_version_lists(q[:n], key_len=16), exp, "rows emptied, host")
    child.close()
    # an empty sealed set: one zero start, no workspace
    em = LevelSet(ctx)
    em.seal()
    assert em.version_tables() == 0 and em.version_lists_work_bytes(100) == 0
    vids, part = em.version_order()
    assert vids.size == 0 and part.tolist() == [0, 0]
    s, i = em.probe_version_lists_keys([b"a", b"b"])
    assert s.tolist() == [0] and i.size == 0
    one = torch.full((1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    em.probe_version_lists_dev(dq, n, one, None, None, key_len=16)
    torch.cuda.synchronize()
    assert one.cpu().numpy().tolist() == [0]
    em.close()
    # n = 0: V + 1 zero starts and nothing else, workspace or not
    V = base.version_tables()
    assert base.version_lists_work_bytes(0) == 0
    starts = torch.full((V + 1,), -1, dtype=torch.int64, device=dev)
    index = torch.full((8,), POISON - (1 << 32), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    base.probe_version_lists_dev(dq, 0, starts, index, None, key_len=16)
    torch.cuda.synchronize()
    assert (starts.cpu().numpy() == 0).all() and (index.cpu().numpy().view(np.uint32) == POISON).all()
    s0, i0 = base.probe_version_lists_keys([])
    assert s0.tolist() == [0] * (V + 1) and i0.size == 0


@pytest.mark.gpu
def test_version_lists_contract(ctx, small_set):
    import torch

    ls, q, mask, ids = small_set
    L = lsmbloom.lib()
    dev = "cuda:0"
    V = ls.version_tables()
    n = 3000
    dq = torch.from_numpy(q[:n]).to(dev)
    exp = own_lists(ls, mask[:n], ids[:, :n])
    need = ls.version_lists_work_bytes(n)
    assert need > ls.lists_work_bytes(n) > 0 and ls.version_lists_work_bytes(1 << 32) == 0
    assert ls.version_lists_work_bytes(2 * n) > need
    # a workspace one byte short, null, misaligned by 8; n = 2^32: LSMB_EINVAL, outputs untouched
    starts = torch.full((V + 1,), -1, dtype=torch.int64, device=dev)
    index = torch.full((8,), POISON - (1 << 32), dtype=torch.int32, device=dev)
    work = torch.empty(need + 16, dtype=torch.uint8, device=dev)
    assert work.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    args = (ls.h, vp(dq.data_ptr()), None, 16, n, vp(starts.data_ptr()), vp(index.data_ptr()), 8)
    assert L.lsmb_lset_probe_version_lists_dev(*args, vp(work.data_ptr()), need - 1, None) == EINVAL
    assert L.lsmb_lset_probe_version_lists_dev(*args, None, need, None) == EINVAL
    assert L.lsmb_lset_probe_version_lists_dev(*args, vp(work.data_ptr() + 8), need, None) == EINVAL
    assert L.lsmb_lset_probe_version_lists_dev(ls.h, vp(dq.data_ptr()), None, 16, 1 << 32, vp(starts.data_ptr()),
                                               vp(index.data_ptr()), 8, vp(work.data_ptr()), need, None) == EINVAL
    assert L.lsmb_lset_probe_version_lists_dev(ls.h, vp(dq.data_ptr()), None, 16, n, None, vp(index.data_ptr()), 8,
                                               vp(work.data_ptr()), need, None) == EINVAL
    with pytest.raises(ValueError):
        ls.probe_version_lists_dev(dq, n, starts, index, work[:need - 1], key_len=16)
    hs, hi = np.full(V + 1, 7, np.uint64), np.full(8, 9, np.uint32)
    assert L.lsmb_lset_probe_version_lists(ls.h, q.ctypes.data_as(lsmbloom.u8p), None, 16, 1 << 32,
                                           hs.ctypes.data_as(lsmbloom.u64p), hi.ctypes.data_as(lsmbloom.u32p), 8) == EINVAL
    assert L.lsmb_lset_probe_version_lists(ls.h, q.ctypes.data_as(lsmbloom.u8p), None, 16, n,
                                           hs.ctypes.data_as(lsmbloom.u64p), None, 8) == EINVAL
    assert (hs == 7).all() and (hi == 9).all()
    torch.cuda.synchronize()
    assert (starts.cpu().numpy() == -1).all() and (index.cpu().numpy().view(np.uint32) == POISON).all()
    # before seal: every entry point refuses (or answers 0)
    un = LevelSet(ctx)
    un.add_filter(L0, 1, always_maybe(), b"a", b"b")
    assert un.version_tables() == 0 and un.version_lists_work_bytes(100) == 0
    with pytest.raises(ValueError):
        un.version_order()
    with pytest.raises(ValueError):
        un.probe_version_lists_keys([b"a"])
    with pytest.raises(ValueError):
        un.probe_version_lists_dev(dq, n, starts, index, work, key_len=16)
    torch.cuda.synchronize()
    assert (starts.cpu().numpy() == -1).all()
    un.close()
    # two probes on two streams with two workspaces, issued back to back
    st = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    ns = (3000, 2500)
    exps = [own_lists(ls, mask[:m], ids[:, :m]) for m in ns]
    outs = []
    for j in range(2):
        outs.append((torch.full((V + 1,), -1, dtype=torch.int64, device=dev),
                     torch.full((exps[j][1].size,), POISON - (1 << 32), dtype=torch.int32, device=dev),
                     torch.empty(ls.version_lists_work_bytes(ns[j]), dtype=torch.uint8, device=dev)))
    torch.cuda.synchronize()
    for j in range(2):
        ls.probe_version_lists_dev(dq, ns[j], outs[j][0], outs[j][1], outs[j][2], key_len=16, stream=st[j].cuda_stream)
    for s in st:
        s.synchronize()
    for j in range(2):
        got = (outs[j][0].cpu().numpy().view(np.uint64), outs[j][1].cpu().numpy().view(np.uint32))
        check_lists(got, exps[j], "stream %d" % j)
    # two consecutive runs are byte-identical
    a = dev_vlists(ls, dq, n)
    b = dev_vlists(ls, dq, n)
    check_lists(a, exp, "run 1")
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.gpu
def test_version_lists_after_edits(ctx, oracle):
    tabs, _ = l0_tables("mixed")
    rows = row_tables()
    a, b, c, d = tabs[0], tabs[1], tabs[3], tabs[4]
    q = queries("var")[:1500]
    parent = LevelSet(ctx)
    for t in (a, b, c):
        add_tables(parent, oracle, L0, [t])
    add_tables(parent, oracle, 0, rows[1])
    parent.seal()
    drop_row = rows[1][2]
    child = parent.derive([b[0], drop_row[0]])
    add_tables(child, oracle, L0, [d])
    child.seal()
    assert parent.version_order()[0].tolist()[:3] == [a[0], b[0], c[0]]
    assert child.version_order()[0].tolist()[:3] == [a[0], c[0], d[0]]  # the positions after b shift down
    assert child.version_tables() == 3 + len(rows[1]) - 1 and drop_row[0] not in child.version_order()[0]
    got_p, got_c = parent.probe_version_lists_keys(q), child.probe_version_lists_keys(q)
    check_lists(got_p, own_lists(parent, *parent.probe_version_keys(q)), "parent")
    check_lists(got_c, own_lists(child, *child.probe_version_keys(q)), "child")
    row1 = [t for t in rows[1] if t[0] != drop_row[0]]
    em, _ = expected_mask(oracle, [a, c, d], q)
    check_lists(got_c, version_lists_from(em, expected_ids(oracle, [row1], q), 3, child.table_order()[0]), "oracle")

    def l0_list(got, v):
        return got[1][int(got[0][v]):int(got[0][v + 1])]

    assert np.array_equal(l0_list(got_c, 0), l0_list(got_p, 0))  # a stays at position 0
    assert np.array_equal(l0_list(got_c, 1), l0_list(got_p, 2))  # c moves from position 2 to 1
    assert l0_list(got_p, 2).size > 0
    child.close()
    parent.close()


@pytest.mark.gpu
def test_cpp_mirror_version_lists_gpu():
    r = subprocess.run([cpp_bin("lset_version_lists_test"), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout
