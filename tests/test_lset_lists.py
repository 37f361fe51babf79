"""Per-table candidate key lists of a level set (lsmb_lset_probe_lists*): the
level-set probe's answer transposed, for a reader that works table by table.
With table j of row r (in the row's sealed order) as ordinal g = base_r + j,

    index[starts[g] : starts[g+1]] = the ascending indices i of the keys with
    min_g <= key i <= max_g && may_contain(filter g, key i)

The expectation everywhere is the set's own probe() (held against the CPU
oracle by tests/test_lset.py), mapped id -> ordinal through table_order() with
unique ids and grouped by numpy's stable argsort; the first GPU test also
derives it from the oracle directly, the pass-count test from a bisect over
the ranges.  Every comparison covers all G + 1 starts and all entries.
"""
import bisect
import ctypes
import os
import subprocess
import time

import numpy as np
import pytest

import keygen
import lsmbloom
from lsmbloom import LevelSet
from lset_support import (POISON, add_tables, always_maybe, build_table, check_lists, cpp_bin, dev_lists, expected_ids,
                          lists_from_ids)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "lset_lists_plan_test.cpp")
NONE = lsmbloom.LSMB_LSET_NONE
vp = ctypes.c_void_p


def lists_from_ordinals(ord_rn, G):
    """uint32 [R, n] ordinals (NONE: no table) -> (starts, index)."""
    return lists_from_ids(ord_rn, np.arange(G, dtype=np.uint32))


# ---------------------------------------------------------------- without a GPU

def test_lset_lists_entry_points_reject_a_null_set():
    L = lsmbloom.lib()
    starts = np.full(4, 7, np.uint64)
    index = np.full(4, 9, np.uint32)
    data = np.zeros(16, np.uint8)
    p8, ps, pi = data.ctypes.data_as(lsmbloom.u8p), starts.ctypes.data_as(lsmbloom.u64p), index.ctypes.data_as(lsmbloom.u32p)
    assert L.lsmb_lset_total_tables(None) == 0
    assert L.lsmb_lset_lists_work_bytes(None, 1000) == 0
    assert L.lsmb_lset_table_order(None, pi, ps) == lsmbloom.LSMB_EINVAL
    assert L.lsmb_lset_table_order(None, None, None) == lsmbloom.LSMB_EINVAL
    assert L.lsmb_lset_probe_lists(None, p8, None, 4, 4, ps, pi, 4) == lsmbloom.LSMB_EINVAL
    assert L.lsmb_lset_probe_lists_dev(None, vp(1), None, 4, 4, vp(1), vp(1), 4, vp(16), 1 << 20, None) == lsmbloom.LSMB_EINVAL
    assert (starts == 7).all() and (index == 9).all()


def test_lset_lists_entry_points_are_in_the_signature_table():
    c = ctypes
    S = lsmbloom.SIGNATURES
    assert S["lsmb_lset_total_tables"] == (c.c_uint64, [vp])
    assert S["lsmb_lset_table_order"] == (c.c_int, [vp, lsmbloom.u32p, lsmbloom.u64p])
    assert S["lsmb_lset_lists_work_bytes"] == (c.c_uint64, [vp, c.c_uint64])
    assert S["lsmb_lset_probe_lists_dev"] == (
        c.c_int, [vp, vp, vp, c.c_uint32, c.c_uint64, vp, vp, c.c_uint64, vp, c.c_uint64, vp])
    assert S["lsmb_lset_probe_lists"] == (
        c.c_int, [vp, lsmbloom.u8p, lsmbloom.u64p, c.c_uint32, c.c_uint64, lsmbloom.u64p, lsmbloom.u32p, c.c_uint64])
    for name in ("lsmb_lset_total_tables", "lsmb_lset_table_order", "lsmb_lset_lists_work_bytes",
                 "lsmb_lset_probe_lists_dev", "lsmb_lset_probe_lists"):
        assert hasattr(lsmbloom.lib(), name)
    for name in ("table_order", "lists_work_bytes", "probe_lists", "probe_lists_keys", "probe_lists_dev"):
        assert callable(getattr(LevelSet, name))


def test_lists_from_ids_on_a_hand_written_example():
    # two rows; table ids 50, 40 (row 0) and 90 (row 1) are ordinals 0, 1, 2
    ids = np.array([[40, 50, NONE, 40], [NONE, 90, 90, NONE]], dtype=np.uint32)
    starts, index = lists_from_ids(ids, [50, 40, 90])
    assert starts.tolist() == [0, 1, 3, 5] and index.tolist() == [1, 0, 3, 1, 2]
    assert starts.dtype == np.uint64 and index.dtype == np.uint32
    s0, i0 = lists_from_ids(np.zeros((0, 5), np.uint32), [])
    assert s0.tolist() == [0] and i0.size == 0


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan_ubsan"])
def test_lset_lists_plan_and_reference_host(tmp_path, flags):
    """The pass count, the workspace layout and lset_lists_ref
    (csrc/lset_lists_plan.hpp) by tests/cpp/lset_lists_plan_test.cpp: a
    stand-alone host program, once plain and once under ASan and UBSan."""
    exe = str(tmp_path / "lset_lists_plan_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, PLAN_SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout


def test_cpp_mirror_level_set_lists_argument_checks():
    r = subprocess.run([cpp_bin("lset_lists_test")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


# ------------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def ctx():
    c = lsmbloom.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def quantile_set(ctx, oracle):
    """Two rows of 4 and 3 tables over 16-byte keys (quantile ranges of 4000
    keys each), 70 001 query keys (members of either row and absent keys,
    shuffled) and probe()'s answers for them, computed once."""
    rows = []
    for r, (seed, cuts) in enumerate([(0x5EED0700, 4), (0x5EED0701, 3)]):
        srt = sorted(bytes(x) for x in keygen.key16(seed, 0, 4000))
        tabs = []
        for c in range(cuts):
            part = srt[c * len(srt) // cuts:(c + 1) * len(srt) // cuts]
            tabs.append(build_table(oracle, 100 * r + c + 1, part, (len(part), 0.01)))
        rows.append(tabs)
    ls = LevelSet(ctx)
    for r, tabs in enumerate(rows):
        add_tables(ls, oracle, r, tabs[::-1])
    ls.seal()
    q = np.concatenate([keygen.key16(0x5EED0700, 0, 4000), keygen.key16(0x5EED0701, 0, 4000),
                        keygen.key16(0x5EED0702, 0, 62001)])
    q = np.ascontiguousarray(q[np.random.default_rng(31).permutation(len(q))])
    assert q.shape == (70001, 16)
    ids = ls.probe(q, key_len=16)
    assert (ids != NONE).sum() > 8000 and (ids == NONE).sum() > 8000
    yield ls, q, ids
    ls.close()


@pytest.mark.gpu
def test_lset_lists_three_rows_match_the_oracle_and_the_probe(ctx, oracle):
    rng = np.random.default_rng(41)
    rows, members = [], []
    for r, ntab in enumerate((3, 40, 300)):
        tabs = []
        for t in range(ntab):
            base = 40 * r + 150 * t  # 100 ids wide, then a gap of 50
            ids = np.sort(rng.choice(100, size=40, replace=False)) + base
            keys = [b"user%08d" % i for i in ids]
            tabs.append(build_table(oracle, 1000 * r + t + 7, keys, (1000, 0.01)))
            members += keys[::3]
        rows.append(tabs)
    ls = LevelSet(ctx)
    flat = [(r, t) for r, tabs in enumerate(rows) for t in range(len(tabs))]
    for j in rng.permutation(len(flat)):
        r, t = flat[j]
        add_tables(ls, oracle, r, [rows[r][t]])
    ls.seal()
    assert ls.total_tables() == 343
    order_ids, base = ls.table_order()
    assert base.tolist() == [0, 3, 43, 343] and base.dtype == np.uint64 and order_ids.dtype == np.uint32
    # the sealed order is ascending min_key: the order the tables were made in
    assert order_ids.tolist() == [t[0] for tabs in rows for t in tabs]
    outside = [b"zzz%05d" % i for i in range(300)] + [b"", b"user", b"\xff" * 40] + [b"a" * (1 + i % 50) for i in range(200)]
    inside = [b"user%08d" % i for i in rng.integers(0, 150 * 300 + 500, 20_011 - len(members) - len(outside))]
    q = members + inside + outside
    q = [q[j] for j in rng.permutation(len(q))]
    assert len(q) == 20_011
    got = ls.probe_lists_keys(q)
    exp_ids = expected_ids(oracle, rows, q)                       # the oracle, directly
    check_lists(got, lists_from_ids(exp_ids, order_ids), "oracle")
    check_lists(got, lists_from_ids(ls.probe_keys(q), order_ids), "probe")
    starts, index = got
    assert starts.shape == (344,) and starts[0] == 0 and int(starts[-1]) == index.size >= len(members)
    # a capacity below the total: the first entries only, the same starts
    s2, i2 = ls.probe_lists(*_packed(q), cap=1000)
    assert np.array_equal(s2, starts) and np.array_equal(i2, index[:1000])
    ls.close()


def _packed(keys):
    data, offs = keygen.pack(keys)
    return data, offs


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025, 2047, 2048, 2049, 70001])
def test_lset_lists_batch_sizes_with_device_keys(quantile_set, n):
    """The wave (64), chunk and tile (2048 elements) edges, more than one tile,
    and a tile that straddles nothing: every row is padded to whole tiles."""
    import torch

    ls, q, ids = quantile_set
    dq = torch.from_numpy(q[:n]).to("cuda:0")
    exp = lists_from_ids(ids[:, :n], ls.table_order()[0])
    check_lists(dev_lists(ls, dq, n), exp, n)
    if n in (65, 2049):  # the host entry point and the any-length key source agree
        check_lists(ls.probe_lists(q[:n], key_len=16), exp, n)
        q7 = np.ascontiguousarray(q[:n, :7])
        check_lists(ls.probe_lists(q7, key_len=7), lists_from_ids(ls.probe(q7, key_len=7), ls.table_order()[0]), n)


def _range_set(ctx, total, nrows, rng):
    """`total` always-maybe tables in `nrows` rows: table t owns the keys
    b't%07d0' .. b't%07d5', row r the tables [total * r // nrows, total * (r + 1)
    // nrows); ids are a permutation, tables are added in shuffled order."""
    ls = LevelSet(ctx)
    ids = rng.permutation(total).astype(np.uint32) + 10
    f = always_maybe()
    t0 = time.perf_counter()
    for t in rng.permutation(total):
        r = next(r for r in range(nrows) if t < total * (r + 1) // nrows)
        ls.add_filter(r, int(ids[t]), f, b"t%07d0" % t, b"t%07d5" % t)
    add_s = time.perf_counter() - t0
    ls.seal()
    return ls, ids, add_s


@pytest.mark.gpu
@pytest.mark.parametrize("total,nrows", [(1, 1), (255, 2), (256, 1), (257, 2), (5000, 3), (65537, 2)])
def test_lset_lists_pass_count_edges(ctx, total, nrows):
    """One, two and three radix passes (256 / 65 536 tables are the edges).
    Adding the 65 537 tables of the three-pass case is the slow part."""
    rng = np.random.default_rng(1000 + total)
    ls, ids, add_s = _range_set(ctx, total, nrows, rng)
    print("adding %d tables took %.2f s" % (total, add_s))
    assert ls.total_tables() == total and ls.rows() == nrows
    order_ids, base = ls.table_order()
    assert np.array_equal(order_ids, ids)  # sealed order = ascending t within a row, rows back to back
    assert base.tolist() == [total * r // nrows for r in range(nrows + 1)]
    n = 50_000
    tq = rng.integers(0, total + 2, n)
    tq[:min(total, n)] = rng.permutation(total)[:n]            # every table (that fits) is asked for
    dq = rng.integers(0, 10, n)                                # last digits 6-9 are outside the range
    keys = [b"t%07d%d" % (t, d) for t, d in zip(tq, dq)]
    # expectation: a bisect over the ranges
    los = [b"t%07d0" % t for t in range(total)]
    exp_ord = np.full((nrows, n), NONE, dtype=np.uint32)
    for i, key in enumerate(keys):
        j = bisect.bisect_right(los, key) - 1
        if j >= 0 and key <= b"t%07d5" % j:
            exp_ord[next(r for r in range(nrows) if j < total * (r + 1) // nrows), i] = j
    exp = lists_from_ordinals(exp_ord, total)
    # (a third of the keys or more name a table there is, 6 of 10 last digits lie inside: 0.2 n or more expected)
    assert n // 6 < int(exp[0][-1]) < n
    got = ls.probe_lists_keys(keys)
    check_lists(got, exp, total)
    check_lists(got, lists_from_ids(ls.probe_keys(keys), order_ids), total)
    ls.close()


@pytest.fixture(scope="module")
def gap_set(ctx):
    """Rows 0 and 2 used, row 1 empty.  Row 0: 'b'..'d', 'f'..'h', 'k'..'m';
    row 2: 'a'..'g' and 'l'..'z' (so a key can be listed by both rows)."""
    ls = LevelSet(ctx)
    f = always_maybe()
    for tid, lo, hi in ((13, b"k", b"m"), (11, b"b", b"d"), (12, b"f", b"h")):
        ls.add_filter(0, tid, f, lo, hi)
    for tid, lo, hi in ((32, b"l", b"z"), (31, b"a", b"g")):
        ls.add_filter(2, tid, f, lo, hi)
    ls.seal()
    yield ls
    ls.close()


@pytest.mark.gpu
def test_lset_lists_skew_and_an_empty_row(gap_set):
    ls = gap_set
    assert ls.rows() == 3 and ls.total_tables() == 5
    order_ids, base = ls.table_order()
    assert order_ids.tolist() == [11, 12, 13, 31, 32] and base.tolist() == [0, 3, 3, 5]
    n = 5000
    # every key in one table: 'f' <= 'g00000' <= 'h' in row 0, and past 'a'..'g' in row 2
    keys = [b"g%05d" % i for i in range(n)]
    starts, index = ls.probe_lists_keys(keys)
    assert starts.tolist() == [0, 0, n, n, n, n] and np.array_equal(index, np.arange(n, dtype=np.uint32))
    # no key anywhere: below every range, between ranges ('h' < 'h00000' < 'k'), above
    for keys in ([b"A%05d" % i for i in range(n)] + [b"", b"i", b"j", b"zz"], [b"h%05d" % i for i in range(n)]):
        starts, index = ls.probe_lists_keys(keys)
        assert starts.tolist() == [0] * 6 and index.size == 0
    # n copies of one key, listed by a table of row 0 and one of row 2
    keys = [b"c"] * n
    starts, index = ls.probe_lists_keys(keys)
    assert starts.tolist() == [0, n, n, n, 2 * n, 2 * n]
    assert np.array_equal(index, np.tile(np.arange(n, dtype=np.uint32), 2))
    # a mix, against the probe: rows 0 and 2 answer, row 1 never does
    rng = np.random.default_rng(43)
    keys = [bytes([97 + int(a)]) + b"%d" % b for a, b in zip(rng.integers(0, 26, n), rng.integers(0, 3, n))]
    keys += [b"b", b"d", b"m", b"a", b"g", b"l", b"z", b"e", b"i"]
    ids = ls.probe_keys(keys)
    assert (ids[1] == NONE).all() and (ids[0] != NONE).any() and (ids[2] != NONE).any()
    assert ((ids[0] != NONE) & (ids[2] != NONE)).any()
    check_lists(ls.probe_lists_keys(keys), lists_from_ids(ids, order_ids), "mix")


@pytest.mark.gpu
def test_lset_lists_capacity(quantile_set):
    import torch

    ls, q, ids = quantile_set
    n = 5000
    dq = torch.from_numpy(q[:n]).to("cuda:0")
    es, ei = lists_from_ids(ids[:, :n], ls.table_order()[0])
    total = ei.size
    assert 100 < total < 2 * n
    for cap in (total, total - 1, 1, total + 7):
        starts, index = dev_lists(ls, dq, n, cap=cap)
        assert np.array_equal(starts, es), cap
        w = min(total, cap)
        assert index.shape == (cap,) and np.array_equal(index[:w], ei[:w]), cap
        assert (index[w:] == POISON).all(), cap  # nothing past min(total, cap) is touched
    # cap = 0 with a null index: a counting call
    G = ls.total_tables()
    starts = torch.full((G + 1,), -1, dtype=torch.int64, device="cuda:0")
    work = torch.empty(ls.lists_work_bytes(n), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ls.probe_lists_dev(dq, n, starts, None, work, key_len=16)
    torch.cuda.synchronize()
    assert np.array_equal(starts.cpu().numpy().view(np.uint64), es)
    # the host form: a counting call, then the first entries only
    s2, i2 = ls.probe_lists(q[:n], key_len=16, cap=0)
    assert np.array_equal(s2, es) and i2.size == 0
    s2, i2 = ls.probe_lists(q[:n], key_len=16, cap=total - 1)
    assert np.array_equal(s2, es) and np.array_equal(i2, ei[:total - 1])
    # a capacity with a null index is refused
    L = lsmbloom.lib()
    assert L.lsmb_lset_probe_lists_dev(ls.h, vp(dq.data_ptr()), None, 16, n, vp(starts.data_ptr()), None, 5,
                                       vp(work.data_ptr()), work.numel(), None) == lsmbloom.LSMB_EINVAL


@pytest.mark.gpu
def test_lset_lists_contract(ctx, quantile_set):
    import torch

    ls, q, ids = quantile_set
    L = lsmbloom.lib()
    dev = "cuda:0"
    G = ls.total_tables()
    assert G == 7
    n = 3000
    dq = torch.from_numpy(q[:n]).to(dev)
    exp = lists_from_ids(ids[:, :n], ls.table_order()[0])
    need = ls.lists_work_bytes(n)
    assert need > 0 and ls.lists_work_bytes(0) == 0 and ls.lists_work_bytes(1 << 32) == 0
    assert ls.lists_work_bytes(2 * n) > need
    # n == 0 writes G + 1 zero starts and nothing else, workspace or not
    starts = torch.full((G + 1,), -1, dtype=torch.int64, device=dev)
    index = torch.full((8,), POISON - (1 << 32), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ls.probe_lists_dev(dq, 0, starts, index, None, key_len=16)
    torch.cuda.synchronize()
    assert (starts.cpu().numpy() == 0).all() and (index.cpu().numpy().view(np.uint32) == POISON).all()
    s0, i0 = ls.probe_lists_keys([])
    assert s0.tolist() == [0] * (G + 1) and i0.size == 0
    # a workspace one byte short, a null one, n > 2^32-1: LSMB_EINVAL, outputs untouched
    starts.fill_(-1)
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    args = (ls.h, vp(dq.data_ptr()), None, 16, n, vp(starts.data_ptr()), vp(index.data_ptr()), 8)
    assert L.lsmb_lset_probe_lists_dev(*args, vp(work.data_ptr()), need - 1, None) == lsmbloom.LSMB_EINVAL
    assert L.lsmb_lset_probe_lists_dev(*args, None, need, None) == lsmbloom.LSMB_EINVAL
    assert L.lsmb_lset_probe_lists_dev(ls.h, vp(dq.data_ptr()), None, 16, 1 << 32, vp(starts.data_ptr()),
                                       vp(index.data_ptr()), 8, vp(work.data_ptr()), need, None) == lsmbloom.LSMB_EINVAL
    with pytest.raises(ValueError):
        ls.probe_lists_dev(dq, n, starts, index, work[:need - 1], key_len=16)
    torch.cuda.synchronize()
    assert (starts.cpu().numpy() == -1).all() and (index.cpu().numpy().view(np.uint32) == POISON).all()
    # two lists probes on two streams with two workspaces, issued back to back
    st = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    ns = (3000, 2500)
    outs = []
    for j in range(2):
        cap = int(lists_from_ids(ids[:, :ns[j]], ls.table_order()[0])[1].size)
        outs.append((torch.full((G + 1,), -1, dtype=torch.int64, device=dev),
                     torch.full((cap,), POISON - (1 << 32), dtype=torch.int32, device=dev),
                     torch.empty(ls.lists_work_bytes(ns[j]), dtype=torch.uint8, device=dev)))
    torch.cuda.synchronize()
    for j in range(2):
        ls.probe_lists_dev(dq, ns[j], outs[j][0], outs[j][1], outs[j][2], key_len=16, stream=st[j].cuda_stream)
    for s in st:
        s.synchronize()
    for j in range(2):
        got = (outs[j][0].cpu().numpy().view(np.uint64), outs[j][1].cpu().numpy().view(np.uint32))
        check_lists(got, lists_from_ids(ids[:, :ns[j]], ls.table_order()[0]), "stream %d" % j)
    # two consecutive runs are byte-identical
    a = dev_lists(ls, dq, n)
    b = dev_lists(ls, dq, n)
    check_lists(a, exp, "run 1")
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    # before seal: every lists entry point refuses (or answers 0)
    un = LevelSet(ctx)
    un.add_filter(0, 1, always_maybe(), b"a", b"b")
    assert un.total_tables() == 0 and un.lists_work_bytes(100) == 0
    with pytest.raises(ValueError):
        un.table_order()
    with pytest.raises(ValueError):
        un.probe_lists_keys([b"a"])
    starts.fill_(-1)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        un.probe_lists_dev(dq, n, starts, index, work, key_len=16)
    torch.cuda.synchronize()
    assert (starts.cpu().numpy() == -1).all()
    un.close()
    # a sealed, empty set: one zero start, no workspace needed
    em = LevelSet(ctx)
    em.seal()
    assert em.total_tables() == 0 and em.lists_work_bytes(100) == 0
    ids0, base0 = em.table_order()
    assert ids0.size == 0 and base0.tolist() == [0]
    s, i = em.probe_lists_keys([b"a", b"b"])
    assert s.tolist() == [0] and i.size == 0
    one = torch.full((1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    em.probe_lists_dev(dq, n, one, None, None, key_len=16)
    torch.cuda.synchronize()
    assert one.cpu().numpy().tolist() == [0]
    em.close()


@pytest.mark.gpu
def test_cpp_mirror_level_set_lists_gpu():
    r = subprocess.run([cpp_bin("lset_lists_test"), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout
