"""The walk probe of a level set (lsmb_lset_probe_walk*): per key, the first
walk step at or after its resume step at which a table passes the
range-and-bloom check, in DB::get's order — L0 newest first, then one table
per row — and that table's Version ordinal; and the same answer as per-table
lists, at most one entry per key.

The expectation is a numpy reduction (walk_support.walk_from) of the Version's
full answer: the CPU oracle's mask and row ids (lset_support.reference), a
bisect over always-maybe ranges, or — only where the keys are not that
workload's: past one resident grid, where the oracle in Python would take
minutes, and for 7-byte keys — the set's own probe_version, which
test_lset_version.py holds against the oracle.  It is never taken from the walk
entry points themselves.  Every comparison covers all n keys.
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
from lset_support import (POISON, add_tables, always_maybe, build_table, check_lists, cpp_bin, dev_walk, dev_walk_lists,
                          expected_ids, expected_mask, l0_tables, low_bits, queries, reference, row_tables)
from walk_support import lists_from_ord, ordinals_of, walk_from

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "lset_walk_plan_test.cpp")
NONE = lsmbloom.LSMB_LSET_NONE
L0 = lsmbloom.LSMB_LSET_ROW_L0
EINVAL = lsmbloom.LSMB_EINVAL
vp = ctypes.c_void_p
WALK_C = ("lsmb_lset_walk_steps", "lsmb_lset_probe_walk_dev", "lsmb_lset_probe_walk",
          "lsmb_lset_walk_lists_work_bytes", "lsmb_lset_probe_walk_lists_dev", "lsmb_lset_probe_walk_lists")


# ---------------------------------------------------------------- without a GPU

def test_walk_from_on_a_hand_written_example():
    # T0 = 2: step 0 looks at position 1, step 1 at position 0; one row of two tables is step 2
    mask = np.array([1, 3, 2, 0], dtype=np.uint64)
    row_ord = ordinals_of(np.array([[40, NONE, 50, NONE]], dtype=np.uint32), [50, 40])
    assert row_ord.tolist() == [[1, NONE, 0, NONE]]
    step, ordv = walk_from(mask, row_ord, 2)
    assert step.tolist() == [1, 0, 0, NONE] and ordv.tolist() == [0, 1, 1, NONE]
    assert step.dtype == np.uint32 and ordv.dtype == np.uint32
    step, ordv = walk_from(mask, row_ord, 2, [2, 1, 1, 0])  # resumed one step past each answer (key 0: two)
    assert step.tolist() == [2, 1, 2, NONE] and ordv.tolist() == [3, 0, 2, NONE]
    starts, index = lists_from_ord(ordv, 4)
    assert starts.tolist() == [0, 1, 1, 2, 3] and index.tolist() == [1, 2, 0]
    assert starts.dtype == np.uint64 and index.dtype == np.uint32
    step, ordv = walk_from(mask, row_ord, 2, [3, NONE, 2, 7])  # at and past W = 3: retired
    assert step.tolist() == [NONE, NONE, 2, NONE] and ordv.tolist() == [NONE, NONE, 2, NONE]
    # no L0 table: the rows alone; no row: L0 alone; neither: nothing
    step, ordv = walk_from(np.zeros(4, np.uint64), row_ord, 0)
    assert step.tolist() == [0, NONE, 0, NONE] and ordv.tolist() == [1, NONE, 0, NONE]
    step, ordv = walk_from(mask, np.zeros((0, 4), np.uint32), 2, [0, 1, 1, 0])
    assert step.tolist() == [1, 1, NONE, NONE] and ordv.tolist() == [0, 0, NONE, NONE]
    step, ordv = walk_from(mask, np.zeros((0, 4), np.uint32), 0)
    assert (step == NONE).all() and (ordv == NONE).all()
    s, i = lists_from_ord(ordv, 0)
    assert s.tolist() == [0] and i.size == 0
    # all 64 positions: position 63 is step 0
    step, ordv = walk_from(np.array([1 << 63 | 1, 1], np.uint64), np.zeros((0, 2), np.uint32), 64, [1, 0])
    assert step.tolist() == [63, 63] and ordv.tolist() == [0, 0]


def test_walk_entry_points_are_in_the_signature_table():
    c = ctypes
    S = lsmbloom.SIGNATURES
    u8p, u32p, u64p = lsmbloom.u8p, lsmbloom.u32p, lsmbloom.u64p
    assert S["lsmb_lset_walk_steps"] == (c.c_uint32, [vp])
    assert S["lsmb_lset_probe_walk_dev"] == (c.c_int, [vp, vp, vp, c.c_uint32, c.c_uint64, vp, vp, vp, vp])
    assert S["lsmb_lset_probe_walk"] == (c.c_int, [vp, u8p, u64p, c.c_uint32, c.c_uint64, u32p, u32p, u32p])
    assert S["lsmb_lset_walk_lists_work_bytes"] == (c.c_uint64, [vp, c.c_uint64])
    assert S["lsmb_lset_probe_walk_lists_dev"] == (
        c.c_int, [vp, vp, vp, c.c_uint32, c.c_uint64, vp, vp, vp, vp, c.c_uint64, vp, c.c_uint64, vp])
    assert S["lsmb_lset_probe_walk_lists"] == (
        c.c_int, [vp, u8p, u64p, c.c_uint32, c.c_uint64, u32p, u32p, u64p, u32p, c.c_uint64])
    for name in WALK_C:
        assert hasattr(lsmbloom.lib(), name)
    for name in ("walk_steps", "probe_walk", "probe_walk_keys", "probe_walk_dev", "walk_lists_work_bytes",
                 "probe_walk_lists", "probe_walk_lists_keys", "probe_walk_lists_dev"):
        assert callable(getattr(LevelSet, name))
    assert lsmbloom.lib().lsmb_abi_version() == 6  # symbols were added, nothing changed


def test_walk_entry_points_reject_a_null_set_and_null_outputs():
    L = lsmbloom.lib()
    u8p, u32p, u64p = lsmbloom.u8p, lsmbloom.u32p, lsmbloom.u64p
    frm = np.full(4, 1, np.uint32)
    step = np.full(4, 5, np.uint32)
    ordv = np.full(4, 6, np.uint32)
    starts = np.full(4, 7, np.uint64)
    index = np.full(4, 9, np.uint32)
    data = np.zeros(16, np.uint8)
    p8, pf, pt, po = data.ctypes.data_as(u8p), frm.ctypes.data_as(u32p), step.ctypes.data_as(u32p), ordv.ctypes.data_as(u32p)
    ps, pi = starts.ctypes.data_as(u64p), index.ctypes.data_as(u32p)
    assert L.lsmb_lset_walk_steps(None) == 0
    assert L.lsmb_lset_walk_lists_work_bytes(None, 1000) == 0
    assert L.lsmb_lset_probe_walk(None, p8, None, 4, 4, pf, pt, po) == EINVAL
    assert L.lsmb_lset_probe_walk(None, p8, None, 4, 4, None, None, None) == EINVAL
    assert L.lsmb_lset_probe_walk_dev(None, vp(1), None, 4, 4, vp(1), vp(1), vp(1), None) == EINVAL
    assert L.lsmb_lset_probe_walk_dev(None, vp(1), None, 4, 4, None, None, None, None) == EINVAL
    assert L.lsmb_lset_probe_walk_lists(None, p8, None, 4, 4, pf, pt, ps, pi, 4) == EINVAL
    assert L.lsmb_lset_probe_walk_lists(None, p8, None, 4, 4, None, None, None, None, 0) == EINVAL
    assert L.lsmb_lset_probe_walk_lists_dev(None, vp(1), None, 4, 4, vp(1), vp(1), vp(1), vp(1), 4, vp(16), 1 << 20,
                                            None) == EINVAL
    assert L.lsmb_lset_probe_walk_lists_dev(None, vp(1), None, 4, 4, None, None, None, None, 0, vp(16), 1 << 20,
                                            None) == EINVAL
    assert b"null level set" in L.lsmb_last_error()
    assert (frm == 1).all() and (step == 5).all() and (ordv == 6).all() and (starts == 7).all() and (index == 9).all()


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan_ubsan"])
def test_lset_walk_plan_and_reference_host(tmp_path, flags):
    """The step mapping, the allowed-positions mask at the 64-bit edge, the
    workspace and lset_walk_ref (csrc/lset_walk_plan.hpp) by
    tests/cpp/lset_walk_plan_test.cpp: a stand-alone host program, once plain
    and once under ASan and UBSan."""
    exe = str(tmp_path / "lset_walk_plan_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, PLAN_SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout


def test_cpp_mirror_walk_argument_checks():
    r = subprocess.run([cpp_bin("lset_walk_test")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


# ------------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def ctx():
    c = lsmbloom.Context(0)
    yield c
    c.close()


def version_set(ctx, oracle, geom, t0, rows=None):
    """The parity workload's first t0 L0 tables (positions 0 .. t0-1) among the
    rows' tables (65 / 5 / 3 unless given), one batch, sealed."""
    tabs, _ = l0_tables(geom)
    rows = row_tables() if rows is None else rows
    placed = [(r, t) for r, row in enumerate(rows) for t in row]
    for j, t in enumerate(tabs[:t0]):
        placed.insert(min(2 * j, len(placed)), (L0, t))
    ls = LevelSet(ctx)
    ls.add_many([r for r, _ in placed], [t[0] for _, t in placed],
                [oracle.serialize(t[1], t[2], t[3]) for _, t in placed], [(t[4], t[5]) for _, t in placed])
    ls.seal()
    assert ls.l0_tables() == t0 and ls.rows() == len(rows)
    return ls


def host_walk(ls, kind, q, resume=None):
    if kind == "var":
        return ls.probe_walk_keys(q, resume=resume)
    data = np.frombuffer(b"".join(q), dtype=np.uint8)
    return ls.probe_walk(data, key_len=16 if kind == "fixed16" else 12, resume=resume)


def host_walk_lists(ls, kind, q, resume=None):
    if kind == "var":
        return ls.probe_walk_lists_keys(q, resume=resume)
    data = np.frombuffer(b"".join(q), dtype=np.uint8)
    return ls.probe_walk_lists(data, key_len=16 if kind == "fixed16" else 12, resume=resume)


def check_walk(got, exp, what=""):
    (step, ordv), (es, eo) = got, exp
    assert step.dtype == np.uint32 and ordv.dtype == np.uint32, what
    assert step.shape == es.shape and np.array_equal(step, es), (what, np.argwhere(step != es)[:10].tolist())
    assert ordv.shape == eo.shape and np.array_equal(ordv, eo), (what, np.argwhere(ordv != eo)[:10].tolist())


def random_resume(rng, n, W):
    """Resume steps over [0, W + 2] with LSMB_LSET_NONE mixed in."""
    resume = rng.integers(0, W + 3, n).astype(np.uint32)
    resume[rng.random(n) < 0.1] = NONE
    return resume


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["sst", "mixed"])
@pytest.mark.parametrize("t0", [0, 1, 8, 33, 64])
def test_walk_matches_the_oracle(ctx, oracle, t0, geom):
    ls = version_set(ctx, oracle, geom, t0)
    W = t0 + 3
    assert ls.walk_steps() == W
    order_ids = ls.table_order()[0]
    rng = np.random.default_rng(100 * t0 + len(geom))
    for kind in ("fixed16", "fixed12", "var"):
        q = queries(kind)
        n = len(q)
        mask, ids = reference(geom, kind)
        mask, row_ord = low_bits(mask, t0) if t0 else np.zeros(n, np.uint64), ordinals_of(ids, order_ids)
        first = walk_from(mask, row_ord, t0)
        check_walk(host_walk(ls, kind, q), first, ("from NULL", kind))
        # the workload has answers at every kind of step: in L0 (t0 > 0), in the rows, nowhere
        assert t0 == 0 or (first[0] < t0).sum() > 30
        # (behind all 64 L0 tables no key gets as far as a row from step 0; the resumed walks below do)
        assert t0 == 64 or (first[0] >= t0).sum() - (first[0] == NONE).sum() > 50
        assert (first[0] == NONE).sum() > 50
        resume = random_resume(rng, n, W)
        exp = walk_from(mask, row_ord, t0, resume)
        assert ((exp[0] != NONE) & (exp[0] > resume)).sum() > 100  # some keys skip steps without a candidate
        check_walk(host_walk(ls, kind, q, resume), exp, ("random from", kind))
        for c in sorted({max(t0, 1) - 1, t0, W - 1}):
            resume = np.full(n, c, np.uint32)
            check_walk(host_walk(ls, kind, q, resume), walk_from(mask, row_ord, t0, resume), ("from", c, kind))
    ls.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fixed16", "var"])
def test_walk_rounds_visit_every_candidate_once(ctx, oracle, kind):
    """The multi-get loop with every candidate treated as a false positive:
    from = step + 1 until every step is NONE.  The rounds' lists together are
    probe_version_lists' lists, every candidate exactly once."""
    t0 = 33
    ls = version_set(ctx, oracle, "mixed", t0)
    W, V = ls.walk_steps(), ls.version_tables()
    q = queries(kind)
    n = len(q)
    mask, ids = reference("mixed", kind)
    mask, row_ord = low_bits(mask, t0), ordinals_of(ids, ls.table_order()[0])
    resume = np.zeros(n, np.uint32)
    last = np.full(n, -1, np.int64)
    seen = [[] for _ in range(V)]
    rounds = 0
    while True:
        starts, index, step = host_walk_lists(ls, kind, q, resume)
        rounds += 1
        assert rounds <= W + 1
        es, eo = walk_from(mask, row_ord, t0, resume)
        assert np.array_equal(step, es), rounds
        check_lists((starts, index), lists_from_ord(eo, V), rounds)
        live = step != NONE
        if not live.any():
            assert index.size == 0
            break
        assert (step[live].astype(np.int64) > last[live]).all()  # strictly ascending per key
        last[live] = step[live]
        for v in np.nonzero(np.diff(starts.astype(np.int64)))[0]:
            seen[v].append(index[int(starts[v]):int(starts[v + 1])])
        resume = np.where(live, step.astype(np.int64) + 1, NONE).astype(np.uint32)
    assert rounds > 4
    if kind == "var":
        full = ls.probe_version_lists_keys(q)
    else:
        full = ls.probe_version_lists(np.frombuffer(b"".join(q), dtype=np.uint8), key_len=16)
    assert int(full[0][V]) > n  # overwritten keys: more candidates than keys
    for v in range(V):
        got = np.sort(np.concatenate(seen[v])) if seen[v] else np.zeros(0, np.uint32)
        assert np.array_equal(got, full[1][int(full[0][v]):int(full[0][v + 1])]), v
    ls.close()


@pytest.fixture(scope="module")
def parity_set(ctx, oracle):
    """T0 = 8 mixed L0 tables and the three rows, the 5 000 16-byte queries on
    the host and the device, and the oracle's answer reduced for a NULL and a
    random resume array, computed once."""
    import torch

    t0 = 8
    ls = version_set(ctx, oracle, "mixed", t0)
    q = np.frombuffer(b"".join(queries("fixed16")), dtype=np.uint8).reshape(-1, 16).copy()
    mask, ids = reference("mixed", "fixed16")
    mask, row_ord = low_bits(mask, t0), ordinals_of(ids, ls.table_order()[0])
    resume = random_resume(np.random.default_rng(77), len(q), ls.walk_steps())
    for a in (mask, row_ord, resume, q):
        a.setflags(write=False)
    yield ls, q, torch.from_numpy(q.copy()).to("cuda:0"), mask, row_ord, resume
    ls.close()


@pytest.mark.gpu
def test_walk_lists_form(parity_set):
    import torch

    ls, q, dq, mask, row_ord, resume = parity_set
    dev = "cuda:0"
    n, t0, V = len(q), ls.l0_tables(), ls.version_tables()
    for res in (None, resume):
        es, eo = walk_from(mask, row_ord, t0, res)
        exp = lists_from_ord(eo, V)
        total = int(exp[0][V])
        assert 1000 < total <= n and (np.diff(exp[0].astype(np.int64)) > 0).sum() > 10
        starts, index, step = dev_walk_lists(ls, dq, n, resume=res)
        check_lists((starts, index), exp, "device")
        assert np.array_equal(step, es)
        starts, index, step = dev_walk_lists(ls, dq, n, resume=res, want_step=False)  # d_step is optional
        check_lists((starts, index), exp, "no step")
        hs, hi, hstep = ls.probe_walk_lists(q, key_len=16, resume=res)
        check_lists((hs, hi), exp, "host")
        assert np.array_equal(hstep, es)
        # the transposition of the per-key form's own ord, too
        pstep, pord = dev_walk(ls, dq, n, resume=res)
        assert np.array_equal(pstep, es) and np.array_equal(pord, eo)
        # a counting call, then capacities below, at and above the total
        counted, _, cstep = dev_walk_lists(ls, dq, n, cap=0, resume=res)
        assert np.array_equal(counted, exp[0]) and np.array_equal(cstep, es)
        for cap in (1, total - 1, total, total + 7):
            starts, index, _ = dev_walk_lists(ls, dq, n, cap=cap, resume=res)
            w = min(total, cap)
            assert np.array_equal(starts, exp[0]), cap
            assert index.shape == (cap,) and np.array_equal(index[:w], exp[1][:w]), cap
            assert (index[w:] == POISON).all(), cap  # nothing past min(total, cap) is touched
        hs, hi, _ = ls.probe_walk_lists(q, key_len=16, cap=total - 5, resume=res)
        assert np.array_equal(hs, exp[0]) and np.array_equal(hi, exp[1][:total - 5])
        # two consecutive runs are byte-identical
        a = dev_walk_lists(ls, dq, n, resume=res)
        b = dev_walk_lists(ls, dq, n, resume=res)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # two probes on two streams with their own workspaces, issued back to back
    st = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    ns = (5000, 3777)
    exps = [walk_from(mask[:m], row_ord[:, :m], t0, resume[:m]) for m in ns]
    d_res = torch.from_numpy(resume.view(np.int32).copy()).to(dev)
    outs = []
    for j in range(2):
        outs.append((torch.full((V + 1,), -1, dtype=torch.int64, device=dev),
                     torch.full((ns[j],), POISON - (1 << 32), dtype=torch.int32, device=dev),
                     torch.empty(ls.walk_lists_work_bytes(ns[j]), dtype=torch.uint8, device=dev),
                     torch.full((ns[j],), POISON - (1 << 32), dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()
    for j in range(2):
        ls.probe_walk_lists_dev(dq, ns[j], outs[j][0], outs[j][1], outs[j][2], step=outs[j][3], resume=d_res,
                                key_len=16, stream=st[j].cuda_stream)
    for s in st:
        s.synchronize()
    for j in range(2):
        es, ei = lists_from_ord(exps[j][1], V)
        got = (outs[j][0].cpu().numpy().view(np.uint64), outs[j][1].cpu().numpy().view(np.uint32)[:ei.size])
        check_lists(got, (es, ei), "stream %d" % j)
        assert np.array_equal(outs[j][3].cpu().numpy().view(np.uint32), exps[j][0])


@pytest.mark.gpu
def test_walk_in_place(parity_set):
    """d_step aliasing d_from: the same answers as with separate buffers."""
    import torch

    ls, q, dq, mask, row_ord, resume = parity_set
    n, t0, V = len(q), ls.l0_tables(), ls.version_tables()
    es, eo = walk_from(mask, row_ord, t0, resume)
    sep = dev_walk(ls, dq, n, resume=resume)
    inp = dev_walk(ls, dq, n, resume=resume, in_place=True)
    check_walk(sep, (es, eo), "separate")
    check_walk(inp, (es, eo), "in place")
    # the lists form, and the host forms with one array for both
    d_fs = torch.from_numpy(resume.view(np.int32).copy()).to("cuda:0")
    starts = torch.full((V + 1,), -1, dtype=torch.int64, device="cuda:0")
    index = torch.full((n,), POISON - (1 << 32), dtype=torch.int32, device="cuda:0")
    work = torch.empty(ls.walk_lists_work_bytes(n), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ls.probe_walk_lists_dev(dq, n, starts, index, work, step=d_fs, resume=d_fs, key_len=16)
    torch.cuda.synchronize()
    assert np.array_equal(d_fs.cpu().numpy().view(np.uint32), es)
    exp = lists_from_ord(eo, V)
    check_lists((starts.cpu().numpy().view(np.uint64), index.cpu().numpy().view(np.uint32)[:exp[1].size]), exp, "lists")
    L = lsmbloom.lib()
    fs, ordv = resume.copy(), np.empty(n, np.uint32)
    pfs = fs.ctypes.data_as(lsmbloom.u32p)
    assert L.lsmb_lset_probe_walk(ls.h, q.ctypes.data_as(lsmbloom.u8p), None, 16, n, pfs, pfs,
                                  ordv.ctypes.data_as(lsmbloom.u32p)) == 0
    check_walk((fs, ordv), (es, eo), "host in place")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049])
def test_walk_batch_sizes_with_device_keys(parity_set, n):
    """The wave (64) and the split's tile (2048 elements) at their edges."""
    ls, q, dq, mask, row_ord, resume = parity_set
    t0, V = ls.l0_tables(), ls.version_tables()
    for res in (None, resume[:n]):
        es, eo = walk_from(mask[:n], row_ord[:, :n], t0, res)
        check_walk(dev_walk(ls, dq, n, resume=res), (es, eo), n)
        starts, index, step = dev_walk_lists(ls, dq, n, resume=res)
        check_lists((starts, index), lists_from_ord(eo, V), n)
        assert np.array_equal(step, es)
    if n in (65, 2049):  # the any-length key source over the same prefix
        q7 = np.ascontiguousarray(q[:n, :7])
        m7, i7 = ls.probe_version(q7, key_len=7)
        check_walk(ls.probe_walk(q7, key_len=7, resume=resume[:n]),
                   walk_from(m7, ordinals_of(i7, ls.table_order()[0]), t0, resume[:n]), "7-byte keys")


@pytest.mark.gpu
def test_walk_grid_stride(ctx, oracle):
    """600 000 aligned 16-byte keys and 300 000 var-len keys: past one resident
    grid of 1024-lane workgroups (2 and 1 per CU on 256 CUs), as
    test_version_lists_grid_stride chooses them.  The full answer is the set's
    own probe_version here (the oracle in Python would take minutes)."""
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
    t0, V, W = 8, ls.version_tables(), ls.walk_steps()
    assert V == 24 and W == 9
    order_ids = ls.table_order()[0]
    gm, gi = ls.probe_version(keys, key_len=16)
    assert (gm[:4000] != 0).sum() > 300 and (gi[0, :4000] != NONE).all()
    dq = torch.from_numpy(keys).to("cuda:0")
    resume = random_resume(rng, n, W)
    row_ord = ordinals_of(gi, order_ids)
    for res in (None, resume):
        es, eo = walk_from(gm, row_ord, t0, res)
        starts, index, step = dev_walk_lists(ls, dq, n, resume=res)
        check_lists((starts, index), lists_from_ord(eo, V), "fixed16")
        assert np.array_equal(step, es)
    check_walk(dev_walk(ls, dq, n, resume=resume), walk_from(gm, row_ord, t0, resume), "fixed16 per key")
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
    es, eo = walk_from(vm, ordinals_of(vi, order_ids), t0, resume[:nv])
    starts, index, step = dev_walk_lists(ls, d_data, nv, resume=resume[:nv], offsets=d_offs, key_len=0)
    check_lists((starts, index), lists_from_ord(eo, V), "var")
    assert np.array_equal(step, es)
    ls.close()


@pytest.mark.gpu
def test_walk_degenerate_sets(ctx, oracle):
    import torch

    dev = "cuda:0"
    tabs, _ = l0_tables("sst")
    rows = row_tables()
    qv = queries("var")
    n = len(qv)
    mask, ids = reference("sst", "var")
    data, offs = keygen.pack(qv)
    d_data = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    rng = np.random.default_rng(5)

    def check_set(ls, m, row_ord, what):
        t0, V, W = ls.l0_tables(), ls.version_tables(), ls.walk_steps()
        assert W == t0 + ls.rows()
        for res in (None, random_resume(rng, n, W)):
            es, eo = walk_from(m, row_ord, t0, res)
            check_walk(ls.probe_walk_keys(qv, resume=res), (es, eo), what)
            check_walk(dev_walk(ls, d_data, n, resume=res, offsets=d_offs, key_len=0), (es, eo), what)
            hs, hi, hstep = ls.probe_walk_lists_keys(qv, resume=res)
            check_lists((hs, hi), lists_from_ord(eo, V), what)
            assert np.array_equal(hstep, es), what
            starts, index, step = dev_walk_lists(ls, d_data, n, resume=res, offsets=d_offs, key_len=0)
            check_lists((starts, index), lists_from_ord(eo, V), what)
            assert np.array_equal(step, es), what
        return walk_from(m, row_ord, t0)

    # an empty sealed set: W = 0, NONE everywhere, one zero start, no workspace
    em = LevelSet(ctx)
    em.seal()
    assert em.walk_steps() == 0 and em.version_tables() == 0 and em.walk_lists_work_bytes(100) == 0
    step, ordv = check_set(em, np.zeros(n, np.uint64), np.zeros((0, n), np.uint32), "empty")
    assert (step == NONE).all() and (ordv == NONE).all()
    em.close()
    # L0 only
    ls = version_set(ctx, oracle, "sst", 9, rows=[])
    assert ls.rows() == 0 and ls.walk_steps() == 9
    step, _ = check_set(ls, low_bits(mask, 9), np.zeros((0, n), np.uint32), "L0 only")
    assert (step != NONE).sum() > 100
    ls.close()
    # rows only: no L0 staging
    ls = version_set(ctx, oracle, "sst", 0)
    assert ls.walk_steps() == 3 and 0 < ls.walk_lists_work_bytes(n) < ls.lists_work_bytes(n)
    step, _ = check_set(ls, np.zeros(n, np.uint64), ordinals_of(ids, ls.table_order()[0]), "rows only")
    assert sorted(set(step.tolist())) == [0, 1, 2, NONE]
    # a row emptied by a derive between two live rows: it never has a candidate, its step stays
    child = ls.derive([t[0] for t in rows[1]])
    child.seal()
    assert child.rows() == 3 and child.tables(1) == 0 and child.walk_steps() == 3
    gone = ids.copy()
    gone[1] = NONE
    step, _ = check_set(child, np.zeros(n, np.uint64), ordinals_of(gone, child.table_order()[0]), "row 1 emptied")
    assert sorted(set(step.tolist())) == [0, 2, NONE]
    child.close()
    # every row emptied, no L0: W = 3 steps, V = 0 tables
    bare = ls.derive([t[0] for row in rows for t in row])
    bare.seal()
    assert bare.walk_steps() == 3 and bare.version_tables() == 0 and bare.walk_lists_work_bytes(n) == 0
    step, ordv = check_set(bare, np.zeros(n, np.uint64), np.full((3, n), NONE, np.uint32), "all rows emptied")
    assert (step == NONE).all() and (ordv == NONE).all()
    bare.close()
    ls.close()
    # filters with no hash: the ranges alone decide, in L0 and in a row
    f = always_maybe()
    ls = LevelSet(ctx)
    ls.add_filter(L0, 1, f, b"user00002000", b"user00006000")
    ls.add_filter(L0, 2, f, b"user00004000", b"user00008000")
    ls.add_filter(0, 10, f, b"user00000000", b"user00004999")
    ls.add_filter(0, 11, f, b"user00005000", b"user0000zzzz")
    ls.seal()
    m = np.array([(b"user00002000" <= k <= b"user00006000") | (b"user00004000" <= k <= b"user00008000") << 1
                  for k in qv], dtype=np.uint64)
    ro = np.array([[0 if b"user00000000" <= k <= b"user00004999" else 1 if b"user00005000" <= k <= b"user0000zzzz"
                    else NONE for k in qv]], dtype=np.uint32)
    step, _ = check_set(ls, m, ro, "no hash")
    assert sorted(set(step.tolist())) == [0, 1, 2, NONE]
    # all keys outside every range
    out = [b"zzzz%05d" % i for i in range(3000)] + [b"", b"A", b"\xff" * 20]
    step, ordv = ls.probe_walk_keys(out)
    assert (step == NONE).all() and (ordv == NONE).all()
    hs, hi, hstep = ls.probe_walk_lists_keys(out)
    assert hs.tolist() == [0] * 5 and hi.size == 0 and (hstep == NONE).all()
    # n = 0: V + 1 zero starts and nothing else
    starts = torch.full((5,), -1, dtype=torch.int64, device=dev)
    index = torch.full((8,), POISON - (1 << 32), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ls.probe_walk_lists_dev(d_data, 0, starts, index, None, offsets=d_offs, key_len=0)
    ls.probe_walk_dev(d_data, 0, None, offsets=d_offs, key_len=0)
    torch.cuda.synchronize()
    assert (starts.cpu().numpy() == 0).all() and (index.cpu().numpy().view(np.uint32) == POISON).all()
    s0, i0, t0_ = ls.probe_walk_lists_keys([])
    assert s0.tolist() == [0] * 5 and i0.size == 0 and t0_.size == 0
    ls.close()


@pytest.mark.gpu
@pytest.mark.parametrize("t0,total,nrows", [(5, 251, 2), (5, 252, 2), (64, 192, 1), (64, 193, 1)])
def test_walk_lists_radix_pass_edges(ctx, t0, total, nrows):
    """V = t0 + total at 256 and 257: one and two radix passes of the split
    over the walk's one answer row; always-maybe filters, so the ranges alone
    decide and the expectation is a bisect."""
    rng = np.random.default_rng(3000 + total)
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
    V = t0 + total
    assert ls.version_tables() == V and V in (256, 257) and np.array_equal(ls.table_order()[0], tids)
    n = 5000
    tq = rng.integers(0, total + 2, n)
    tq[:min(total, n)] = rng.permutation(total)[:n]
    keys = [b"t%07d%d" % (t, d) for t, d in zip(tq, rng.integers(0, 10, n))]
    los = [b"t%07d0" % t for t in range(total)]
    row_ord = np.full((nrows, n), NONE, dtype=np.uint32)
    mask = np.zeros(n, dtype=np.uint64)
    for i, key in enumerate(keys):
        j = bisect.bisect_right(los, key) - 1
        if j >= 0 and key <= b"t%07d5" % j:
            row_ord[next(r for r in range(nrows) if j < total * (r + 1) // nrows), i] = j
        for v, (lo, hi) in enumerate(l0_rg):
            if lo <= key <= hi:
                mask[i] |= np.uint64(1 << v)
    for res in (None, random_resume(rng, n, t0 + nrows)):
        es, eo = walk_from(mask, row_ord, t0, res)
        exp = lists_from_ord(eo, V)
        if res is not None:  # answers in L0, in the rows and at the top of the ordinals
            assert (es < t0).sum() > 100 and ((es >= t0) & (es != NONE)).sum() > 100 and int(eo[eo != NONE].max()) >= V - 20
        starts, index, step = ls.probe_walk_lists_keys(keys, resume=res)
        check_lists((starts, index), exp, total)
        assert np.array_equal(step, es)
    ls.close()


@pytest.mark.gpu
def test_walk_after_edits(ctx, oracle):
    """derive + add + seal: the flush's table, arriving last, is step 0; the
    survivors keep their relative order behind it."""
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
    assert parent.walk_steps() == child.walk_steps() == 4
    assert child.version_order()[0].tolist()[:3] == [a[0], c[0], d[0]]
    row1 = [t for t in rows[1] if t[0] != drop_row[0]]
    for ls, l0, row in ((parent, [a, b, c], rows[1]), (child, [a, c, d], row1)):
        em, _ = expected_mask(oracle, l0, q)
        ro = ordinals_of(expected_ids(oracle, [row], q), ls.table_order()[0])
        es, eo = walk_from(em, ro, 3)
        got = ls.probe_walk_keys(q)
        check_walk(got, (es, eo), "edit")
        # step 0 is the newest arrival (position 2), whoever it is; then positions 1 and 0
        newest = (em >> np.uint64(2)) & np.uint64(1) == 1
        assert newest.sum() > 3 and (got[0][newest] == 0).all() and (got[1][newest] == 2).all()
        assert ((got[0] == 0) == newest).all()
        hs, hi, hstep = ls.probe_walk_lists_keys(q)
        check_lists((hs, hi), lists_from_ord(eo, ls.version_tables()), "edit lists")
    # in the child, c moved from step 0 (the parent's newest) to step 1 and a stays last of L0
    vids = child.version_order()[0]
    step, ordv = child.probe_walk_keys(q)
    assert set(vids[ordv[step == 0]].tolist()) == {d[0]} and set(vids[ordv[step == 1]].tolist()) == {c[0]}
    assert set(vids[ordv[step == 2]].tolist()) == {a[0]}
    pstep, pord = parent.probe_walk_keys(q)
    assert set(parent.version_order()[0][pord[pstep == 0]].tolist()) == {c[0]}
    child.close()
    parent.close()


@pytest.mark.gpu
def test_walk_contract(parity_set, ctx):
    import torch

    ls, q, dq, mask, row_ord, resume = parity_set
    L = lsmbloom.lib()
    dev = "cuda:0"
    V = ls.version_tables()
    n = 3000
    need = ls.walk_lists_work_bytes(n)
    assert need > 0 and ls.walk_lists_work_bytes(1 << 32) == 0 and ls.walk_lists_work_bytes(0) == 0
    assert ls.walk_lists_work_bytes(2 * n) > need and need < ls.version_lists_work_bytes(n)
    d_res = torch.from_numpy(resume[:n].view(np.int32).copy()).to(dev)
    step = torch.full((n,), POISON - (1 << 32), dtype=torch.int32, device=dev)
    ordv = torch.full((n,), POISON - (1 << 32), dtype=torch.int32, device=dev)
    starts = torch.full((V + 1,), -1, dtype=torch.int64, device=dev)
    index = torch.full((8,), POISON - (1 << 32), dtype=torch.int32, device=dev)
    work = torch.empty(need + 16, dtype=torch.uint8, device=dev)
    assert work.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    keys = (ls.h, vp(dq.data_ptr()), None, 16)
    fs = (vp(d_res.data_ptr()), vp(step.data_ptr()))
    out = (vp(starts.data_ptr()), vp(index.data_ptr()), 8)
    # the per-key form: a null d_ord, null keys
    assert L.lsmb_lset_probe_walk_dev(*keys, n, *fs, None, None) == EINVAL
    assert L.lsmb_lset_probe_walk_dev(ls.h, None, None, 16, n, *fs, vp(ordv.data_ptr()), None) == EINVAL
    # the lists form: a workspace one byte short, null, misaligned by 8; n = 2^32; null starts; a capacity without an index
    assert L.lsmb_lset_probe_walk_lists_dev(*keys, n, *fs, *out, vp(work.data_ptr()), need - 1, None) == EINVAL
    assert L.lsmb_lset_probe_walk_lists_dev(*keys, n, *fs, *out, None, need, None) == EINVAL
    assert L.lsmb_lset_probe_walk_lists_dev(*keys, n, *fs, *out, vp(work.data_ptr() + 8), need, None) == EINVAL
    assert L.lsmb_lset_probe_walk_lists_dev(*keys, 1 << 32, *fs, *out, vp(work.data_ptr()), need, None) == EINVAL
    assert L.lsmb_lset_probe_walk_lists_dev(*keys, n, *fs, None, vp(index.data_ptr()), 8, vp(work.data_ptr()), need,
                                            None) == EINVAL
    assert L.lsmb_lset_probe_walk_lists_dev(*keys, n, *fs, vp(starts.data_ptr()), None, 5, vp(work.data_ptr()), need,
                                            None) == EINVAL
    with pytest.raises(ValueError):
        ls.probe_walk_lists_dev(dq, n, starts, index, work[:need - 1], step=step, resume=d_res, key_len=16)
    # the host forms
    hq = q.ctypes.data_as(lsmbloom.u8p)
    hf, ht, ho = resume[:n].copy(), np.full(n, 5, np.uint32), np.full(n, 6, np.uint32)
    hs, hi = np.full(V + 1, 7, np.uint64), np.full(8, 9, np.uint32)
    pf, pt, po = (x.ctypes.data_as(lsmbloom.u32p) for x in (hf, ht, ho))
    ps, pi = hs.ctypes.data_as(lsmbloom.u64p), hi.ctypes.data_as(lsmbloom.u32p)
    assert L.lsmb_lset_probe_walk(ls.h, hq, None, 16, n, pf, pt, None) == EINVAL
    assert L.lsmb_lset_probe_walk(ls.h, None, None, 16, n, pf, pt, po) == EINVAL
    assert L.lsmb_lset_probe_walk_lists(ls.h, hq, None, 16, 1 << 32, pf, pt, ps, pi, 8) == EINVAL
    assert L.lsmb_lset_probe_walk_lists(ls.h, hq, None, 16, n, pf, pt, None, pi, 8) == EINVAL
    assert L.lsmb_lset_probe_walk_lists(ls.h, hq, None, 16, n, pf, pt, ps, None, 8) == EINVAL
    # before seal: every entry point refuses (or answers 0)
    un = LevelSet(ctx)
    un.add_filter(L0, 1, always_maybe(), b"a", b"z")
    un.add_filter(0, 2, always_maybe(), b"a", b"z")
    assert un.walk_steps() == 0 and un.walk_lists_work_bytes(100) == 0
    assert L.lsmb_lset_probe_walk_dev(un.h, vp(dq.data_ptr()), None, 16, n, *fs, vp(ordv.data_ptr()), None) == EINVAL
    assert L.lsmb_lset_probe_walk_lists_dev(un.h, vp(dq.data_ptr()), None, 16, n, *fs, *out, vp(work.data_ptr()), need,
                                            None) == EINVAL
    assert L.lsmb_lset_probe_walk(un.h, hq, None, 16, n, pf, pt, po) == EINVAL
    assert L.lsmb_lset_probe_walk_lists(un.h, hq, None, 16, n, pf, pt, ps, pi, 8) == EINVAL
    with pytest.raises(ValueError):
        un.probe_walk_keys([b"a"])
    with pytest.raises(ValueError):
        un.probe_walk_lists_keys([b"a"])
    with pytest.raises(ValueError):
        un.probe_walk_dev(dq, n, ordv, step=step, resume=d_res, key_len=16)
    un.close()
    # nothing was written by any of the refused calls
    torch.cuda.synchronize()
    assert (step.cpu().numpy().view(np.uint32) == POISON).all() and (ordv.cpu().numpy().view(np.uint32) == POISON).all()
    assert (starts.cpu().numpy() == -1).all() and (index.cpu().numpy().view(np.uint32) == POISON).all()
    assert np.array_equal(d_res.cpu().numpy().view(np.uint32), resume[:n])
    assert np.array_equal(hf, resume[:n]) and (ht == 5).all() and (ho == 6).all() and (hs == 7).all() and (hi == 9).all()


@pytest.mark.gpu
def test_cpp_mirror_walk_gpu():
    r = subprocess.run([cpp_bin("lset_walk_test"), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout
