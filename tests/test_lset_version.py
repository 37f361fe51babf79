"""A level set's L0 part and the Version probe (lsmb_lset_probe_version): one
sealed set answers the whole walk of DB::get / Snapshot::get over a Version
(src/db/mod.rs:238-267, src/db/snapshot.rs:40-69) from one hash per key:

    mask[i] bit j = min_j <= key_i <= max_j && may_contain(filter_j, key_i)
                    for the L0 table at position j (order of arrival),
    ids[r, i]     = exactly what lsmb_lset_probe answers.

Expected masks come from the CPU oracle's may_contain (its batched probe) and
Python's bytes ordering (the same lexicographic order as Rust's [u8]); expected
ids from expected_ids of tests/test_lset.py; never from the library.  Every
comparison is exact equality over all answers.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import keygen
import lsmbloom
from lsmbloom import BloomFilter, FilterSet, LevelSet
from lset_support import (SIZINGS, add_tables, build_table, cpp_bin, expected_ids, expected_mask, k12, kvar, l0_ranges,
                          l0_tables, low_bits, queries, reference, row_tables)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = lsmbloom.LSMB_LSET_NONE
L0 = lsmbloom.LSMB_LSET_ROW_L0
EINVAL = lsmbloom.LSMB_EINVAL
vp = ctypes.c_void_p
SST = (1000, 0.01)


# ---------------------------------------------------------------- without a GPU

def test_constants_and_null_arguments():
    L = lsmbloom.lib()
    assert lsmbloom.LSMB_LSET_ROW_L0 == 0x80000000 and lsmbloom.LSMB_LSET_L0_MAX == 64
    assert L.lsmb_abi_version() == 6
    for name in ("lsmb_lset_l0_tables", "lsmb_lset_l0_order", "lsmb_lset_probe_version", "lsmb_lset_probe_version_dev"):
        assert hasattr(L, name) and name in lsmbloom.SIGNATURES
    for name in ("l0_tables", "l0_order", "probe_version", "probe_version_keys", "probe_version_dev"):
        assert callable(getattr(LevelSet, name))
    keys = np.zeros(16, np.uint8)
    mask = np.full(4, 777, np.uint64)
    ids = np.full(4, 777, np.uint32)
    p8, pm, pi = keys.ctypes.data_as(lsmbloom.u8p), mask.ctypes.data_as(lsmbloom.u64p), ids.ctypes.data_as(lsmbloom.u32p)
    assert L.lsmb_lset_probe_version(None, p8, None, 4, 4, pm, pi) == EINVAL
    assert L.lsmb_lset_probe_version_dev(None, vp(1), None, 4, 4, vp(1), vp(1), None) == EINVAL
    assert L.lsmb_lset_l0_order(None, pi) == EINVAL
    assert L.lsmb_lset_l0_tables(None) == 0
    assert L.lsmb_lset_tables(None, L0) == 0
    assert (mask == 777).all() and (ids == 777).all()


def test_fset_plan_host(tmp_path):
    """The planning a filter set and a level set's L0 part share
    (csrc/fset_plan.hpp): region masks, size classes and the plain host
    statement of the L0 answer against brute force over random overlapping
    ranges — nested, identical, touching at one key, an empty-string bound,
    bounds longer than 16 bytes sharing their first 16 — for 0, 1, 8, 9 and 64
    tables (tests/cpp/fset_plan_test.cpp), under ASan and UBSan."""
    exe = str(tmp_path / "fset_plan_test")
    src = os.path.join(ROOT, "tests", "cpp", "fset_plan_test.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout


def test_cpp_mirror_version_argument_checks():
    r = subprocess.run([cpp_bin("lset_version_test")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


# ------------------------------------------------------------------- on the GPU
#
# The parity workload (l0_tables, row_tables, queries, reference) is lset_support's.

def probe_kind(ls, kind, q):
    if kind == "var":
        return ls.probe_version_keys(q)
    data = np.frombuffer(b"".join(q), dtype=np.uint8)
    return ls.probe_version(data, key_len=16 if kind == "fixed16" else 12)


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["sst", "mixed"])
@pytest.mark.parametrize("t0", [1, 8, 9, 17, 33, 64])
def test_version_probe_matches_range_and_bloom_checks(oracle, t0, geom):
    assert lsmbloom.params(40000, 0.01)[0] > 64 * 1024  # one-byte entries: past the LDS tables even alone
    assert lsmbloom.params(40, 1e-4)[1] > 8
    tabs, _ = l0_tables(geom)
    rows = row_tables()
    ctx = lsmbloom.Context(0)
    sets = {}
    # no row: single adds, blocks and words alternating
    ls = LevelSet(ctx)
    for j, t in enumerate(tabs[:t0]):
        if t[3] == 0 or j % 2:
            ls.add_filter(L0, t[0], BloomFilter(t[1], t[3], t[2]), t[4], t[5])
        else:
            ls.add(L0, t[0], oracle.serialize(t[1], t[2], t[3]), t[4], t[5])
    sets[0] = ls
    # one row of 65 tables: single adds, the row's interleaved with L0's
    ls = LevelSet(ctx)
    for j in range(65):
        add_tables(ls, oracle, 0, [rows[0][64 - j]])
        if j < t0:
            add_tables(ls, oracle, L0, [tabs[j]])
    sets[1] = ls
    # three rows: one batch, L0 tables spread through it (position = index order)
    placed = [(r, t) for r, row in enumerate(rows) for t in row]
    for j, t in enumerate(tabs[:t0]):
        placed.insert(2 * j, (L0, t))
    ls = LevelSet(ctx)
    ls.add_many([r for r, _ in placed], [t[0] for _, t in placed],
                [oracle.serialize(t[1], t[2], t[3]) for _, t in placed], [(t[4], t[5]) for _, t in placed])
    sets[3] = ls
    for nrows, ls in sets.items():
        assert ls.l0_tables() == t0 == ls.tables(L0) and ls.rows() == nrows
        ls.seal()
        assert ls.l0_order().tolist() == [t[0] for t in tabs[:t0]]
        for kind in ("fixed16", "fixed12", "var"):
            q = queries(kind)
            mask, ids = reference(geom, kind)
            for n in (1, 255, 256, 257, 5000):
                gm, gi = probe_kind(ls, kind, q[:n])
                assert gm.dtype == np.uint64 and gm.shape == (n,) and gi.shape == (nrows, n)
                em = low_bits(mask[:n], t0)
                assert np.array_equal(gm, em), (nrows, kind, n, np.argwhere(gm != em)[:5])
                assert np.array_equal(gi, ids[:nrows, :n]), (nrows, kind, n, np.argwhere(gi != ids[:nrows, :n])[:5])
        ls.close()
    ctx.close()


@pytest.mark.gpu
def test_version_probe_eight_byte_entries(oracle):
    """64 filters of one small sizing: one class of 64 members, the only LDS
    table with 8-byte entries (64 SST-sized filters do not fit and are walked
    from L2)."""
    nb, k = lsmbloom.params(40, 0.01)
    assert (nb + 31) // 32 * 32 * 8 <= 64 * 1024
    rng = np.random.default_rng(68)
    tabs = []
    for j, (lo, hi) in enumerate(l0_ranges()):
        a = int(lo[4:12]) if len(lo) >= 12 else 0
        b = int(hi[4:12]) if len(hi) >= 12 and hi[4:12].isdigit() else 9999
        mem = sorted({m for m in [kvar(int(i), int(i) % 25) for i in rng.integers(a, b + 1, 20)] + [lo, hi]
                      if lo <= m <= hi})
        data, offs = keygen.pack(mem)
        tabs.append((j, oracle.build_var(data, offs, nb, k), nb, k, lo, hi))
    q = queries("var")[:2000]
    exp, inr = expected_mask(oracle, tabs, q)
    assert ((inr & ~exp) != 0).any() and (exp >> np.uint64(32)).any() and (exp & np.uint64(0xFFFFFFFF)).any()
    ctx = lsmbloom.Context(0)
    ls = LevelSet(ctx)
    for t in tabs:
        add_tables(ls, oracle, L0, [t])
    ls.seal()
    gm, gi = ls.probe_version_keys(q)
    assert np.array_equal(gm, exp), np.argwhere(gm != exp)[:5]
    assert gi.shape == (0, len(q))
    ls.close()
    ctx.close()


@pytest.mark.gpu
def test_version_probe_grid_stride_agrees_with_the_two_probes(oracle):
    """600 000 keys: past 8 workgroups x 256 lanes (2 x 1024) on each of 256 CUs."""
    n = 600_000
    keys = keygen.key16(0x5EED0700, 0, n)
    srt = sorted(bytes(x) for x in keys[:4000])
    rng = np.random.default_rng(66)
    ctx = lsmbloom.Context(0)
    fs, ls, only_rows = FilterSet(ctx), LevelSet(ctx), LevelSet(ctx)
    for j in range(8):  # overlapping quantile ranges, members from inside
        a = int(rng.integers(0, 3000))
        part = srt[a:a + int(rng.integers(200, 1000))]
        t = build_table(oracle, 50 + j, part[::2], SST)
        blk = oracle.serialize(t[1], t[2], t[3])
        assert fs.add(blk, part[0], part[-1]) == j  # slot j = position j
        ls.add(L0, t[0], blk, part[0], part[-1])
    for c in range(16):
        part = srt[c * 250:(c + 1) * 250]
        t = build_table(oracle, 900 + c, part, (250, 0.01))
        for s in (ls, only_rows):
            add_tables(s, oracle, 0, [t])
    ls.seal()
    only_rows.seal()
    gm, gi = ls.probe_version(keys, key_len=16)
    assert np.array_equal(gm, fs.probe(keys, key_len=16))
    assert np.array_equal(gi, only_rows.probe(keys, key_len=16))
    assert np.array_equal(gi, ls.probe(keys, key_len=16))
    assert (gm[:4000] != 0).sum() > 300 and (gm[4000:] == 0).sum() > 100_000 and (gi[0, :4000] != NONE).all()
    for s in (fs, ls, only_rows):
        s.close()
    ctx.close()


@pytest.mark.gpu
def test_version_probe_without_l0_without_rows_and_n_zero(oracle):
    import torch
    dev = torch.device("cuda:0")
    L = lsmbloom.lib()
    tabs, _ = l0_tables("sst")
    rows = row_tables()
    q = queries("var")[:700]
    data, offs = keygen.pack(q)
    d_data = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    n = len(q)
    ctx = lsmbloom.Context(0)
    st = torch.cuda.Stream(dev)
    # rows only: a zero mask, and the ids of probe()
    ls = LevelSet(ctx)
    add_tables(ls, oracle, 0, rows[1])
    add_tables(ls, oracle, 1, rows[2])
    canary_m = np.full(4, 777, np.uint64)
    canary_i = np.full(8, 777, np.uint32)
    pk, pm, pi = data.ctypes.data_as(lsmbloom.u8p), canary_m.ctypes.data_as(lsmbloom.u64p), canary_i.ctypes.data_as(lsmbloom.u32p)
    po = offs.ctypes.data_as(lsmbloom.u64p)
    assert L.lsmb_lset_probe_version(ls.h, pk, po, 0, 4, pm, pi) == EINVAL  # before seal
    assert L.lsmb_lset_l0_order(ls.h, pi) == EINVAL
    assert (canary_m == 777).all() and (canary_i == 777).all()
    ls.seal()
    assert ls.l0_tables() == 0 and ls.l0_order().size == 0
    gm, gi = ls.probe_version_keys(q)
    assert (gm == 0).all() and gm.shape == (n,)
    assert np.array_equal(gi, ls.probe_keys(q)) and np.array_equal(gi, expected_ids(oracle, [rows[1], rows[2]], q))
    dm = torch.full((n,), -1, dtype=torch.int64, device=dev)
    do = torch.full((2 * n,), 12345, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ls.probe_version_dev(d_data, n, dm, do, offsets=d_offs, stream=st.cuda_stream)
    st.synchronize()
    assert bool((dm == 0).all()) and np.array_equal(do.cpu().numpy().view(np.uint32).reshape(2, n), gi)
    with pytest.raises(ValueError):
        ls.probe_version_dev(d_data, n, dm, None, offsets=d_offs)  # rows need an output
    assert L.lsmb_lset_probe_version_dev(ls.h, vp(d_data.data_ptr()), vp(d_offs.data_ptr()), 0, n, None,
                                         vp(do.data_ptr()), None) == EINVAL  # the mask is never optional
    # n = 0 writes nothing
    dm.fill_(-1)
    do.fill_(12345)
    torch.cuda.synchronize()
    ls.probe_version_dev(d_data, 0, dm, do, offsets=d_offs, stream=st.cuda_stream)
    st.synchronize()
    assert bool((dm == -1).all()) and bool((do == 12345).all())
    assert L.lsmb_lset_probe_version(ls.h, pk, po, 0, 0, pm, pi) == lsmbloom.LSMB_OK
    assert (canary_m == 777).all() and (canary_i == 777).all()
    em, ei = ls.probe_version_keys([])
    assert em.shape == (0,) and ei.shape == (2, 0)
    ls.close()
    # L0 only: no row, d_out = NULL
    ls = LevelSet(ctx)
    for t in tabs[:9]:
        add_tables(ls, oracle, L0, [t])
    ls.seal()
    assert ls.rows() == 0 and ls.total_tables() == 0 and ls.l0_tables() == 9
    exp, _ = expected_mask(oracle, tabs[:9], q)
    dm.fill_(-1)
    torch.cuda.synchronize()
    ls.probe_version_dev(d_data, n, dm, None, offsets=d_offs, stream=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(dm.cpu().numpy().view(np.uint64), exp)
    gm, gi = ls.probe_version_keys(q)
    assert np.array_equal(gm, exp) and gi.shape == (0, n)
    assert ls.probe_keys(q).shape == (0, n)  # the rows' probe still sees no row
    # the same bytes on every run, whatever the stream
    dm2 = torch.full((n,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ls.probe_version_dev(d_data, n, dm2, None, offsets=d_offs)
    torch.cuda.synchronize()
    assert bool((dm == dm2).all())
    ls.close()
    # a sealed set of nothing
    ls = LevelSet(ctx)
    ls.seal()
    gm, gi = ls.probe_version_keys(q[:5])
    assert (gm == 0).all() and gi.shape == (0, 5)
    ls.close()
    ctx.close()


@pytest.mark.gpu
def test_version_edits_keep_l0_positions(oracle):
    tabs, _ = l0_tables("mixed")
    rows = row_tables()
    a, b, c, d, e = tabs[0], tabs[1], tabs[3], tabs[4], tabs[6]
    q = queries("var")[:1500]
    ctx = lsmbloom.Context(0)
    parent = LevelSet(ctx)
    for t in (a, b, c):
        add_tables(parent, oracle, L0, [t])
    add_tables(parent, oracle, 0, rows[1])
    parent.seal()
    drop_row = rows[1][2]

    def check(ls, l0, row, what):
        assert ls.l0_order().tolist() == [t[0] for t in l0], what
        gm, gi = ls.probe_version_keys(q)
        em, _ = expected_mask(oracle, l0, q)
        assert np.array_equal(gm, em), what
        assert np.array_equal(gi, expected_ids(oracle, [row], q)), what

    check(parent, [a, b, c], rows[1], "parent")
    child = parent.derive([b[0], drop_row[0]])
    assert child.dropped == 2 and child.l0_tables() == 2
    add_tables(child, oracle, L0, [d])
    child.seal()
    row1 = [t for t in rows[1] if t[0] != drop_row[0]]
    check(child, [a, c, d], row1, "child")
    s = child.stats()
    assert s["tables"] == 3 + len(row1) and s["inherited"] == 2 + len(row1)
    assert s["uploaded_bytes"] == 8 * ((d[2] + 63) // 64)  # only d's bytes crossed
    check(parent, [a, b, c], rows[1], "parent after the child is sealed")
    # a second derive in the chain: c goes, e arrives
    grand = child.derive([c[0]])
    add_tables(grand, oracle, L0, [e])
    grand.seal()
    check(grand, [a, d, e], row1, "grandchild")
    g = grand.stats()
    assert g["inherited"] == 2 + len(row1) and g["uploaded_bytes"] == 8 * ((e[2] + 63) // 64)
    child.close()
    check(parent, [a, b, c], rows[1], "parent after the child is closed")
    check(grand, [a, d, e], row1, "grandchild after its parent is closed")
    parent.close()
    check(grand, [a, d, e], row1, "grandchild alone")
    grand.close()
    ctx.close()


@pytest.mark.gpu
def test_l0_cap_and_all_or_nothing(oracle):
    tabs, _ = l0_tables("sst")
    rows = row_tables()
    q = queries("fixed12")[:600]
    ctx = lsmbloom.Context(0)
    ls = LevelSet(ctx)
    for t in tabs[:60]:
        add_tables(ls, oracle, L0, [t])
    add_tables(ls, oracle, 0, rows[2])
    before = (ls.stats(), ls.l0_tables(), ls.rows(), ls.tables(0), ls.tables(L0))
    # 60 + 5 L0 tables in a batch with 3 row tables: the fifth L0 table is the 65th
    placed = [(L0, tabs[60]), (1, rows[1][0]), (L0, tabs[61]), (L0, tabs[62]), (1, rows[1][1]), (L0, tabs[63]),
              (L0, tabs[0]), (1, rows[1][2])]
    with pytest.raises(ValueError) as ei:
        ls.add_many([r for r, _ in placed], [t[0] + 500 for _, t in placed],
                    [oracle.serialize(t[1], t[2], t[3]) for _, t in placed], [(t[4], t[5]) for _, t in placed])
    assert ei.value.status.tolist() == [0, 0, 0, 0, 0, 0, EINVAL, 0]
    assert "table 6" in str(ei.value) and str(tabs[0][0] + 500) in str(ei.value)
    assert (ls.stats(), ls.l0_tables(), ls.rows(), ls.tables(0), ls.tables(L0)) == before
    for t in tabs[60:64]:
        add_tables(ls, oracle, L0, [t])
    assert ls.l0_tables() == 64
    full = (ls.stats(), ls.l0_tables(), ls.rows())
    for add in (lambda: ls.add(L0, 9999, oracle.serialize(tabs[0][1], tabs[0][2], tabs[0][3]), b"a", b"b"),
                lambda: ls.add_filter(L0, 9999, BloomFilter(tabs[0][1], tabs[0][3], tabs[0][2]), b"a", b"b")):
        with pytest.raises(ValueError):
            add()
    with pytest.raises(ValueError):
        ls.add(9, 1, oracle.serialize(tabs[0][1], tabs[0][2], tabs[0][3]), b"a", b"b")  # any other row >= 8
    with pytest.raises(ValueError):
        ls.add(L0 + 1, 1, oracle.serialize(tabs[0][1], tabs[0][2], tabs[0][3]), b"a", b"b")
    assert (ls.stats(), ls.l0_tables(), ls.rows()) == full
    ls.seal()
    gm, gi = probe_kind(ls, "fixed12", q)
    em, _ = expected_mask(oracle, tabs, q)
    assert np.array_equal(gm, em) and np.array_equal(gi, expected_ids(oracle, [rows[2]], q))
    ls.close()
    # min_key > max_key in L0: seal names the table and the set stays unsealed
    ls = LevelSet(ctx)
    add_tables(ls, oracle, L0, [tabs[0]])
    t = tabs[3]
    ls.add(L0, 4242, oracle.serialize(t[1], t[2], t[3]), t[5], t[4])
    with pytest.raises(ValueError) as ei:
        ls.seal()
    assert "4242" in str(ei.value) and str(tabs[0][0]) not in str(ei.value)
    with pytest.raises(ValueError):
        ls.probe_version_keys([b"a"])
    ls.close()
    ctx.close()


@pytest.mark.gpu
def test_device_built_tables_reach_l0(oracle):
    import torch
    rng = np.random.default_rng(67)
    tabs = []
    for j in range(12):  # 4 overlapping L0 tables, 8 disjoint row tables
        l0 = j % 3 == 0
        first = int(rng.integers(0, 500)) if l0 else 1000 * j
        ks = sorted({k12(int(i)) for i in rng.integers(first, first + 800, 300)})
        nb, k = lsmbloom.params(*SIZINGS[(j // 3 + j) % 3])  # the L0 tables take all three sizings
        tabs.append((L0 if l0 else j % 2, 300 + j, ks, nb, k))
    run = [x for t in tabs for x in t[2]]
    data, offs = keygen.pack(run)
    seg = np.zeros(13, np.uint64)
    np.cumsum([len(t[2]) for t in tabs], out=seg[1:])
    nb, kk = [t[3] for t in tabs], [t[4] for t in tabs]
    dev = torch.device("cuda:0")
    ctx = lsmbloom.Context(0)
    d_data = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    words = torch.full((int(lsmbloom.build_batch_layout(nb)[-1]),), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.build_batch_dev(d_data, len(run), seg, nb, kk, words, offsets=d_offs)
    built = LevelSet(ctx)
    built.add_built([t[0] for t in tabs], [t[1] for t in tabs], words, nb, kk, [(t[2][0], t[2][-1]) for t in tabs])
    del words
    loaded = LevelSet(ctx)
    otabs = []
    for row, tid, ks, b, k in tabs:
        d, o = keygen.pack(ks)
        otabs.append((row, (tid, oracle.build_var(d, o, b, k), b, k, ks[0], ks[-1])))
    loaded.add_many([r for r, _ in otabs], [t[0] for _, t in otabs],
                    [oracle.serialize(t[1], t[2], t[3]) for _, t in otabs], [(t[4], t[5]) for _, t in otabs])
    q = [k12(int(i)) for i in rng.integers(0, 12500, 3000)] + run[::7]
    for s in (built, loaded):
        assert s.l0_tables() == 4 and s.rows() == 2
        s.seal()
        assert s.l0_order().tolist() == [300, 303, 306, 309]
    bm, bi = built.probe_version_keys(q)
    lm, li = loaded.probe_version_keys(q)
    assert np.array_equal(bm, lm) and np.array_equal(bi, li)
    em, _ = expected_mask(oracle, [t for r, t in otabs if r == L0], q)
    assert np.array_equal(bm, em)
    l0_members = {x for t in tabs if t[0] == L0 for x in t[2]}
    queried = sum(x in l0_members for x in q)  # every one of them sets a bit: no false negatives
    assert queried > 100 and (em != 0).sum() >= queried
    assert built.stats()["uploaded_bytes"] == 0  # nothing crossed from the host
    built.close()
    loaded.close()
    ctx.close()


@pytest.mark.gpu
def test_rows_only_entry_points_ignore_l0(oracle):
    tabs, _ = l0_tables("mixed")
    rows = row_tables()
    q = queries("var")[:2000]
    ctx = lsmbloom.Context(0)
    with_l0, without = LevelSet(ctx), LevelSet(ctx)
    for r in (1, 2):
        for s in (with_l0, without):
            add_tables(s, oracle, r - 1, rows[r])
    for t in tabs[:10]:
        add_tables(with_l0, oracle, L0, [t])
    with_l0.seal()
    without.seal()
    assert with_l0.rows() == without.rows() == 2
    assert with_l0.total_tables() == without.total_tables() == 8
    a, b = with_l0.table_order(), without.table_order()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert [with_l0.tables(r) for r in range(8)] == [without.tables(r) for r in range(8)]
    assert np.array_equal(with_l0.probe_keys(q), without.probe_keys(q))
    la, lb = with_l0.probe_lists_keys(q), without.probe_lists_keys(q)
    assert np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1])
    assert with_l0.lists_work_bytes(len(q)) == without.lists_work_bytes(len(q))
    assert with_l0.stats()["tables"] == without.stats()["tables"] + 10
    with_l0.close()
    without.close()
    ctx.close()


@pytest.mark.gpu
def test_cpp_mirror_version_gpu():
    r = subprocess.run([cpp_bin("lset_version_test"), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout
