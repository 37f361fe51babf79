"""Device-resident level sets (lsmb_lset): the batched form of DB::get's walk
over L1 and below (src/db/mod.rs:255-267), where the tables of a level have
pairwise disjoint key ranges and the answer per key and level is one table id
or none:

    out[r, i] = table_id of the one table t of row r with
                min_t <= key_i <= max_t && may_contain(filter_t, key_i), else NONE

Expected answers come from the CPU oracle's may_contain (the checker), Python's
bytes ordering (the same lexicographic order as Rust's [u8]) and bisect over
each row's sorted ranges; never from the library.  Every comparison is exact
equality over all rows() * n answers.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import keygen
import lsmbloom
from lsmbloom import BloomFilter, FilterSet, LevelSet
from lset_support import SIZINGS, add_tables, build_table, cpp_bin, expected_ids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = lsmbloom.LSMB_LSET_NONE
vp = ctypes.c_void_p


# ---------------------------------------------------------------- without a GPU

def test_lset_open_without_context_is_einval_and_null_getters_are_zero():
    L = lsmbloom.lib()
    h = vp()
    assert L.lsmb_lset_open(None, ctypes.byref(h)) == lsmbloom.LSMB_EINVAL
    assert L.lsmb_lset_open(None, None) == lsmbloom.LSMB_EINVAL
    assert L.lsmb_lset_rows(None) == 0
    assert L.lsmb_lset_tables(None, 0) == 0
    assert L.lsmb_lset_tables(None, 7) == 0
    L.lsmb_lset_close(None)


def test_lset_entry_points_reject_a_null_set():
    L = lsmbloom.lib()
    one = np.zeros(16, np.uint8)
    w = np.zeros(2, np.uint64)
    out = np.zeros(4, np.uint32)
    p8 = one.ctypes.data_as(lsmbloom.u8p)
    assert L.lsmb_lset_add(None, 0, 1, p8, 12, p8, 1, p8, 1) == lsmbloom.LSMB_EINVAL
    assert L.lsmb_lset_add_words(None, 0, 1, w.ctypes.data_as(lsmbloom.u64p), 128, 7, p8, 1, p8, 1) == lsmbloom.LSMB_EINVAL
    assert L.lsmb_lset_seal(None) == lsmbloom.LSMB_EINVAL
    assert L.lsmb_lset_probe(None, p8, None, 4, 4, out.ctypes.data_as(lsmbloom.u32p)) == lsmbloom.LSMB_EINVAL
    assert L.lsmb_lset_probe_dev(None, vp(1), None, 4, 4, vp(1), None) == lsmbloom.LSMB_EINVAL
    assert lsmbloom.LSMB_LSET_NONE == 0xFFFFFFFF and lsmbloom.LSMB_LSET_MAX_LEVELS == 8


def test_lset_row_order_and_search_host(tmp_path):
    """The per-row ordering, the disjointness check of lsmb_lset_seal and the
    plain statement of the kernel's search (csrc/lset_order.hpp) against brute
    force (tests/cpp/lset_order_test.cpp), under ASan and UBSan."""
    exe = str(tmp_path / "lset_order_test")
    src = os.path.join(ROOT, "tests", "cpp", "lset_order_test.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout


def test_cpp_mirror_level_set_argument_checks():
    r = subprocess.run([cpp_bin("lset_test")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


# ------------------------------------------------------------------- on the GPU

@pytest.mark.gpu
def test_lset_three_rows_match_range_and_bloom_checks(oracle):
    assert lsmbloom.params(1000, 0.01)[0] < 1 << 14 < lsmbloom.params(40000, 0.01)[0]
    assert lsmbloom.params(40, 1e-4)[1] > 8
    rng = np.random.default_rng(21)
    rows, members = [], []
    for r, ntab in enumerate((1, 65, 300)):
        tabs = []
        for t in range(ntab):
            base = 40 * r + 150 * t  # 100 ids wide, then a gap of 50
            ids = np.sort(rng.choice(100, size=40, replace=False)) + base
            keys = [b"user%08d" % i for i in ids]
            k0 = (r, t) == (1, 5)  # one filter with no hash: only the range decides
            tabs.append(build_table(oracle, 1000 * r + t + 7, keys, SIZINGS[t % 4], k=0 if k0 else None))
            members.append((r, tabs[-1][0], keys[::3]))
        rows.append(tabs)
    ctx = lsmbloom.Context(0)
    ls = LevelSet(ctx)
    flat = [(r, n) for r, tabs in enumerate(rows) for n in range(len(tabs))]
    for j in rng.permutation(len(flat)):  # any order, rows interleaved
        r, n = flat[j]
        add_tables(ls, oracle, r, [rows[r][n]])
    assert ls.rows() == 3 and [ls.tables(r) for r in range(4)] == [1, 65, 300, 0]
    ls.seal()
    q = [kk for _, _, ks in members for kk in ks]                                  # members
    q += [b"user%08d" % i for i in rng.integers(0, 150 * 300 + 500, 20_000)]       # mostly absent: ranges and gaps
    alltabs = [t for tabs in rows for t in tabs]
    q += [t[4] for t in alltabs] + [t[5] for t in alltabs]                         # inclusive bounds
    q += [t[4][:-1] for t in alltabs] + [t[5] + b"\x00" for t in alltabs]          # just outside them
    q += [b"", b"user", b"\xff" * 40]
    got = ls.probe_keys(q)
    assert got.dtype == np.uint32 and got.shape == (3, len(q))
    exp = expected_ids(oracle, rows, q)
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:10]
    # every member is reported by its own table, in its own row
    at = 0
    for r, tid, ks in members:
        assert (got[r, at:at + len(ks)] == tid).all()
        at += len(ks)
    assert (got == NONE).any() and (got != NONE).sum() > at  # both answers occur (false positives, k = 0, bounds)
    ls.close()
    ctx.close()


@pytest.mark.gpu
def test_lset_long_bounds_sharing_their_first_16_bytes(oracle):
    # 13 runs of 10 tables; every bound of a run starts with the same 16 bytes
    # and is 24..40 bytes long, so the prefix search ties and the full compares decide
    tabs, members = [], []
    for g in range(13):
        pre = b"prefix-%04d-----" % g
        assert len(pre) == 16
        for j in range(10):
            keys = sorted(pre + b"%02d/%03d" % (j, i) + b"x" * (2 + (7 * i + j) % 17) for i in range(6))
            assert all(24 <= len(kk) <= 40 for kk in keys)
            tabs.append(build_table(oracle, 10 * g + j, keys, (1000, 0.01)))
            members += keys
    assert len(tabs) == 130
    ctx = lsmbloom.Context(0)
    ls = LevelSet(ctx)
    order = np.random.default_rng(22).permutation(len(tabs))
    add_tables(ls, oracle, 0, [tabs[j] for j in order])
    ls.seal()
    q = list(members)
    for g in range(13):
        pre = b"prefix-%04d-----" % g
        q += [pre, pre[:-1], pre + b"\x00", pre + b"\xff", pre + b"05", pre + b"05/", pre + b"05/999" + b"z" * 20]
        q += [pre + b"%02d/%03d" % (j, i) + b"y" * (1 + (i + j) % 18) for j in range(10) for i in range(7)]
    q += [t[4] for t in tabs] + [t[5] for t in tabs]
    q += [t[4][:-1] for t in tabs] + [t[5] + b"\x00" for t in tabs] + [t[4][:16] for t in tabs] + [t[5][:17] for t in tabs]
    got = ls.probe_keys(q)
    exp = expected_ids(oracle, [tabs], q)
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:10]
    assert (got[0, :len(members)] != NONE).all() and (got == NONE).sum() > 13 * 7
    ls.close()
    ctx.close()


@pytest.mark.gpu
def test_lset_fixed_16_byte_keys_and_device_probe(oracle):
    import torch

    rows = []
    for r, (seed, cuts) in enumerate([(0x5EED0500, 4), (0x5EED0501, 3)]):
        keys = keygen.key16(seed, 0, 4000)
        srt = sorted(bytes(x) for x in keys)
        tabs = []
        for c in range(cuts):  # quantile ranges: disjoint, each with its own filter
            part = srt[c * len(srt) // cuts:(c + 1) * len(srt) // cuts]
            tabs.append(build_table(oracle, 100 * r + c, part, (len(part), 0.01)))
        rows.append(tabs)
    ctx = lsmbloom.Context(0)
    ls = LevelSet(ctx)
    for r, tabs in enumerate(rows):
        add_tables(ls, oracle, r, tabs[::-1])
    ls.seal()
    q = np.concatenate([keygen.key16(0x5EED0500, 0, 400), keygen.key16(0x5EED0501, 100, 300),
                        keygen.key16(0x5EED0600, 0, 325)])
    assert q.shape == (1025, 16)
    exp = expected_ids(oracle, rows, [bytes(x) for x in q])
    st = torch.cuda.Stream("cuda:0")
    for n in (1025, 1):
        got = ls.probe(q[:n], key_len=16)
        assert got.shape == (2, n)
        assert np.array_equal(got, exp[:, :n]), n
        dq = torch.from_numpy(np.ascontiguousarray(q[:n])).to("cuda:0")
        dout = torch.full((2 * n,), 12345, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        ls.probe_dev(dq, n, dout, key_len=16, stream=st.cuda_stream)
        st.synchronize()
        assert np.array_equal(dout.cpu().numpy().view(np.uint32).reshape(2, n), got), n
    assert (exp[0, :400] != NONE).all() and (exp[1, 400:700] != NONE).all()
    # unaligned fixed-length keys (the any-length key source)
    q7 = np.ascontiguousarray(q[:700, :7])
    assert np.array_equal(ls.probe(q7, key_len=7), expected_ids(oracle, rows, [bytes(x) for x in q7]))
    ls.close()
    ctx.close()


@pytest.mark.gpu
def test_lset_row_of_five_thousand_tables(oracle):
    ntab = 5000
    tabs = []
    for t in range(ntab):
        keys = [b"k%07d" % (20 * t + 2 * i) for i in range(8)]  # 8 even ids, then a gap
        tabs.append(build_table(oracle, t ^ 0x5A5A, keys, (8, 0.01)))
    ctx = lsmbloom.Context(0)
    ls = LevelSet(ctx)
    rng = np.random.default_rng(23)
    add_tables(ls, oracle, 0, [tabs[j] for j in rng.permutation(ntab)])
    assert ls.tables(0) == ntab
    ls.seal()
    ids = np.concatenate([rng.integers(0, 20 * ntab + 40, 22_000), 20 * rng.integers(0, ntab, 8_000)])  # + members
    q = [b"k%07d" % i for i in ids]
    got = ls.probe_keys(q)
    exp = expected_ids(oracle, [tabs], q)
    assert got.shape == (1, 30_000)
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:10]
    assert (exp[0, 22_000:] != NONE).all() and (exp == NONE).sum() > 5000
    ls.close()
    ctx.close()


@pytest.mark.gpu
def test_lset_contract(oracle):
    ctx = lsmbloom.Context(0)
    L = lsmbloom.lib()
    a = build_table(oracle, 11, [b"a", b"b", b"c"], (100, 0.01))
    c = build_table(oracle, 22, [b"c", b"d"], (100, 0.01))   # min_key == a's max_key
    e = build_table(oracle, 33, [b"e", b"f"], (100, 0.01))
    ls = LevelSet(ctx)
    with pytest.raises(ValueError):
        ls.probe_keys([b"a"])  # before seal
    with pytest.raises(ValueError):
        ls.probe_keys([])
    add_tables(ls, oracle, 0, [a])
    good = oracle.serialize(a[1], a[2], a[3])
    with pytest.raises(ValueError):
        ls.add(8, 1, good, b"x", b"y")  # row >= 8
    with pytest.raises(ValueError):
        ls.add(0, NONE, good, b"x", b"y")  # the NONE id
    with pytest.raises(ValueError):
        ls.add(0, 1, bytes([7, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]), b"x", b"y")  # num_bits == 0 with k > 0
    with pytest.raises(ValueError):
        ls.add_filter(0, 1, BloomFilter(np.zeros(0, np.uint64), 7, 0), b"x", b"y")
    for bad in (b"", b"\xff\xff\xff\xff", bytes([7, 0, 0, 0, 0xE8, 3, 0, 0, 100, 0, 0, 0]), good + b"extra", good[:-1]):
        with pytest.raises(lsmbloom.Corruption):
            ls.add(0, 1, bad, b"x", b"y")
    assert ls.rows() == 1 and ls.tables(0) == 1  # nothing rejected was kept
    # an empty row (1) between two used rows answers NONE
    add_tables(ls, oracle, 2, [e])
    assert ls.rows() == 3 and ls.tables(1) == 0
    ls.seal()
    ls.seal()  # sealing a sealed set changes nothing
    with pytest.raises(ValueError):
        ls.add(0, 44, good, b"x", b"y")  # after seal
    with pytest.raises(ValueError):
        ls.add_filter(0, 44, BloomFilter(a[1], a[3], a[2]), b"x", b"y")
    q = [b"a", b"b", b"e", b"f", b"g", b""]
    got = ls.probe_keys(q)
    assert np.array_equal(got, expected_ids(oracle, [[a], [], [e]], q))
    assert got[0].tolist() == [11, 11, NONE, NONE, NONE, NONE] and (got[1] == NONE).all()
    assert got[2].tolist()[:2] == [NONE, NONE] and got[2].tolist()[2:4] == [33, 33]
    assert ls.probe_keys([]).shape == (3, 0)  # n = 0
    guard = np.full(4, 777, np.uint32)
    assert L.lsmb_lset_probe(ls.h, None, None, 0, 0, guard.ctypes.data_as(lsmbloom.u32p)) == lsmbloom.LSMB_OK
    assert (guard == 777).all()
    ls.close()
    # an overlapping pair: seal names both tables and leaves the set unsealed
    ls = LevelSet(ctx)
    add_tables(ls, oracle, 3, [e, c, a])
    with pytest.raises(ValueError) as ei:
        ls.seal()
    assert "11" in str(ei.value) and "22" in str(ei.value) and "33" not in str(ei.value)
    with pytest.raises(ValueError):
        ls.probe_keys([b"a"])
    ls.close()
    # a sealed, empty set: no rows, nothing written, LSMB_OK
    ls = LevelSet(ctx)
    ls.seal()
    assert ls.rows() == 0
    assert ls.probe_keys([b"a", b"b"]).shape == (0, 2)
    one = np.zeros(8, np.uint8)
    assert L.lsmb_lset_probe(ls.h, one.ctypes.data_as(lsmbloom.u8p), None, 4, 2,
                             guard.ctypes.data_as(lsmbloom.u32p)) == lsmbloom.LSMB_OK
    assert (guard == 777).all()
    ls.close()
    ctx.close()


@pytest.mark.gpu
def test_lset_agrees_with_a_filter_set_of_64_tables(oracle):
    rng = np.random.default_rng(24)
    tabs = []
    for t in range(64):
        ids = np.sort(rng.choice(100, size=40, replace=False)) + 150 * t
        tabs.append(build_table(oracle, 9000 + t, [b"user%08d" % i for i in ids], (1000, 0.01)))
    ctx = lsmbloom.Context(0)
    fs, ls = FilterSet(ctx), LevelSet(ctx)
    id_of_slot = {}
    for j in rng.permutation(64):
        tid, w, nb, k, lo, hi = tabs[j]
        id_of_slot[fs.add(oracle.serialize(w, nb, k), lo, hi)] = tid
        ls.add(0, tid, oracle.serialize(w, nb, k), lo, hi)
    ls.seal()
    q = [kk for t in tabs for kk in (t[4], t[5])] + [b"user%08d" % i for i in rng.integers(0, 150 * 64 + 100, 6000)]
    masks = fs.probe_keys(q)
    implied = []
    for m in (int(x) for x in masks):
        assert m & (m - 1) == 0  # disjoint ranges: at most one table per key
        implied.append(id_of_slot[m.bit_length() - 1] if m else NONE)
    got = ls.probe_keys(q)
    assert got[0].tolist() == implied
    assert np.array_equal(got, expected_ids(oracle, [tabs], q))
    fs.close()
    ls.close()
    ctx.close()


@pytest.mark.gpu
def test_cpp_mirror_level_set_gpu():
    r = subprocess.run([cpp_bin("lset_test"), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout
