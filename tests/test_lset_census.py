"""The fill census of a resident Version (lsmb_lset_census,
lsmb_lset_version_geometry), the segmented popcount kernel behind it
(k_popcount_segs through lsmb_popcount_segs_dev) and the arithmetic on its
counts (lsmb_fill_fpr, lsmb_fill_keys).

Expected counts come from the test's own words (numpy's unpackbits and sum),
the filters from the CPU oracle, expected orders from the tables themselves,
the arithmetic from Python's math; never from the library.  Every count
comparison is exact equality.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import keygen
import lsmbloom
from lsmbloom import BloomFilter, LevelSet
from lset_support import SST, batch_args, cpp_bin, mk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L0 = lsmbloom.LSMB_LSET_ROW_L0
EINVAL = lsmbloom.LSMB_EINVAL
vp = ctypes.c_void_p
# a word, a 16-byte unit and an odd word count; an SST-sized filter of 9 586 bits; one wave iteration of 4 096 B
# and the item cut of 64 KiB, each +- 1 bit; the batched build's largest table; and last what params(1000, 0.01)
# gives, 9 568 bits
NBITS = [0, 1, 63, 64, 65, 127, 128, 129, 9586, 32767, 32768, 32769, 524287, 524288, 524289, 1310720, 9568]
assert NBITS[-1] == SST[0]


def popcnt(words, nbits):
    """The set bits among bits 0 .. nbits-1 of LE u64 words (or their bytes)."""
    b = np.ascontiguousarray(words).view(np.uint8)
    return int(np.unpackbits(b[:(nbits + 7) // 8], bitorder="little")[:nbits].sum(dtype=np.uint64))


# ------------------------------------------------------------- without a GPU

@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan-ubsan"])
def test_popcount_plan_host(tmp_path, san):
    """popcount_segs_ref, popcount_items and popcount_fold of
    csrc/popcount_seg.hpp against a bit-by-bit loop over NBITS, the items
    tiling every table in pieces of at most 64 KiB, 2^32-1 bits planned
    without overflow (tests/cpp/popcount_seg_test.cpp, its own program)."""
    exe = str(tmp_path / "popcount_seg_test")
    src = os.path.join(ROOT, "tests", "cpp", "popcount_seg_test.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + san + ["-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout


def test_cpp_mirror_census_argument_checks():
    r = subprocess.run([cpp_bin("lset_census_test")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


def test_census_entry_points_are_exported_and_reject_null():
    L = lsmbloom.lib()
    for name in ("lsmb_popcount_segs_dev", "lsmb_lset_version_geometry", "lsmb_lset_census", "lsmb_fill_fpr",
                 "lsmb_fill_keys"):
        assert hasattr(L, name) and name in lsmbloom.SIGNATURES
    assert callable(lsmbloom.Context.popcount_segs_dev)
    assert callable(LevelSet.version_geometry) and callable(LevelSet.census)
    assert LevelSet.census.__code__.co_varnames[:2] == ("self", "stream")
    nb = np.full(2, 7, np.uint32)
    kk = np.full(2, 7, np.uint32)
    sb = np.full(2, 7, np.uint64)
    assert L.lsmb_lset_version_geometry(None, nb.ctypes.data_as(lsmbloom.u32p), kk.ctypes.data_as(lsmbloom.u32p)) == EINVAL
    assert L.lsmb_lset_census(None, sb.ctypes.data_as(lsmbloom.u64p), None) == EINVAL
    assert "null" in L.lsmb_last_error().decode()
    assert (nb == 7).all() and (kk == 7).all() and (sb == 7).all()
    assert L.lsmb_popcount_segs_dev(None, vp(16), 1, vp(32), None) == EINVAL
    assert L.lsmb_popcount_segs_dev(None, None, 0, None, None) == EINVAL
    assert L.lsmb_abi_version() == 6


def test_fill_arithmetic_matches_math():
    """Both sides evaluate the same formula in doubles; libm's pow and log
    differ by ulps, hence 1e-12 relative."""
    rng = np.random.default_rng(71)
    cases = [(9586, 7, 4793), (9586, 7, 4967), (64, 1, 1), (64, 1, 63), (1, 3, 1), (2 ** 32 - 1, 7, 2 ** 31),
             (2 ** 32 - 1, 30, 2 ** 32 - 2), (1310720, 7, 655360), (384, 14, 200)]
    for _ in range(200):
        m = int(rng.integers(1, 2 ** 32))
        cases.append((m, int(rng.integers(1, 41)), int(rng.integers(1, m)) if m > 1 else 1))
    for m, k, x in cases:
        fpr, keys = lsmbloom.fill_fpr(m, k, x), lsmbloom.fill_keys(m, k, x)
        e_fpr = math.pow(x / m, k)
        assert abs(fpr - e_fpr) <= 1e-12 * e_fpr, (m, k, x, fpr, e_fpr)
        if x < m:
            e_keys = -(m / k) * math.log(1.0 - x / m)
            assert abs(keys - e_keys) <= 1e-12 * abs(e_keys), (m, k, x, keys, e_keys)
    # half the bits set: 2^-7, and m ln 2 / k keys, the load BloomFilter::new sizes for
    assert lsmbloom.fill_fpr(9586, 7, 4793) == pytest.approx(2.0 ** -7, rel=1e-12)
    assert lsmbloom.fill_keys(9586, 7, 4793) == pytest.approx(9586 / 7 * math.log(2), rel=1e-12)


def test_fill_arithmetic_edges():
    f, g = lsmbloom.fill_fpr, lsmbloom.fill_keys
    # k = 0: may_contain is always true; no count of keys can be told
    assert f(9586, 0, 0) == 1.0 and f(9586, 0, 4000) == 1.0 and f(9586, 0, 9586) == 1.0 and f(0, 0, 0) == 1.0
    assert math.isnan(g(9586, 0, 4000)) and math.isnan(g(0, 0, 0))
    # X = 0: an empty filter
    assert f(9586, 7, 0) == 0.0 and g(9586, 7, 0) == 0.0 and math.copysign(1.0, g(9586, 7, 0)) == 1.0
    # X = m: a full one
    assert f(9586, 7, 9586) == 1.0 and g(9586, 7, 9586) == math.inf
    assert f(1, 3, 1) == 1.0 and g(1, 3, 1) == math.inf
    # X > m: no such filter
    assert math.isnan(f(9586, 7, 9587)) and math.isnan(g(9586, 7, 9587))
    assert math.isnan(f(9586, 0, 9587)) and math.isnan(f(0, 0, 1)) and math.isnan(f(64, 7, 2 ** 63))


# ----------------------------------------------------------------- the kernel

SMALL = NBITS[:12]  # up to 32 769 bits: the many segments of the 4 097 case


@pytest.mark.gpu
@pytest.mark.parametrize("nbits", [[], [9586], [129, 0, 32769, 1, 524289], (SMALL * 340)[:4080] + NBITS],
                         ids=["0", "1", "5", "4097"])
def test_popcount_kernel_counts_every_segment_below_nbits_and_nothing_else(nbits):
    """Random words, so the bits at and above nbits of a last word are mostly
    ones; 16 bytes of ones after every segment (the pad word of an arena slot
    and its neighbour); sources at varied 16-byte offsets; d_out between guard
    words; 1, 5 and 4 097 segments each leave three idle waves in the last
    workgroup, and the last holds every size of NBITS."""
    import torch

    nseg = len(nbits)
    assert nseg in (0, 1, 5, 4097) and (nseg < 4097 or set(nbits) == set(NBITS))
    off, at = [], 16
    for i, nb in enumerate(nbits):
        at += 16 * (i % 4)  # varied 16-byte offsets, the segments not back to back
        off.append(at)
        at = (at + (nb + 63) // 64 * 8 + 16 + 15) // 16 * 16
    src_h = keygen.stream_bytes(0x5EEDCE25 + nseg, at + 64)
    exp = np.zeros(nseg, np.uint64)
    for s, (a, nb) in enumerate(zip(off, nbits)):
        n = (nb + 63) // 64 * 8
        exp[s] = popcnt(src_h[a:a + n], nb)
        src_h[a + n:a + n + 16] = 0xFF
        if nb % 64:
            assert popcnt(src_h[a:a + n + 16], n * 8 + 128) > exp[s]  # a kernel that does not mask counts more
    if nseg == 4097:
        assert exp[-2] > 600000 and exp[4080] == 0
    src = torch.from_numpy(src_h).to("cuda:0")
    GUARD = 0x5A5A5A5A5A5A5A5A
    out = torch.full((nseg + 8,), GUARD, dtype=torch.int64, device="cuda:0")
    assert src.data_ptr() % 16 == 0
    pairs = [[src.data_ptr() + a, nb] for a, nb in zip(off, nbits)]
    segs = torch.tensor(pairs if pairs else [[0, 0]], dtype=torch.int64, device="cuda:0")
    ctx = lsmbloom.Context(0)
    L = lsmbloom.lib()
    assert L.lsmb_popcount_segs_dev(ctx.h, None, 1, vp(out.data_ptr()), None) == EINVAL
    assert L.lsmb_popcount_segs_dev(ctx.h, vp(segs.data_ptr()), 1, None, None) == EINVAL
    st = torch.cuda.Stream("cuda:0")
    torch.cuda.synchronize()
    ctx.popcount_segs_dev(segs, nseg, out[4:], stream=st.cuda_stream)
    st.synchronize()
    got = out.cpu().numpy().view(np.uint64)
    assert (got[:4] == GUARD).all() and (got[4 + nseg:] == GUARD).all()
    bad = np.nonzero(got[4:4 + nseg] != exp)[0]
    assert bad.size == 0, (bad[:10], [nbits[i] for i in bad[:10]], got[4:4 + nseg][bad[:10]], exp[bad[:10]])
    assert np.array_equal(src.cpu().numpy(), src_h)
    ctx.close()


@pytest.mark.gpu
def test_cpp_mirror_census_gpu():
    r = subprocess.run([cpp_bin("lset_census_test"), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout


# ------------------------------------------------------------------ a Version

BIG = 8 * (2 * 65536 + 24) + 5  # above 64 KiB of words: three items, the last of 25 bytes


def _version(oracle):
    """(l0, rows): three L0 tables, a row of five with mixed geometries (one of
    no hash, one of one bit, one of three items) and a row of 300 SST-sized
    ones; every table (table_id, words, num_bits, k, lo, hi)."""
    l0 = [mk(oracle, 9000, 300, *SST), mk(oracle, 9001, 350, 64 * 7, 3), mk(oracle, 9002, 5000, 0, 0)]
    mixed = [mk(oracle, 100, 0, *SST), mk(oracle, 101, 150, 64, 0), mk(oracle, 102, 300, 1, 3),
             mk(oracle, 103, 450, BIG, 7, nkeys=100), mk(oracle, 104, 600, 64 * 151, 7)]
    sst = [mk(oracle, 1000 + t, 150 * t, *SST, nkeys=40 + t % 60) for t in range(300)]
    return l0, [mixed, sst]


def _expected(l0, rows):
    """(ids, num_bits, num_hashes, set_bits) in version_order's order: L0 by
    position, then every row by min_key."""
    order = list(l0) + [t for row in rows for t in sorted(row, key=lambda t: t[4])]
    return (np.array([t[0] for t in order], np.uint32), np.array([t[2] for t in order], np.uint32),
            np.array([t[3] for t in order], np.uint32), np.array([popcnt(t[1], t[2]) for t in order], np.uint64))


def _check_census(ls, exp, what=""):
    ids, nb, kk, sb, fpr, keys = ls.census()
    e_ids, e_nb, e_kk, e_sb = exp
    assert np.array_equal(ids, e_ids) and np.array_equal(ids, ls.version_order()[0]), what
    g_nb, g_kk = ls.version_geometry()
    assert np.array_equal(nb, e_nb) and np.array_equal(g_nb, e_nb), what
    assert np.array_equal(kk, e_kk) and np.array_equal(g_kk, e_kk), what
    assert sb.dtype == np.uint64 and sb.shape == e_sb.shape, what
    bad = np.nonzero(sb != e_sb)[0]
    assert bad.size == 0, (what, bad[:10], ids[bad[:10]], sb[bad[:10]], e_sb[bad[:10]])
    for m, k, x, f, n in zip(e_nb, e_kk, e_sb, fpr, keys):
        m, k, x = int(m), int(k), int(x)
        if k == 0:
            assert f == 1.0 and math.isnan(n), what
        else:
            assert f == pytest.approx(math.pow(x / m, k), rel=1e-12), what
            assert n == (math.inf if x == m else pytest.approx(-(m / k) * math.log(1.0 - x / m), rel=1e-12)), what


def _load(ctx, oracle, l0, rows, stray=None, seed=5):
    """The tables through add_many in a shuffled order (L0 in position order);
    table id `stray` through add_words instead, with ones in every bit of its
    last word at and above num_bits."""
    ls = LevelSet(ctx)
    placed = [(r, t) for r, row in enumerate(rows) for t in row if t[0] != stray]
    rng = np.random.default_rng(seed)
    placed = [placed[int(i)] for i in rng.permutation(len(placed))] + [(L0, t) for t in l0]
    ls.add_many(*batch_args(oracle, placed))
    for r, row in enumerate(rows):
        for t in row:
            if t[0] == stray:
                w = t[1].copy()
                assert t[2] % 64
                w[-1] |= np.uint64((1 << 64) - (1 << (t[2] % 64)))
                assert popcnt(w, t[2]) == popcnt(t[1], t[2]) < popcnt(w, 64 * w.size)
                ls.add_filter(r, t[0], BloomFilter(w, t[3], t[2]), t[4], t[5])
    ls.seal()
    return ls


@pytest.mark.gpu
def test_census_of_a_version_in_version_order(oracle):
    l0, rows = _version(oracle)
    exp = _expected(l0, rows)
    assert exp[3][2] == 0 and exp[1][2] == 0          # the L0 table of no bits
    assert 0 < exp[3][3] < 4000 and exp[1][3] == SST[0]
    ctx = lsmbloom.Context(0)
    L = lsmbloom.lib()
    ls = LevelSet(ctx)
    sb = np.full(4, 7, np.uint64)
    assert L.lsmb_lset_census(ls.h, sb.ctypes.data_as(lsmbloom.u64p), None) == EINVAL  # unsealed
    assert L.lsmb_lset_version_geometry(ls.h, None, None) == EINVAL and (sb == 7).all()
    with pytest.raises(ValueError):
        ls.census()
    ls.seal()  # V == 0
    assert L.lsmb_lset_census(ls.h, None, None) == lsmbloom.LSMB_OK
    assert all(a.size == 0 for a in ls.census())
    ls.close()
    ls = _load(ctx, oracle, l0, rows, stray=1007)
    assert L.lsmb_lset_census(ls.h, None, None) == EINVAL  # null output, V > 0
    before = ls.stats()
    assert before["tables"] == 308 and before["upload_copies"] >= 2
    _check_census(ls, exp, "loaded")
    import torch
    st = torch.cuda.Stream("cuda:0")
    ids, nb, kk, sb2, fpr, keys = ls.census(stream=st.cuda_stream)  # again, on a stream of the caller's
    assert np.array_equal(sb2, exp[3])
    assert ls.stats() == before  # [2] uploaded_bytes and [3] upload_copies among them
    by_id = dict(zip(ids.tolist(), sb2.tolist()))
    assert by_id[102] == 1 and by_id[101] == 0 and by_id[9002] == 0
    assert by_id[103] == popcnt(rows[0][3][1], BIG) > 300
    ls.close()
    ctx.close()


@pytest.mark.gpu
def test_census_after_version_edits(oracle):
    """A derive child (shared words), a derive_packed(REPACK_ALL) child (moved
    words) and a set filled by build_batch_dev + add_built (words that never
    crossed the host) each answer their own tables' counts; the parent's
    census is the same after its children are closed."""
    import torch

    l0, rows = _version(oracle)
    rows = [rows[0], rows[1][:40]]
    ctx = lsmbloom.Context(0)
    parent = _load(ctx, oracle, l0, rows, stray=1003)
    exp = _expected(l0, rows)
    _check_census(parent, exp, "parent")
    first = parent.census()[3].copy()
    drops = [103, 1005, 9001, 1039]
    new = mk(oracle, 7777, 150 * 50, 64 * 9 + 1, 11)
    c_l0 = [t for t in l0 if t[0] not in drops]
    c_rows = [[t for t in row if t[0] not in drops] for row in rows]
    c_rows[1] = c_rows[1] + [new]
    c_exp = _expected(c_l0, c_rows)
    children = []
    for what, repack in (("derive", None), ("derive_packed", "all")):
        ch = parent.derive(drops, repack=repack)
        assert ch.dropped == 4 and (ch.moved[0] == 44 if repack else ch.moved == (0, 0))
        ch.add_many(*batch_args(oracle, [(1, new)]))
        ch.seal()
        _check_census(ch, c_exp, what)
        children.append(ch)
    _check_census(parent, exp, "parent, its children alive")
    for ch in children:
        ch.close()
    assert np.array_equal(parent.census()[3], first)
    # the packed child after its parent is closed
    ch = parent.derive(drops, repack="all")
    ch.add_many(*batch_args(oracle, [(1, new)]))
    ch.seal()
    parent.close()
    _check_census(ch, c_exp, "derive_packed, the parent closed")
    ch.close()
    # filters built on the device and routed in device to device
    geoms = [SST, (64, 1), (16385, 7), SST, (65, 40), SST]
    tabs = []
    for j, (nb, k) in enumerate(geoms):
        ks = [b"user%08d" % i for i in range(150 * j, 150 * j + 40 + 13 * j)]
        d, o = keygen.pack(ks)
        tabs.append((600 + j, oracle.build_var(d, o, nb, k), nb, k, ks[0], ks[-1], ks))
    run = [k for t in tabs for k in t[6]]
    data, offs = keygen.pack(run)
    seg = np.zeros(len(tabs) + 1, np.uint64)
    np.cumsum([len(t[6]) for t in tabs], out=seg[1:])
    nbs, kks = [t[2] for t in tabs], [t[3] for t in tabs]
    d_data = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to("cuda:0")
    d_offs = torch.from_numpy(offs.view(np.int64)).to("cuda:0")
    words = torch.full((int(lsmbloom.build_batch_layout(nbs)[-1]),), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.build_batch_dev(d_data, len(run), seg, nbs, kks, words, offsets=d_offs)
    built = LevelSet(ctx)
    built.add_built([L0 if j == 4 else 0 for j in range(6)], [t[0] for t in tabs], words, nbs, kks,
                    [(t[4], t[5]) for t in tabs])
    del words
    built.seal()
    assert built.stats()["uploaded_bytes"] == 0
    _check_census(built, _expected([tabs[4][:6]], [[t[:6] for j, t in enumerate(tabs) if j != 4]]), "add_built")
    built.close()
    ctx.close()


@pytest.mark.gpu
def test_a_saturated_table_is_visible(oracle):
    """A filter of 9 586 bits and k = 7 (params(1000, 0.01) itself gives
    9 568 bits and k = 7: the same filter to three digits).  At 1 000 keys the
    expected fill is 1 - exp(-7 * 1000 / 9586) = 0.518, so the predicted rate
    is 0.518^7 = 0.0100, inside [0.005, 0.02]; with 20 000 keys the expected
    fill is 1 - exp(-14.6), a rate above 0.9.  The key count the fill gives
    back has a standard deviation of about 8 keys at 1 000 (27.7 bits of the
    fill's, over 7 * 0.482), so 5 % is six of them."""
    nb, k = 9586, 7
    tabs = []
    for tid, first, n in ((1, 0, 20000), (2, 50000, 1000)):
        ks = [b"user%08d" % i for i in range(first, first + n)]
        d, o = keygen.pack(ks)
        tabs.append((tid, oracle.build_var(d, o, nb, k), nb, k, ks[0], ks[-1]))
    ctx = lsmbloom.Context(0)
    ls = LevelSet(ctx)
    ls.add_many(*batch_args(oracle, [(0, t) for t in tabs]))
    ls.seal()
    ids, g_nb, g_k, sb, fpr, keys = ls.census()
    assert ids.tolist() == [1, 2] and g_nb.tolist() == [nb, nb] and g_k.tolist() == [k, k]
    assert sb.tolist() == [popcnt(t[1], nb) for t in tabs]
    print("fill %s of %d bits, fpr %s, keys %s" % (sb.tolist(), nb, fpr.tolist(), keys.tolist()))
    assert fpr[0] > 0.9
    assert 0.005 <= fpr[1] <= 0.02
    assert abs(keys[1] - 1000) <= 50
    assert keys[0] > 5 * 1000  # several times the estimate: a table to rewrite
    ls.close()
    ctx.close()
