"""Per-table candidate key lists of a filter set (lsmb_fset_probe_lists*): the
probe's answer transposed, for a reader that works table by table.

    index[starts[s] : starts[s+1]] = the ascending indices i of the keys with
    (min_s <= key i <= max_s) && may_contain(filter s, key i)

Expected lists come from the CPU oracle's may_contain and Python's bytes
ordering (expected_masks, as tests/test_fset.py) through lists_from_masks;
every GPU test also holds the lists against the set's own mask probe.
"""
import ctypes
import subprocess

import numpy as np
import pytest

import keygen
import lset_support
import lsmbloom
from lsmbloom import BloomFilter, FilterSet
from lset_support import check_mask_lists as check_lists, cpp_bin, lists_from_masks

vp = ctypes.c_void_p


def expected_masks(oracle, tables, keys):
    """tables: {slot: (words, num_bits, k, lo, hi)} -> uint64 mask per key."""
    return np.array(lset_support.expected_masks(oracle, tables, keys), dtype=np.uint64)


def sst_tables(oracle, ntab, per, seed):
    """As tests/test_fset.py::sst_tables: ntab SSTable-like runs of `per` sorted
    keys (overlapping ranges for even tables, disjoint for odd ones), filters
    sized as SSTableBuilder::with_estimated_keys(per)."""
    rng = np.random.default_rng(seed)
    tabs = []
    for t in range(ntab):
        base = t * 10_000 if t % 2 else (t // 2) * 3_000
        ids = np.sort(rng.choice(20_000, size=per, replace=False)) + base
        keys = [b"user%08d" % i for i in ids]
        nb, k = lsmbloom.params(per, 0.01)
        data, offs = keygen.pack(keys)
        w = oracle.build_var(data, offs, nb, k)
        tabs.append((keys, w, nb, k))
    return tabs


# ---------------------------------------------------------------- without a GPU

def test_lists_entry_points_reject_a_null_set():
    L = lsmbloom.lib()
    starts = np.zeros(65, np.uint64)
    index = np.zeros(4, np.uint32)
    data = np.zeros(4, np.uint8)
    assert L.lsmb_fset_probe_lists(None, data.ctypes.data_as(lsmbloom.u8p), None, 1, 4,
                                   starts.ctypes.data_as(lsmbloom.u64p), index.ctypes.data_as(lsmbloom.u32p),
                                   4) == lsmbloom.LSMB_EINVAL
    assert L.lsmb_fset_probe_lists_dev(None, vp(1), None, 1, 4, vp(1), vp(1), 4, None) == lsmbloom.LSMB_EINVAL


def test_lists_entry_points_are_in_the_signature_table():
    c = ctypes
    assert lsmbloom.SIGNATURES["lsmb_fset_probe_lists_dev"] == (
        c.c_int, [vp, vp, vp, c.c_uint32, c.c_uint64, vp, vp, c.c_uint64, vp])
    assert lsmbloom.SIGNATURES["lsmb_fset_probe_lists"] == (
        c.c_int, [vp, lsmbloom.u8p, lsmbloom.u64p, c.c_uint32, c.c_uint64, lsmbloom.u64p, lsmbloom.u32p, c.c_uint64])
    for name in ("lsmb_fset_probe_lists_dev", "lsmb_fset_probe_lists"):
        assert hasattr(lsmbloom.lib(), name)


def test_lists_from_masks_on_a_hand_written_example():
    # key 0 in table 0; key 1 in tables 0 and 5; key 2 nowhere; key 3 in table 63; key 4 in table 5
    masks = [1, (1 << 5) | 1, 0, 1 << 63, 1 << 5]
    starts, index = lists_from_masks(masks)
    assert index.tolist() == [0, 1, 1, 4, 3]
    assert starts.tolist() == [0] + [2] * 5 + [4] * 58 + [5]
    assert starts.dtype == np.uint64 and index.dtype == np.uint32
    s0, i0 = lists_from_masks([])
    assert s0.tolist() == [0] * 65 and i0.size == 0


def test_cpp_mirror_lists_argument_checks():
    r = subprocess.run([cpp_bin("fset_lists_test")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


# ------------------------------------------------------------------- on the GPU

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 70_001]


class Sst8:
    """One set of 8 SST-sized tables in slots 0..7 (one-byte mask rows) and
    70 001 var-len queries with their oracle masks, shared by the tests below;
    a test's n keys are the first n."""

    def __init__(self, oracle):
        self.ctx = lsmbloom.Context(0)
        self.fs = FilterSet(self.ctx)
        tabs = sst_tables(oracle, 8, 1000, 7)
        self.tables = {}
        for keys, w, nb, k in tabs:
            s = self.fs.add(oracle.serialize(w, nb, k), keys[0], keys[-1])
            self.tables[s] = (w, nb, k, keys[0], keys[-1])
        assert self.fs.live_mask() == 0xFF
        rng = np.random.default_rng(23)
        q = [kk for keys, *_ in tabs for kk in keys]                                      # members
        q += [keys[0] for keys, *_ in tabs] + [keys[-1] for keys, *_ in tabs]             # the bounds themselves
        q += [b"user%08d" % i for i in rng.integers(0, 90_000, max(SIZES) - len(q))]      # mostly absent
        self.q = [q[i] for i in rng.permutation(len(q))]
        assert len(self.q) == max(SIZES)
        self.masks = expected_masks(oracle, self.tables, self.q)

    def close(self):
        self.fs.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def sst8(oracle):
    s = Sst8(oracle)
    yield s
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_lists_sizes_around_every_boundary(sst8, n):
    """n around a wave (64), the chunk group of one wave (256), a tile (1024),
    several tiles (the cross-tile scan, whose step is 256 tiles) and a tail."""
    q, masks = sst8.q[:n], sst8.masks[:n]
    got = sst8.fs.probe_lists_keys(q)
    check_lists(got, masks, "oracle")
    check_lists(got, sst8.fs.probe_keys(q), "mask probe")
    if n >= 1024:
        assert masks.any() and int(got[0][64]) > 0


@pytest.mark.gpu
def test_lists_slot_placement(oracle, sst8):
    """Live slots {0, 5, 63}: 8-byte mask rows, dead slots' runs empty, slot
    63's run right; slots 0..7 (one-byte rows) are the shared set."""
    ctx = lsmbloom.Context(0)
    fs = FilterSet(ctx)
    tabs = sst_tables(oracle, 3, 1000, 31)
    keep = {0: tabs[0], 5: tabs[1], 63: tabs[2]}
    nb0, k0 = lsmbloom.params(1000, 0.01)
    filler = BloomFilter(np.full(lsmbloom.num_words(nb0), ~np.uint64(0), np.uint64), k0, nb0)  # answers "maybe" to all
    tables = {}
    for s in range(64):
        if s in keep:
            keys, w, nb, k = keep[s]
            assert fs.add_filter(BloomFilter(w, k, nb), keys[0], keys[-1]) == s
            tables[s] = (w, nb, k, keys[0], keys[-1])
        else:
            assert fs.add_filter(filler, b"", b"\xff" * 8) == s
    for s in range(64):
        if s not in keep:
            fs.remove(s)
    assert fs.live_mask() == (1 << 0) | (1 << 5) | (1 << 63)
    rng = np.random.default_rng(5)
    q = [kk for keys, *_ in tabs for kk in keys[::2]] + [b"user%08d" % i for i in rng.integers(0, 40_000, 1500)]
    q = [q[i] for i in rng.permutation(len(q))]
    masks = expected_masks(oracle, tables, q)
    starts, index = got = fs.probe_lists_keys(q)
    check_lists(got, masks, "oracle")
    check_lists(got, fs.probe_keys(q), "mask probe")
    for s in range(64):
        if s not in keep:
            assert starts[s] == starts[s + 1], s
    assert int(starts[64] - starts[63]) >= 500  # table 63's members, after every other run
    assert np.array_equal(index[int(starts[63]):], np.nonzero(masks >> np.uint64(63))[0])
    fs.close()
    ctx.close()
    # slots 0..7: one-byte rows
    assert sst8.fs.live_mask() == 0xFF
    check_lists(sst8.fs.probe_lists_keys(sst8.q[:3000]), sst8.masks[:3000], "one-byte rows")


@pytest.mark.gpu
def test_lists_densest_and_emptiest(oracle):
    ctx = lsmbloom.Context(0)
    fs = FilterSet(ctx)
    rng = np.random.default_rng(41)
    keys = sorted(b"user%08d" % i for i in rng.choice(50_000, size=3000, replace=False))
    nb, k = lsmbloom.params(1000, 0.01)
    data, offs = keygen.pack(keys)
    w = oracle.build_var(data, offs, nb, k)
    tables = {}
    for _ in range(4):
        s = fs.add_filter(BloomFilter(w, k, nb), keys[0], keys[-1])
        tables[s] = (w, nb, k, keys[0], keys[-1])
    n = len(keys)
    # every table lists every key: 4 n entries, more than the default capacity of n
    starts, index = got = fs.probe_lists_keys(keys)
    assert starts.tolist() == [0, n, 2 * n, 3 * n] + [4 * n] * 61
    assert np.array_equal(index, np.tile(np.arange(n, dtype=np.uint32), 4))
    check_lists(got, expected_masks(oracle, tables, keys), "oracle")
    check_lists(got, fs.probe_keys(keys), "mask probe")
    # keys above every max_key: nothing
    above = [b"zzzz%08d" % i for i in range(n)]
    starts, index = got = fs.probe_lists_keys(above)
    assert starts.tolist() == [0] * 65 and index.size == 0
    check_lists(got, expected_masks(oracle, tables, above), "oracle")
    check_lists(got, fs.probe_keys(above), "mask probe")
    fs.close()
    ctx.close()


@pytest.mark.gpu
def test_lists_truncation(sst8):
    """cap < total: starts still exact, entries [0, cap) are the prefix, nothing
    at or past cap is written; cap = 0 with a null index counts."""
    import torch

    n = 4097
    q, masks = sst8.q[:n], sst8.masks[:n]
    es, ei = lists_from_masks(masks)
    total = int(es[64])
    assert total >= 64
    cap = total // 2
    data, offs = keygen.pack(q)
    L = lsmbloom.lib()
    # host entry point
    starts = np.full(65, 0xA5A5A5A5, np.uint64)
    index = np.full(total, 0xFFFFFFFF, np.uint32)
    rc = L.lsmb_fset_probe_lists(sst8.fs.h, data.ctypes.data_as(lsmbloom.u8p), offs.ctypes.data_as(lsmbloom.u64p), 0, n,
                                 starts.ctypes.data_as(lsmbloom.u64p), index.ctypes.data_as(lsmbloom.u32p), cap)
    assert rc == 0
    assert np.array_equal(starts, es)
    assert np.array_equal(index[:cap], ei[:cap])
    assert (index[cap:] == 0xFFFFFFFF).all()
    starts0 = np.full(65, 0xA5A5A5A5, np.uint64)
    rc = L.lsmb_fset_probe_lists(sst8.fs.h, data.ctypes.data_as(lsmbloom.u8p), offs.ctypes.data_as(lsmbloom.u64p), 0, n,
                                 starts0.ctypes.data_as(lsmbloom.u64p), None, 0)
    assert rc == 0 and np.array_equal(starts0, es)
    # device entry point: the buffer past cap is the caller's and stays untouched
    dd = torch.from_numpy(data).to("cuda:0")
    do = torch.from_numpy(offs.view(np.int64)).to("cuda:0")
    dstarts = torch.full((65,), -1, dtype=torch.int64, device="cuda:0")
    dindex = torch.full((total,), -1, dtype=torch.int32, device="cuda:0")
    sst8.fs.probe_lists_dev(dd, n, dstarts, dindex[:cap], offsets=do)
    torch.cuda.synchronize()
    assert np.array_equal(dstarts.cpu().numpy().view(np.uint64), es)
    got = dindex.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:cap], ei[:cap])
    assert (got[cap:] == 0xFFFFFFFF).all()
    dstarts.fill_(-1)
    sst8.fs.probe_lists_dev(dd, n, dstarts, None, offsets=do)
    torch.cuda.synchronize()
    assert np.array_equal(dstarts.cpu().numpy().view(np.uint64), es)


def _key16_set(oracle, fs, sizes, seed):
    """Tables of 16-B keys, table t sized new(sizes[t], .01) -> (tables, member keys)."""
    tables, members = {}, []
    for t, sized in enumerate(sizes):
        nk = 200_000 if sized >= 10**9 else min(sized, 1000)
        keys = keygen.key16(seed + t, 0, nk)
        rows = sorted(bytes(r) for r in keys)
        nb, k = lsmbloom.params(sized, 0.01)
        w = oracle.build_fixed(keys, 16, nb, k)
        lo, hi = rows[len(rows) // 8], rows[-1 - len(rows) // 8]
        s = fs.add_filter(BloomFilter(w, k, nb), lo, hi)
        tables[s] = (w, nb, k, lo, hi)
        members.append(keys[:700])
    return tables, members


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [(1000,) * 8, (1000, 4000) * 2, (10**9, 5000, 1000)],
                         ids=["same-size", "two-classes", "saturated-mixed"])
def test_lists_fixed_keys_on_every_probe_kernel(oracle, sizes):
    """16-B keys (Fixed16) and key_len = 7 (FixedN) into the same-size sliced
    kernel, the size-class kernel, and the L2 walk next to a 2^32-1-bit
    filter: whichever probe writes the rows, the lists are their transpose.
    (Var-len keys go through probe_lists_keys in the tests above.)"""
    ctx = lsmbloom.Context(0)
    fs = FilterSet(ctx)
    tables, members = _key16_set(oracle, fs, sizes, 0x5EED0900)
    q = np.concatenate(members + [keygen.key16(0x5EED0A00, 0, 3001)])
    q = np.ascontiguousarray(q[np.random.default_rng(3).permutation(q.shape[0])])
    got = fs.probe_lists(q, key_len=16)
    masks = expected_masks(oracle, tables, [bytes(r) for r in q])
    assert masks.any()
    check_lists(got, masks, "oracle, 16-B keys")
    check_lists(got, fs.probe(q, key_len=16), "mask probe, 16-B keys")
    q7 = np.ascontiguousarray(q[:2500, :7])
    got7 = fs.probe_lists(q7, key_len=7)
    check_lists(got7, expected_masks(oracle, tables, [bytes(r) for r in q7]), "oracle, 7-B keys")
    check_lists(got7, fs.probe(q7, key_len=7), "mask probe, 7-B keys")
    fs.close()
    ctx.close()


@pytest.mark.gpu
def test_lists_more_tiles_than_one_scan_step(oracle):
    """300 001 keys are 293 tiles: the scan over tiles takes 256 a step, so
    its carry between steps and its partial last step decide every start past
    the first 262 144 keys.  Every range holds every key here, so the oracle's
    probe alone gives the masks."""
    ctx = lsmbloom.Context(0)
    fs = FilterSet(ctx)
    nb, k = lsmbloom.params(1000, 0.01)
    n = 300_001
    q = keygen.key16(0x5EED0D00, 0, n)
    masks = np.zeros(n, np.uint64)
    for t in range(8):
        keys = np.ascontiguousarray(q[t * 30_000:t * 30_000 + 1000])  # members spread over the tiles' range
        w = oracle.build_fixed(keys, 16, nb, k)
        s = fs.add_filter(BloomFilter(w, k, nb), b"", b"\xff" * 17)
        masks |= oracle.probe([(w, nb, k)], q, key_len=16)[:, 0].astype(np.uint64) << np.uint64(s)
    got = fs.probe_lists(q, key_len=16)
    assert int(got[0][64]) >= 8000
    check_lists(got, masks, "oracle")
    check_lists(got, fs.probe(q, key_len=16), "mask probe")
    fs.close()
    ctx.close()


@pytest.mark.gpu
def test_lists_device_entry_point_and_streams(oracle):
    """probe_lists_dev on device keys equals the host call; then lists probes
    on 5 streams share the set's scratch (each waits for the one before it)
    across 3 rounds with an add and a remove between rounds."""
    import torch

    ctx = lsmbloom.Context(0)
    fs = FilterSet(ctx)
    tables, members = _key16_set(oracle, fs, (1000,) * 8, 0x5EED0B00)
    q = np.concatenate(members + [keygen.key16(0x5EED0C00, 0, 4401)])
    q = np.ascontiguousarray(q[np.random.default_rng(9).permutation(q.shape[0])])
    n = q.shape[0]
    masks = expected_masks(oracle, tables, [bytes(r) for r in q])
    es, ei = lists_from_masks(masks)
    total = int(es[64])
    host = fs.probe_lists(q, key_len=16)
    check_lists(host, masks, "oracle")
    check_lists(host, fs.probe(q, key_len=16), "mask probe")
    dq = torch.from_numpy(q).to("cuda:0")
    dstarts = torch.full((65,), -1, dtype=torch.int64, device="cuda:0")
    dindex = torch.full((total + 16,), -1, dtype=torch.int32, device="cuda:0")  # (the tables share keys: total > n)
    fs.probe_lists_dev(dq, n, dstarts, dindex, key_len=16)
    torch.cuda.synchronize()
    assert np.array_equal(dstarts.cpu().numpy().view(np.uint64), host[0])
    assert np.array_equal(dindex.cpu().numpy().view(np.uint32)[:total], host[1])
    streams = [torch.cuda.Stream("cuda:0") for _ in range(5)]
    outs = [(torch.full_like(dstarts, -1), torch.full_like(dindex, -1)) for _ in streams]
    w0, nb0, k0 = tables[0][:3]
    for rep in range(3):
        for st, (s_out, i_out) in zip(streams, outs):
            fs.probe_lists_dev(dq, n, s_out, i_out, key_len=16, stream=st.cuda_stream)
        extra = fs.add_filter(BloomFilter(w0, k0, nb0), b"", b"")  # empty-range table: no key is in it
        fs.remove(extra)
    torch.cuda.synchronize()
    for s_out, i_out in outs:
        assert np.array_equal(s_out.cpu().numpy().view(np.uint64), es)
        got = i_out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:total], ei)
        assert (got[total:] == 0xFFFFFFFF).all()
    fs.close()
    ctx.close()


@pytest.mark.gpu
def test_lists_empty_set_and_no_keys():
    import torch

    ctx = lsmbloom.Context(0)
    fs = FilterSet(ctx)
    starts, index = fs.probe_lists_keys([b"a", b"b"])  # empty set
    assert starts.tolist() == [0] * 65 and index.size == 0
    dq = torch.zeros(32, dtype=torch.uint8, device="cuda:0")
    dstarts = torch.full((65,), -1, dtype=torch.int64, device="cuda:0")
    fs.probe_lists_dev(dq, 2, dstarts, None, key_len=16)
    torch.cuda.synchronize()
    assert dstarts.cpu().tolist() == [0] * 65
    dstarts.fill_(-1)
    fs.probe_lists_dev(dq, 0, dstarts, None, key_len=16)
    torch.cuda.synchronize()
    assert dstarts.cpu().tolist() == [0] * 65
    with pytest.raises(ValueError):
        fs.probe_lists_dev(dq, 1 << 32, dstarts, None, key_len=16)  # indices are 32-bit
    fs.close()
    ctx.close()


@pytest.mark.gpu
def test_cpp_mirror_lists_gpu():
    r = subprocess.run([cpp_bin("fset_lists_test"), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout
