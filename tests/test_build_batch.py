"""The batched build: many SSTable filters from one key run in one launch per
geometry class (lsmb_build_batch_*: src/sstable/builder.rs:74,93,177-182 for
every output table of src/compaction/scheduler.rs:147-177), and the
device-to-device route of the built words into a level set
(lsmb_lset_add_batch_dev).

Without a GPU: the plan, the layout and build_batch_ref
(csrc/build_batch_plan.hpp) on the CPU under ASan and UBSan, the layout
against a restatement of the arena's slot rule, and the argument checks.  On
the GPU: every filter word against the CPU oracle's build of the segment
(exact equality), serialized blocks against the oracle's serialize, and probe
answers against a second level set loaded from oracle-serialized blocks.
"""
import ctypes
import os
import subprocess
import zlib

import numpy as np
import pytest

import keygen
import lsmbloom
from lsmbloom import LevelSet, u8p, u32p, u64p
from lset_support import cpp_bin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = lsmbloom.LSMB_EINVAL
vp = ctypes.c_void_p
SST = lsmbloom.params(1000, 0.01)  # SSTableBuilder's filter: (9586, 7)
WAVE_MAX = 65536                   # kBbWaveMaxBits (csrc/build_batch_plan.hpp): the wave class's largest filter
COUNTS = (0, 1, 63, 64, 65, 1000)
BITS = (64, 65, 9586, 16383, 16384, 16385, WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1, 1310720)
KS = (0, 1, 7, 40)


def p(a, t):
    return a.ctypes.data_as(t)


def slot_words(num_bits):
    """The arena's slot rule restated (lset_slot_bytes in lset_arena.hpp, arena_chunks of
    tests/test_lset_versions.py): max(words * 8, 8) bytes rounded up to 16."""
    nw = (num_bits + 63) // 64
    return (max(nw * 8, 8) + 15) // 16 * 16 // 8


def _has_gpu():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


# ---------------------------------------------------------------- without a GPU

def test_plan_layout_and_reference_build_host(tmp_path):
    """tests/cpp/build_batch_plan_test.cpp: the items of every table partition
    its keys exactly once, every class within its LDS, slots 16-byte aligned
    and disjoint, build_batch_ref over 16-byte and 1..300-byte keys equal to a
    literal per-key insert loop; a stand-alone program under ASan and UBSan."""
    exe = str(tmp_path / "build_batch_plan_test")
    src = os.path.join(ROOT, "tests", "cpp", "build_batch_plan_test.cpp")
    # the plan header compiles the library's xxh3.hpp / bloom_math.hpp for the host: they include the
    # HIP headers (for __host__ __device__) and carry `#pragma unroll` for the device compiler
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout


def test_layout_equals_the_arena_slot_rule():
    rng = np.random.default_rng(41)
    nb = np.concatenate([np.array([0, 1, 63, 64, 65, 127, 128, 129, 9586, 1310720, 2**32 - 1], dtype=np.uint64),
                         rng.integers(0, 1 << 21, 300, dtype=np.uint64)]).astype(np.uint32)
    woff = lsmbloom.build_batch_layout(nb)
    exp = np.zeros(nb.size + 1, dtype=np.uint64)
    np.cumsum([slot_words(int(b)) for b in nb], out=exp[1:])
    assert np.array_equal(woff, exp)
    assert all(int(w) % 2 == 0 for w in woff)  # 16-byte-aligned slots
    assert np.array_equal(lsmbloom.build_batch_layout([]), np.zeros(1, np.uint64))
    assert lsmbloom.build_batch_max_bits() == 1310720 == 40 * 1024 * 32


def test_parts_at_least_one_and_non_decreasing():
    for nb in BITS + (0,):
        last = 1
        for keys in list(range(0, 70)) + list(range(70, 400000, 1009)) + [2**40, 2**64 - 1]:
            parts = lsmbloom.build_batch_parts(keys, nb)
            assert parts >= last >= 1, (nb, keys)
            last = parts
        assert lsmbloom.build_batch_parts(1000, nb) == 1  # an SSTable's keys are one item
    assert lsmbloom.build_batch_parts(10**6, SST[0]) >= 2


def test_entry_points_are_exported_and_reject_null():
    L = lsmbloom.lib()
    for name in ("lsmb_build_batch_max_bits", "lsmb_build_batch_layout", "lsmb_build_batch_parts",
                 "lsmb_build_batch_dev", "lsmb_build_batch_blocks", "lsmb_lset_add_batch_dev"):
        assert hasattr(L, name) and name in lsmbloom.SIGNATURES
    assert callable(lsmbloom.Context.build_batch_dev) and callable(lsmbloom.Context.build_batch_blocks)
    assert callable(LevelSet.add_built)
    nb = np.array([64, SST[0]], np.uint32)
    kk = np.array([1, 7], np.uint32)
    seg = np.array([0, 3, 10], np.uint64)
    woff = np.full(3, 7, np.uint64)
    boff = np.full(3, 7, np.uint64)
    blocks = np.full(2048, 0xAB, np.uint8)
    keys = np.zeros(160, np.uint8)
    fake = vp(0x1000)  # never dereferenced: every call below fails its checks first
    # layout: null outputs / inputs
    assert L.lsmb_build_batch_layout(2, p(nb, u32p), None) == EINVAL
    assert L.lsmb_build_batch_layout(2, None, p(woff, u64p)) == EINVAL and (woff == 7).all()
    # device build: null context, then null arguments, a descending seg, seg past n, a short buffer,
    # a misaligned buffer, a table of no bits with k > 0 and a table past the limit
    dev = lambda c, sg=seg, b=nb, k=kk, w=vp(0x2000), cap=1 << 20, n=10: L.lsmb_build_batch_dev(  # noqa: E731
        c, vp(0x3000), None, 16, n, 2, None if sg is None else p(sg, u64p), None if b is None else p(b, u32p),
        None if k is None else p(k, u32p), w, cap, None)
    assert dev(None) == EINVAL
    assert dev(fake, sg=None) == EINVAL and dev(fake, b=None) == EINVAL and dev(fake, k=None) == EINVAL
    assert dev(fake, w=None) == EINVAL
    assert dev(fake, sg=np.array([0, 5, 4], np.uint64)) == EINVAL
    assert dev(fake, n=9) == EINVAL
    assert dev(fake, cap=int(lsmbloom.build_batch_layout(nb)[-1]) - 1) == EINVAL
    assert dev(fake, w=vp(0x2008)) == EINVAL
    assert dev(fake, b=np.array([0, SST[0]], np.uint32)) == EINVAL
    assert dev(fake, b=np.array([64, 1310721], np.uint32)) == EINVAL
    assert b"table 1" in L.lsmb_last_error()
    # blocks: no host fallback (ten keys are far below lsmb_host_max_keys), outputs untouched
    blk = lambda c, bo=boff, sg=seg: L.lsmb_build_batch_blocks(  # noqa: E731
        c, p(keys, u8p), None, 16, 10, 2, p(sg, u64p), p(nb, u32p), p(kk, u32p), p(blocks, u8p), blocks.size,
        None if bo is None else p(bo, u64p))
    assert blk(None) == EINVAL and (boff == 7).all() and (blocks == 0xAB).all()
    assert blk(fake, bo=None) == EINVAL
    assert blk(fake, sg=np.array([0, 5, 4], np.uint64)) == EINVAL and (boff == 7).all() and (blocks == 0xAB).all()
    # a too-small blocks buffer still learns the size
    rc = L.lsmb_build_batch_blocks(fake, p(keys, u8p), None, 16, 10, 2, p(seg, u64p), p(nb, u32p), p(kk, u32p),
                                   p(blocks, u8p), 100, p(boff, u64p))
    assert rc == EINVAL and (blocks == 0xAB).all()
    assert list(boff) == [0, lsmbloom.serialized_size(64), lsmbloom.serialized_size(64) + lsmbloom.serialized_size(SST[0])]
    # level set: null set
    assert L.lsmb_lset_add_batch_dev(None, 2, p(nb, u32p), p(nb, u32p), vp(0x2000), p(woff, u64p), p(nb, u32p),
                                     p(kk, u32p), p(keys, u8p), p(woff, u64p), None) == EINVAL


def test_batched_build_needs_a_device():
    """No fallback: without a device lsmb_open fails (LSMB_ENODEV), and the
    batched host entry point refuses a NULL context whatever the key count."""
    try:
        ctx = lsmbloom.Context(0)
    except lsmbloom.LsmbError as e:
        assert e.code == lsmbloom.LSMB_ENODEV and not _has_gpu()
    else:
        assert _has_gpu()
        ctx.close()
    L = lsmbloom.lib()
    nb, kk, seg = np.array([SST[0]], np.uint32), np.array([7], np.uint32), np.array([0, 1], np.uint64)
    keys, boff, out = np.zeros(16, np.uint8), np.zeros(2, np.uint64), np.zeros(4096, np.uint8)
    assert L.lsmb_build_batch_blocks(None, p(keys, u8p), None, 16, 1, 1, p(seg, u64p), p(nb, u32p), p(kk, u32p),
                                     p(out, u8p), out.size, p(boff, u64p)) == EINVAL
    assert not out.any()




def test_cpp_mirror_build_batch_argument_checks():
    r = subprocess.run([cpp_bin("build_batch_test")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


# ---------------------------------------------------------------- on the GPU

GUARD = 64  # u64 words after the packed buffer


def run_batch(ctx, data, offs, key_len, n, seg, nb, kk, words=None):
    """One lsmb_build_batch_dev over host keys copied to the device -> (the
    packed words and the guard after them as uint64, the device tensor)."""
    import torch
    dev = torch.device("cuda:0")
    total = int(lsmbloom.build_batch_layout(nb)[-1])
    d_data = torch.from_numpy(np.concatenate([np.ascontiguousarray(data, np.uint8).reshape(-1),
                                              np.zeros(16, np.uint8)])).to(dev)
    d_offs = None if offs is None else torch.from_numpy(np.ascontiguousarray(offs, np.uint64).view(np.int64)).to(dev)
    if words is None:
        words = torch.full((total + GUARD,), -1, dtype=torch.int64, device=dev)  # every byte 0xFF
    torch.cuda.synchronize()
    woff = ctx.build_batch_dev(d_data, n, seg, nb, kk, words[:total], offsets=d_offs, key_len=key_len)
    torch.cuda.synchronize()
    return words.cpu().numpy().view(np.uint64), woff, words


def check_words(oracle, got, woff, tables, what=""):
    """tables: [(data, offs or None, num_bits, k)] per table, the oracle's input."""
    for t, (data, offs, nb, k) in enumerate(tables):
        nw = (nb + 63) // 64
        if nw == 0:
            continue
        n = (offs.size - 1) if offs is not None else data.size // 16
        if n == 0:
            exp = np.zeros(nw, np.uint64)
        elif offs is not None:
            exp = oracle.build_var(data, offs, nb, k)
        else:
            exp = oracle.build_fixed(data, 16, nb, k)
        w = got[int(woff[t]):int(woff[t]) + nw]
        assert np.array_equal(w, exp), (what, t, n, nb, k, int(np.count_nonzero(w != exp)))


@pytest.mark.gpu
def test_small_and_ragged_tables_from_one_run(oracle):
    """Six new(1000, 0.01) tables of 0, 1, 63, 64, 65 and 1 000 16-byte keys,
    unclaimed keys on both sides, a buffer of 0xFF and a guard after it."""
    before, after = 5, 3
    n = before + sum(COUNTS) + after
    keys = keygen.key16(0x5EEDBB01, 0, n)
    seg = np.zeros(len(COUNTS) + 1, np.uint64)
    seg[0] = before
    seg[1:] = before + np.cumsum(COUNTS)
    nb, kk = [SST[0]] * len(COUNTS), [SST[1]] * len(COUNTS)
    ctx = lsmbloom.Context(0)
    got, woff, _ = run_batch(ctx, keys, None, 16, n, seg, nb, kk)
    ctx.close()
    total = int(woff[-1])
    assert (got[total:] == np.uint64(2**64 - 1)).all(), "guard overwritten"
    tables = [(keys[int(seg[t]):int(seg[t + 1])].reshape(-1), None, SST[0], SST[1]) for t in range(len(COUNTS))]
    check_words(oracle, got, woff, tables)
    assert not got[int(woff[0]):int(woff[1])].any()  # no keys: all-zero words were written over the 0xFF
    for t in range(len(COUNTS)):  # pad words are written as zero
        nw = (SST[0] + 63) // 64
        assert not got[int(woff[t]) + nw:int(woff[t + 1])].any()


def _mixed_run():
    """Var-len keys of 1..300 bytes over tables at the plan test's shapes, one
    segment of all-equal keys and two tables split into parts (one per class)."""
    shapes = []
    r = 0
    for b in BITS:
        shapes.append((COUNTS[r % 6], b, 7))
        r += 1
    for c in COUNTS:
        for k in KS:
            shapes.append((c, BITS[r % 10], k))
            r += 1
    shapes.append((0, 0, 0))
    kw = next(c for c in range(1, 1 << 20) if lsmbloom.build_batch_parts(c, SST[0]) >= 2)
    kg = next(c for c in range(1, 1 << 22, 512) if lsmbloom.build_batch_parts(c, 1310720) >= 2)
    shapes += [(kw, SST[0], 7), (2 * kw + 5, 64, 1), (kg, 1310720, 7)]
    equal_at = len(shapes)
    shapes.append((200, SST[0], 7))  # all-equal keys
    n = 4 + sum(s[0] for s in shapes) + 2
    lens = 1 + (np.arange(n, dtype=np.uint64) * np.uint64(7)) % np.uint64(300)
    seg = np.zeros(len(shapes) + 1, np.uint64)
    seg[0] = 4
    seg[1:] = 4 + np.cumsum([s[0] for s in shapes])
    lens[int(seg[equal_at]):int(seg[equal_at + 1])] = 23
    offs = np.zeros(n + 1, np.uint64)
    np.cumsum(lens, out=offs[1:])
    data = keygen.stream_bytes(0x5EEDBB02, int(offs[-1]))
    a = int(offs[int(seg[equal_at])])
    for i in range(1, 200):
        data[a + 23 * i:a + 23 * (i + 1)] = data[a:a + 23]
    return shapes, seg, data, offs, n


@pytest.mark.gpu
def test_mixed_classes_varlen_keys_and_split_tables(oracle):
    shapes, seg, data, offs, n = _mixed_run()
    nb, kk = [s[1] for s in shapes], [s[2] for s in shapes]
    assert any(lsmbloom.build_batch_parts(s[0], s[1]) >= 2 and s[1] <= WAVE_MAX for s in shapes)
    assert any(lsmbloom.build_batch_parts(s[0], s[1]) >= 2 and s[1] > WAVE_MAX for s in shapes)
    ctx = lsmbloom.Context(0)
    got, woff, words = run_batch(ctx, data, offs, 0, n, seg, nb, kk)
    total = int(woff[-1])
    assert (got[total:] == np.uint64(2**64 - 1)).all(), "guard overwritten"
    tables = []
    for t, s in enumerate(shapes):
        lo, hi = int(seg[t]), int(seg[t + 1])
        o = offs[lo:hi + 1]
        tables.append((data[int(o[0]):int(o[-1])], o - o[0], s[1], s[2]))
    check_words(oracle, got, woff, tables, "first run")
    for t, s in enumerate(shapes):  # tail bits past num_bits stay clear
        if s[1] % 64:
            assert int(got[int(woff[t]) + (s[1] + 63) // 64 - 1]) >> (s[1] % 64) == 0
    # again into the now dirty buffer (built filters, not 0xFF): the same bytes
    again, _, _ = run_batch(ctx, data, offs, 0, n, seg, nb, kk, words=words)
    ctx.close()
    assert np.array_equal(again, got)


@pytest.mark.gpu
def test_fixed_keys_of_odd_length_and_unaligned_base(oracle):
    """FixedN's path: 11-byte keys, and 16-byte keys on a base that is not 16-byte aligned."""
    import torch
    ctx = lsmbloom.Context(0)
    n = 700
    raw = keygen.stream_bytes(0x5EEDBB05, 11 * n)
    seg, nb, kk = [0, 1, 300, 700], [64, SST[0], 16385], [1, 7, 7]
    got, woff, _ = run_batch(ctx, raw, None, 11, n, seg, nb, kk)
    for t in range(3):
        part = raw[11 * seg[t]:11 * seg[t + 1]]
        o = np.arange(0, part.size + 1, 11, dtype=np.uint64)
        exp = oracle.build_var(part, o, nb[t], kk[t])
        assert np.array_equal(got[int(woff[t]):int(woff[t]) + exp.size], exp), t
    keys = keygen.key16(0x5EEDBB06, 0, 500)
    dev = torch.device("cuda:0")
    buf = torch.zeros(8 + 16 * 500 + 16, dtype=torch.uint8, device=dev)
    buf[8:8 + 16 * 500] = torch.from_numpy(keys.reshape(-1)).to(dev)
    words = torch.full((int(lsmbloom.build_batch_layout([SST[0]])[-1]),), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.build_batch_dev(buf[8:], 500, [0, 500], [SST[0]], [SST[1]], words, key_len=16)
    torch.cuda.synchronize()
    exp = oracle.build_fixed(keys, 16, *SST)
    assert np.array_equal(words.cpu().numpy().view(np.uint64)[:exp.size], exp)
    ctx.close()


@pytest.mark.gpu
def test_rejections_leave_the_buffer_untouched():
    import torch
    dev = torch.device("cuda:0")
    ctx = lsmbloom.Context(0)
    keys = torch.from_numpy(keygen.key16(0x5EEDBB03, 0, 100).reshape(-1)).to(dev)
    nb, kk, seg = [SST[0], 64], [7, 1], [0, 60, 100]
    total = int(lsmbloom.build_batch_layout(nb)[-1])
    words = torch.full((total + GUARD,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def build(seg=seg, nb=nb, kk=kk, w=words, n=100):
        ctx.build_batch_dev(keys, n, seg, nb, kk, w, key_len=16)

    for bad in (dict(w=words[:total - 1]),                      # words_cap too small
                dict(seg=[0, 60, 59]),                          # seg descends
                dict(n=99),                                     # seg[ntab] > n
                dict(nb=[SST[0], 1310721]),                     # above the size limit (and the buffer would be short)
                dict(nb=[0, 64], kk=[7, 1]),                    # no bits with k > 0
                dict(w=words.view(torch.uint8)[8:].view(torch.int64))):  # not 16-byte aligned
        with pytest.raises(ValueError):
            build(**bad)
    torch.cuda.synchronize()
    assert bool((words == -1).all()), "a rejected batch wrote to the buffer"
    # no tables: fine, and nothing is written
    ctx.build_batch_dev(keys, 100, [0], [], [], words, key_len=16)
    torch.cuda.synchronize()
    assert bool((words == -1).all())
    ctx.close()


@pytest.mark.gpu
def test_blocks_equal_the_oracles_serialize_and_load_into_a_level_set(oracle):
    counts = (40, 0, 1, 65, 300, 1000)
    shapes = [SST, SST, (64, 1), (16385, 7), (WAVE_MAX + 1, 7), SST]
    ranges, tabs = [], []
    first = 0
    for c in counts:
        ks = [b"user%08d" % (first + i) for i in range(c)]
        tabs.append(ks)
        ranges.append((b"user%08d" % first, b"user%08d" % (first + max(c, 1) - 1)))
        first += c + 50
    run = [b"zzz-unclaimed"] + [k for ks in tabs for k in ks] + [b"zzz-unclaimed-too"]
    data, offs = keygen.pack(run)
    seg = np.zeros(len(counts) + 1, np.uint64)
    seg[0] = 1
    seg[1:] = 1 + np.cumsum(counts)
    nb, kk = [s[0] for s in shapes], [s[1] for s in shapes]
    ctx = lsmbloom.Context(0)
    blocks, boff = ctx.build_batch_blocks(data, seg, nb, kk, offsets=offs)
    exp_blocks = []
    for t, ks in enumerate(tabs):
        d, o = keygen.pack(ks)
        w = oracle.build_var(d, o, nb[t], kk[t]) if ks else np.zeros((nb[t] + 63) // 64, np.uint64)
        exp_blocks.append(oracle.serialize(w, nb[t], kk[t]))
        assert int(boff[t + 1] - boff[t]) == lsmbloom.serialized_size(nb[t])
        assert blocks[int(boff[t]):int(boff[t + 1])].tobytes() == exp_blocks[t], t
    assert blocks.size == int(boff[-1])
    # the same bytes load as a batch: lsmb_lset_add_batch on the returned arrays as they are, then
    # LevelSet.add_many on the blocks cut at block_off; CRCs from zlib, checked on the device copies
    L = lsmbloom.lib()
    rows = np.zeros(len(counts), np.uint32)
    ids = np.arange(10, 10 + len(counts), dtype=np.uint32)
    kd, ko = keygen.pack([k for r in ranges for k in r])
    cut = [blocks[int(boff[t]):int(boff[t + 1])].tobytes() for t in range(len(counts))]
    crcs = np.array([zlib.crc32(b) for b in cut], np.uint32)
    status = np.full(len(counts), 99, np.int32)
    raw = LevelSet(ctx)
    rc = L.lsmb_lset_add_batch(raw.h, len(counts), p(rows, u32p), p(ids, u32p), p(blocks, u8p), p(boff, u64p),
                               p(crcs, u32p), p(kd, u8p), p(ko, u64p), p(status, ctypes.POINTER(ctypes.c_int32)))
    assert rc == 0 and not status.any(), L.lsmb_last_error()
    assert raw.tables(0) == len(counts)
    raw.close()
    ls = LevelSet(ctx)
    assert not ls.add_many(rows, ids, cut, ranges, crcs=crcs).any()
    ls.seal()
    got = ls.probe_keys(run)
    for t in range(len(counts)):
        assert (got[0, int(seg[t]):int(seg[t + 1])] == ids[t]).all()
    assert got[0, 0] == lsmbloom.LSMB_LSET_NONE and got[0, -1] == lsmbloom.LSMB_LSET_NONE
    ls.close()
    ctx.close()


def _level_tables(oracle):
    """~40 tables over two rows with disjoint ranges: (row, id, keys, num_bits, k, oracle block)."""
    tabs = []
    odd = {3: (64, 1), 11: (16385, 7), 17: (WAVE_MAX + 1, 7), 29: (65, 40)}
    for j in range(40):
        row, first = j % 2, 150 * (j // 2) + 40 * (j % 2)
        rng = np.random.default_rng(2000 + j)
        ids = np.sort(rng.choice(100, size=40, replace=False)) + first
        ks = [b"user%08d" % i for i in ids]
        nb, k = odd.get(j, SST)
        d, o = keygen.pack(ks)
        tabs.append((row, 500 + j, ks, nb, k, oracle.serialize(oracle.build_var(d, o, nb, k), nb, k)))
    return tabs


def _built_set(ctx, tabs, into=None):
    """tabs through build_batch_dev and add_built into a new (or the given) set."""
    import torch
    run = [k for t in tabs for k in t[2]]
    data, offs = keygen.pack(run)
    seg = np.zeros(len(tabs) + 1, np.uint64)
    np.cumsum([len(t[2]) for t in tabs], out=seg[1:])
    nb, kk = [t[3] for t in tabs], [t[4] for t in tabs]
    dev = torch.device("cuda:0")
    d_data = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    words = torch.full((int(lsmbloom.build_batch_layout(nb)[-1]),), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.build_batch_dev(d_data, len(run), seg, nb, kk, words, offsets=d_offs)
    ls = into if into is not None else LevelSet(ctx)
    ls.add_built([t[0] for t in tabs], [t[1] for t in tabs], words, nb, kk, [(t[2][0], t[2][-1]) for t in tabs])
    del words  # add_built has returned: the source buffer is free to go
    return ls


def _loaded_set(ctx, tabs):
    ls = LevelSet(ctx)
    ls.add_many([t[0] for t in tabs], [t[1] for t in tabs], [t[5] for t in tabs], [(t[2][0], t[2][-1]) for t in tabs])
    return ls


@pytest.mark.gpu
def test_built_words_go_into_a_level_set_device_to_device(oracle):
    tabs = _level_tables(oracle)
    q = [b"user%08d" % i for i in range(0, 150 * 20 + 200)]  # every member and the absent ids between them
    q += [b"", b"user", b"\xff" * 20]
    ctx = lsmbloom.Context(0)
    built, ref = _built_set(ctx, tabs), _loaded_set(ctx, tabs)
    st = built.stats()
    assert st["tables"] == 40 and st["uploaded_bytes"] == 0 and st["upload_copies"] == 0
    assert st["filter_bytes"] == ref.stats()["filter_bytes"] and st["chunk_bytes"] == ref.stats()["chunk_bytes"]
    built.seal()
    ref.seal()
    a, b = built.probe_keys(q), ref.probe_keys(q)
    assert a.shape == b.shape == (2, len(q)) and np.array_equal(a, b)
    assert int((a != lsmbloom.LSMB_LSET_NONE).sum()) >= 40 * 40  # every member is found

    # a Version edit: three tables go, one built table comes
    drop = [tabs[4][1], tabs[9][1], tabs[30][1]]
    rng = np.random.default_rng(2100)
    ks = [b"user%08d" % i for i in np.sort(rng.choice(100, size=60, replace=False)) + 150 * 2]  # table 4's gap, row 0
    d, o = keygen.pack(ks)
    new = (0, 900, ks, SST[0], SST[1], oracle.serialize(oracle.build_var(d, o, *SST), *SST))
    child = _built_set(ctx, [new], into=built.derive(drop))
    assert child.dropped == 3
    cs = child.stats()
    assert cs["tables"] == 38 and cs["inherited"] == 37 and cs["uploaded_bytes"] == 0 and cs["upload_copies"] == 0
    child.seal()
    ref2 = _loaded_set(ctx, [t for t in tabs if t[1] not in drop] + [new])
    ref2.seal()
    assert np.array_equal(child.probe_keys(q), ref2.probe_keys(q))
    assert np.array_equal(built.probe_keys(q), b)  # the parent is untouched

    # a batch with one invalid row leaves the set as it was
    ls = _built_set(ctx, tabs[:6])
    before = ls.stats()
    bad = [(8,) + tabs[7][1:]] + [tabs[8]]
    with pytest.raises(ValueError):
        _built_set(ctx, [tabs[8]] + bad, into=ls)
    assert ls.stats() == before and ls.tables(0) == 3 and ls.tables(1) == 3
    # ... and so does a word_off that is not the layout's
    import torch
    L = lsmbloom.lib()
    w = torch.zeros(1024, dtype=torch.int64, device="cuda:0")
    one = np.array([0], np.uint32)
    nb1, k1 = np.array([SST[0]], np.uint32), np.array([7], np.uint32)
    kd, ko = keygen.pack([b"a", b"b"])
    for woff in ([0, 152], [2, 152], [0, 150 - 2]):
        wo = np.array(woff, np.uint64)
        assert L.lsmb_lset_add_batch_dev(ls.h, 1, p(one, u32p), p(one, u32p), vp(w.data_ptr()), p(wo, u64p),
                                         p(nb1, u32p), p(k1, u32p), p(kd, u8p), p(ko, u64p), None) == EINVAL
    assert ls.stats() == before
    for s in (ls, child, ref2, built, ref):
        s.close()
    ctx.close()


@pytest.mark.gpu
def test_cpp_mirror_build_batch_gpu():
    r = subprocess.run([cpp_bin("build_batch_test"), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout
