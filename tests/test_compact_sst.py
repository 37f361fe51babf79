"""The surviving keys of a compaction's merged data blocks, resolved on the
device (lsmb_compact_sst_*): which entries of the input tables' blocks
MergeIterator keeps (the lowest source index of equal keys,
src/iterator/merge.rs:15,55-56,98-121), less the tombstones a bottommost
compaction drops (src/compaction/scheduler.rs:147-158); the survivor count, the
survivors' keys as a device key run, and the output table's bloom block.

Without a GPU: the key order, the searches and compact_sst_ref
(csrc/sst_compact.hpp) on the CPU under ASan and UBSan against a std::map merge,
and the argument checks.  On the GPU: the gathered key run, the totals and the
filter bytes against a dict merge written here and the CPU oracle's filter over
the model's keys, exact equality.
"""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import keygen
import lsmbloom
import sst_support as ss
from lsmbloom import sstable, u8p, u32p, u64p
from lset_support import cpp_bin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECORRUPT = lsmbloom.LSMB_EINVAL, lsmbloom.LSMB_ECORRUPT
BAD = lsmbloom.LSMB_SST_BAD_BLOCK
vp = ctypes.c_void_p
SST = lsmbloom.params(1000, 0.01)  # SSTableBuilder's filter: (9586, 7)
SENTINEL = 0x5A5A5A5A              # blk_entries before a call
CANARY = 0x5A                      # every byte behind a device buffer
GUARD = 256                        # bytes of canary behind work, key_data and key_offsets


def p(a, t):
    return a.ctypes.data_as(t)


# ---------------------------------------------------------------- the model

def parse_entries(blk):
    """[(key, vlen)] of a block in entry order, None when it is malformed."""
    keys = ss.parse_block(blk)
    if keys is None:
        return None
    blk = bytes(blk)
    (n,) = struct.unpack_from("<H", blk, len(blk) - 2)
    data_end = len(blk) - 2 - 2 * n
    out = []
    for i in range(n):
        (off,) = struct.unpack_from("<H", blk, data_end + 2 * i)
        out.append((keys[i], struct.unpack_from("<H", blk, off + 2)[0]))
    return out


def merge_model(sources, drop):
    """sources: newest first, each a list of blocks.  A dict merge: the newest
    version of each key; survivors in (source, block, entry) order.  A
    malformed or empty block holds nothing.
    -> (survivor keys, entries seen, bad blocks, newest {key: (source, vlen)})."""
    newest, seen, bad = {}, 0, 0
    parsed = [[parse_entries(b) or None for b in src] for src in sources]
    for s, src in enumerate(parsed):
        for es in src:
            for k, vlen in es or ():
                newest.setdefault(k, (s, vlen))
    keys = []
    for s, src in enumerate(parsed):
        for es in src:
            if not es:
                bad += 1
                continue
            seen += len(es)
            keys += [k for k, vlen in es if newest[k][0] == s and not (drop and vlen == 0)]
    return keys, seen, bad, newest


def lay(sources, before=(), after=(), tail=0):
    """The sources' blocks with unclaimed blocks in front and behind, every
    block at an odd offset with junk around it -> (bytes, blk_off, blk_len, sseg)."""
    blocks = list(before) + [b for src in sources for b in src] + list(after)
    buf, blk_off, blk_len = ss.place(blocks, odd=True, tail=tail)
    sseg = (np.concatenate([[0], np.cumsum([len(src) for src in sources])]) + len(before)).astype(np.uint64)
    return buf, blk_off, blk_len, sseg


def canaried(torch, nbytes, dev):
    """A uint8 device tensor of nbytes + GUARD bytes, all CANARY, 16-byte aligned."""
    return torch.full((nbytes + GUARD,), CANARY, dtype=torch.uint8, device=dev)


def run_dev(ctx, buf, blk_off, blk_len, sseg, drop):
    """Mark, the totals read back, gather into buffers sized from them ->
    (keys, offsets, totals, blk_entries); the canaries behind the work buffer,
    the key bytes and the offsets are checked here."""
    import torch
    dev = torch.device("cuda:0")
    d_bytes = torch.from_numpy(np.array(buf, dtype=np.uint8)).to(dev)
    wb = lsmbloom.compact_sst_work_bytes(blk_len)
    work = canaried(torch, wb, dev)
    totals = torch.full((4,), -1, dtype=torch.int64, device=dev)
    ent = torch.full((max(len(blk_off), 1),), SENTINEL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.compact_sst_mark_dev(d_bytes, blk_off, blk_len, sseg, drop, work[:wb], totals, blk_entries=ent)
    torch.cuda.synchronize()
    tot = [int(x) for x in totals.cpu().numpy().view(np.uint64)]
    surv, kbytes = tot[0], tot[1]
    key_data = canaried(torch, kbytes, dev)
    offs = canaried(torch, 8 * (surv + 1), dev)
    torch.cuda.synchronize()
    ctx.compact_sst_gather_dev(d_bytes, blk_off, blk_len, sseg, work[:wb], key_data[:kbytes],
                               offs[:8 * (surv + 1)].view(torch.int64))
    torch.cuda.synchronize()
    assert bool((work[wb:] == CANARY).all()), "the work buffer's canary"
    assert bool((key_data[kbytes:] == CANARY).all()), "the key bytes' canary"
    assert bool((offs[8 * (surv + 1):] == CANARY).all()), "the offsets' canary"
    o = offs[:8 * (surv + 1)].cpu().numpy().view(np.uint64)
    data = key_data[:kbytes].cpu().numpy().tobytes()
    assert o[0] == 0 and int(o[-1]) == kbytes and (np.diff(o.astype(np.int64)) >= 0).all()
    keys = [data[int(o[i]):int(o[i + 1])] for i in range(surv)]
    return keys, o, tot, ent.cpu().numpy().view(np.uint32)[:len(blk_off)]


def check_against_model(ctx, sources, drop, before=(), after=(), tail=0):
    buf, blk_off, blk_len, sseg = lay(sources, before, after, tail)
    keys, offs, tot, ent = run_dev(ctx, buf, blk_off, blk_len, sseg, drop)
    exp, seen, bad, _ = merge_model(sources, drop)
    assert keys == exp
    assert list(offs) == list(np.concatenate([[0], np.cumsum([len(k) for k in exp])]).astype(np.uint64))
    assert tot == [len(exp), sum(len(k) for k in exp), seen, bad]
    b0, b1 = int(sseg[0]), int(sseg[-1])
    assert (ent[:b0] == SENTINEL).all() and (ent[b1:] == SENTINEL).all(), "an unclaimed block's entry was written"
    flat = [b for src in sources for b in src]
    assert [int(e) for e in ent[b0:b1]] == [len(parse_entries(b) or ()) or BAD for b in flat]
    return buf, blk_off, blk_len, sseg, exp


def oracle_block(oracle, keys, nb, k):
    nw = (nb + 63) // 64
    if keys:
        data, offs = keygen.pack(keys)
        words = oracle.build_var(data, offs, nb, k)
    else:
        words = np.zeros(nw, np.uint64)
    return oracle.serialize(words, nb, k)


def hand_made():
    """k1 live / tombstone / live, k2 tombstone / live / -, k3 - / tombstone /
    live, k4 and k5 in the oldest source only (live, tombstone), the empty key
    live in source 2 only, "ab" in source 0 and "abc" in source 1."""
    return [[ss.encode_block([(b"ab", b"v"), (b"k1", b"live"), (b"k2", b"")])],
            [ss.encode_block([(b"abc", b"v"), (b"k1", b""), (b"k2", b"live"), (b"k3", b"")])],
            [ss.encode_block([(b"", b"v"), (b"k1", b"live"), (b"k3", b"live"), (b"k4", b"live"), (b"k5", b"")])]]


def seeded_sources():
    """4 sources over a space of 2 000 keys of 0 .. 40 bytes with shared 8- and
    16-byte prefixes, about 30 % tombstones, a few long values (blocks of one
    entry), cut at 256 bytes; source 1 ends in one block of 200 short entries
    that sort behind every other key, half of which source 3 holds too."""
    rng = np.random.default_rng(0xC0FFEE)
    space = {b""}
    while len(space) < 2000:
        pre = (b"", b"prefix08", b"prefix16prefix16")[int(rng.integers(3))]
        tail = int(rng.integers(0, 41 - len(pre)))
        space.add(pre + rng.integers(0, 0xF0, tail, dtype=np.uint8).tobytes())
    space = sorted(space)
    shorts = [b"\xff" + struct.pack(">H", i) for i in range(200)]
    sources = []
    for s in range(4):
        es = []
        for k in space:
            if rng.random() < 0.45:
                r = rng.random()
                es.append((k, b"" if r < 0.3 else bytes(int(rng.integers(1, 20))) if r < 0.97 else bytes(250)))
        blocks = ss.split_into_blocks(es, block_size=256)
        if s == 1:
            blocks.append(ss.encode_block([(k, b"" if i % 3 == 0 else b"v") for i, k in enumerate(shorts)]))
        if s == 3:
            blocks += ss.split_into_blocks([(k, b"old") for k in shorts[::2]], block_size=256)
        sources.append(blocks)
    return sources


# ---------------------------------------------------------------- without a GPU

def test_key_order_searches_and_reference_host(tmp_path):
    """tests/cpp/sst_compact_test.cpp: the key order (prefixes, the empty key,
    differences in byte 0, 7, 8 and the last, bytes >= 0x80), the two searches
    at their edges, compact_sst_ref against a std::map merge on the seeded case,
    every malformed block in a newer and in an older source.  A stand-alone
    program under ASan and UBSan, every block in an allocation of exactly its
    length."""
    exe = str(tmp_path / "sst_compact_test")
    src = os.path.join(ROOT, "tests", "cpp", "sst_compact_test.cpp")
    # (the flags of test_build_batch_sst.py's host test: the header compiles xxh3.hpp / bloom_math.hpp for the host)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout


def test_the_model_on_the_hand_made_case():
    """The dict merge itself, on the case whose answer can be read off."""
    src = hand_made()
    assert merge_model(src, 0)[0] == [b"ab", b"k1", b"k2", b"abc", b"k3", b"", b"k4", b"k5"]
    assert merge_model(src, 1)[0] == [b"ab", b"k1", b"abc", b"", b"k4"]
    assert merge_model(src, 0)[1:3] == (12, 0)
    assert merge_model([[b"\xff" * 9, ss.encode_block([])] + src[0]], 1)[:3] == ([b"ab", b"k1"], 3, 2)


def test_entry_points_are_exported_and_reject_bad_arguments():
    L = lsmbloom.lib()
    for name in ("lsmb_compact_sst_work_bytes", "lsmb_compact_sst_mark_dev", "lsmb_compact_sst_gather_dev",
                 "lsmb_compact_sst_bloom"):
        assert hasattr(L, name) and name in lsmbloom.SIGNATURES
    for name in ("compact_sst_mark_dev", "compact_sst_gather_dev", "compact_sst_bloom"):
        assert callable(getattr(lsmbloom.Context, name))
    assert callable(lsmbloom.compact_sst_work_bytes) and callable(sstable.compact_filter)
    assert "compact_sst_bloom" in open(os.path.join(ROOT, "storage-engine_amd", "cpp", "lsm_bloom.hpp")).read()

    # the sizing: per block 56 bytes and a flag bit per entry it could hold (len / 2 of them: entries may overlap)
    assert lsmbloom.compact_sst_work_bytes([]) == 0
    assert lsmbloom.compact_sst_work_bytes([0, 1, 2]) == 3 * 56
    assert lsmbloom.compact_sst_work_bytes([4096]) == 56 + 8 * 32
    assert lsmbloom.compact_sst_work_bytes([200000, 130]) == 2 * 56 + 8 * (1024 + 1)
    assert L.lsmb_compact_sst_work_bytes(3, None) == 0

    bo = np.array([0, 100, 300], np.uint64)
    bl = np.array([100, 200, 100], np.uint32)
    sseg = np.array([0, 1, 3], np.uint64)
    fake = vp(0x1000)  # never dereferenced: every call below fails its checks first
    need = lsmbloom.compact_sst_work_bytes(bl)

    def mark(c=fake, by=vp(0x3000), nbytes=400, nblk=3, o=bo, ln=bl, sg=sseg, w=vp(0x2000), wb=need, t=vp(0x5000)):
        return L.lsmb_compact_sst_mark_dev(c, by, nbytes, nblk, None if o is None else p(o, u64p),
                                           None if ln is None else p(ln, u32p), 2, None if sg is None else p(sg, u64p), 1,
                                           w, wb, vp(0x4000), t, None)

    assert mark(c=None) == EINVAL and mark(sg=None) == EINVAL and mark(w=None) == EINVAL and mark(t=None) == EINVAL
    assert mark(o=None) == EINVAL and mark(ln=None) == EINVAL      # NULL blk_off / blk_len with nblk > 0
    assert mark(by=None) == EINVAL                                 # NULL d_bytes with a non-empty claimed block
    assert mark(sg=np.array([0, 2, 1], np.uint64)) == EINVAL       # sseg descends
    assert mark(nblk=2) == EINVAL                                  # sseg[nsrc] > nblk
    assert mark(nbytes=399) == EINVAL                              # the last block leaves the buffer
    assert b"block 2" in L.lsmb_last_error()
    assert mark(o=np.array([0, 2**64 - 50, 300], np.uint64)) == EINVAL  # ... also where off + len wraps
    assert mark(wb=need - 1) == EINVAL                             # work_bytes too small
    assert b"work_bytes" in L.lsmb_last_error()
    assert mark(w=vp(0x2008)) == EINVAL                            # not 16-byte aligned

    def gather(c=fake, sg=sseg, w=vp(0x2000), kd=vp(0x6000), ko=vp(0x7000), nbytes=400):
        return L.lsmb_compact_sst_gather_dev(c, vp(0x3000), nbytes, 3, p(bo, u64p), p(bl, u32p), 2,
                                             None if sg is None else p(sg, u64p), w, kd, 64, ko, 8, None)

    assert gather(c=None) == EINVAL and gather(sg=None) == EINVAL and gather(w=None) == EINVAL
    assert gather(kd=None) == EINVAL and gather(ko=None) == EINVAL and gather(ko=vp(0x7004)) == EINVAL
    assert gather(nbytes=399) == EINVAL and gather(w=vp(0x2008)) == EINVAL

    # host bytes in, the bloom block out: no host fallback, outputs untouched
    data = np.zeros(400, np.uint8)
    bloom = np.full(2048, 0xAB, np.uint8)
    blen, cnt = ctypes.c_uint64(7), ctypes.c_uint64(7)
    nb, kk = ctypes.c_uint32(7), ctypes.c_uint32(7)

    def one(c=fake, sg=sseg, nbytes=400, fpr=0.01, ln=ctypes.byref(blen)):
        return L.lsmb_compact_sst_bloom(c, p(data, u8p), nbytes, 3, p(bo, u64p), p(bl, u32p), 2, p(sg, u64p), 0, 1000, fpr,
                                        p(bloom, u8p), bloom.size, ln, ctypes.byref(cnt), ctypes.byref(nb), ctypes.byref(kk))

    untouched = lambda: (bloom == 0xAB).all() and (blen.value, cnt.value, nb.value, kk.value) == (7, 7, 7, 7)  # noqa: E731
    assert one(c=None) == EINVAL and untouched()                   # a NULL ctx is refused whatever the size
    assert one(ln=None) == EINVAL and untouched()
    assert one(fpr=0.0) == EINVAL and one(fpr=1.0) == EINVAL and untouched()
    assert one(sg=np.array([0, 2, 1], np.uint64)) == EINVAL and untouched()
    assert one(nbytes=399) == EINVAL and untouched()


def test_cpp_mirror_compact_sst_argument_checks():
    r = subprocess.run([cpp_bin("compact_sst_test")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


# ---------------------------------------------------------------- on the GPU

@pytest.mark.gpu
@pytest.mark.parametrize("drop", [0, 1])
def test_hand_made_three_sources(oracle, drop):
    src = hand_made()
    want = [b"ab", b"k1", b"abc", b"", b"k4"] if drop else [b"ab", b"k1", b"k2", b"abc", b"k3", b"", b"k4", b"k5"]
    ctx = lsmbloom.Context(0)
    buf, blk_off, blk_len, sseg = lay(src, [b"\xff" * 3], [b"\xff" * 3])
    keys, offs, tot, ent = run_dev(ctx, buf, blk_off, blk_len, sseg, drop)
    assert keys == want
    assert tot == [len(want), sum(len(k) for k in want), 12, 0]
    assert [int(e) for e in ent] == [SENTINEL, 3, 4, 5, SENTINEL]
    block, nb, k, count = ctx.compact_sst_bloom(buf, blk_off, blk_len, sseg, drop, expected_items=1000, fpr=0.01)
    ctx.close()
    assert (nb, k) == SST and count == len(want)  # entry_count: what the meta block of the output table says
    assert block == oracle_block(oracle, want, *SST)


@pytest.fixture(scope="module")
def seeded():
    return seeded_sources()


def test_seeded_model_has_every_class(seeded):
    """From the dict model alone: the case reaches every kind of verdict."""
    per_key = {}
    sizes = []
    for s, src in enumerate(seeded):
        for b in src:
            es = parse_entries(b)
            sizes.append(len(es))
            for k, vlen in es:
                per_key.setdefault(k, []).append((s, vlen))
    assert min(sizes) == 1 and max(sizes) > 64 and sum(1 for src in seeded if len(src) > 20) == 4
    vs = per_key.values()
    assert any(len(v) > 1 and any(vl > 0 for _, vl in v[1:]) for v in vs), "shadowed-live"
    assert any(len(v) > 1 and v[0][1] > 0 and any(vl == 0 for _, vl in v[1:]) for v in vs), "live-over-older-tombstone"
    assert any(len(v) > 1 and v[0][1] == 0 and any(vl > 0 for _, vl in v[1:]) for v in vs), "tombstone-over-older-live"
    assert any(len(v) == 1 and v[0][1] == 0 for v in vs), "tombstone-only"
    assert any(8 < len(k) and k.startswith(b"prefix08") for k in per_key) and b"" in per_key
    for drop in (0, 1):
        keys, seen, bad, _ = merge_model(seeded, drop)
        assert 0 < len(keys) < seen and bad == 0
    assert len(merge_model(seeded, 1)[0]) < len(merge_model(seeded, 0)[0]) == len(per_key)


@pytest.mark.gpu
@pytest.mark.parametrize("drop", [0, 1])
def test_seeded_model(oracle, seeded, drop):
    ctx = lsmbloom.Context(0)
    buf, blk_off, blk_len, sseg, exp = check_against_model(ctx, seeded, drop, [b"\xff" * 3], [b"\xff" * 3])
    assert all(int(o) % 2 == 1 for o in blk_off)
    block, nb, k, count = ctx.compact_sst_bloom(buf, blk_off, blk_len, sseg, drop, expected_items=1000, fpr=0.01)
    assert (nb, k, count) == (SST[0], SST[1], len(exp))
    assert block == oracle_block(oracle, exp, *SST)
    block, nb, k, count = ctx.compact_sst_bloom(buf, blk_off, blk_len, sseg, drop, expected_items=0, fpr=0.01)
    ctx.close()
    assert (nb, k) == lsmbloom.params(max(len(exp), 1), 0.01) and count == len(exp)
    assert block == oracle_block(oracle, exp, nb, k)


@pytest.mark.gpu
def test_survivors_above_the_batched_builds_limit(oracle):
    """200 000 distinct 16-byte keys in two sources that share half of theirs:
    the filter sized for the survivors is above build_batch_max_bits(), so the
    gather -> build_var_dev_new route carries it."""
    n = 200_000
    newer = [(b"%016d" % i, b"12345678") for i in range(0, 2 * n // 3)]
    older = [(b"%016d" % i, b"abcdefgh") for i in range(n // 3, n)]
    src = [ss.split_into_blocks(newer, 4096), ss.split_into_blocks(older, 4096)]
    buf, blk_off, blk_len, sseg = lay(src)
    ctx = lsmbloom.Context(0)
    block, nb, k, count = ctx.compact_sst_bloom(buf, blk_off, blk_len, sseg, 1, expected_items=0, fpr=0.01)
    ctx.close()
    assert count == n and (nb, k) == lsmbloom.params(n, 0.01) and nb > lsmbloom.build_batch_max_bits()
    assert block == oracle_block(oracle, [b"%016d" % i for i in range(n)], nb, k)


@pytest.mark.gpu
def test_edges(oracle):
    ctx = lsmbloom.Context(0)
    src = hand_made()
    empty_block = oracle.serialize(np.zeros((SST[0] + 63) // 64, np.uint64), *SST)
    # one source: only the tombstone drop
    assert check_against_model(ctx, [src[2]], 1)[4] == [b"", b"k1", b"k3", b"k4"]
    assert check_against_model(ctx, [src[2]], 0)[4] == [b"", b"k1", b"k3", b"k4", b"k5"]
    # no sources: totals all zero, offsets == [0], the empty filter's block; unclaimed blocks keep their entries
    buf, blk_off, blk_len, sseg, exp = check_against_model(ctx, [], 1, before=src[0], after=src[1])
    assert exp == [] and list(sseg) == [1]
    assert ctx.compact_sst_bloom(buf, blk_off, blk_len, sseg, 1, expected_items=1000) == (empty_block, SST[0], SST[1], 0)
    assert ctx.compact_sst_bloom(buf, blk_off, blk_len, sseg, 0)[1:] == lsmbloom.params(1, 0.01) + (0,)
    # a source with no blocks between two others
    assert check_against_model(ctx, [src[0], [], src[2]], 0, before=[b"\xff" * 7])[4] == \
        [b"ab", b"k1", b"k2", b"", b"k3", b"k4", b"k5"]
    # all entries dropped: the empty filter's block, offsets == [0]
    tombs = [ss.split_into_blocks([(b"t%04d" % i, b"") for i in range(300)], 256),
             ss.split_into_blocks([(b"t%04d" % i, b"") for i in range(150, 400)], 256)]
    buf, blk_off, blk_len, sseg, exp = check_against_model(ctx, tombs, 1)
    assert exp == []
    assert ctx.compact_sst_bloom(buf, blk_off, blk_len, sseg, 1, expected_items=1000) == (empty_block, SST[0], SST[1], 0)
    assert len(check_against_model(ctx, tombs, 0)[4]) == 400
    # a single-entry block longer than 65 535 bytes in a newer source, among ordinary blocks
    big = b"m" * 300
    newer = ss.split_into_blocks([(b"a%03d" % i, b"v") for i in range(50)] + [(big, bytes(65535))]
                                 + [(b"z%03d" % i, b"") for i in range(50)], 256)
    assert max(len(b) for b in newer) > 65535
    older = ss.split_into_blocks([(b"a%03d" % i, b"old") for i in range(0, 80, 2)] + [(big, b"old"), (big + b"m", b"old")]
                                 + [(b"z%03d" % i, b"old") for i in range(40, 60)], 256)
    for drop in (0, 1):
        exp = check_against_model(ctx, [newer, older], drop)[4]
        assert exp.count(big) == 1 and big + b"m" in exp and b"z045" not in exp[len(exp) - 12:]
    ctx.close()


@pytest.mark.gpu
def test_a_source_that_is_not_ascending_only_adds_keys(oracle, seeded):
    """Two blocks of the newest source swapped: a search may miss, never hit
    falsely.  Every key whose newest version is live still passes may_contain."""
    src = [list(s) for s in seeded]
    src[0][1], src[0][-2] = src[0][-2], src[0][1]
    ctx = lsmbloom.Context(0)
    buf, blk_off, blk_len, sseg = lay(src)
    for drop in (0, 1):
        keys, _, tot, ent = run_dev(ctx, buf, blk_off, blk_len, sseg, drop)
        exp, seen, bad, newest = merge_model(src, drop)  # (the dict merge does not depend on the order)
        assert tot[2:] == [seen, 0] and BAD not in ent
        assert tot[0] >= len(exp) and set(exp) <= set(keys)
    block, nb, k, count = ctx.compact_sst_bloom(buf, blk_off, blk_len, sseg, 1, expected_items=0)  # returns: LSMB_OK
    ctx.close()
    words = np.frombuffer(block[12:], dtype=np.uint64)
    live = [key for key, (s, vlen) in newest.items() if vlen > 0]
    assert len(live) > 500 and count >= len(live)
    assert all(oracle.may_contain(words, nb, k, key) for key in live)


@pytest.mark.gpu
def test_malformed_blocks_in_a_newer_source(oracle):
    """Every block of sst_support.malformed_blocks in the newest source in turn,
    and an empty block: reported in d_blk_entries and totals[3], the other
    blocks' verdicts as if it were absent; the canaries behind the work buffer,
    the key bytes and the offsets untouched (run_dev).  The byte buffer ends in
    256 KiB of zeros, more than three u16 fields can address from a block's
    start, so that even a wrong parse would stay inside the allocation."""
    newer = ss.split_into_blocks([(b"user%08d" % i, b"" if i % 3 == 0 else b"v" * 9) for i in range(0, 200, 2)], 256)
    older = ss.split_into_blocks([(b"user%08d" % i, b"old") for i in range(0, 200, 3)], 256)
    bad = dict(ss.malformed_blocks())
    bad["no entries"] = ss.encode_block([])
    ctx = lsmbloom.Context(0)
    absent = {drop: merge_model([newer, older], drop)[0] for drop in (0, 1)}
    first = None
    for i, (name, blk) in enumerate(bad.items()):
        src = [newer[:3] + [blk] + newer[3:], older]
        drop = i % 2
        buf, blk_off, blk_len, sseg, exp = check_against_model(ctx, src, drop, [b"\xff" * 3], [b"\xff" * 3], tail=256 << 10)
        assert exp == absent[drop], name
        first = first or (buf, blk_off, blk_len, sseg)
    # the one-call form: LSMB_ECORRUPT, the source and the block named
    buf, blk_off, blk_len, sseg = first
    with pytest.raises(lsmbloom.Corruption):
        ctx.compact_sst_bloom(buf, blk_off, blk_len, sseg, 0, expected_items=1000)
    L = lsmbloom.lib()
    assert b"source 0" in L.lsmb_last_error() and b"block %d" % (int(sseg[0]) + 3) in L.lsmb_last_error()
    data = np.array(buf, dtype=np.uint8)
    out = np.full(2048, 0xAB, np.uint8)
    blen = ctypes.c_uint64(7)
    rc = L.lsmb_compact_sst_bloom(ctx.h, p(data, u8p), data.size, blk_off.size, p(blk_off, u64p), p(blk_len, u32p), 2,
                                  p(sseg, u64p), 0, 1000, 0.01, p(out, u8p), out.size, ctypes.byref(blen), None, None, None)
    assert rc == ECORRUPT and (out == 0xAB).all() and blen.value == 7
    ctx.close()


@pytest.mark.gpu
def test_rejections_leave_every_buffer_untouched():
    import torch
    dev = torch.device("cuda:0")
    ctx = lsmbloom.Context(0)
    src = hand_made()
    buf, blk_off, blk_len, sseg = lay(src, [b"\xff" * 3], [])
    d_bytes = torch.from_numpy(np.array(buf, dtype=np.uint8)).to(dev)
    wb = lsmbloom.compact_sst_work_bytes(blk_len)
    work = canaried(torch, wb, dev)
    totals = torch.full((4,), SENTINEL, dtype=torch.int64, device=dev)
    ent = torch.full((len(blk_off),), SENTINEL, dtype=torch.int32, device=dev)
    key_data = canaried(torch, 64, dev)
    offs = canaried(torch, 8 * 16, dev)
    torch.cuda.synchronize()

    def mark(by=d_bytes, bo=blk_off, bl=blk_len, sg=sseg, w=work[:wb]):
        ctx.compact_sst_mark_dev(by, bo, bl, sg, 1, w, totals, blk_entries=ent)

    def gather(by=d_bytes, bo=blk_off, bl=blk_len, sg=sseg, w=work[:wb], ko=offs[:8 * 16]):
        ctx.compact_sst_gather_dev(by, bo, bl, sg, w, key_data[:64], ko.view(torch.int64))

    long_len = blk_len.copy()
    long_len[-1] = buf.size - int(blk_off[-1]) + 1
    common = (dict(sg=[1, int(sseg[2]), int(sseg[1]), int(sseg[3])]),  # sseg descends
              dict(sg=[1, 2, 3, int(sseg[3]) + 1]),                    # sseg[nsrc] > nblk
              dict(bl=long_len),                                        # a claimed block leaves the buffer
              dict(by=d_bytes[:int(blk_off[-1])]),                      # ... of a shorter buffer
              dict(by=None),                                            # NULL bytes with non-empty blocks
              dict(w=work[8:wb + 8]))                                   # not 16-byte aligned
    need = lsmbloom.compact_sst_work_bytes(blk_len[1:])                 # of the claimed blocks alone
    assert need < wb
    mark(w=work[:need])                                                 # (exactly enough; the totals are checked below)
    torch.cuda.synchronize()
    work.fill_(CANARY), totals.fill_(SENTINEL), ent.fill_(SENTINEL)
    torch.cuda.synchronize()
    for bad in common + (dict(w=work[:need - 8]),):                     # work_bytes too small
        with pytest.raises(ValueError):
            mark(**bad)
    for bad in common:
        with pytest.raises(ValueError):
            gather(**bad)
    # the NULL arguments and misaligned offsets, which only the C ABI itself can be handed
    L = lsmbloom.lib()

    def raw_gather(c=ctx.h, s=sseg, w=vp(work.data_ptr()), kd=vp(key_data.data_ptr()), ko=vp(offs.data_ptr())):
        return L.lsmb_compact_sst_gather_dev(c, vp(d_bytes.data_ptr()), d_bytes.numel(), blk_off.size, p(blk_off, u64p),
                                             p(blk_len, u32p), 3, None if s is None else p(s, u64p), w, kd, 64, ko, 16, None)

    for bad in (dict(c=None), dict(s=None), dict(w=None), dict(kd=None), dict(ko=None), dict(ko=vp(offs.data_ptr() + 4))):
        assert raw_gather(**bad) == EINVAL, bad

    def raw(c=ctx.h, o=blk_off, ln=blk_len, s=sseg, w=vp(work.data_ptr()), t=vp(totals.data_ptr())):
        return L.lsmb_compact_sst_mark_dev(c, vp(d_bytes.data_ptr()), d_bytes.numel(), blk_off.size,
                                           None if o is None else p(o, u64p), None if ln is None else p(ln, u32p), 3,
                                           None if s is None else p(s, u64p), 1, w, wb, vp(ent.data_ptr()), t, None)

    for bad in (dict(c=None), dict(o=None), dict(ln=None), dict(s=None), dict(w=None), dict(t=None)):
        assert raw(**bad) == EINVAL, bad
    torch.cuda.synchronize()
    assert bool((work == CANARY).all()) and bool((totals == SENTINEL).all()) and bool((ent == SENTINEL).all())
    assert bool((key_data == CANARY).all()) and bool((offs == CANARY).all()), "a rejected call wrote to a buffer"
    # capacities below the mark's totals: the run is truncated, nothing is written at or past them
    mark()
    torch.cuda.synchronize()
    assert totals.cpu().tolist() == [5, 9, 12, 0]  # ab, k1, abc, the empty key, k4
    ctx.compact_sst_gather_dev(d_bytes, blk_off, blk_len, sseg, work[:wb], key_data[:5], offs[:8 * 3].view(torch.int64))
    torch.cuda.synchronize()
    assert key_data[:5].cpu().numpy().tobytes() == b"abk1a" and bool((key_data[5:] == CANARY).all())
    assert offs[:24].view(torch.int64).cpu().tolist() == [0, 2, 4] and bool((offs[24:] == CANARY).all())
    ctx.close()


def _write_table(tmp_path, ctx, j, entries):
    """One SSTable file: 512-byte data blocks from sst_support, the index over
    them and the tail of finish_sstable with the store's new(1000, 0.01) filter."""
    blocks = ss.split_into_blocks(entries, 512)
    index, at = b"", 0
    for b in blocks:
        index += sstable.encode_index_entry(ss.parse_block(b)[-1], at, len(b))
        at += len(b)
    arena = sstable.KeyArena()
    for k, _ in entries:
        arena.add(k)
    path = str(tmp_path / ("%06d.sst" % j))
    sstable.finish_sstable(path, b"".join(blocks), j, arena, index, ctx=ctx)
    return path


@pytest.mark.gpu
def test_compact_filter_of_three_files(oracle, tmp_path):
    ctx = lsmbloom.Context(0)
    tables = [[(b"user%06d" % i, b"" if (i + j) % 4 == 0 else b"v%d" % j) for i in range(100 * j, 100 * j + 250)]
              for j in range(3)]
    paths = [_write_table(tmp_path, ctx, 40 + j, t) for j, t in enumerate(tables)]
    sources = [ss.split_into_blocks(t, 512) for t in tables]
    for drop in (False, True):
        exp = merge_model(sources, drop)[0]
        assert 250 < len(exp) <= 450
        block, nb, k, count = sstable.compact_filter(paths, drop, ctx=ctx, expected_keys=1000)
        assert (nb, k, count) == (SST[0], SST[1], len(exp)) and block == oracle_block(oracle, exp, *SST)
        block, nb, k, count = sstable.compact_filter(paths, drop, fpr=0.02, ctx=ctx)
        assert (nb, k) == lsmbloom.params(len(exp), 0.02) and count == len(exp)
        assert block == oracle_block(oracle, exp, nb, k)
    # the other order of the files is another compaction
    assert sstable.compact_filter(paths[::-1], True, ctx=ctx)[3] == len(merge_model(sources[::-1], True)[0])
    # a file whose block is damaged: Corruption, as rebuild_filters raises it
    raw = bytearray(open(paths[1], "rb").read())
    region, bo, bl, _ = sstable.read_blocks(paths[1])
    raw[int(bo[1]) + int(bl[1]) - 2:int(bo[1]) + int(bl[1])] = b"\xff\xff"  # the count of the second block
    open(paths[1], "wb").write(bytes(raw))
    with pytest.raises(lsmbloom.Corruption):
        sstable.compact_filter(paths, False, ctx=ctx)
    ctx.close()


@pytest.mark.gpu
def test_cpp_mirror_compact_sst_gpu():
    r = subprocess.run([cpp_bin("compact_sst_test"), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout
