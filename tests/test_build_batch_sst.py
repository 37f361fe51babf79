"""The batched build from the tables' data blocks (lsmb_build_batch_sst_*): the
filters of written SSTables straight from their blocks
([klen u16][vlen u16][key][value] ... [off u16 ...][n u16],
src/sstable/block/builder.rs:40-76), one launch per geometry class, in the
packed layout lsmb_lset_add_batch_dev takes.

Without a GPU: the block format, the plan and build_batch_sst_ref
(csrc/sst_blocks.hpp) on the CPU under ASan and UBSan with every block in an
allocation of exactly its length, the argument checks, the index parser.  On
the GPU: every filter word against the CPU oracle's build of the keys a literal
Python parser (sst_support.parse_block) extracts, exact equality; malformed
blocks among good ones; and the loop the census opened: saturated filters found,
rebuilt from the files' blocks and installed in the next Version.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import keygen
import lsmbloom
import sst_support as ss
from lsmbloom import LevelSet, sstable, u8p, u32p, u64p
from lset_support import cpp_bin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECORRUPT = lsmbloom.LSMB_EINVAL, lsmbloom.LSMB_ECORRUPT
BAD = lsmbloom.LSMB_SST_BAD_BLOCK
vp = ctypes.c_void_p
i32p = ctypes.POINTER(ctypes.c_int32)
SST = lsmbloom.params(1000, 0.01)  # SSTableBuilder's filter: (9586, 7)
WAVE_MAX = 65536                   # kBbWaveMaxBits (csrc/build_batch_plan.hpp): the wave class's largest filter
MAX_BITS = 1310720
GUARD = 64                         # u64 words after the packed buffer
SENTINEL = 0x5A5A5A5A              # blk_entries before a call


def p(a, t):
    return a.ctypes.data_as(t)


def entries(n, first=0, vlen=100, step=1):
    """n sorted entries: 12-byte keys, vlen-byte values."""
    return [(b"user%08d" % (first + step * i), bytes([(first + i) & 0xFF]) * vlen) for i in range(n)]


# ---------------------------------------------------------------- without a GPU

def test_parse_plan_and_reference_host(tmp_path):
    """tests/cpp/sst_blocks_test.cpp: well-formed blocks (0 .. 200 entries, empty
    and 300-byte keys, tombstones, a single entry past 65 535 bytes, odd
    offsets) equal to a literal insert loop over a plain parser's keys;
    malformed blocks and 4 000 random strings reported and never read out of
    bounds; the plan partitions every table's blocks exactly once.  A
    stand-alone program under ASan and UBSan, every block in an allocation of
    exactly its length."""
    exe = str(tmp_path / "sst_blocks_test")
    src = os.path.join(ROOT, "tests", "cpp", "sst_blocks_test.cpp")
    # (the flags of test_plan_layout_and_reference_build_host: the header compiles xxh3.hpp / bloom_math.hpp for the host)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout


def test_support_encoder_parser_and_generators():
    """The helper against itself and the reference's rule: blocks close at
    block_size, a first entry is always accepted, parse(encode(x)) = x's keys."""
    es = entries(1000)
    blocks = ss.split_into_blocks(es, 4096)
    assert all(len(b) <= 4096 for b in blocks) and len(blocks) == 30  # 34 entries of 116 bytes, their offsets and the count
    assert [k for b in blocks for k in ss.parse_block(b)] == [k for k, _ in es]
    # one more entry would not have fitted
    assert all(len(b) + 4 + 12 + 100 > 4096 for b in blocks[:-1])
    big = ss.split_into_blocks([(b"k" * 300, b"v" * 65535), (b"z", b"")], 4096)
    assert len(big) == 2 and len(big[0]) > 65535 and ss.parse_block(big[0]) == [b"k" * 300]
    assert ss.parse_block(ss.encode_block([])) == [] and ss.parse_block(ss.encode_block([(b"", b"")])) == [b""]
    bad = ss.malformed_blocks()
    assert len(bad) >= 30 and all(ss.parse_block(b) is None for b in bad.values())


def test_entry_points_are_exported_and_reject_bad_arguments():
    L = lsmbloom.lib()
    for name in ("lsmb_build_batch_sst_parts", "lsmb_build_batch_sst_dev", "lsmb_build_batch_sst_blocks"):
        assert hasattr(L, name) and name in lsmbloom.SIGNATURES
    assert callable(lsmbloom.Context.build_batch_sst_dev) and callable(lsmbloom.Context.build_batch_sst_blocks)
    assert callable(sstable.parse_index_block) and callable(sstable.read_blocks) and callable(sstable.rebuild_filters)
    assert "build_batch_sst_blocks" in open(os.path.join(ROOT, "storage-engine_amd", "cpp", "lsm_bloom.hpp")).read()
    assert lsmbloom.LSMB_SST_BAD_BLOCK == 0xFFFFFFFF

    nb = np.array([64, SST[0]], np.uint32)
    kk = np.array([1, 7], np.uint32)
    bo = np.array([0, 100, 300], np.uint64)
    bl = np.array([100, 200, 100], np.uint32)
    bseg = np.array([0, 1, 3], np.uint64)
    fake = vp(0x1000)  # never dereferenced: every call below fails its checks first
    total = int(lsmbloom.build_batch_layout(nb)[-1])

    def dev(c=fake, by=vp(0x3000), nbytes=400, nblk=3, o=bo, ln=bl, sg=bseg, b=nb, k=kk, w=vp(0x2000), cap=1 << 20):
        return L.lsmb_build_batch_sst_dev(c, by, nbytes, nblk, None if o is None else p(o, u64p),
                                          None if ln is None else p(ln, u32p), 2, None if sg is None else p(sg, u64p),
                                          None if b is None else p(b, u32p), None if k is None else p(k, u32p), w, cap,
                                          vp(0x4000), None)

    assert dev(c=None) == EINVAL
    assert dev(sg=None) == EINVAL and dev(b=None) == EINVAL and dev(k=None) == EINVAL and dev(w=None) == EINVAL
    assert dev(o=None) == EINVAL and dev(ln=None) == EINVAL          # NULL blk_off / blk_len with nblk > 0
    assert dev(by=None) == EINVAL                                    # NULL d_bytes with a non-empty claimed block
    assert dev(sg=np.array([0, 2, 1], np.uint64)) == EINVAL          # bseg descends
    assert dev(nblk=2) == EINVAL                                     # bseg[ntab] > nblk
    assert dev(nbytes=399) == EINVAL                                 # the last block leaves the buffer
    assert b"block 2" in L.lsmb_last_error()
    assert dev(o=np.array([0, 2**64 - 50, 300], np.uint64)) == EINVAL  # ... also where off + len wraps
    assert dev(cap=total - 1) == EINVAL                              # words_cap below word_off[ntab]
    assert dev(w=vp(0x2008)) == EINVAL                               # not 16-byte aligned
    assert dev(b=np.array([0, SST[0]], np.uint32)) == EINVAL         # no bits with k > 0
    assert dev(b=np.array([64, MAX_BITS + 1], np.uint32)) == EINVAL  # above lsmb_build_batch_max_bits()
    assert b"table 1" in L.lsmb_last_error()
    # an unclaimed block may lie anywhere: only the claimed ones are checked (and here that is all that is)
    assert dev(sg=np.array([0, 1, 2], np.uint64), nbytes=300, cap=total - 1) == EINVAL
    assert b"words_cap" in L.lsmb_last_error()

    # host bytes in, blooms out: no host fallback, outputs untouched
    data = np.zeros(400, np.uint8)
    boff = np.full(3, 7, np.uint64)
    blooms = np.full(2048, 0xAB, np.uint8)
    ent = np.full(2, 9, np.uint64)
    st = np.full(2, 9, np.int32)

    def blk(c=fake, sg=bseg, cap=blooms.size, off=boff, nbytes=400):
        return L.lsmb_build_batch_sst_blocks(c, p(data, u8p), nbytes, 3, p(bo, u64p), p(bl, u32p), 2, p(sg, u64p),
                                             p(nb, u32p), p(kk, u32p), p(blooms, u8p), cap,
                                             None if off is None else p(off, u64p), p(ent, u64p), p(st, i32p))

    untouched = lambda: (boff == 7).all() and (blooms == 0xAB).all() and (ent == 9).all() and (st == 9).all()  # noqa: E731
    assert blk(c=None) == EINVAL and untouched()                     # a NULL ctx is refused whatever the size
    assert blk(off=None) == EINVAL
    assert blk(sg=np.array([0, 2, 1], np.uint64)) == EINVAL and untouched()
    assert blk(nbytes=399) == EINVAL and untouched()
    # a too-small blooms buffer still learns the size
    assert blk(cap=100) == EINVAL and (blooms == 0xAB).all() and (ent == 9).all() and (st == 9).all()
    assert list(boff) == [0, lsmbloom.serialized_size(64), lsmbloom.serialized_size(64) + lsmbloom.serialized_size(SST[0])]


def test_parts_at_least_one_and_non_decreasing_in_bytes():
    for nb in (0, 64, SST[0], WAVE_MAX, WAVE_MAX + 1, MAX_BITS):
        last = 1
        for nbytes in list(range(0, 70)) + list(range(70, 64 << 20, 100003)) + [2**40]:
            parts = lsmbloom.build_batch_sst_parts(1 << 20, nbytes, nb)
            assert parts >= last >= 1, (nb, nbytes)
            last = parts
        assert lsmbloom.build_batch_sst_parts(0, 0, nb) == 1
        assert lsmbloom.build_batch_sst_parts(29, 29 * 4096, nb) == 1   # an SSTable's blocks are one item
        assert lsmbloom.build_batch_sst_parts(3, 2**40, nb) == 3        # a block has one owner
    assert lsmbloom.build_batch_sst_parts(1000, 1000 * 4096, SST[0]) >= 2


def test_parse_index_block_round_trips_and_rejects_truncation():
    ents = [(b"user%08d" % (100 * i), 4096 * i, 4000 + i) for i in range(5)] + [(b"", 2**40, 2**33), (b"k" * 300, 7, 0)]
    buf = b"".join(sstable.encode_index_entry(*e) for e in ents)
    assert sstable.parse_index_block(buf) == ents
    assert sstable.parse_index_block(b"") == []
    for cut in (1, 2, 17, len(buf) - 1, len(buf) - 16, len(buf) - 17 - 300):
        with pytest.raises(lsmbloom.Corruption):
            sstable.parse_index_block(buf[:cut])
    with pytest.raises(lsmbloom.Corruption):
        sstable.parse_index_block(buf + b"\x00")  # one byte left: too short for a key length


def test_cpp_mirror_build_batch_sst_argument_checks():
    r = subprocess.run([cpp_bin("build_batch_sst_test")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


# ---------------------------------------------------------------- on the GPU

def table_keys(blocks):
    return [k for b in blocks for k in ss.parse_block(b)]


def oracle_words(oracle, keys, nb, k):
    nw = (nb + 63) // 64
    if not keys or nw == 0:
        return np.zeros(nw, np.uint64)
    data, offs = keygen.pack(keys)
    return oracle.build_var(data, offs, nb, k)


def lay_out(tables, before, after, tail=0):
    """tables: per table a list of blocks; before / after: unclaimed blocks in
    front of and behind them in the numbering.  In the byte buffer the first
    unclaimed block lies in front, the others in the middle of the tables'
    blocks and the last at the end, every block at an odd offset with junk
    around it -> (bytes, blk_off, blk_len, bseg)."""
    claimed = [b for t in tables for b in t]
    blocks = list(before) + claimed + list(after)
    nb0 = len(before)
    order = list(range(nb0, nb0 + len(claimed)))                # the byte order of the block numbers
    for j in range(1, nb0):
        order.insert(len(order) // 2, j)
    order = ([0] if nb0 else []) + order + list(range(nb0 + len(claimed), len(blocks)))
    buf, offs, lens = ss.place([blocks[i] for i in order], tail=tail)
    blk_off = np.zeros(len(blocks), np.uint64)
    blk_len = np.zeros(len(blocks), np.uint32)
    blk_off[order], blk_len[order] = offs, lens
    bseg = (np.concatenate([[0], np.cumsum([len(t) for t in tables])]) + nb0).astype(np.uint64)
    return buf, blk_off, blk_len, bseg


def run_sst(ctx, buf, blk_off, blk_len, bseg, nb, kk, words=None):
    """One lsmb_build_batch_sst_dev -> (the packed words and the guard after
    them as uint64, word_off, the device words, blk_entries as uint32)."""
    import torch
    dev = torch.device("cuda:0")
    total = int(lsmbloom.build_batch_layout(nb)[-1])
    d_bytes = torch.from_numpy(np.array(buf, dtype=np.uint8)).to(dev)
    if words is None:
        words = torch.full((total + GUARD,), -1, dtype=torch.int64, device=dev)  # every byte 0xFF
    ent = torch.full((max(len(blk_off), 1),), SENTINEL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    woff = ctx.build_batch_sst_dev(d_bytes, blk_off, blk_len, bseg, nb, kk, words[:total], blk_entries=ent)
    torch.cuda.synchronize()
    return words.cpu().numpy().view(np.uint64), woff, words, ent.cpu().numpy().view(np.uint32)[:len(blk_off)]


def check_tables(oracle, got, woff, tables, nb, kk, skip=()):
    for t, blocks in enumerate(tables):
        if t in skip:
            continue
        exp = oracle_words(oracle, table_keys(blocks), nb[t], kk[t])
        w = got[int(woff[t]):int(woff[t]) + exp.size]
        assert np.array_equal(w, exp), (t, len(blocks), nb[t], kk[t], int(np.count_nonzero(w != exp)))
        assert not got[int(woff[t]) + exp.size:int(woff[t + 1])].any(), ("pad words", t)
        if nb[t] % 64:  # tail bits past num_bits stay clear
            assert int(got[int(woff[t]) + exp.size - 1]) >> (nb[t] % 64) == 0


def check_entries(ent, bseg, tables, bad=()):
    b = int(bseg[0])
    assert (ent[:b] == SENTINEL).all() and (ent[int(bseg[-1]):] == SENTINEL).all(), "an unclaimed block's entry was written"
    for blocks in tables:
        for blk in blocks:
            assert int(ent[b]) == (BAD if b in bad else len(ss.parse_block(blk))), b
            b += 1
    assert b == int(bseg[-1])


@pytest.mark.gpu
def test_ragged_tables_unclaimed_blocks_and_odd_offsets(oracle):
    """Tables of no blocks, of one empty block and of 1, 63, 64, 65 and 1 000
    entries in 4 KiB blocks at new(1000, 0.01); unclaimed blocks in front of,
    among and behind the tables' bytes; a buffer of 0xFF and a guard after it."""
    tables = [[], [ss.encode_block([])]] + [ss.split_into_blocks(entries(c, 5000 * c), 4096) for c in (1, 63, 64, 65, 1000)]
    assert len(tables[-1]) == 30 and len(tables[2]) == 1
    before = [ss.encode_block(entries(7, 90000)), b"\xff" * 9, ss.encode_block(entries(3, 91000))]
    after = [b"\xff" * 5]
    buf, blk_off, blk_len, bseg = lay_out(tables, before, after)
    assert all(int(o) % 2 == 1 for o in blk_off)
    claimed_lo = min(int(blk_off[b]) for b in range(int(bseg[0]), int(bseg[-1])))
    claimed_hi = max(int(blk_off[b]) for b in range(int(bseg[0]), int(bseg[-1])))
    assert blk_off[0] < claimed_lo < blk_off[1] < claimed_hi < blk_off[-1]  # in front, among, behind
    nb, kk = [SST[0]] * len(tables), [SST[1]] * len(tables)
    ctx = lsmbloom.Context(0)
    got, woff, _, ent = run_sst(ctx, buf, blk_off, blk_len, bseg, nb, kk)
    ctx.close()
    total = int(woff[-1])
    assert (got[total:] == np.uint64(2**64 - 1)).all(), "guard overwritten"
    check_tables(oracle, got, woff, tables, nb, kk)
    assert not got[int(woff[0]):int(woff[2])].any()  # no keys: all-zero words were written over the 0xFF
    check_entries(ent, bseg, tables)


def _classes_and_parts():
    """Every (num_bits, k) of the two classes' edges, one table split into parts
    per class (the block count by search), a single-entry block past 64 KiB,
    empty keys, tombstones, keys of every XXH3 length class and one table
    whose every key is equal."""
    tables, nb, kk = [], [], []
    r = 0
    for bits in (64, SST[0], WAVE_MAX, WAVE_MAX + 1, MAX_BITS):
        for k in (0, 1, 7, 40):
            tables.append(ss.split_into_blocks(entries((1, 63, 64, 65, 130, 200)[r % 6], 1000 * r, vlen=r % 9), 512))
            nb.append(bits)
            kk.append(k)
            r += 1
    pool = ss.split_into_blocks(entries(45000, 0), 4096)
    sizes = np.cumsum([0] + [len(b) for b in pool])
    for bits in (SST[0], MAX_BITS):
        n = next(n for n in range(1, len(pool) + 1) if lsmbloom.build_batch_sst_parts(n, int(sizes[n]), bits) >= 2)
        tables.append(pool[:n])
        nb.append(bits)
        kk.append(7)
    raw = keygen.stream_bytes(0x5EEDB10C, 301 * 150 + 65535)
    varied = sorted({bytes(raw[301 * i:301 * i + (7 * i) % 301]) for i in range(150)})  # 0 .. 300 bytes, the empty key too
    assert b"" in varied
    tables.append(ss.split_into_blocks([(k, b"v" * (len(k) % 5)) for k in varied], 4096))
    tables.append([ss.encode_block([(b"k" * 300, bytes(raw[-65535:]))]), ss.encode_block([(b"", b""), (b"t", b"")])])
    assert len(tables[-1][0]) > 65536
    tables.append(ss.split_into_blocks([(b"user%08d" % i, b"") for i in range(400)], 512))  # tombstones
    tables.append(ss.split_into_blocks([(b"the same key", b"v%d" % i) for i in range(300)], 512))
    nb += [WAVE_MAX + 1, SST[0], SST[0], SST[0]]
    kk += [7, 7, 7, 7]
    return tables, nb, kk


@pytest.mark.gpu
def test_classes_parts_long_blocks_and_a_dirty_buffer(oracle):
    tables, nb, kk = _classes_and_parts()
    split = [t for t in range(len(tables))
             if lsmbloom.build_batch_sst_parts(len(tables[t]), sum(len(b) for b in tables[t]), nb[t]) >= 2]
    assert any(nb[t] <= WAVE_MAX for t in split) and any(nb[t] > WAVE_MAX for t in split)
    buf, blk_off, blk_len, bseg = lay_out(tables, [b"\xff" * 3], [b"\xff" * 3])
    ctx = lsmbloom.Context(0)
    got, woff, words, ent = run_sst(ctx, buf, blk_off, blk_len, bseg, nb, kk)
    total = int(woff[-1])
    assert (got[total:] == np.uint64(2**64 - 1)).all(), "guard overwritten"
    check_tables(oracle, got, woff, tables, nb, kk)
    check_entries(ent, bseg, tables)
    # again into the now dirty buffer (built filters, not 0xFF): the same bytes
    again, _, _, ent2 = run_sst(ctx, buf, blk_off, blk_len, bseg, nb, kk, words=words)
    ctx.close()
    assert np.array_equal(again, got) and np.array_equal(ent2, ent)


@pytest.mark.gpu
def test_malformed_blocks_among_good_ones(oracle):
    """Four tables, tables 1 and 3 holding one malformed block each, every
    generator of sst_support.malformed_blocks in turn (the ones
    tests/cpp/sst_blocks_test.cpp runs under the sanitizers).  The byte buffer
    ends in 256 KiB of zeros, more than three u16 fields can address from a
    block's start, so that even a wrong parse would stay inside the
    allocation: this checks the reporting."""
    bad = list(ss.malformed_blocks().items())
    good = [ss.split_into_blocks(entries(150, 1000 * t, vlen=20), 512) for t in range(4)]
    nb, kk = [SST[0], SST[0], WAVE_MAX + 1, WAVE_MAX + 1], [7, 7, 7, 7]
    ctx = lsmbloom.Context(0)
    first = None
    for i in range(0, len(bad), 2):
        (n1, b1), (n3, b3) = bad[i], bad[(i + 1) % len(bad)]
        tables = [list(g) for g in good]
        tables[1].insert(2, b1)
        tables[3].append(b3)
        buf, blk_off, blk_len, bseg = lay_out(tables, [b"\xff" * 3], [b"\xff" * 3], tail=256 << 10)
        bad_at = {int(bseg[1]) + 2, int(bseg[4]) - 1}
        got, woff, _, ent = run_sst(ctx, buf, blk_off, blk_len, bseg, nb, kk)
        assert (got[int(woff[-1]):] == np.uint64(2**64 - 1)).all(), ("guard overwritten", n1, n3)
        check_tables(oracle, got, woff, tables, nb, kk, skip=(1, 3))
        check_entries(ent, bseg, tables, bad=bad_at)
        assert sorted(np.nonzero(ent == BAD)[0]) == sorted(bad_at), (n1, n3)
        if first is None:
            first = (tables, buf, blk_off, blk_len, bseg)
    # host bytes in, blooms out: the status per table, the first error named
    tables, buf, blk_off, blk_len, bseg = first
    blooms, boff, entries_, status = ctx.build_batch_sst_blocks(buf, blk_off, blk_len, bseg, nb, kk)
    assert list(status) == [0, ECORRUPT, 0, ECORRUPT]
    L = lsmbloom.lib()
    assert b"table 1" in L.lsmb_last_error() and b"block %d" % (int(bseg[1]) + 2) in L.lsmb_last_error()
    for t in (0, 2):
        exp = oracle.serialize(oracle_words(oracle, table_keys(tables[t]), nb[t], kk[t]), nb[t], kk[t])
        assert blooms[int(boff[t]):int(boff[t + 1])].tobytes() == exp, t
        assert int(entries_[t]) == 150
    # the C return value itself
    nba, kka = np.array(nb, np.uint32), np.array(kk, np.uint32)
    data = np.array(buf, dtype=np.uint8)
    out, off2 = np.zeros(blooms.size, np.uint8), np.zeros(5, np.uint64)
    rc = L.lsmb_build_batch_sst_blocks(ctx.h, p(data, u8p), data.size, blk_off.size, p(blk_off, u64p), p(blk_len, u32p), 4,
                                       p(bseg, u64p), p(nba, u32p), p(kka, u32p), p(out, u8p), out.size, p(off2, u64p),
                                       None, None)
    assert rc == ECORRUPT and b"table 1" in L.lsmb_last_error()
    assert np.array_equal(off2, boff)
    ctx.close()


@pytest.mark.gpu
def test_rejections_leave_every_buffer_untouched():
    import torch
    dev = torch.device("cuda:0")
    ctx = lsmbloom.Context(0)
    tables = [ss.split_into_blocks(entries(100, 0), 512), ss.split_into_blocks(entries(40, 5000), 512)]
    buf, blk_off, blk_len, bseg = lay_out(tables, [b"\xff" * 3], [])
    d_bytes = torch.from_numpy(np.array(buf, dtype=np.uint8)).to(dev)
    nb, kk = [SST[0], 64], [7, 1]
    total = int(lsmbloom.build_batch_layout(nb)[-1])
    words = torch.full((total + GUARD,), -1, dtype=torch.int64, device=dev)
    ent = torch.full((len(blk_off),), SENTINEL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def build(by=d_bytes, bo=blk_off, bl=blk_len, sg=bseg, nb=nb, kk=kk, w=words[:total]):
        ctx.build_batch_sst_dev(by, bo, bl, sg, nb, kk, w, blk_entries=ent)

    long_len = blk_len.copy()
    long_len[-1] = buf.size - int(blk_off[-1]) + 1
    for bad in (dict(w=words[:total - 1]),                                   # words_cap too small
                dict(sg=[1, int(bseg[2]), int(bseg[1])]),                    # bseg descends
                dict(sg=[1, int(bseg[1]), int(bseg[2]) + 1]),                # bseg[ntab] > nblk
                dict(bl=long_len),                                           # a claimed block leaves the buffer
                dict(by=d_bytes[:int(blk_off[-1])]),                         # ... of a shorter buffer
                dict(by=None),                                               # NULL bytes with non-empty blocks
                dict(nb=[SST[0], MAX_BITS + 1]),                             # above the size limit
                dict(nb=[0, 64], kk=[7, 1]),                                 # no bits with k > 0
                dict(w=words.view(torch.uint8)[8:8 + 8 * total].view(torch.int64))):  # not 16-byte aligned
        with pytest.raises(ValueError):
            build(**bad)
    # the NULL arguments, which only the C ABI itself can be handed
    L = lsmbloom.lib()
    bo, bl, sg = blk_off, blk_len, bseg
    nba, kka = np.array(nb, np.uint32), np.array(kk, np.uint32)

    def raw(c=ctx.h, o=bo, ln=bl, s=sg, b=nba, k=kka, w=vp(words.data_ptr())):
        return L.lsmb_build_batch_sst_dev(c, vp(d_bytes.data_ptr()), d_bytes.numel(), bo.size,
                                          None if o is None else p(o, u64p), None if ln is None else p(ln, u32p), 2,
                                          None if s is None else p(s, u64p), None if b is None else p(b, u32p),
                                          None if k is None else p(k, u32p), w, total, vp(ent.data_ptr()), None)

    for bad in (dict(c=None), dict(o=None), dict(ln=None), dict(s=None), dict(b=None), dict(k=None), dict(w=None)):
        assert raw(**bad) == EINVAL, bad
    torch.cuda.synchronize()
    assert bool((words == -1).all()) and bool((ent == SENTINEL).all()), "a rejected batch wrote to a buffer"
    # no tables: fine, and nothing is written
    ctx.build_batch_sst_dev(d_bytes, blk_off, blk_len, [0], [], [], words, blk_entries=ent)
    torch.cuda.synchronize()
    assert bool((words == -1).all()) and bool((ent == SENTINEL).all())
    ctx.close()


def _write_table(tmp_path, ctx, j, keys):
    """One SSTable file: 4 KiB data blocks from sst_support, the index over them
    and the tail of finish_sstable with the store's new(1000, 0.01) filter."""
    blocks = ss.split_into_blocks([(k, b"v" * 100) for k in keys], 4096)
    index, at = b"", 0
    for b in blocks:
        index += sstable.encode_index_entry(ss.parse_block(b)[-1], at, len(b))
        at += len(b)
    arena = sstable.KeyArena()
    for k in keys:
        arena.add(k)
    path = str(tmp_path / ("%06d.sst" % j))
    sstable.finish_sstable(path, b"".join(blocks), j, arena, index, ctx=ctx)
    return path


@pytest.mark.gpu
def test_saturated_filters_found_rebuilt_from_blocks_and_installed(oracle, tmp_path):
    """The loop the census opened: six tables of 3 000 keys behind new(1000,
    0.01) filters; the census names them saturated; their filters are rebuilt
    right-sized from the files' data blocks and installed in the next Version."""
    import torch
    dev = torch.device("cuda:0")
    ctx = lsmbloom.Context(0)
    n, fpr = 3000, 0.01
    big = lsmbloom.params(n, fpr)
    keys = [[b"user%08d" % (20000 * (j // 2) + 8000 * (j % 2) + 2 * i) for i in range(n)] for j in range(6)]
    rows, ids = [j % 2 for j in range(6)], [700 + j for j in range(6)]
    ranges = [(ks[0], ks[-1]) for ks in keys]
    paths = [_write_table(tmp_path, ctx, ids[j], keys[j]) for j in range(6)]

    ls = LevelSet(ctx)
    for j, path in enumerate(paths):
        _, bloom, meta = sstable.read_tail(path)
        assert meta["entry_count"] == n and (meta["min_key"], meta["max_key"]) == ranges[j]
        ls.add(rows[j], ids[j], bloom, meta["min_key"], meta["max_key"])
    ls.seal()
    small = {ids[j]: oracle_words(oracle, keys[j], *SST) for j in range(6)}
    cid, cnb, ckk, set_bits, cfpr, _ = ls.census()
    assert sorted(cid) == ids and (cnb == SST[0]).all() and (ckk == SST[1]).all()
    for i, tid in enumerate(cid):
        assert int(set_bits[i]) == int(sum(bin(int(w)).count("1") for w in small[int(tid)]))
    # 3 000 keys in a filter sized for 1 000: (1 - e^(-7 * 3000 / 9586))^7 = 0.44 against the 0.01 asked for
    assert (cfpr > 0.3).all()

    # host route: right-sized bloom blocks from the files
    exp_words = [oracle_words(oracle, keys[j], *big) for j in range(6)]
    rebuilt = sstable.rebuild_filters(paths, fpr, ctx=ctx)
    for j, (block, nb_j, k_j, ent_j) in enumerate(rebuilt):
        assert (nb_j, k_j, ent_j) == (big[0], big[1], n)
        assert block == oracle.serialize(exp_words[j], *big), j

    # device route: the data regions uploaded as they stand, one build, derive + add_built + seal
    # every member and the absent keys between them
    q = [b"user%08d" % (20000 * (j // 2) + 8000 * (j % 2) + i) for j in range(6) for i in range(2 * n)]
    q += [b"", b"user", b"\xff" * 20]
    parent_before = ls.probe_keys(q)
    regions, offs, lens, bseg = [], [], [], [0]
    for path in paths:
        region, bo, bl, _ = sstable.read_blocks(path)
        offs.append(bo + np.uint64(sum(r.size for r in regions)))
        regions.append(region)
        lens.append(bl)
        bseg.append(bseg[-1] + bo.size)
    d_bytes = torch.from_numpy(np.concatenate(regions)).to(dev)
    nbs, kks = [big[0]] * 6, [big[1]] * 6
    words = torch.full((int(lsmbloom.build_batch_layout(nbs)[-1]),), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.build_batch_sst_dev(d_bytes, np.concatenate(offs), np.concatenate(lens), bseg, nbs, kks, words)
    child = ls.derive(ids)
    assert child.dropped == 6
    child.add_built(rows, ids, words, nbs, kks, ranges)
    del words
    child.seal()
    cid, cnb, ckk, set_bits, cfpr, _ = child.census()
    assert sorted(cid) == ids and (cnb == big[0]).all() and (ckk == big[1]).all()
    for i, tid in enumerate(cid):
        assert int(set_bits[i]) == int(sum(bin(int(w)).count("1") for w in exp_words[ids.index(int(tid))]))
    assert (cfpr < 0.02).all()
    st = child.stats()
    assert st["tables"] == 6 and st["uploaded_bytes"] == 0 and st["upload_copies"] == 0
    ref = LevelSet(ctx)
    ref.add_many(rows, ids, [oracle.serialize(exp_words[j], *big) for j in range(6)], ranges)
    ref.seal()
    a, b = child.probe_keys(q), ref.probe_keys(q)
    assert a.shape == (2, len(q)) and np.array_equal(a, b)
    assert int((a != lsmbloom.LSMB_LSET_NONE).sum()) >= 6 * n  # every member is found
    assert np.array_equal(ls.probe_keys(q), parent_before)     # the parent's answers are unchanged
    for s in (ref, child, ls):
        s.close()
    ctx.close()


@pytest.mark.gpu
def test_cpp_mirror_build_batch_sst_gpu():
    r = subprocess.run([cpp_bin("build_batch_sst_test"), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout
