"""The store's data blocks for the tests of the batched build from blocks
(test_build_batch_sst.py): an encoder that follows BlockBuilder
(src/sstable/block/builder.rs:40-76), a literal per-entry parser of the format
(the tests' oracle for which keys a block holds) and the malformed blocks.  No
tests here, and nothing below comes from the library."""
import struct

import numpy as np


def encode_block(entries):
    """BlockBuilder::add for every (key, value), then build (block/builder.rs:50-75):
    [klen u16][vlen u16][key][value] ... [off u16 ...][n u16].  Like the
    reference's `as u16`, lengths and offsets wrap; only a first entry can be
    that long."""
    data = bytearray()
    offs = []
    for k, v in entries:
        offs.append(len(data) & 0xFFFF)
        data += struct.pack("<HH", len(k) & 0xFFFF, len(v) & 0xFFFF) + bytes(k) + bytes(v)
    return bytes(data) + b"".join(struct.pack("<H", o) for o in offs) + struct.pack("<H", len(offs))


def split_into_blocks(entries, block_size=4096):
    """SSTableBuilder's cut of sorted entries into blocks by BlockBuilder::add's
    fullness rule (block/builder.rs:41-47): the first entry is always accepted,
    estimated_size() + entry_size > block_size closes the block."""
    blocks, cur, data = [], [], 0
    for k, v in entries:
        size = 4 + len(k) + len(v)
        if cur and data + 2 * len(cur) + 2 + size > block_size:
            blocks.append(encode_block(cur))
            cur, data = [], 0
        cur.append((k, v))
        data += size
    if cur:
        blocks.append(encode_block(cur))
    return blocks


def parse_block(blk):
    """The keys of a block in entry order, entry by entry, or None when the
    block is malformed: the rule of include/lsmbloom.h, read the plain way."""
    blk = bytes(blk)
    if len(blk) < 2:
        return None
    (n,) = struct.unpack_from("<H", blk, len(blk) - 2)
    if 2 + 2 * n > len(blk):
        return None
    data_end = len(blk) - 2 - 2 * n
    keys = []
    for i in range(n):
        (off,) = struct.unpack_from("<H", blk, data_end + 2 * i)
        if off + 4 > data_end:
            return None
        klen, vlen = struct.unpack_from("<HH", blk, off)
        if off + 4 + klen + vlen > data_end:
            return None
        keys.append(blk[off + 4:off + 4 + klen])
    return keys


def malformed_blocks():
    """{name: bytes}: the malformed blocks of tests/cpp/sst_blocks_test.cpp, each
    one checked here to be malformed by parse_block."""
    good = encode_block([(b"user%08d" % i, b"v" * 9) for i in range(5)])  # 5 entries of 25 bytes: data_end = 125
    data_end = len(good) - 2 - 10

    def patched(at, v):
        return good[:at] + struct.pack("<H", v) + good[at + 2:]

    out = {
        "len 0": b"",
        "len 1": b"\x00",
        "n past len": patched(len(good) - 2, 70),
        "n = 65535": patched(len(good) - 2, 65535),
        "off == data_end": patched(data_end + 4, data_end),
        "off past len": patched(data_end + 4, 65535),
        "off + 4 > data_end": patched(data_end + 2, data_end - 2),
        "klen overruns": patched(100, 13),
        "klen = 65535": patched(50, 65535),
        "vlen overruns": patched(102, 10),
        "vlen = 65535": patched(27, 65535),
        "all 0xFF": b"\xff" * 100,
        "all 0xFF, long": b"\xff" * 200000,  # n = 65 535 fits; every offset, klen and vlen is 65 535
    }
    rng = np.random.default_rng(77)
    for r in range(40):
        b = rng.integers(0, 256, int(rng.integers(0, 601)), dtype=np.uint8).tobytes()
        if parse_block(b) is None:
            out["random %d" % r] = b
    for name, b in out.items():
        assert parse_block(b) is None, name
    return out


def place(blocks, gap=b"\xee", odd=True, tail=0):
    """Blocks laid into one byte buffer with `gap` between them, each at an odd
    offset when `odd` -> (bytes uint8 with `tail` zero bytes behind, blk_off
    uint64, blk_len uint32)."""
    buf = bytearray()
    offs = []
    for b in blocks:
        buf += gap
        if odd and len(buf) % 2 == 0:
            buf += gap[:1] or b"\xee"
        offs.append(len(buf))
        buf += b
    buf += bytes(tail)
    return (np.frombuffer(bytes(buf), dtype=np.uint8), np.array(offs, dtype=np.uint64),
            np.array([len(b) for b in blocks], dtype=np.uint32))
