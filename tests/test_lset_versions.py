"""The life cycle of a level set (lsmb_lset) across Versions: a batched,
optionally CRC-checked load (lsmb_lset_add_batch, the segmented CRC kernel
behind it) and successor snapshots that share the resident filter words
(lsmb_lset_derive, the edit of src/compaction/scheduler.rs:163-177:
retain(!input_ids.contains(id)) over every level, then push), with
lsmb_lset_stats counting what was uploaded and what is kept alive.

Expected probe answers come from the CPU oracle's may_contain, Python's bytes
order and bisect (expected_ids of tests/test_lset.py); CRCs from zlib.crc32;
never from the library.  Every comparison is exact equality over all answers.
"""
import ctypes
import os
import subprocess
import zlib

import numpy as np
import pytest

import keygen
import lsmbloom
from lsmbloom import LevelSet
from lset_support import (CHUNK, SST, batch_args, block, check_lists, cpp_bin, edit_queries, expected_ids, lists_from_ids,
                          mk)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = lsmbloom.LSMB_LSET_NONE
vp = ctypes.c_void_p
def check_probe(ls, oracle, rows, q, what=""):
    """Var-len keys through probe_keys, and the 12-byte ones again as fixed-length keys."""
    exp = expected_ids(oracle, rows, q)
    got = ls.probe_keys(q)
    assert got.shape == exp.shape, what
    assert np.array_equal(got, exp), (what, np.argwhere(got != exp)[:10])
    fixed = [i for i, kk in enumerate(q) if len(kk) == 12][:1000]
    data = np.frombuffer(b"".join(q[i] for i in fixed), dtype=np.uint8)
    assert np.array_equal(ls.probe(data, key_len=12), exp[:, fixed]), what
    return exp


def arena_chunks(nwords):
    """Chunks a fresh set touches for filters of these word counts, in order:
    16-byte-aligned slots bump-allocated in 4 MiB chunks, a larger filter in a chunk of its own."""
    chunks, used, cap = 0, 0, 0
    for nw in nwords:
        b = (max(nw * 8, 8) + 15) // 16 * 16
        if chunks == 0 or used + b > cap:
            chunks, used, cap = chunks + 1, 0, max(b, CHUNK)
        used += b
    return chunks


# ---------------------------------------------------------------- without a GPU

def test_crc_segment_arithmetic_host(tmp_path):
    """crc_seg_ref (csrc/crc_seg.hpp), the serial statement of k_crc32_seg's
    pieces and tree, against a bit-at-a-time CRC-32 at every length of a small
    block and at the piece, wave and 128 KiB boundaries
    (tests/cpp/crc_seg_test.cpp), under ASan and UBSan; the combine triples it
    prints against lsmb_crc32_combine."""
    exe = str(tmp_path / "crc_seg_test")
    src = os.path.join(ROOT, "tests", "cpp", "crc_seg_test.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout
    triples = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("combine ")]
    assert len(triples) == 8
    for ca, cb, lb, whole in triples:
        assert lsmbloom.crc32_combine(int(ca, 16), int(cb, 16), int(lb)) == int(whole, 16)
    a, b = b"bloom block header", bytes(range(256)) * 5
    assert lsmbloom.crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(a + b)


def test_arena_placement_host(tmp_path):
    """lset_place (csrc/lset_arena.hpp), the pure placement every level-set add
    plans before it allocates or copies, against the one-table-at-a-time bump
    loop it replaced, restated (tests/cpp/lset_arena_test.cpp): empty batches,
    16-byte slots, runs ending on the 4 MiB boundary, filters of and past 4 MiB,
    an inherited tail, a full arena, chains of random batches; slots aligned,
    disjoint and in bounds, spans tiling the tables, packed offsets equal to the
    batched build's layout, chunk counts equal to arena_chunks above.  Under
    ASan and UBSan."""
    exe = str(tmp_path / "lset_arena_test")
    src = os.path.join(ROOT, "tests", "cpp", "lset_arena_test.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout


def test_version_entry_points_are_exported_and_reject_null():
    L = lsmbloom.lib()
    for name in ("lsmb_lset_derive", "lsmb_lset_add_batch", "lsmb_lset_stats", "lsmb_crc32_seg_dev"):
        assert hasattr(L, name) and name in lsmbloom.SIGNATURES
    for name in ("derive", "add_many", "stats"):
        assert callable(getattr(LevelSet, name))
    h = vp(123)
    ids = np.array([1, 2], np.uint32)
    nd = np.full(1, 7, np.uint64)
    pi, pn = ids.ctypes.data_as(lsmbloom.u32p), nd.ctypes.data_as(lsmbloom.u64p)
    assert L.lsmb_lset_derive(None, pi, 2, pn, ctypes.byref(h)) == lsmbloom.LSMB_EINVAL
    assert h.value is None and nd[0] == 7  # *out is cleared, *dropped untouched
    assert L.lsmb_lset_derive(None, None, 2, None, ctypes.byref(h)) == lsmbloom.LSMB_EINVAL
    assert L.lsmb_lset_derive(None, None, 0, None, None) == lsmbloom.LSMB_EINVAL
    one = np.zeros(16, np.uint8)
    off = np.array([0, 12], np.uint64)
    koff = np.array([0, 1, 2], np.uint64)
    st = np.full(1, 5, np.int32)
    p8 = one.ctypes.data_as(lsmbloom.u8p)
    assert L.lsmb_lset_add_batch(None, 1, pi, pi, p8, off.ctypes.data_as(lsmbloom.u64p), None, p8,
                                 koff.ctypes.data_as(lsmbloom.u64p),
                                 st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == lsmbloom.LSMB_EINVAL
    assert L.lsmb_lset_add_batch(None, 0, None, None, None, None, None, None, None, None) == lsmbloom.LSMB_EINVAL
    out = np.full(6, 9, np.uint64)
    assert L.lsmb_lset_stats(None, out.ctypes.data_as(lsmbloom.u64p)) == lsmbloom.LSMB_EINVAL
    assert (out == 9).all() and st[0] == 5
    assert L.lsmb_crc32_seg_dev(None, vp(16), 1, vp(16), None) == lsmbloom.LSMB_EINVAL
    assert L.lsmb_abi_version() == 6




def test_cpp_mirror_version_argument_checks():
    r = subprocess.run([cpp_bin("lset_versions_test")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


def test_arena_chunks_of_the_test_itself():
    assert arena_chunks([]) == 0 and arena_chunks([0]) == 1 and arena_chunks([1] * 1000) == 1
    assert arena_chunks([CHUNK // 8]) == 1 and arena_chunks([CHUNK // 8, 1]) == 2
    assert arena_chunks([1, CHUNK // 8 + 1, 1]) == 3  # a filter past a chunk takes one of its own


# ------------------------------------------------------------------- on the GPU

@pytest.mark.gpu
def test_segmented_crc_kernel_matches_zlib():
    """k_crc32_seg through lsmb_crc32_seg_dev: lengths around every boundary
    of its geometry (16 B pieces, one piece per lane, 128 KiB, past it), odd
    tails, unaligned segments, and a last workgroup that is not full."""
    import torch

    lens = list(range(0, 8 * 130, 8)) + [1208, 1209, 1215, 1, 7, 15, 17, 1023, 1025, 4800, 32768 - 8, 32768, 32776,
                                         131072 - 8, 131072, 131072 + 8, 131073, 262152]
    shifts = [0] * len(lens)
    lens += [64, 1208, 5000]
    shifts += [4, 8, 1]  # not 16-byte aligned: the byte loop
    assert len(lens) % 4 != 0
    offs, at = [], 0
    for n, s in zip(lens, shifts):
        offs.append(at + s)
        at += (n + s + 15) // 16 * 16 + 16
    host = keygen.stream_bytes(0x5EED0C2C, at)
    dev = torch.from_numpy(host).to("cuda:0")
    base = dev.data_ptr()
    assert base % 16 == 0
    segs = torch.tensor([[base + o, n] for o, n in zip(offs, lens)], dtype=torch.int64, device="cuda:0")
    out = torch.full((len(lens) + 3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    ctx = lsmbloom.Context(0)
    st = torch.cuda.Stream("cuda:0")
    torch.cuda.synchronize()
    ctx.crc32_seg_dev(segs, len(lens), out, stream=st.cuda_stream)
    st.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    exp = np.array([zlib.crc32(host[o:o + n].tobytes()) for o, n in zip(offs, lens)], dtype=np.uint32)
    bad = np.nonzero(got[:len(lens)] != exp)[0]
    assert bad.size == 0, [(lens[i], shifts[i], hex(got[i]), hex(exp[i])) for i in bad[:10]]
    assert (got[len(lens):] == 0x5A5A5A5A).all()  # nothing past nseg is written
    ctx.crc32_seg_dev(segs, 0, out, stream=st.cuda_stream)  # nseg == 0: nothing launched
    st.synchronize()
    ctx.close()


@pytest.mark.gpu
def test_cpp_mirror_versions_gpu():
    r = subprocess.run([cpp_bin("lset_versions_test"), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout


def _two_rows(oracle):
    """Two rows, 36 tables each, 150 ids apart; among the SST-sized filters one
    of every size at which the load takes another path."""
    special = {
        (0, 3): (0, 0),                # no bits, no hash: a 12-byte block
        (0, 5): (64, 7),               # one word: a 20-byte block
        (0, 8): (64, 0),               # k = 0
        (0, 20): (1 << 20, 7),         # 128 KiB: the last length of the segmented kernel's wave path
        (1, 2): (1 << 21, 7),          # 256 KiB: past it, the CRC goes through the workgroup kernel
        (1, 9): ((1 << 25) + 64, 7),   # just past a 4 MiB chunk: a chunk of its own
        (1, 14): lsmbloom.params(40, 1e-4),  # k > 8
    }
    rows = []
    for r in range(2):
        rows.append([mk(oracle, 1000 * r + t + 7, 40 * r + 150 * t, *special.get((r, t), SST)) for t in range(36)])
    return rows


@pytest.fixture(scope="module")
def two_rows(oracle):
    return _two_rows(oracle)


@pytest.mark.gpu
def test_batch_load_equals_the_per_table_loop(oracle, two_rows):
    rows = two_rows
    rng = np.random.default_rng(31)
    flat = [(r, t) for r, tabs in enumerate(rows) for t in tabs]
    placed = [flat[j] for j in rng.permutation(len(flat))]  # any order, rows interleaved
    args = batch_args(oracle, placed)
    crcs = [zlib.crc32(b) for b in args[2]]
    assert sorted(len(b) for b in args[2])[:2] == [12, 20] and max(len(b) for b in args[2]) == 12 + (1 << 22) + 8
    nwords = [(t[2] + 63) // 64 for _, t in placed]
    touched = arena_chunks(nwords)
    assert 2 <= touched <= 3  # the first chunk, the large filter's own and, unless it came last, one more
    q = edit_queries(rows, rng, 150 * 36 + 200, 3000)
    assert len(q) <= 4000
    ctx = lsmbloom.Context(0)
    loop = LevelSet(ctx)
    for r, t in placed:
        loop.add(r, t[0], block(oracle, t), t[4], t[5])
    loop.seal()
    exp = check_probe(loop, oracle, rows, q, "loop")
    assert (exp != NONE).sum() > 1000 and (exp == NONE).sum() > 1000
    s_loop = loop.stats()
    assert s_loop["upload_copies"] == sum(1 for n in nwords if n)  # one copy per table
    for what, cc in (("batch", None), ("batch+crc", crcs)):
        ls = LevelSet(ctx)
        status = ls.add_many(*args, crcs=cc)
        assert status.dtype == np.int32 and status.shape == (72,) and (status == 0).all()
        assert ls.rows() == 2 and ls.tables(0) == 36 and ls.tables(1) == 36
        s = ls.stats()
        print(what, s)
        assert s["upload_copies"] <= touched + 1, s
        assert s["tables"] == 72 and s["inherited"] == 0
        assert s["uploaded_bytes"] == s["filter_bytes"] == 8 * sum(nwords) == s_loop["uploaded_bytes"]
        assert s["chunk_bytes"] == s_loop["chunk_bytes"] >= s["filter_bytes"]
        ls.seal()
        got = ls.probe_keys(q)
        assert np.array_equal(got, exp), (what, np.argwhere(got != exp)[:10])
        assert np.array_equal(got, loop.probe_keys(q)), what
        ls.close()
    # an empty batch is LSMB_OK and adds nothing; a batch after seal is refused
    ls = LevelSet(ctx)
    assert ls.add_many([], [], [], []).shape == (0,) and ls.stats()["tables"] == 0
    ls.seal()
    with pytest.raises(ValueError):
        ls.add_many(*batch_args(oracle, placed[:2]))
    ls.close()
    loop.close()
    ctx.close()


@pytest.mark.gpu
def test_batch_corruption_is_all_or_nothing(oracle, two_rows):
    rows = two_rows
    ctx = lsmbloom.Context(0)
    ls = LevelSet(ctx)
    for t in rows[0][:3]:  # a set that already holds something
        ls.add(0, t[0], block(oracle, t), t[4], t[5])
    placed = [(0, rows[0][4]), (0, rows[0][5]), (1, rows[1][1]), (0, rows[0][6]), (1, rows[1][2]), (1, rows[1][3])]
    args = batch_args(oracle, placed)
    good = args[2]
    crcs = [zlib.crc32(b) for b in good]
    assert [len(b) for b in good][1] == 20 and len(good[0]) == 12 + 8 * lsmbloom.num_words(SST[0])
    assert len(good[4]) == 12 + (256 << 10)
    before = (ls.tables(0), ls.tables(1), ls.stats())

    def refused(blocks, cc, idx, exc=lsmbloom.Corruption):
        with pytest.raises(exc) as ei:
            ls.add_many(args[0], args[1], blocks, args[3], crcs=cc)
        assert np.nonzero(ei.value.status)[0].tolist() == [idx], ei.value.status
        assert "table %d of the batch (id %d)" % (idx, args[1][idx]) in str(ei.value)
        assert (ls.tables(0), ls.tables(1), ls.stats()) == before
        return ei.value

    # one flipped bit in the words of the 20-byte block, an SST-sized one and the 256 KiB one
    for idx, byte, bit in ((1, 12 + 5, 3), (0, 12 + 700, 0), (4, 12 + 200_001, 7)):
        bad = list(good)
        b = bytearray(good[idx])
        b[byte] ^= 1 << bit
        bad[idx] = bytes(b)
        e = refused(bad, crcs, idx)
        assert e.status[idx] == lsmbloom.LSMB_ECORRUPT and "CRC-32" in str(e)
    # a wrong CRC over intact bytes fails the same way
    wrong = list(crcs)
    wrong[3] ^= 0x00010000
    refused(good, wrong, 3)
    # a truncated block fails header validation, with or without CRCs, before anything is uploaded
    short = list(good)
    short[2] = good[2][:-8]
    for cc in (None, crcs):
        refused(short, cc, 2)
    assert ls.stats()["uploaded_bytes"] == before[2]["uploaded_bytes"]
    # an argument error is LSMB_EINVAL for its table
    args_bad = list(args)
    args_bad[1] = list(args[1])
    args_bad[1][5] = NONE
    with pytest.raises(ValueError) as ei:
        ls.add_many(*args_bad, crcs=crcs)
    assert np.nonzero(ei.value.status)[0].tolist() == [5] and ei.value.status[5] == lsmbloom.LSMB_EINVAL
    assert (ls.tables(0), ls.tables(1), ls.stats()) == before
    # the same batch with the right bytes then succeeds and probes exactly
    assert (ls.add_many(*args, crcs=crcs) == 0).all()
    assert (ls.tables(0), ls.tables(1)) == (before[0] + 3, before[1] + 3)
    ls.seal()
    mine = [rows[0][:3] + [t for r, t in placed if r == 0], [t for r, t in placed if r == 1]]
    check_probe(ls, oracle, mine, edit_queries(mine, np.random.default_rng(32), 150 * 8, 1500), "after the refusals")
    ls.close()
    ctx.close()


def _ids_of(rows):
    return [[t[0] for t in row] for row in rows]


@pytest.mark.gpu
def test_derive_shares_the_parent_and_outlives_it(oracle):
    rows = [[mk(oracle, 100 * (r + 1) + t, 40 * r + 150 * t, *SST) for t in range(40)] for r in range(2)]
    rows[0][7] = (777,) + rows[0][7][1:]   # one id held by two tables, in different rows
    rows[1][11] = (777,) + rows[1][11][1:]
    rng = np.random.default_rng(33)
    ctx = lsmbloom.Context(0)
    parent = LevelSet(ctx)
    placed = [(r, t) for r, tabs in enumerate(rows) for t in tabs]
    parent.add_many(*batch_args(oracle, placed))
    with pytest.raises(ValueError):
        parent.derive([103])  # an unsealed parent
    parent.seal()
    L = lsmbloom.lib()
    h = vp()
    assert L.lsmb_lset_derive(parent.h, None, 3, None, ctypes.byref(h)) == lsmbloom.LSMB_EINVAL and h.value is None
    assert L.lsmb_lset_derive(parent.h, None, 0, None, None) == lsmbloom.LSMB_EINVAL
    q = edit_queries(rows, rng, 150 * 41 + 200, 2500)
    check_probe(parent, oracle, rows, q, "parent")
    s_parent = parent.stats()
    drops = [777, 103, 215, 239, 99999]  # 777 twice, 99999 absent
    child = parent.derive(drops)
    assert child.dropped == 5
    assert child.rows() == 2 and child.tables(0) == 38 and child.tables(1) == 37
    with pytest.raises(ValueError):
        child.probe_keys([b"user00000000"])  # unsealed
    new = [(0, mk(oracle, 5001, 150 * 3, *SST)),            # into the gap table 103 left
           (0, mk(oracle, 5002, 150 * 40, 1 << 15, 5)),     # past the row's last table
           (1, mk(oracle, 5003, 40 + 150 * 15, 640, 3))]    # into the gap table 215 left
    child.add(new[0][0], new[0][1][0], block(oracle, new[0][1]), new[0][1][4], new[0][1][5])
    child.add_many(*batch_args(oracle, new[1:]), crcs=[zlib.crc32(block(oracle, t)) for _, t in new[1:]])
    child.seal()
    crow = [[t for t in row if t[0] not in drops] for row in rows]
    for r, t in new:
        crow[r].append(t)
    s = child.stats()
    assert s["tables"] == 78 and s["inherited"] == 75
    assert s["uploaded_bytes"] == 8 * sum((t[2] + 63) // 64 for _, t in new)  # the three new filters only
    assert s["upload_copies"] == 2  # one add, one batch in one chunk
    assert s["chunk_bytes"] == s_parent["chunk_bytes"] + CHUNK  # the parent's chunk and one of its own
    cexp = check_probe(child, oracle, crow, q, "child")
    assert np.array_equal(parent.probe_keys(q), expected_ids(oracle, rows, q))  # the parent is untouched
    assert parent.stats() == s_parent
    # the child's lists are the ones its probe implies
    ids, base = child.table_order()
    assert base.tolist() == [0, 40, 78]
    check_lists(child.probe_lists_keys(q), lists_from_ids(cexp, ids), "child lists")
    # a second child of the same parent: neither writes where the other did
    other = parent.derive([100])
    other.add(0, 6001, block(oracle, new[0][1]), b"zz0", b"zz1")
    other.seal()
    assert np.array_equal(child.probe_keys(q), cexp)
    other.close()
    assert np.array_equal(parent.probe_keys(q), expected_ids(oracle, rows, q))
    parent.close()  # the child holds the shared chunks now
    assert np.array_equal(child.probe_keys(q), cexp)
    assert child.stats() == s
    # and the other order: a grandchild closed before its parent
    grand = child.derive([5002])
    grand.seal()
    gexp = expected_ids(oracle, [[t for t in row if t[0] != 5002] for row in crow], q)
    assert np.array_equal(grand.probe_keys(q), gexp)
    assert grand.stats()["uploaded_bytes"] == 0 and grand.stats()["inherited"] == 77
    grand.close()
    assert np.array_equal(child.probe_keys(q), cexp)
    child.close()
    ctx.close()


@pytest.mark.gpu
def test_chain_of_six_versions_lets_go_of_the_first(oracle):
    tabs = [mk(oracle, t, 150 * t, *SST) for t in range(12)]
    rng = np.random.default_rng(34)
    q = edit_queries([tabs], rng, 150 * 20, 1500)
    ctx = lsmbloom.Context(0)
    cur = LevelSet(ctx)
    cur.add_many(*batch_args(oracle, [(0, t) for t in tabs]))
    cur.seal()
    check_probe(cur, oracle, [tabs], q, "generation 0")
    assert cur.stats()["chunk_bytes"] == CHUNK
    live = list(tabs)
    for g in range(1, 7):
        nxt = cur.derive([2 * g - 2, 2 * g - 1])  # two of the original tables go
        assert nxt.dropped == 2
        t = mk(oracle, 100 + g, 150 * (12 + g), *SST)
        nxt.add_many(*batch_args(oracle, [(0, t)]), crcs=[zlib.crc32(block(oracle, t))])
        nxt.seal()
        cur.close()  # the parent goes right after the seal
        cur = nxt
        live = [x for x in live if x[0] not in (2 * g - 2, 2 * g - 1)] + [t]
        check_probe(cur, oracle, [live], q, "generation %d" % g)
        s = cur.stats()
        assert s["tables"] == 12 - g and s["inherited"] == 11 - g
        # every generation brought one chunk; the first one's is held while one of its tables is
        assert s["chunk_bytes"] == (g + (1 if g < 6 else 0)) * CHUNK, (g, s)
    assert [t[0] for t in live] == [101, 102, 103, 104, 105, 106]  # every original table is gone
    s = cur.stats()
    assert s["chunk_bytes"] == 6 * CHUNK  # none of generation 0's
    assert s["filter_bytes"] == 6 * 8 * lsmbloom.num_words(SST[0])
    assert 0 < s["occupancy"] < 0.001  # what a caller reads before it rebuilds a fresh set
    cur.close()
    ctx.close()


@pytest.mark.gpu
def test_bad_edit_leaves_the_child_unsealed_and_the_parent_whole(oracle):
    tabs = [mk(oracle, 10 + t, 150 * t, *SST) for t in range(6)]
    rng = np.random.default_rng(35)
    q = edit_queries([tabs], rng, 150 * 8, 1200)
    ctx = lsmbloom.Context(0)
    parent = LevelSet(ctx)
    parent.add_many(*batch_args(oracle, [(0, t) for t in tabs]))
    parent.seal()
    over = mk(oracle, 4242, 150 * 2 + 50, *SST)  # starts inside table 12's range
    assert tabs[2][4] < over[4] < tabs[2][5]
    child = parent.derive([])
    assert child.dropped == 0
    child.add_many(*batch_args(oracle, [(0, over)]))
    with pytest.raises(ValueError) as ei:
        child.seal()
    assert "12" in str(ei.value) and "4242" in str(ei.value) and "overlap" in str(ei.value)
    with pytest.raises(ValueError):
        child.probe_keys([b"user00000000"])  # still unsealed
    check_probe(parent, oracle, [tabs], q, "parent after the refused seal")
    child.close()
    # the edit again, without the inherited table in the way
    child = parent.derive([12])
    child.add_many(*batch_args(oracle, [(0, over)]))
    child.seal()
    check_probe(child, oracle, [[t for t in tabs if t[0] != 12] + [over]], q, "child")
    check_probe(parent, oracle, [tabs], q, "parent")
    parent.close()
    child.close()
    ctx.close()
