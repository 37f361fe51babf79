"""A derive that repacks sparse arena chunks on the device
(lsmb_lset_derive_packed) and the segmented copy kernel behind it
(k_copy_segs through lsmb_copy_segs_dev).

Expected probe answers come from the CPU oracle's may_contain, Python's bytes
order and bisect (expected_ids of tests/test_lset.py, expected_mask of
tests/test_lset_version.py), expected orders from the tables themselves, the
copy's expected bytes from numpy slices; never from the library.  Every
comparison is exact equality over all answers.
"""
import ctypes
import subprocess

import numpy as np
import pytest

import keygen
import lsmbloom
from lsmbloom import LevelSet
from lset_support import (CHUNK, SST, batch_args, check_lists, cpp_bin, edit_queries, expected_ids, expected_mask,
                          lists_from_ids, mk)

L0 = lsmbloom.LSMB_LSET_ROW_L0
ALL = lsmbloom.LSMB_LSET_REPACK_ALL
EINVAL = lsmbloom.LSMB_EINVAL
vp = ctypes.c_void_p
ITER = 4096  # one iteration of a wave of k_copy_segs: 64 lanes x 4 loads in flight x 16 B (csrc/lset_repack.hpp)
LENS = [0, 16, 32, 1008, 1024, 1040, 1216, ITER - 16, ITER, ITER + 16, 65536, 65552, 1 << 20]


def slot(t):
    """The arena slot of table t: its words, at least 8 bytes, rounded up to 16."""
    return (max((t[2] + 63) // 64 * 8, 8) + 15) // 16 * 16


def nbytes(t):
    return (t[2] + 63) // 64 * 8


# ------------------------------------------------------------------ the kernel

@pytest.mark.gpu
@pytest.mark.parametrize("lens", [[], [1216], [1040, 0, ITER + 16, 16, 65552], (LENS[:10] * 410)[:4084] + LENS],
                         ids=["0", "1", "5", "4097"])
def test_copy_kernel_moves_every_segment_and_nothing_else(lens):
    """Every length at which k_copy_segs takes another path (nothing, the
    unit loop alone, whole iterations, both; one item's bytes and past it; a
    megabyte on one wave), sources at varied 16-byte offsets, destinations
    between 16-byte guards; 1, 5 and 4 097 segments each leave three idle
    waves in the last workgroup."""
    import torch

    nseg = len(lens)
    assert nseg in (0, 1, 5, 4097) and (nseg < 4097 or set(lens) == set(LENS))
    s_off, d_off, sa, da = [], [], 16, 16
    for i, n in enumerate(lens):
        sa += 16 * (i % 4)  # varied 16-byte offsets, segments of the source not back to back
        s_off.append(sa)
        d_off.append(da)
        sa += n
        da += n + 16  # a guard after every destination
    tail = 4096
    src_h = keygen.stream_bytes(0x5EEDC09A + nseg, sa + 64)
    dst_h = np.full(da + tail, 0xA5, np.uint8)
    src = torch.from_numpy(src_h).to("cuda:0")
    dst = torch.from_numpy(dst_h).to("cuda:0")
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    trip = [[src.data_ptr() + a, dst.data_ptr() + b, n] for a, b, n in zip(s_off, d_off, lens)]
    segs = torch.tensor(trip if trip else [[0, 0, 0]], dtype=torch.int64, device="cuda:0")
    ctx = lsmbloom.Context(0)
    st = torch.cuda.Stream("cuda:0")
    torch.cuda.synchronize()
    ctx.copy_segs_dev(segs, nseg, stream=st.cuda_stream)
    st.synchronize()
    exp = dst_h.copy()
    for a, b, n in zip(s_off, d_off, lens):
        exp[b:b + n] = src_h[a:a + n]
    got = dst.cpu().numpy()
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (bad[:10], got[bad[:10]], exp[bad[:10]])  # destinations, guards and the bytes past the last
    assert np.array_equal(src.cpu().numpy(), src_h)
    ctx.close()


@pytest.mark.gpu
def test_cpp_mirror_repack_gpu():
    r = subprocess.run([cpp_bin("lset_repack_mirror_test"), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout


# ------------------------------------------------------------------- the chain

def _base(oracle):
    """Three rows of 30 tables and five L0 tables; among the SST-sized filters
    a 64-bit one, an odd word count, no bits with no hash, and k = 40."""
    special = {(0, 4): (64, 7), (1, 6): (64 * 151, 7), (2, 1): (0, 0), (2, 9): (4096, 40), (0, 17): (64 * 3, 5)}
    rows = [[mk(oracle, 1000 * (r + 1) + t, 40 * r + 150 * t, *special.get((r, t), SST)) for t in range(30)]
            for r in range(3)]
    l0 = [mk(oracle, 9000 + j, 500 + 75 * j, *((64 * 7, 3) if j == 2 else SST)) for j in range(5)]
    return rows, l0


def _order(rows):
    """table_order from the tables: every row by min_key, rows back to back."""
    ids, base = [], [0]
    for row in rows:
        ids += [t[0] for t in sorted(row, key=lambda t: t[4])]
        base.append(len(ids))
    return ids, base


def _check_version(ls, oracle, rows, l0, q, exp, what):
    """exp: (mask, ids) for (rows, l0) over q, from the oracle."""
    em, ei = exp
    gm, gi = ls.probe_version_keys(q)
    assert np.array_equal(gm, em), (what, np.argwhere(gm != em)[:10])
    assert np.array_equal(gi, ei), (what, np.argwhere(gi != ei)[:10])
    assert np.array_equal(ls.probe_keys(q), ei), what
    ids, base = ls.table_order()
    oi, ob = _order(rows)
    assert ids.tolist() == oi and base.tolist() == ob, what
    assert ls.l0_order().tolist() == [t[0] for t in l0], what
    check_lists(ls.probe_lists_keys(q), lists_from_ids(ei, oi), what)


def _expect(oracle, rows, l0, q):
    return expected_mask(oracle, l0, q)[0], expected_ids(oracle, rows, q)


@pytest.mark.gpu
def test_packed_chain_holds_one_chunk_and_answers_as_the_plain_chain(oracle):
    rows, l0 = _base(oracle)
    rng = np.random.default_rng(41)
    q = edit_queries(rows + [l0], rng, 150 * 40, 700)
    ctx = lsmbloom.Context(0)
    base = LevelSet(ctx)
    base.add_many(*batch_args(oracle, [(r, t) for r, row in enumerate(rows) for t in row] + [(L0, t) for t in l0]))
    base.seal()
    exp = _expect(oracle, rows, l0, q)
    assert (exp[1] != lsmbloom.LSMB_LSET_NONE).sum() > 200 and np.count_nonzero(exp[0]) > 10
    _check_version(base, oracle, rows, l0, q, exp, "base")
    assert base.stats()["chunk_bytes"] == CHUNK
    plain = packed = base
    for g in range(1, 7):
        # two tables go: of the rows, and at g = 3 and 5 one of L0; one arrives: in a row, at even g in L0
        drops = [rows[g % 3][2 * g][0], l0[1][0] if g in (3, 5) else rows[(g + 1) % 3][2 * g + 1][0]]
        new = mk(oracle, 5000 + g, 150 * (31 + g), *(SST if g != 4 else (64 * 9, 11)))
        new_row = L0 if g % 2 == 0 else g % 3
        nrows = [[t for t in row if t[0] not in drops] for row in rows]
        nl0 = [t for t in l0 if t[0] not in drops]
        survivors = [t for row in nrows for t in row] + nl0
        assert len(survivors) == sum(len(r) for r in rows) + len(l0) - 2
        if new_row == L0:
            nl0.append(new)
        else:
            nrows[new_row].append(new)
        exp = _expect(oracle, nrows, nl0, q)
        nxt = []
        for what, cur, repack in (("plain", plain, None), ("packed", packed, "all")):
            ls = cur.derive(drops, repack=repack)
            assert ls.dropped == 2
            assert ls.moved == ((len(survivors), sum(slot(t) for t in survivors)) if repack else (0, 0)), (what, g)
            ls.add_many(*batch_args(oracle, [(new_row, new)]))
            ls.seal()
            _check_version(ls, oracle, nrows, nl0, q, exp, "%s generation %d" % (what, g))
            nxt.append(ls)
        if g > 1:
            plain.close()
            packed.close()
        plain, packed = nxt
        sp, sk = plain.stats(), packed.stats()
        assert sk["chunk_bytes"] == CHUNK, (g, sk)           # the survivors and the new table, in one chunk of its own
        assert sp["chunk_bytes"] == (g + 1) * CHUNK, (g, sp)  # a chunk per edit, and generation 0's
        for s in (sp, sk):
            assert s["uploaded_bytes"] == nbytes(new) and s["upload_copies"] == 1, (g, s)  # the new table only
            assert s["tables"] == len(survivors) + 1
            assert s["filter_bytes"] == sum(nbytes(t) for t in survivors) + nbytes(new)
        assert sp["inherited"] == sk["inherited"] == len(survivors)
        rows, l0 = nrows, nl0
    base.close()
    _check_version(plain, oracle, rows, l0, q, exp, "plain, the base closed")
    _check_version(packed, oracle, rows, l0, q, exp, "packed, the base closed")
    plain.close()
    packed.close()
    ctx.close()


# ---------------------------------------------------------------- independence

@pytest.mark.gpu
def test_packed_child_and_parent_outlive_each_other(oracle):
    rows = [[mk(oracle, 100 * (r + 1) + t, 40 * r + 150 * t, *SST) for t in range(12)] for r in range(2)]
    l0 = [mk(oracle, 900 + j, 300 + 75 * j, *SST) for j in range(3)]
    rng = np.random.default_rng(42)
    q = edit_queries(rows + [l0], rng, 150 * 14, 500)
    exp = _expect(oracle, rows, l0, q)
    ctx = lsmbloom.Context(0)

    def load():
        p = LevelSet(ctx)
        p.add_many(*batch_args(oracle, [(r, t) for r, row in enumerate(rows) for t in row] + [(L0, t) for t in l0]))
        p.seal()
        return p

    drops = [rows[0][3][0], l0[0][0]]
    crow = [[t for t in row if t[0] not in drops] for row in rows]
    cl0 = [t for t in l0 if t[0] not in drops]
    cexp = _expect(oracle, crow, cl0, q)
    # the child after its parent is closed: it holds none of the parent's chunks
    parent = load()
    child = parent.derive(drops, repack="all")
    assert child.moved[0] == 25 and child.stats()["chunk_bytes"] == CHUNK
    child.seal()
    parent.close()
    _check_version(child, oracle, crow, cl0, q, cexp, "child, its parent closed")
    child.close()
    # the parent after the child is closed: its words were only read
    parent = load()
    s_parent = parent.stats()
    child = parent.derive(drops, repack="all")
    child.seal()
    _check_version(child, oracle, crow, cl0, q, cexp, "child")
    child.close()
    _check_version(parent, oracle, rows, l0, q, exp, "parent, the child closed")
    assert parent.stats() == s_parent
    parent.close()
    ctx.close()


# ------------------------------------------------------------------- threshold

@pytest.mark.gpu
def test_threshold_moves_the_sparse_chunk_and_shares_the_dense_one(oracle):
    dense = [mk(oracle, 1, 0, 3 << 23, 7)] + [mk(oracle, 10 + t, 150 * (t + 1), *SST) for t in range(8)]
    assert nbytes(dense[0]) == 3 << 20
    lone = mk(oracle, 77, 150 * 10, *SST)
    rows = [dense + [lone]]
    rng = np.random.default_rng(43)
    q = edit_queries(rows, rng, 150 * 13, 400)
    ctx = lsmbloom.Context(0)
    grand = LevelSet(ctx)
    grand.add_many(*batch_args(oracle, [(0, t) for t in dense]))
    grand.seal()
    parent = grand.derive([])
    parent.add_many(*batch_args(oracle, [(0, lone)]))  # a chunk for one filter: 290 ppm live
    parent.seal()
    grand.close()
    assert parent.stats()["chunk_bytes"] == 2 * CHUNK
    exp = _expect(oracle, rows, [], q)
    _check_version(parent, oracle, rows, [], q, exp, "parent")
    plain = parent.derive([])
    s_plain = plain.stats()
    # half: the sparse chunk's table moves, the dense chunk (3 MiB and more of 4 live) stays shared
    half = parent.derive([], repack=0.5)
    assert half.moved == (1, slot(lone))
    s = half.stats()
    assert s["chunk_bytes"] == 2 * CHUNK and s["inherited"] == 10 and s["uploaded_bytes"] == 0 == s["upload_copies"]
    extra = mk(oracle, 78, 150 * 11, *SST)
    half.add_many(*batch_args(oracle, [(0, extra)]))  # lands behind the moved table, not in a third chunk
    assert half.stats()["chunk_bytes"] == 2 * CHUNK
    half.seal()
    rows_x = [rows[0] + [extra]]
    _check_version(half, oracle, rows_x, [], q, _expect(oracle, rows_x, [], q), "half")
    half.close()
    # zero: lsmb_lset_derive in every respect
    zero = parent.derive([], repack=0)
    assert zero.moved == (0, 0) and zero.dropped == 0
    assert zero.stats() == s_plain
    for ls in (zero, plain):
        ls.add_many(*batch_args(oracle, [(0, extra)]))
        ls.seal()
    assert zero.stats() == plain.stats() and zero.stats()["chunk_bytes"] == 3 * CHUNK
    _check_version(zero, oracle, rows_x, [], q, _expect(oracle, rows_x, [], q), "zero")
    assert np.array_equal(zero.probe_keys(q), plain.probe_keys(q))
    zero.close()
    plain.close()
    _check_version(parent, oracle, rows, [], q, exp, "parent after its children")
    parent.close()
    ctx.close()


@pytest.mark.gpu
def test_filter_in_a_chunk_of_its_own_moves_only_under_all(oracle):
    big = mk(oracle, 500, 150 * 5, 8 * (CHUNK + 16), 7, nkeys=60)
    assert slot(big) == CHUNK + 16 and slot(big) > 64 * 65536  # more than 64 copy items
    small = [mk(oracle, 10 + t, 150 * t, *SST) for t in range(4)]
    rows = [small + [big]]
    rng = np.random.default_rng(44)
    members = [b"user%08d" % i for i in range(150 * 5, 150 * 5 + 100)]
    q = edit_queries(rows, rng, 150 * 8, 300) + members
    exp = _expect(oracle, rows, [], q)
    assert (exp[1][0] == 500).sum() >= 60  # its members hit
    ctx = lsmbloom.Context(0)
    parent = LevelSet(ctx)
    parent.add_many(*batch_args(oracle, [(0, t) for t in rows[0]]))
    parent.seal()
    assert parent.stats()["chunk_bytes"] == 2 * CHUNK + 16
    # live == capacity is not below any share: at 1.0 the big filter stays, the sparse chunk's four move
    one = parent.derive([], repack=1.0)
    assert one.moved == (4, sum(slot(t) for t in small))
    assert one.stats()["chunk_bytes"] == 2 * CHUNK + 16  # the big filter's chunk, shared, and one of its own
    one.seal()
    _check_version(one, oracle, rows, [], q, exp, "repack=1.0")
    one.close()
    every = parent.derive([], repack="all")
    assert every.moved == (5, sum(slot(t) for t in rows[0]))
    assert every.stats()["chunk_bytes"] == 2 * CHUNK + 16  # both its own
    every.seal()
    parent.close()
    _check_version(every, oracle, rows, [], q, exp, "all, the parent closed")
    every.close()
    ctx.close()


# ---------------------------------------------------------------------- errors

@pytest.mark.gpu
def test_packed_derive_argument_errors_and_the_empty_child(oracle):
    tabs = [mk(oracle, 10 + t, 150 * t, *SST) for t in range(5)]
    l0 = [mk(oracle, 20, 100, *SST)]
    ctx = lsmbloom.Context(0)
    parent = LevelSet(ctx)
    parent.add_many(*batch_args(oracle, [(0, t) for t in tabs] + [(L0, t) for t in l0]))
    L = lsmbloom.lib()
    mv = np.full(2, 9, np.uint64)
    pm = mv.ctypes.data_as(lsmbloom.u64p)
    h = vp(123)
    assert L.lsmb_lset_derive_packed(parent.h, None, 0, ALL, None, pm, ctypes.byref(h), None) == EINVAL  # unsealed
    assert h.value is None and (mv == 9).all()
    with pytest.raises(ValueError):
        parent.derive([], repack="all")
    parent.seal()
    assert L.lsmb_lset_derive_packed(parent.h, None, 0, ALL, None, pm, None, None) == EINVAL  # null out
    h = vp(123)
    assert L.lsmb_lset_derive_packed(parent.h, None, 0, ALL + 1, None, pm, ctypes.byref(h), None) == EINVAL
    assert h.value is None and (mv == 9).all() and "min_ppm" in L.lsmb_last_error().decode()
    h = vp(123)
    assert L.lsmb_lset_derive_packed(parent.h, None, 2, ALL, None, pm, ctypes.byref(h), None) == EINVAL  # null drop_ids
    assert h.value is None
    for bad in (1.5, -0.1, "some"):
        with pytest.raises(ValueError):
            parent.derive([], repack=bad)
    s_parent = parent.stats()
    # every table dropped: an empty child that seals
    child = parent.derive([t[0] for t in tabs + l0], repack="all")
    assert child.dropped == 6 and child.moved == (0, 0)
    s = child.stats()
    assert s["tables"] == 0 and s["chunk_bytes"] == 0 and s["inherited"] == 0
    child.seal()
    q = [t[4] for t in tabs] + [b"", b"user"]
    gm, gi = child.probe_version_keys(q)
    assert not gm.any() and (gi == lsmbloom.LSMB_LSET_NONE).all()
    child.close()
    assert parent.stats() == s_parent
    exp = _expect(oracle, [tabs], l0, q)
    _check_version(parent, oracle, [tabs], l0, q, exp, "parent after the refusals")
    parent.close()
    ctx.close()
