"""Reference models, table builders and workloads shared by the level-set and
filter-set test modules (test_lset*.py, test_fset*.py, test_gpu_wide_moduli.py),
and the one way they reach a C++ mirror test binary.  No tests here: every
expectation below comes from the CPU oracle, Python's bytes ordering and numpy,
never from the library."""
import bisect
import functools
import os
import subprocess

import numpy as np

import keygen
import lsmbloom
from lsmbloom import BloomFilter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = lsmbloom.LSMB_LSET_NONE


def cpp_bin(target):
    """storage-engine_amd/build/<target>, made first where it is missing."""
    path = os.path.join(ROOT, "storage-engine_amd", "build", target)
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "storage-engine_amd"), "build/" + target], check=True)
    return path


# ------------------------------------------------- level-set rows (test_lset.py)

def expected_ids(oracle, rows, keys):
    """rows: per row, a list of (table_id, words, num_bits, k, lo, hi) with
    disjoint [lo, hi] -> uint32 [len(rows), len(keys)]."""
    out = np.full((len(rows), len(keys)), NONE, dtype=np.uint32)
    for r, tabs in enumerate(rows):
        tabs = sorted(tabs, key=lambda t: t[4])
        los = [t[4] for t in tabs]
        for a, b in zip(tabs, tabs[1:]):
            assert a[4] <= a[5] < b[4], "the test's own tables overlap"
        for i, key in enumerate(keys):
            j = bisect.bisect_right(los, key) - 1  # the last table whose min_key <= key
            if j < 0:
                continue
            tid, w, nb, k, _lo, hi = tabs[j]
            if key <= hi and oracle.may_contain(w, nb, k, key):
                out[r, i] = tid
    return out


def build_table(oracle, tid, keys, sizing, k=None):
    """(table_id, words, num_bits, k, min_key, max_key) of sorted `keys`, the
    filter sized by lsmbloom.params(*sizing); k overrides num_hashes."""
    nb, kk = lsmbloom.params(*sizing)
    data, offs = keygen.pack(keys)
    w = oracle.build_var(data, offs, nb, kk if k is None else k)
    return (tid, w, nb, kk if k is None else k, keys[0], keys[-1])


def add_tables(ls, oracle, row, tabs):
    """Adds a row's tables: most from the serialized block, every third and
    each k = 0 one from the filter words."""
    for tid, w, nb, k, lo, hi in tabs:
        if k == 0 or tid % 3 == 0:
            ls.add_filter(row, tid, BloomFilter(w, k, nb), lo, hi)
        else:
            ls.add(row, tid, oracle.serialize(w, nb, k), lo, hi)


SIZINGS = [(40, 0.01), (1000, 0.01), (40000, 0.01), (40, 1e-4)]  # SST-small, < 2^14 bits, > 2^14 bits, k > 8


# ----------------------------------- per-table lists (test_lset_lists.py)

POISON = 0xDEADBEEF


def lists_from_ids(ids_rn, order_ids):
    """probe()'s uint32 [R, n] table ids + table_order()'s ids (unique) ->
    (starts uint64[G + 1], index uint32[total])."""
    order_ids = np.asarray(order_ids, dtype=np.uint32)
    G = order_ids.size
    assert np.unique(order_ids).size == G, "the expectation needs unique table ids"
    R, n = ids_rn.shape
    flat = ids_rn.reshape(-1)                      # (row, key) order
    hit = flat != NONE
    sorter = np.argsort(order_ids, kind="stable")
    if G:
        pos = np.searchsorted(order_ids[sorter], flat[hit])
        assert (order_ids[sorter][pos] == flat[hit]).all()
        ordinal = sorter[pos]
    else:
        assert not hit.any()
        ordinal = np.zeros(0, np.int64)
    key_idx = np.tile(np.arange(n, dtype=np.uint32), R)[hit]
    by_table = np.argsort(ordinal, kind="stable")
    starts = np.searchsorted(ordinal[by_table], np.arange(G + 1), side="left").astype(np.uint64)
    return starts, key_idx[by_table]


def check_lists(got, exp, what=""):
    starts, index = got
    es, ei = exp
    assert starts.dtype == np.uint64 and starts.shape == es.shape, what
    assert index.dtype == np.uint32, what
    assert np.array_equal(starts, es), (what, np.argwhere(starts != es)[:10])
    assert index.shape == ei.shape and np.array_equal(index, ei), (what, index[:20], ei[:20])
    for g in np.nonzero(np.diff(es.astype(np.int64)) > 1)[0][:50]:  # (implied by equality; states the contract)
        run = index[int(es[g]):int(es[g + 1])]
        assert (np.diff(run.astype(np.int64)) > 0).all(), (what, g)


def always_maybe():
    """A 64-bit filter with no hash: may_contain is always true, so only the
    range decides, and adding it is cheap."""
    return BloomFilter(np.zeros(1, np.uint64), 0, 64)


def dev_lists(ls, dq, n, cap=None, key_len=16, offsets=None, stream=None, work=None):
    """probe_lists_dev into fresh tensors: starts pre-filled with -1, index
    (cap entries; None: sized by a counting call) with POISON.  Returns
    (starts uint64, index uint32 [cap]) on the host, the whole index buffer."""
    import torch

    G = ls.total_tables()
    dev = dq.device
    if work is None:
        work = torch.empty(max(ls.lists_work_bytes(n), 1), dtype=torch.uint8, device=dev)
    starts = torch.full((G + 1,), -1, dtype=torch.int64, device=dev)
    if cap is None:
        torch.cuda.synchronize()
        ls.probe_lists_dev(dq, n, starts, None, work, offsets=offsets, key_len=key_len, stream=stream)
        torch.cuda.synchronize()
        cap = int(starts[G].item())
        starts.fill_(-1)
    index = torch.full((max(cap, 1),), POISON - (1 << 32), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ls.probe_lists_dev(dq, n, starts, index[:cap] if cap else None, work, offsets=offsets, key_len=key_len,
                       stream=stream)
    torch.cuda.synchronize()
    return starts.cpu().numpy().view(np.uint64), index.cpu().numpy().view(np.uint32)[:cap]


# ------------------------------------ the L0 part (test_lset_version.py)

def expected_mask(oracle, tabs, keys):
    """tabs: the L0 tables in position order, (table_id, words, num_bits, k,
    lo, hi) with any overlap -> (mask, in-range mask), uint64 [len(keys)] each."""
    assert len(tabs) <= 64
    if not tabs or not keys:
        return np.zeros(len(keys), dtype=np.uint64), np.zeros(len(keys), dtype=np.uint64)
    data, offs = keygen.pack(keys)
    bits = oracle.probe([(t[1], t[2], t[3]) for t in tabs], data, offs)  # [n, ceil(F/8)], bit f%8 of byte f/8
    wide = np.zeros((len(keys), 8), dtype=np.uint8)
    wide[:, :bits.shape[1]] = bits
    may = wide.view("<u8").reshape(-1)
    order = sorted(range(len(keys)), key=lambda i: keys[i])
    sk = [keys[i] for i in order]
    idx = np.array(order, dtype=np.int64)
    inr = np.zeros(len(keys), dtype=np.uint64)
    for j, t in enumerate(tabs):
        a, b = bisect.bisect_left(sk, t[4]), bisect.bisect_right(sk, t[5])  # min_j <= key <= max_j
        if a < b:
            inr[idx[a:b]] |= np.uint64(1 << j)
    return may & inr, inr


# The parity workload: ids 0 .. 9999 as keys "user%08d" (12 bytes), the same
# plus four digits (16 bytes) and the same plus "abcd" and a run of x (16 .. 40
# bytes, so the keys of one id share their first 16).  64 L0 tables over that
# space, the special ranges first so that every T0 >= 8 holds them.
SST_SIZING = (1000, 0.01)


def k12(i):
    return b"user%08d" % i


def k16(i, tail):
    return b"user%08d%04d" % (i, tail)


def kvar(i, r):
    return b"user%08d" % i + b"abcd" + b"x" * r


def l0_ranges():
    rng = np.random.default_rng(61)
    rg = [None] * 64
    rg[0] = (k12(2000), k12(5000))
    rg[1] = (b"user", b"user\xff")                                          # spans every key of the workload
    rg[2] = rg[0]                                                           # identical ranges
    rg[3] = (k12(2500), k12(2600))                                          # nested
    rg[4] = (rg[0][1], k12(5200))                                           # touches table 0 at one key
    rg[5] = (b"", k12(3000))                                                # an empty-string bound
    rg[6] = (b"user00004000abcdAA", b"user00004000abcd" + b"zz" * 5)        # long bounds sharing their first 16
    rg[7] = (k12(4100), k12(4100))                                          # one key
    for j in range(8, 64):
        a = int(rng.integers(0, 9000))
        rg[j] = (k12(a), k12(a + int(rng.integers(1, 3000))) + (b"9999" if j % 3 == 0 else b""))
    return rg


def sizing_of(geom, j):
    """(num_bits, k) of L0 table j: all SST-sized, or mixed over SIZINGS with
    one filter of no hash (table 5: only its range decides)."""
    if geom == "sst":
        return lsmbloom.params(*SST_SIZING)
    nb, k = lsmbloom.params(*SIZINGS[j % 4])
    return (nb, 0) if j == 5 else (nb, k)


@functools.lru_cache(maxsize=None)
def l0_tables(geom):
    import oracle_ct
    oracle = oracle_ct.load()
    rng = np.random.default_rng(62)
    tabs, members = [], []
    for j, (lo, hi) in enumerate(l0_ranges()):
        a = int(lo[4:12]) if len(lo) >= 12 else 0
        b = int(hi[4:12]) if len(hi) >= 12 and hi[4:12].isdigit() else 9999
        ids = rng.integers(a, b + 1, 400)
        cand = [k12(i) for i in ids] + [k16(i, i * 7 % 10000) for i in ids] + [kvar(i, i % 25) for i in ids]
        cand += [lo, hi, lo + b"\x00", lo + b"zz"]
        mem = sorted({c for c in cand if lo <= c <= hi})
        assert mem
        nb, k = sizing_of(geom, j)
        data, offs = keygen.pack(mem)
        tabs.append((7000 + j, oracle.build_var(data, offs, nb, k), nb, k, lo, hi))
        members.append(frozenset(mem))
    return tabs, members


@functools.lru_cache(maxsize=None)
def row_tables():
    """Three rows: 65 tables, 5 and 3, disjoint within a row."""
    import oracle_ct
    oracle = oracle_ct.load()
    rows = []
    for r, ntab in enumerate((65, 5, 3)):
        tabs = []
        width = 10000 // ntab
        for t in range(ntab):
            ids = range(t * width + r, t * width + width - 20, 3)
            keys = sorted([k12(i) for i in ids] + [kvar(i, i % 25) for i in ids][::2] + [k16(i, i * 7 % 10000) for i in ids][::2])
            tabs.append(build_table(oracle, 100 * (r + 1) + t, keys, SIZINGS[(t + r) % 4]))
        rows.append(tabs)
    return rows


@functools.lru_cache(maxsize=None)
def queries(kind):
    """5000 keys of one kind, shuffled (every prefix of them is a fair sample)."""
    rng = np.random.default_rng({"fixed16": 63, "fixed12": 64, "var": 65}[kind])
    tabs, members = l0_tables("sst")
    ids = [int(i) for i in rng.integers(0, 11000, 5000)]
    if kind == "fixed16":
        q = [k16(i, int(t)) for i, t in zip(ids[:3000], rng.integers(0, 10000, 3000))]
        q += [k16(i, i * 7 % 10000) for i in ids[3000:4600]]           # the members' form
        q += [b"zzzz%012d" % i for i in ids[:100]]                     # outside every range
        pool = [m for mem in members for m in mem if len(m) == 16]
    elif kind == "fixed12":
        q = [k12(i) for i in ids[:4500]] + [b"zzzz%08d" % i for i in ids[:100]]
        pool = [m for mem in members for m in mem if len(m) == 12]
    else:
        q = [kvar(i, int(r)) for i, r in zip(ids[:2500], rng.integers(0, 25, 2500))]
        q += [k12(i) for i in ids[2500:3200]] + [k16(i, i * 7 % 10000) for i in ids[3200:3600]]
        q += [b"", b"u", b"user", b"user0000", b"zzz", b"\xff" * 40, b"user00004000abcd", b"user00004000abcdAA",
              b"user00004000abcdA", b"user00004000abcdzzzzzzzzzzz", b"user00004000abcdzzzzzzzzz"]
        for t in tabs:
            q += [t[4], t[5], t[4][:-1], t[5] + b"\x00", t[5][:16], t[4] + b"\xff"]
        pool = [m for mem in members for m in mem]
    q += [pool[int(i)] for i in rng.integers(0, len(pool), 5000 - len(q))]
    assert len(q) == 5000
    q = [q[int(i)] for i in rng.permutation(5000)]
    if kind != "var":
        assert len({len(x) for x in q}) == 1
    else:
        assert min(len(x) for x in q) == 0 and max(len(x) for x in q) == 40
    return q


@functools.lru_cache(maxsize=None)
def reference(geom, kind):
    """(mask of all 64 tables, ids of the three rows) for queries(kind): bit j
    depends on table j alone, so the first T0 tables' answer is the low T0 bits."""
    import oracle_ct
    oracle = oracle_ct.load()
    tabs, members = l0_tables(geom)
    q = queries(kind)
    mask, inr = expected_mask(oracle, tabs, q)
    ids = expected_ids(oracle, row_tables(), q)
    # the inputs exercise what they should (over the first 8 tables, which every T0 >= 8 holds)
    low = np.uint64(0xFF)
    assert ((inr & ~mask & low) != 0).any(), "no key in range of a table and masked out by its filter"
    assert any(bin(int(m) & 0xFF).count("1") >= 2 for m in mask), "no key with two bits set"
    assert (inr == 0).any(), "no key outside every L0 range"
    assert any((int(m) >> j) & 1 and x not in members[j] for x, m in zip(q, mask) for j in range(8)), "no false positive"
    mask.setflags(write=False)
    ids.setflags(write=False)
    return mask, ids


def low_bits(mask, t0):
    return mask if t0 == 64 else mask & np.uint64((1 << t0) - 1)


# ------- Version lists and the walk's device forms (test_lset_version_lists.py,
# test_lset_walk.py, test_lset_model.py)

def version_lists_from(mask, ids, t0, order_ids):
    """probe_version()'s (mask uint64[n], ids uint32[R, n]) + table_order()'s
    ids (unique) -> (starts uint64[t0 + G + 1], index uint32[total]): the L0
    lists by position, then lists_from_ids' behind them."""
    mask = np.asarray(mask, dtype=np.uint64)
    l0 = [np.nonzero((mask >> np.uint64(j)) & np.uint64(1))[0].astype(np.uint32) for j in range(t0)]
    rs, ri = lists_from_ids(ids, order_ids)
    l0_starts = np.zeros(t0, dtype=np.uint64)
    if t0:
        l0_starts[1:] = np.cumsum([x.size for x in l0[:-1]], dtype=np.uint64)
    e0 = np.uint64(sum(x.size for x in l0))
    return (np.concatenate([l0_starts, rs + e0]).astype(np.uint64),
            np.concatenate(l0 + [ri]).astype(np.uint32))


def dev_vlists(ls, dq, n, cap=None, key_len=16, offsets=None, stream=None, work=None):
    """probe_version_lists_dev into fresh tensors: starts pre-filled with -1,
    index (cap entries; None: sized by a counting call) with POISON.  Returns
    (starts uint64, index uint32 [cap]) on the host, the whole index buffer."""
    import torch

    V = ls.version_tables()
    dev = dq.device
    if work is None:
        work = torch.empty(max(ls.version_lists_work_bytes(n), 1), dtype=torch.uint8, device=dev)
    starts = torch.full((V + 1,), -1, dtype=torch.int64, device=dev)
    if cap is None:
        torch.cuda.synchronize()
        ls.probe_version_lists_dev(dq, n, starts, None, work, offsets=offsets, key_len=key_len, stream=stream)
        torch.cuda.synchronize()
        cap = int(starts[V].item())
        starts.fill_(-1)
    index = torch.full((max(cap, 1),), POISON - (1 << 32), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ls.probe_version_lists_dev(dq, n, starts, index[:cap] if cap else None, work, offsets=offsets, key_len=key_len,
                               stream=stream)
    torch.cuda.synchronize()
    return starts.cpu().numpy().view(np.uint64), index.cpu().numpy().view(np.uint32)[:cap]


def dev_walk(ls, dq, n, resume=None, key_len=16, offsets=None, stream=None, in_place=False, want_step=True):
    """probe_walk_dev into POISON-filled tensors -> (step or None, ord) on the
    host.  in_place: step is the resume tensor itself."""
    import torch

    dev = dq.device
    d_res = torch.from_numpy(np.asarray(resume, np.uint32).view(np.int32).copy()).to(dev) if resume is not None else None
    d_ord = torch.full((max(n, 1),), POISON - (1 << 32), dtype=torch.int32, device=dev)
    if in_place:
        d_step = d_res
    else:
        d_step = torch.full((max(n, 1),), POISON - (1 << 32), dtype=torch.int32, device=dev) if want_step else None
    torch.cuda.synchronize()
    ls.probe_walk_dev(dq, n, d_ord, step=d_step, resume=d_res, offsets=offsets, key_len=key_len, stream=stream)
    torch.cuda.synchronize()
    step = d_step.cpu().numpy().view(np.uint32)[:n] if d_step is not None else None
    if d_res is not None and not in_place:
        assert np.array_equal(d_res.cpu().numpy().view(np.uint32), np.asarray(resume, np.uint32))  # only read
    return step, d_ord.cpu().numpy().view(np.uint32)[:n]


def dev_walk_lists(ls, dq, n, cap=None, resume=None, key_len=16, offsets=None, stream=None, work=None, want_step=True):
    """probe_walk_lists_dev into fresh tensors: starts pre-filled with -1, index
    (cap entries; None: sized by a counting call) and step with POISON.  Returns
    (starts uint64, index uint32 [cap], step uint32 [n] or None) on the host."""
    import torch

    V = ls.version_tables()
    dev = dq.device
    if work is None:
        work = torch.empty(max(ls.walk_lists_work_bytes(n), 1), dtype=torch.uint8, device=dev)
    d_res = torch.from_numpy(np.asarray(resume, np.uint32).view(np.int32).copy()).to(dev) if resume is not None else None
    starts = torch.full((V + 1,), -1, dtype=torch.int64, device=dev)
    kw = dict(resume=d_res, offsets=offsets, key_len=key_len, stream=stream)
    if cap is None:
        torch.cuda.synchronize()
        ls.probe_walk_lists_dev(dq, n, starts, None, work, **kw)
        torch.cuda.synchronize()
        cap = int(starts[V].item())
        starts.fill_(-1)
    index = torch.full((max(cap, 1),), POISON - (1 << 32), dtype=torch.int32, device=dev)
    step = torch.full((max(n, 1),), POISON - (1 << 32), dtype=torch.int32, device=dev) if want_step else None
    torch.cuda.synchronize()
    ls.probe_walk_lists_dev(dq, n, starts, index[:cap] if cap else None, work, step=step, **kw)
    torch.cuda.synchronize()
    return (starts.cpu().numpy().view(np.uint64), index.cpu().numpy().view(np.uint32)[:cap],
            step.cpu().numpy().view(np.uint32)[:n] if want_step else None)


# ------------------------------- Version edits (test_lset_versions.py)

CHUNK = 4 << 20  # the arena's chunk (include/lsmbloom.h)
SST = lsmbloom.params(1000, 0.01)  # SSTableBuilder's filter


def mk(oracle, tid, first, nb, k, nkeys=40):
    """(table_id, words, num_bits, k, min_key, max_key): nkeys keys out of the
    100 ids from `first`, in a filter of exactly (nb, k)."""
    rng = np.random.default_rng(1000 + tid)
    ids = np.sort(rng.choice(100, size=nkeys, replace=False)) + first
    keys = [b"user%08d" % i for i in ids]
    data, offs = keygen.pack(keys)
    w = oracle.build_var(data, offs, nb, k) if nb else np.zeros(0, np.uint64)
    return (tid, w, nb, k, keys[0], keys[-1])


def block(oracle, t):
    return oracle.serialize(t[1] if t[2] else np.zeros(1, np.uint64), t[2], t[3])


def batch_args(oracle, placed):
    """placed: [(row, table)] -> the arguments of LevelSet.add_many (no CRCs)."""
    return ([r for r, _ in placed], [t[0] for _, t in placed], [block(oracle, t) for _, t in placed],
            [(t[4], t[5]) for _, t in placed])


def edit_queries(rows, rng, span, nrand):
    """Members' neighbours, random ids over the whole span, every bound and the keys just outside it."""
    tabs = [t for row in rows for t in row]
    q = [b"user%08d" % i for i in rng.integers(0, span, nrand)]
    q += [t[4] for t in tabs] + [t[5] for t in tabs]
    q += [t[4][:-1] for t in tabs] + [t[5] + b"\x00" for t in tabs]
    q += [b"", b"user", b"\xff" * 40]
    return q


# ------------------------------ filter sets (test_fset.py, test_fset_lists.py)

def expected_masks(oracle, tables, keys):
    """tables: {slot: (words, num_bits, k, lo, hi)} -> list of uint64 masks."""
    data, offs = keygen.pack(keys)
    out = [0] * len(keys)
    for s, (w, nb, k, lo, hi) in tables.items():
        hit = oracle.probe([(w, nb, k)], data, offsets=offs)[:, 0]
        for i, key in enumerate(keys):
            if hit[i] and lo <= key <= hi:
                out[i] |= 1 << s
    return out


def lists_from_masks(masks):
    """uint64 mask per key -> (starts uint64[65], index uint32[total])."""
    masks = np.asarray(masks, dtype=np.uint64)
    starts = np.zeros(65, dtype=np.uint64)
    runs = []
    for s in range(64):
        idx = np.nonzero((masks >> np.uint64(s)) & np.uint64(1))[0].astype(np.uint32)
        runs.append(idx)
        starts[s + 1] = starts[s] + np.uint64(idx.size)
    return starts, (np.concatenate(runs) if runs else np.zeros(0, np.uint32))


def check_mask_lists(got, masks, what=""):
    starts, index = got
    es, ei = lists_from_masks(masks)
    assert starts.dtype == np.uint64 and starts.shape == (65,), what
    assert index.dtype == np.uint32, what
    assert np.array_equal(starts, es), (what, starts, es)
    assert np.array_equal(index, ei), what
