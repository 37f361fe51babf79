"""The walk probe's expectation (tests/test_lset_walk.py): numpy reductions of
a Version's full answer — an L0 mask and the rows' answers, as lset_support's
reference() takes them from the CPU oracle — to each key's first candidate in
DB::get's order, and that answer's per-table lists.  No tests here, and
nothing below calls the library."""
import numpy as np

import lsmbloom

NONE = lsmbloom.LSMB_LSET_NONE


def ordinals_of(ids_rn, order_ids):
    """probe()'s uint32 [R, n] table ids + table_order()'s ids (unique) -> the
    rows' ordinals, uint32 [R, n], NONE kept."""
    ids_rn = np.asarray(ids_rn, dtype=np.uint32)
    order_ids = np.asarray(order_ids, dtype=np.uint32)
    assert np.unique(order_ids).size == order_ids.size, "the expectation needs unique table ids"
    out = np.full(ids_rn.shape, NONE, dtype=np.uint32)
    hit = ids_rn != NONE
    if hit.any():
        sorter = np.argsort(order_ids, kind="stable")
        pos = np.searchsorted(order_ids[sorter], ids_rn[hit])
        assert (order_ids[sorter][pos] == ids_rn[hit]).all()
        out[hit] = sorter[pos].astype(np.uint32)
    return out


def walk_from(mask, row_ord, t0, resume=None):
    """mask uint64[n] (bit j = L0 position j, j < t0), row_ord uint32 [R, n]
    (the rows' ordinal answering key i in row r, or NONE), resume uint32[n]
    (None: all zero) -> (step uint32[n], ord uint32[n]): the first walk step
    w >= resume[i] with a candidate, step w < t0 looking at position t0-1-w,
    step t0 + r at row r, and that candidate's Version ordinal."""
    mask = np.asarray(mask, dtype=np.uint64)
    row_ord = np.asarray(row_ord, dtype=np.uint32)
    n, R = mask.size, row_ord.shape[0]
    W = t0 + R
    step = np.full(n, NONE, dtype=np.uint32)
    ordv = np.full(n, NONE, dtype=np.uint32)
    if W == 0 or n == 0:
        return step, ordv
    resume = np.zeros(n, dtype=np.uint32) if resume is None else np.asarray(resume, dtype=np.uint32)
    cand = np.zeros((W, n), dtype=bool)
    cord = np.full((W, n), NONE, dtype=np.uint32)
    for w in range(t0):
        p = t0 - 1 - w
        cand[w] = ((mask >> np.uint64(p)) & np.uint64(1)).astype(bool)
        cord[w] = p
    for r in range(R):
        cand[t0 + r] = row_ord[r] != NONE
        cord[t0 + r] = np.where(cand[t0 + r], row_ord[r].astype(np.uint64) + t0, NONE).astype(np.uint32)
    ok = cand & (np.arange(W, dtype=np.uint64)[:, None] >= resume[None, :].astype(np.uint64))
    found = ok.any(axis=0)
    first = ok.argmax(axis=0)
    step[found] = first[found].astype(np.uint32)
    ordv[found] = cord[first, np.arange(n)][found]
    return step, ordv


def lists_from_ord(ordv, V):
    """ord uint32[n] (NONE: in no list) -> (starts uint64[V + 1], index
    uint32[total]): per Version ordinal the ascending key indices."""
    ordv = np.asarray(ordv, dtype=np.uint32)
    idx = np.nonzero(ordv != NONE)[0]
    by_table = np.argsort(ordv[idx], kind="stable")
    starts = np.searchsorted(ordv[idx][by_table], np.arange(V + 1), side="left").astype(np.uint64)
    return starts, idx[by_table].astype(np.uint32)
