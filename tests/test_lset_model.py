"""Seeded chains of random Version edits against a model of the level set
(tests/lset_model.py): derive of every kind, drops, adds through every route,
edits that must fail, several children of one parent, sets closed in any
order, and after every edit every order entry point and every probe form of
the sets involved, host and device, held against the model with exact
equality.  A filter set gets the same treatment over slot churn.

The expectation is lset_model.Expect's: per-table columns from the CPU oracle
and Python's bytes order, composed in numpy; nothing in it comes from the
library.  A failure names the seed, the step and the first differing key, and
replays as script(seed)[:step + 1].
"""
import functools
import itertools
import zlib

import numpy as np
import pytest

import keygen
import lsmbloom
import lset_model as M
from lsmbloom import BloomFilter, FilterSet, LevelSet
from lset_support import (NONE, POISON, batch_args, block, check_mask_lists, dev_lists, dev_vlists, dev_walk,
                          dev_walk_lists, expected_masks, k12, kvar, lists_from_masks)

SEEDS = [1, 2, 3, 4, 5, 6]
L0_HEAVY = 6  # this seed opens with 61 L0 tables and sends most adds there


@functools.lru_cache(maxsize=None)
def plan(seed):
    """(steps, var-len queries, 16-byte queries) of a seed, each computed once."""
    steps = M.script(seed, l0_heavy=seed == L0_HEAVY)
    specs = M.specs_of(steps)
    return steps, M.var_queries(specs, np.random.default_rng([seed, 1])), M.k16_queries(specs, np.random.default_rng([seed, 2]))


# ---------------------------------------------------------------- without a GPU

def test_model_on_a_hand_written_version():
    """Six tables whose ranges are whole cells and whose queried keys are
    members or outside every range, so every answer below follows from the
    ranges alone: row 0 holds A (cell 0) and B (cell 2), row 1 C (cell 1),
    row 2 D (cell 0), L0 E (cells 0-1) then F (cell 1).  The edit drops C,
    which empties row 1 under row 2, and E, whose id comes back as an L0
    table over cells 1-2 that arrives behind F."""
    none, sst = (0, 0), (9586, 7)
    A, B, C = M.Spec(1, 0, 1, *none, False, 90), M.Spec(2, 2, 1, *none, False, 90), M.Spec(3, 1, 1, *none, False, 90)
    D, E, F = M.Spec(4, 0, 1, *sst, False, 90), M.Spec(5, 0, 2, *none, False, 40), M.Spec(6, 1, 1, *none, False, 90)
    E2 = M.Spec(5, 1, 2, *sst, False, 40)
    for s, lo, hi in ((A, 0, 99), (B, 200, 299), (C, 100, 199), (D, 0, 99), (E, 0, 199), (F, 100, 199), (E2, 100, 299)):
        assert M.table(s).t[4:] == (k12(lo), k12(hi))
    parent = M.Version(0)
    for row, s in ((0, A), (1, C), (0, B), (2, D), (M.L0, E), (M.L0, F)):
        parent.add(row, s, "add")
    assert parent.stats() == dict(tables=6, inherited=0, filter_bytes=1200, uploaded_bytes=1200)
    child, dropped = parent.derive(1, [3, 5, M.UNKNOWN])
    child.add(M.L0, E2, "many")
    assert dropped == 2
    assert child.stats() == dict(tables=5, inherited=4, filter_bytes=2400, uploaded_bytes=1200)
    assert child.nrows == 3 and [len(r) for r in child.rows] == [2, 0, 1, 0]
    assert child.table_order() == ([1, 2, 4], [0, 2, 2, 3])
    assert child.l0_order() == [6, 5] and parent.l0_order() == [5, 6]
    assert child.version_order() == ([6, 5, 1, 2, 4], [0, 2, 4, 4, 5])
    assert child.walk_steps() == 5 and child.l0_overlap()
    q = [k12(50), k12(150), k12(250), k12(350), k12(99) + b"\x00", kvar(150, 5)]
    ex = M.Expect(q)
    resume = np.array([3, 1, 1, 0, 0, 5], np.uint32)
    a = ex.answers(child, resume)
    N = int(NONE)
    assert a["ids"].tolist() == [[1, N, 2, N, N, N], [N] * 6, [4, N, N, N, N, N]]
    assert a["mask"].tolist() == [0, 3, 2, 0, 0, 3]
    assert [x.tolist() for x in a["lists"]] == [[0, 1, 2, 3], [0, 2, 0]]
    assert [x.tolist() for x in a["vlists"]] == [[0, 2, 5, 6, 7, 8], [1, 5, 1, 2, 5, 0, 2, 0]]
    # step 0 looks at L0 position 1 (the re-added id, arrived last), step 1 at F, steps 2 .. 4 at the rows
    assert [x.tolist() for x in a["walk"]] == [[2, 0, 0, N, N, 0], [2, 1, 1, N, N, 1]]
    assert [x.tolist() for x in a["walk_lists"]] == [[0, 0, 3, 4, 4, 4], [1, 2, 5, 0]]
    assert [x.tolist() for x in a["walk_from"]] == [[4, 1, 2, N, N, N], [4, 0, 3, N, N, N]]
    assert [x.tolist() for x in a["walk_from_lists"]] == [[0, 1, 1, 1, 2, 3], [1, 2, 0]]
    # the parent is as it was: E at position 0 answers cells 0 and 1 and the key between them, C answers in row 1
    p = ex.answers(parent)
    assert p["mask"].tolist() == [1, 3, 0, 0, 1, 3]
    assert p["ids"].tolist() == [[1, N, 2, N, N, N], [N, 3, N, N, N, 3], [4, N, N, N, N, N]]


def test_scripts_are_replayable_and_respect_their_own_limits():
    for seed in SEEDS:
        steps = plan(seed)[0]
        assert steps == M.script(seed, l0_heavy=seed == L0_HEAVY) and len(steps) == 31
        for i, st, live, info in M.replay(steps):  # Version.add refuses a taken cell, a held id, a 65th L0 table
            assert 1 <= len(live) <= M.MAX_LIVE and all(v.sealed for v in live.values())
            assert i == 0 or (len(st.drops) <= 5 and len(st.adds) <= 3)
            assert set(st.verify) <= set(live)
            for v in live.values():
                ids = [s.tid for s in v.every()]
                assert len(set(ids)) == len(ids)
            big = [s for _, s, route in st.adds if M.is_big(s)]
            assert all(route != "built" for _, s, route in st.adds if M.is_big(s)) and len(big) <= 1
        assert sum(1 for s in M.specs_of(steps) if M.is_big(s)) <= 1
        assert "parent=" in M.show(steps[-1]) and "\n" not in M.show(steps[-1])


def test_scripts_cover_what_they_are_for():
    seen = set()
    for seed in SEEDS:
        seen |= M.coverage(plan(seed)[0])
    for what in sorted(M.REQUIRED):
        assert what in seen, "no committed seed exercises: %s" % what
    assert len(M.REQUIRED) == len(M.KINDS) + len(M.ROUTES) + 12


@pytest.mark.parametrize("seed", SEEDS)
def test_every_verification_has_something_to_get_wrong(seed):
    steps, qv, q16 = plan(seed)
    assert {b"", b"user", b"\xff" * 40} <= set(qv) and len(qv) >= 1100 and len(q16) >= 400
    ex = M.Expect(qv)
    for i, st, live, info in M.replay(steps):
        for x in st.verify:
            tx = ex.texture(live[x])
            what = (seed, i, x, tx)
            assert tx["row_hits"] >= 100, what
            assert tx["rejected"] >= 1, what
            assert tx["false_positives"] >= 1, what
            assert tx["two_l0_bits"] >= 1 or not live[x].l0_overlap(), what
    e16 = M.Expect(q16)  # the 16-byte queries of the device forms find tables too
    last = M.replay(steps)
    *_, (i, st, live, info) = last
    assert all(e16.texture(v)["row_hits"] >= 20 for v in live.values())


# ------------------------------------------------------------------- on the GPU

def differ(got, exp, keys=None, index_of_keys=False):
    """None, or where two arrays first differ (and the key there)."""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape != exp.shape or got.dtype != exp.dtype:
        return "shape/dtype %s %s, expected %s %s" % (got.shape, got.dtype, exp.shape, exp.dtype)
    bad = np.argwhere(got != exp)
    if bad.size == 0:
        return None
    at = tuple(int(x) for x in bad[0])
    msg = "%d differ, first at %s: got %s, expected %s" % (len(bad), at, got[at], exp[at])
    if keys is not None:
        k = int(exp[at]) if index_of_keys else at[-1]
        msg += ", key %r" % (keys[k] if k < len(keys) else None)
    return msg


class Verifier:
    """One script's queries on the host and the device, its expectations, and the comparisons."""

    def __init__(self, seed):
        import torch

        self.seed = seed
        self.steps, self.qv, self.q16 = plan(seed)
        self.ev, self.e16 = M.Expect(self.qv), M.Expect(self.q16)
        dev = torch.device("cuda:0")
        self.d_var = torch.from_numpy(np.concatenate([self.ev.data, np.zeros(16, np.uint8)])).to(dev)
        self.d_offs = torch.from_numpy(self.ev.offs.view(np.int64)).to(dev)
        self.d_16 = torch.from_numpy(self.e16.data.copy()).to(dev)
        self.stream = torch.cuda.Stream(dev)
        self.answers = {}
        self.count = 0
        self.where = ""

    def same(self, name, got, exp, keys=None, index_of_keys=False):
        d = differ(got, exp, keys, index_of_keys)
        assert d is None, "%s: %s: %s" % (self.where, name, d)

    def same_lists(self, name, got, exp, keys):
        self.same(name + " starts", got[0], exp[0])
        self.same(name + " index", got[1], exp[1], keys, index_of_keys=True)

    def expected(self, x, v):
        """(var-len answers, 16-byte answers, var-len resume, 16-byte resume) of set x, computed once."""
        if x not in self.answers:
            rng = np.random.default_rng([self.seed, 3, x])
            rv, r16 = M.resume_for(rng, self.ev.n, v.walk_steps()), M.resume_for(rng, self.e16.n, v.walk_steps())
            self.answers[x] = (self.ev.answers(v, rv), self.e16.answers(v, r16), rv, r16)
        return self.answers[x]

    def verify(self, ls, x, v):
        self.count += 1
        self.structure(ls, v)
        av, a16, rv, r16 = self.expected(x, v)
        self.host(ls, av, rv)
        if self.count % 3 == 0:
            st = self.stream.cuda_stream if (self.count // 3) % 2 else None
            self.device(ls, v, a16, r16, self.d_16, self.e16.n, dict(key_len=16, offsets=None, stream=st), self.q16,
                        "16-byte device keys")
            self.device(ls, v, av, rv, self.d_var, self.ev.n, dict(key_len=0, offsets=self.d_offs, stream=st), self.qv,
                        "device offsets")

    def structure(self, ls, v):
        eq = self.same
        eq("rows", ls.rows(), v.nrows)
        eq("tables(r)", [ls.tables(r) for r in range(M.NROWS)], [len(r) for r in v.rows])
        eq("l0_tables", ls.l0_tables(), len(v.l0))
        eq("l0_order", ls.l0_order(), np.array(v.l0_order(), np.uint32))
        ids, base = ls.table_order()
        eq("table_order ids", ids, np.array(v.table_order()[0], np.uint32))
        eq("table_order base", base, np.array(v.table_order()[1], np.uint64))
        eq("total_tables", ls.total_tables(), len(v.table_order()[0]))
        eq("version_tables", ls.version_tables(), len(v.every()))
        vids, part = ls.version_order()
        eq("version_order ids", vids, np.array(v.version_order()[0], np.uint32))
        eq("version_order parts", part, np.array(v.version_order()[1], np.uint64))
        eq("walk_steps", ls.walk_steps(), v.walk_steps())
        s = ls.stats()
        assert {k: s[k] for k in v.stats()} == v.stats(), "%s: stats %s, expected %s" % (self.where, s, v.stats())

    def host(self, ls, a, resume):
        q, eq = self.qv, self.same
        eq("probe", ls.probe_keys(q), a["ids"], q)
        gm, gi = ls.probe_version_keys(q)
        eq("probe_version mask", gm, a["mask"], q)
        eq("probe_version ids", gi, a["ids"], q)
        self.same_lists("probe_lists", ls.probe_lists_keys(q), a["lists"], q)
        self.same_lists("probe_version_lists", ls.probe_version_lists_keys(q), a["vlists"], q)
        for res, walk, lists in ((None, "walk", "walk_lists"), (resume, "walk_from", "walk_from_lists")):
            what = "from a resume vector" if res is not None else "from step 0"
            step, ordv = ls.probe_walk_keys(q, resume=res)
            eq("probe_walk step " + what, step, a[walk][0], q)
            eq("probe_walk ord " + what, ordv, a[walk][1], q)
            starts, index, step = ls.probe_walk_lists_keys(q, resume=res)
            eq("probe_walk_lists step " + what, step, a[walk][0], q)
            self.same_lists("probe_walk_lists " + what, (starts, index), a[lists], q)

    def device(self, ls, v, a, resume, d, n, kw, q, form):
        import torch

        eq = self.same
        R = v.nrows
        poison = POISON - (1 << 32)
        out = torch.full((max(R * n, 1),), poison, dtype=torch.int32, device=d.device)
        torch.cuda.synchronize()
        ls.probe_dev(d, n, out, **kw)
        torch.cuda.synchronize()
        eq("probe_dev, " + form, out.cpu().numpy().view(np.uint32)[:R * n].reshape(R, n), a["ids"], q)
        out.fill_(poison)
        mask = torch.full((n,), -0x2152411021524111, dtype=torch.int64, device=d.device)
        torch.cuda.synchronize()
        ls.probe_version_dev(d, n, mask, out if R else None, **kw)
        torch.cuda.synchronize()
        eq("probe_version_dev mask, " + form, mask.cpu().numpy().view(np.uint64), a["mask"], q)
        eq("probe_version_dev ids, " + form, out.cpu().numpy().view(np.uint32)[:R * n].reshape(R, n), a["ids"], q)
        self.same_lists("probe_lists_dev, " + form, dev_lists(ls, d, n, **kw), a["lists"], q)
        self.same_lists("probe_version_lists_dev, " + form, dev_vlists(ls, d, n, **kw), a["vlists"], q)
        for res, walk, lists in ((None, "walk", "walk_lists"), (resume, "walk_from", "walk_from_lists")):
            what = form + (", from a resume vector" if res is not None else ", from step 0")
            step, ordv = dev_walk(ls, d, n, resume=res, **kw)
            eq("probe_walk_dev step, " + what, step, a[walk][0], q)
            eq("probe_walk_dev ord, " + what, ordv, a[walk][1], q)
            starts, index, step = dev_walk_lists(ls, d, n, resume=res, **kw)
            eq("probe_walk_lists_dev step, " + what, step, a[walk][0], q)
            self.same_lists("probe_walk_lists_dev, " + what, (starts, index), a[lists], q)


def row_of(row):
    return lsmbloom.LSMB_LSET_ROW_L0 if row == M.L0 else row


def crc_of(oracle, t):
    return zlib.crc32(block(oracle, t))


def add_built(ctx, ls, placed):
    """placed: [(row, Table)] through Context.build_batch_dev into a
    0xFF-filled tensor, then device to device into the set."""
    import torch

    run = [k for _, t in placed for k in t.keys]
    data, offs = keygen.pack(run)
    seg = np.zeros(len(placed) + 1, np.uint64)
    np.cumsum([len(t.keys) for _, t in placed], out=seg[1:])
    nb, kk = [t.spec.nb for _, t in placed], [t.spec.k for _, t in placed]
    assert max(nb) <= lsmbloom.build_batch_max_bits()
    dev = torch.device("cuda:0")
    d_data = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    words = torch.full((int(lsmbloom.build_batch_layout(nb)[-1]),), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.build_batch_dev(d_data, len(run), seg, nb, kk, words, offsets=d_offs)
    ls.add_built([row_of(r) for r, _ in placed], [t.spec.tid for _, t in placed], words, nb, kk,
                 [(t.t[4], t.t[5]) for _, t in placed])


def apply_adds(ctx, oracle, ls, adds):
    """A step's adds in order, neighbours of one batched route in one call."""
    for route, grp in itertools.groupby(adds, key=lambda a: a[2]):
        placed = [(row, M.table(spec)) for row, spec, _ in grp]
        if route == "add":
            for row, t in placed:
                ls.add(row_of(row), t.t[0], block(oracle, t.t), t.t[4], t.t[5])
        elif route == "add_filter":
            for row, t in placed:
                ls.add_filter(row_of(row), t.t[0], BloomFilter(t.t[1], t.t[3], t.t[2]), t.t[4], t.t[5])
        elif route == "built":
            add_built(ctx, ls, placed)
        else:
            args = batch_args(oracle, [(row_of(row), t.t) for row, t in placed])
            status = ls.add_many(*args, crcs=[zlib.crc32(b) for b in args[2]] if route == "many_crc" else None)
            assert not status.any()


def run_script(seed, ctx, oracle):
    vf = Verifier(seed)
    sets = {}
    try:
        for i, st, live, info in M.replay(vf.steps):
            vf.where = "seed %d, step %d (%s)" % (seed, i, M.show(st))
            if st.parent is None:
                ls = LevelSet(ctx)
            else:
                parent = sets[st.parent]
                if st.bad_seal:  # a second child whose table overlaps a neighbour: its seal fails, it goes
                    row, spec = st.bad_seal
                    before = parent.stats()
                    doomed = parent.derive([])
                    doomed.add_many(*batch_args(oracle, [(row, M.table(spec).t)]))
                    with pytest.raises(ValueError, match="overlap"):
                        doomed.seal()
                    doomed.close()
                    assert parent.stats() == before, vf.where
                ls = parent.derive(st.drops, repack=st.kind, stream=vf.stream.cuda_stream if i % 2 else None)
                surv = info["survivors"]
                assert ls.dropped == info["dropped"], (vf.where, ls.dropped, info["dropped"])
                if st.kind in (None, 0):
                    assert ls.moved == (0, 0), (vf.where, ls.moved)
                elif st.kind == "all":
                    assert ls.moved == (len(surv), sum(M.slot(s) for s in surv)), (vf.where, ls.moved)
                else:
                    assert ls.moved[0] <= len(surv), (vf.where, ls.moved)
                if st.bad_batch:  # one wrong CRC: Corruption, and no trace of the batch
                    pair, which = st.bad_batch
                    args = batch_args(oracle, [(row_of(row), M.table(spec).t) for row, spec in pair])
                    crcs = [zlib.crc32(b) for b in args[2]]
                    crcs[which] ^= 0x00010000
                    before = ls.stats()
                    with pytest.raises(lsmbloom.Corruption) as ei:
                        ls.add_many(*args, crcs=crcs)
                    assert np.nonzero(ei.value.status)[0].tolist() == [which], vf.where
                    assert ls.stats() == before, (vf.where, ls.stats(), before)
            sets[i] = ls
            apply_adds(ctx, oracle, ls, st.adds)
            ls.seal()
            for c in st.close:
                sets.pop(c).close()
            for x in st.verify:
                vf.where = "seed %d, step %d (%s), set %d" % (seed, i, M.show(st), x)
                vf.verify(sets[x], x, live[x])
    finally:
        for ls in sets.values():
            ls.close()
    return vf.count


@pytest.fixture(scope="module")
def ctx():
    c = lsmbloom.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_random_edit_chain_matches_the_model(ctx, oracle, seed):
    assert run_script(seed, ctx, oracle) > 60  # verifications; three sets an edit, all of them every fifth


# ------------------------------------------------- filter-set slot churn

@pytest.mark.gpu
@pytest.mark.parametrize("seed,prefill", [(11, 0), (12, 27), (13, 57)])
def test_filter_set_slot_churn(ctx, oracle, seed, prefill):
    """Random add / add_checked / add_filter / remove: from nothing (1- and
    2-byte rows), across 32 slots (4-byte rows) and up to the 64-slot limit
    and back down."""
    import torch

    ops = M.fset_script(seed, prefill)
    specs = [op[1] for op in ops if op[0] != "remove"]
    q = M.var_queries(specs, np.random.default_rng([seed, 1]), nrand=60)[:400]
    data, offs = keygen.pack(q)
    n = len(q)
    dev = torch.device("cuda:0")
    d_data = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    fs = FilterSet(ctx)
    held, arrival, most, widths = {}, [], 0, set()
    for j, op in enumerate(ops):
        where = "seed %d, op %d %r" % (seed, j, op[:1] + (tuple(op[1]),) if op[0] != "remove" else op)
        if op[0] == "remove":
            s = arrival.pop(op[1])
            fs.remove(s)
            del held[s]
        else:
            t = M.table(op[1]).t
            if op[0] == "add":
                s = fs.add(block(oracle, t), t[4], t[5])
            elif op[0] == "add_checked":
                s = fs.add_checked(block(oracle, t), crc_of(oracle, t), t[4], t[5])
            else:
                s = fs.add_filter(BloomFilter(t[1], t[3], t[2]), t[4], t[5])
            assert 0 <= s < 64 and s not in held, (where, s, sorted(held))
            held[s] = t[1:]
            arrival.append(s)
        most = max(most, len(held))
        if j < prefill - 1:
            continue
        live = sum(1 << s for s in held)
        assert fs.live_mask() == live, where
        masks = expected_masks(oracle, held, q)
        exp = np.array(masks, dtype=np.uint64)
        d = differ(fs.probe_keys(q), exp, q)
        assert d is None, (where, "probe", d)
        check_mask_lists(fs.probe_lists_keys(q), masks, (where, "probe_lists"))
        for rb in (1, 2, 4, 8):
            if rb < 8 and live >> (8 * rb):
                continue  # a live slot does not fit: the entry point refuses
            widths.add(rb)
            out = torch.full((n * rb,), 0xA5, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            fs.probe_dev(d_data, n, out, offsets=d_offs, row_bytes=rb)
            torch.cuda.synchronize()
            d = differ(out.cpu().numpy().view("<u%d" % rb), exp.astype("<u%d" % rb), q)
            assert d is None, (where, "probe_dev, %d-byte rows" % rb, d)
        es, ei = lists_from_masks(masks)
        starts = torch.full((65,), -1, dtype=torch.int64, device=dev)
        index = torch.full((max(ei.size, 1),), POISON - (1 << 32), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        fs.probe_lists_dev(d_data, n, starts, index[:ei.size] if ei.size else None, offsets=d_offs)
        torch.cuda.synchronize()
        check_mask_lists((starts.cpu().numpy().view(np.uint64), index.cpu().numpy().view(np.uint32)[:ei.size]), masks,
                         (where, "probe_lists_dev"))
    fs.close()
    assert (most == 64 or prefill != 57) and widths >= ({1, 2, 4, 8} if prefill == 0 else {8})
