"""A model of a level set's state across Version edits, and seeded scripts of
random edit chains that walk the library and the model together
(tests/test_lset_model.py).  No tests here, no call of the library and no GPU:
a script is plain data from a numpy Generator, the model is Python lists, and
every expected answer is a numpy composition of per-table columns — the CPU
oracle's probe of that one filter over the query list, and the in-range test
by Python's bytes comparison — through the references the feature tests use
(lists_from_ids, version_lists_from, walk_from, lists_from_ord).

Key space: ids in cells of 100, keys "user%08d" of an id.  A row table owns one
cell that is free in its row, so rows stay disjoint by construction; an L0 table
spans one to three adjacent cells, so L0 tables overlap whenever they share a
cell, and every L0 table holds its cells' anchor keys, so two overlapping L0
tables always answer one key together.  About one table in eight has long
bounds that share their first 16 bytes (the keys of one id plus "abcd" and a
run of x), which keeps the prefix-tie search in play after edits.
"""
import collections
import functools

import numpy as np

import keygen
from lset_support import NONE, k12, k16, kvar, lists_from_ids, version_lists_from
from walk_support import lists_from_ord, ordinals_of, walk_from

L0 = "L0"         # the row of an L0 table in a script (the driver passes LSMB_LSET_ROW_L0)
NROWS = 4         # adds go to rows 0 .. 3
NCELL = 48        # cells of the key space
L0_MAX = 64       # LSMB_LSET_L0_MAX
MAX_LIVE = 5      # sets open at once
CHUNK = 4 << 20   # the arena's chunk
KINDS = (None, 0, 0.25, 0.5, 0.9, "all")
ROUTES = ("add", "add_filter", "many", "many_crc", "built")
GEOMS = ((9586, 7), (64, 1), (192, 5), (0, 0), (4096, 40), (16385, 7), (65537, 7))
WEAK = ((64, 1), (192, 5))  # filters that answer non-members: the false positives of every verification
BIG_ITEMS = (4_000_000, 0.01)  # the one filter past a chunk, sized as BloomFilter::new sizes it
UNKNOWN = 9_000_000  # ids from here are held by no table

# A table: its id, first cell and cell count, filter geometry, long bounds or
# not, and how many of its cells' ids are members.
Spec = collections.namedtuple("Spec", "tid first ncell nb k long nkeys")
# One edit.  parent: the index of the sealed set derived from (None: a fresh
# set), the new set's index is the step's own; kind: the derive; drops: ids;
# adds: ((row, Spec, route), ...), in order, L0 arrivals included; bad_batch:
# (((row, Spec), (row, Spec)), which) a batch whose CRC `which` is wrong, given
# to the new set before its adds; bad_seal: (row, Spec) a table overlapping a
# neighbour, given to a second, plain child of the parent whose seal must fail;
# close: indices closed after the seal; verify: indices verified after that.
Step = collections.namedtuple("Step", "parent kind drops adds bad_batch bad_seal close verify")


def anchor(cell):
    return 100 * cell + 50


def nwords(nb):
    return (nb + 63) // 64


def nbytes(spec):
    return 8 * nwords(spec.nb)


def slot(spec):
    """The arena slot of a table: its words, at least 8 bytes, rounded up to 16."""
    return (max(nbytes(spec), 8) + 15) // 16 * 16


def is_big(spec):
    return nbytes(spec) > CHUNK


def member_keys(spec):
    """The sorted member keys of a table; keys[0] and keys[-1] are its bounds."""
    rng = np.random.default_rng([1000, spec.tid, spec.first, spec.ncell, spec.nb, spec.k, int(spec.long), spec.nkeys])
    if spec.long:  # the keys of one id: bounds of 16 and 36 bytes that share their first 16
        i = anchor(spec.first)
        runs = sorted({0, 5, 20} | {int(r) for r in rng.choice(21, size=8, replace=False)})
        return [kvar(i, r) for r in runs]
    span = 100 * spec.ncell
    ids = {int(i) for i in rng.choice(span, size=min(spec.nkeys, span), replace=False)}
    if spec.ncell > 1 or spec.nkeys >= 90:  # L0 tables and the overlapping ones cover their cells whole
        ids |= {0, span - 1}
    ids = sorted(i + 100 * spec.first for i in ids)
    keys = [k12(i) for i in ids] + [k16(i, i * 7 % 10000) for i in ids[1:-1][::4]]
    for c in range(spec.first, spec.first + spec.ncell):
        keys += [k12(anchor(c)), kvar(anchor(c), 5)]
    return sorted(set(keys))


Table = collections.namedtuple("Table", "spec t keys members")


@functools.lru_cache(maxsize=None)
def table(spec):
    """Spec -> Table: t the (id, words, num_bits, k, min_key, max_key) of
    lset_support.mk, the words built by the oracle."""
    import oracle_ct
    oracle = oracle_ct.load()
    keys = member_keys(spec)
    data, offs = keygen.pack(keys)
    w = oracle.build_var(data, offs, spec.nb, spec.k) if spec.nb else np.zeros(0, np.uint64)
    w.setflags(write=False)
    return Table(spec, (spec.tid, w, spec.nb, spec.k, keys[0], keys[-1]), keys, frozenset(keys))


def big_geometry():
    import oracle_ct
    return oracle_ct.load().params(*BIG_ITEMS)


# ------------------------------------------------------------------- the model

class Version:
    """What a set holds and what its header promises of lsmb_lset_stats."""

    def __init__(self, index, parent=None):
        self.index = index
        self.parent = parent.index if parent is not None else None
        self.ancestors = (parent.ancestors | {parent.index}) if parent is not None else frozenset()
        self.depth = parent.depth + 1 if parent is not None else 0
        self.l0 = []                             # arrival order
        self.rows = [[] for _ in range(NROWS)]   # any order
        self.nrows = 0                           # rows(child) >= rows(parent), whatever empties
        self.inherited = 0
        self.uploaded_bytes = 0                  # host adds only
        self.sealed = False

    def every(self):
        return [s for row in self.rows for s in row] + self.l0

    def derive(self, index, drops):
        """-> (child, dropped): the survivors in their rows, L0 in its order."""
        drops = set(drops)
        child = Version(index, self)
        child.rows = [[s for s in row if s.tid not in drops] for row in self.rows]
        child.l0 = [s for s in self.l0 if s.tid not in drops]
        child.nrows = self.nrows
        child.inherited = len(child.every())
        return child, len(self.every()) - child.inherited

    def add(self, row, spec, route):
        assert not self.sealed and spec.tid not in {s.tid for s in self.every()}
        if row == L0:
            assert len(self.l0) < L0_MAX
            self.l0.append(spec)
        else:
            assert self.free(row, spec.first)
            self.rows[row].append(spec)
            self.nrows = max(self.nrows, row + 1)
        if route != "built":
            self.uploaded_bytes += nbytes(spec)

    def free(self, row, cell):
        return all(s.first != cell for s in self.rows[row])

    def stats(self):
        tabs = self.every()
        return dict(tables=len(tabs), inherited=self.inherited, filter_bytes=sum(nbytes(s) for s in tabs),
                    uploaded_bytes=self.uploaded_bytes)

    # what the order entry points answer
    def table_order(self):
        """(ids, base): every row by min_key (its cell), rows 0 .. nrows - 1 back to back."""
        ids, base = [], [0]
        for row in self.rows[:self.nrows]:
            ids += [s.tid for s in sorted(row, key=lambda s: s.first)]
            base.append(len(ids))
        return ids, base

    def l0_order(self):
        return [s.tid for s in self.l0]

    def version_order(self):
        ids, base = self.table_order()
        t0 = len(self.l0)
        return self.l0_order() + ids, [0] + [t0 + b for b in base]

    def walk_steps(self):
        return len(self.l0) + self.nrows

    def l0_overlap(self):
        """Two L0 tables share a cell."""
        seen = set()
        for s in self.l0:
            cells = set(range(s.first, s.first + s.ncell))
            if cells & seen:
                return True
            seen |= cells
        return False


# ----------------------------------------------------------------- the scripts

def _weights(seed, l0_heavy):
    """Odd seeds open with every row in use; even ones with two, so that rows() grows along a chain."""
    return dict(base_rows=(10, 6, 2, 2) if seed % 2 else (12, 8), base_l0=61 if l0_heavy else 3,
                p_l0=0.75 if l0_heavy else 0.3)


def script(seed, edits=30, l0_heavy=False):
    """A replayable list of Steps: step 0 opens a fresh set, every later one
    derives from a sealed live set.  All the randomness is drawn here."""
    rng = np.random.default_rng(seed)
    wt = _weights(seed, l0_heavy)
    state = dict(tid=0, big=False, full=False)
    live = {}
    steps = []

    def new_spec(first, ncell, tid=None, route_ok=True, nkeys=40, geom=None):
        if tid is None:
            state["tid"] += 1
            tid = state["tid"]
        long = ncell == 1 and nkeys == 40 and rng.random() < 0.125
        if geom is None:
            geom = GEOMS[int(rng.integers(len(GEOMS)))]
        return Spec(tid, first, ncell, geom[0], geom[1], bool(long), nkeys)

    def place(v, row_hint=None, geom=None):
        """(row, Spec) for the next table of v: L0 while it has room, else a free cell of a row."""
        if row_hint is None:
            row_hint = L0 if (rng.random() < wt["p_l0"] and len(v.l0) < L0_MAX) else int(rng.integers(NROWS))
        if row_hint == L0:
            ncell = int(rng.integers(1, 4))
            return L0, new_spec(int(rng.integers(0, NCELL - ncell + 1)), ncell, geom=geom)
        cells = [c for c in range(NCELL) if v.free(row_hint, c)]
        return row_hint, new_spec(cells[int(rng.integers(len(cells)))], 1, geom=geom)

    def route():
        return ROUTES[int(rng.integers(len(ROUTES)))]

    # step 0: a fresh set, two weak filters among its tables
    v = Version(0)
    adds = []
    for r, count in enumerate(wt["base_rows"]):
        for j in range(count):
            geom = WEAK[j] if r == 0 and j < 2 else None
            row, spec = place(v, r, geom)
            adds.append((row, spec, route()))
            v.add(*adds[-1])
    for _ in range(wt["base_l0"]):
        row, spec = place(v, L0)
        adds.append((row, spec, route()))
        v.add(*adds[-1])
    v.sealed = True
    live[0] = v
    steps.append(Step(None, None, (), tuple(adds), None, None, (), (0,)))

    for i in range(1, edits + 1):
        keys = sorted(live)
        parent = live[keys[int(rng.integers(len(keys)))]]
        kind = KINDS[int(rng.integers(len(KINDS)))]
        # the drops: ids of the rows and of L0, never the last weak filter, never below ten row tables
        tabs = parent.every()
        nrow_tabs = sum(len(r) for r in parent.rows)
        weak = {s.tid for s in tabs if (s.nb, s.k) in WEAK}
        in_l0 = set(parent.l0_order())
        drops = []

        def may_go(s):
            gone = set(drops) | {s.tid}
            if not weak - gone:
                return False
            if s.tid not in in_l0 and nrow_tabs - len(gone - in_l0) < 10:
                return False
            if l0_heavy and not state["full"] and s.tid in in_l0:  # L0 climbs to its cap first
                return False
            return not (is_big(s) and i < 2 * edits // 3)  # the own-chunk filter stays for most of the script

        used = [r for r in range(NROWS) if parent.rows[r]]
        small = [r for r in used[:-1] if len(parent.rows[r]) <= 4]
        if small and rng.random() < 0.15:  # a whole row under a higher one that stays in use
            cand = list(parent.rows[small[int(rng.integers(len(small)))]])
        else:
            cand = [tabs[int(j)] for j in rng.permutation(len(tabs))[:int(rng.integers(0, 5))]]
        for s in cand:
            if may_go(s):
                drops.append(s.tid)
        readd = drops[0] if drops and rng.random() < 0.3 else None
        if rng.random() < 0.2:
            drops.insert(int(rng.integers(len(drops) + 1)), UNKNOWN + i)
        child, _ = parent.derive(i, drops)
        # edits that must fail and leave no trace
        bad_batch = bad_seal = None
        if rng.random() < 0.2:
            scratch, _ = parent.derive(i, drops)
            pair = []
            for _ in range(2):
                row, spec = place(scratch)
                scratch.add(row, spec, "many_crc")
                pair.append((row, spec))
            bad_batch = (tuple(pair), int(rng.integers(2)))
        full = [(r, s) for r in range(NROWS) for s in parent.rows[r]]
        if full and rng.random() < 0.2:
            r, s = full[int(rng.integers(len(full)))]
            bad_seal = (r, new_spec(s.first, 1, nkeys=90, geom=GEOMS[0]))
        # the adds
        adds = []
        nadd = int(rng.integers(0, 4))
        if readd is not None:
            nadd = max(nadd, 1)
        climbing = l0_heavy and not state["full"]
        if climbing:
            nadd = max(nadd, 2)
        for j in range(nadd):
            geom = None
            if not state["big"] and (i == 2 or rng.random() < 0.1):
                state["big"] = True
                row, spec = place(child, int(rng.integers(NROWS)), geom=big_geometry())
                spec = spec._replace(long=False)
                adds.append((row, spec, ROUTES[int(rng.integers(4))]))  # never built: past build_batch_max_bits()
            else:
                row, spec = place(child, L0 if climbing and len(child.l0) < L0_MAX else None, geom=geom)
                if j == 0 and readd is not None:
                    state["tid"] -= 1
                    spec = spec._replace(tid=readd)
                adds.append((row, spec, route()))
            child.add(*adds[-1])
        child.sealed = True
        live[i] = child
        state["full"] = state["full"] or len(child.l0) == L0_MAX
        # closes: sometimes one, and always down to MAX_LIVE; any set, the new one included
        close = []
        while len(live) > MAX_LIVE or (len(live) > 1 and not close and rng.random() < 0.35):
            keys = sorted(live)
            close.append(keys[int(rng.integers(len(keys)))])
            del live[close[-1]]
        # verified: the child, its parent, one other; every fifth edit and at the end, all
        if i % 5 == 0 or i == edits:
            verify = sorted(live)
        else:
            verify = [x for x in (i, parent.index) if x in live]
            others = [x for x in sorted(live) if x not in verify]
            if others:
                verify.append(others[int(rng.integers(len(others)))])
        steps.append(Step(parent.index, kind, tuple(drops), tuple(adds), bad_batch, bad_seal, tuple(close),
                          tuple(verify)))
    return steps


def show(step):
    """A step on one line."""
    def tab(s):
        return "%d@%d+%d(%d,%d)%s" % (s.tid, s.first, s.ncell, s.nb, s.k, "L" if s.long else "")
    return ("parent=%s kind=%r drops=%s adds=[%s]%s%s close=%s verify=%s" % (
        step.parent, step.kind, list(step.drops),
        ", ".join("%s:%s:%s" % (r, tab(s), route) for r, s, route in step.adds),
        " bad_batch=[%s]#%d" % (", ".join("%s:%s" % (r, tab(s)) for r, s in step.bad_batch[0]), step.bad_batch[1])
        if step.bad_batch else "",
        " bad_seal=%s:%s" % (step.bad_seal[0], tab(step.bad_seal[1])) if step.bad_seal else "",
        list(step.close), list(step.verify)))


def replay(steps):
    """Walks the model through a script: yields (i, step, live, info) after
    step i's closes, live the open Versions by index, info what the edit did:
    dropped, survivors (Specs, derive order: rows, then L0), the parent."""
    live = {}
    for i, st in enumerate(steps):
        if st.parent is None:
            child, dropped, surv, parent = Version(i), 0, [], None
        else:
            parent = live[st.parent]
            child, dropped = parent.derive(i, st.drops)
            surv = child.every()
        for row, spec, route in st.adds:
            child.add(row, spec, route)
        child.sealed = True
        live[i] = child
        for c in st.close:
            del live[c]
        yield i, st, live, dict(dropped=dropped, survivors=surv, parent=parent, child=child)


def coverage(steps):
    """The names of what a script exercises (tests/test_lset_model.py says
    which must occur over the committed seeds)."""
    seen = set()
    after_parent = collections.defaultdict(set)  # parent index -> children verified after it was closed
    was_full = set()                             # sets whose L0 reached L0_MAX
    packed = set()                               # sets derived with "all" that moved something
    for i, st, live, info in replay(steps):
        child, parent = info["child"], info["parent"]
        for _, s, route in st.adds:
            seen.add("route:%s" % route)
        if len(child.l0) == L0_MAX:
            was_full.add(i)
        if parent is not None:
            seen.add("kind:%r" % (st.kind,))
            held = {s.tid for s in parent.every()}
            if any(d not in held for d in st.drops):
                seen.add("unknown id")
            if any(s.tid in st.drops and s.tid in held for _, s, _ in st.adds):
                seen.add("re-added id")
            if st.bad_batch:
                seen.add("failed batch")
            if st.bad_seal:
                seen.add("failed seal")
            for r in range(NROWS):
                if parent.rows[r] and not child.rows[r] and any(child.rows[x] for x in range(r + 1, NROWS)):
                    seen.add("emptied row under a used one")
            if st.kind == "all" and info["survivors"]:  # a child that continues in the moved tables' chunk
                if any(route == "built" for _, _, route in st.adds):
                    seen.add("built add into a packed child")
                packed.add(i)
                if st.parent in packed and parent.parent not in set(live) | set(st.close) and i in st.verify:
                    seen.add("packed child of a packed child, the grandparent closed")
            if any(is_big(s) for s in info["survivors"]):
                if st.kind == "all":
                    seen.add("own-chunk filter moved by all")
                elif st.kind:
                    seen.add("own-chunk filter under a fraction")
            if st.parent in was_full and sum(1 for s in parent.l0 if s.tid not in st.drops) < L0_MAX:
                seen.add("L0 at its cap, then below")
        for x in st.verify:
            v = live[x]
            if v.parent is not None and v.parent not in live:
                after_parent[v.parent].add(x)
                if len(after_parent[v.parent]) >= 2:
                    seen.add("two children verified after their parent")
            if v.depth >= 3 and not (v.ancestors & set(live)):
                seen.add("three derives deep, every ancestor closed")
    return seen


REQUIRED = ({"kind:%r" % (k,) for k in KINDS} | {"route:%s" % r for r in ROUTES} |
            {"failed seal", "failed batch", "re-added id", "unknown id", "emptied row under a used one",
             "two children verified after their parent", "three derives deep, every ancestor closed",
             "own-chunk filter under a fraction", "own-chunk filter moved by all", "L0 at its cap, then below",
             "built add into a packed child", "packed child of a packed child, the grandparent closed"})


def specs_of(steps):
    """Every table a script ever gives a set that seals, in order of appearance."""
    out, seen = [], set()
    for st in steps:
        for _, s, _ in st.adds:
            if s not in seen:
                seen.add(s)
                out.append(s)
    return out


# ----------------------------------------------------------------- the queries

def var_queries(specs, rng, nrand=300):
    """edit_queries-style: every bound and the keys just outside it, members,
    a key inside every range that is no member, the cells' anchors, random ids,
    and b"", b"user", b"\\xff" * 40; shuffled."""
    q = [k12(int(i)) for i in rng.integers(0, 100 * NCELL + 200, nrand)]
    for s in specs:
        t = table(s)
        lo, hi = t.t[4], t.t[5]
        q += [lo, hi, lo[:-1], hi + b"\x00"]
        q += [t.keys[int(j)] for j in rng.choice(len(t.keys), size=min(8, len(t.keys)), replace=False)]
        if s.long:
            q += [lo + b"a", kvar(anchor(s.first), 21)]
        else:
            inside = [i for i in range(int(lo[4:12]) + 1, int(hi[4:12])) if k12(i) not in t.members]
            q += [k12(inside[int(rng.integers(len(inside)))])] if inside else []
    for c in range(NCELL):
        q += [k12(anchor(c)), kvar(anchor(c), 5)]
    q += [b"", b"user", b"\xff" * 40]
    return [q[int(j)] for j in rng.permutation(len(q))]


def k16_queries(specs, rng, nrand=250):
    """16-byte keys: the tables' 16-byte members, the same ids with other
    tails, random ids, and the long tables' 16-byte lower bounds."""
    ids = [int(i) for i in rng.integers(0, 100 * NCELL + 200, nrand)]
    q = [k16(i, i * 7 % 10000) for i in ids[:nrand // 2]] + [k16(i, int(rng.integers(10000))) for i in ids[nrand // 2:]]
    for s in specs:
        t = table(s)
        mem = [k for k in t.keys if len(k) == 16]
        q += [mem[int(j)] for j in rng.choice(len(mem), size=min(4, len(mem)), replace=False)] if mem else []
    assert all(len(k) == 16 for k in q)
    return [q[int(j)] for j in rng.permutation(len(q))]


# ------------------------------------------------------------ the expectations

class Expect:
    """The expected answers of Versions over one fixed query list."""

    def __init__(self, keys):
        import oracle_ct
        self.oracle = oracle_ct.load()
        self.keys = list(keys)
        self.n = len(self.keys)
        self.data, self.offs = keygen.pack(self.keys)
        self._col = {}

    def columns(self, spec):
        """(may_contain, in range, member) of every query for one table, bool [n] each."""
        if spec not in self._col:
            t = table(spec)
            _, w, nb, k, lo, hi = t.t
            if k:
                may = (self.oracle.probe([(w, nb, k)], self.data, offsets=self.offs)[:, 0] & 1).astype(bool)
            else:
                may = np.ones(self.n, dtype=bool)  # no hash: only the range decides
            inr = np.fromiter((lo <= key <= hi for key in self.keys), dtype=bool, count=self.n)
            mem = np.fromiter((key in t.members for key in self.keys), dtype=bool, count=self.n)
            for a in (may, inr, mem):
                a.setflags(write=False)
            self._col[spec] = (may, inr, mem)
        return self._col[spec]

    def hit(self, spec):
        may, inr, _ = self.columns(spec)
        return may & inr

    def ids(self, v):
        """probe(): uint32 [nrows, n]."""
        out = np.full((v.nrows, self.n), NONE, dtype=np.uint32)
        for r in range(v.nrows):
            for s in v.rows[r]:
                h = self.hit(s)
                assert (out[r, h] == NONE).all(), "the model's own row tables overlap"
                out[r, h] = s.tid
        return out

    def mask(self, v):
        """probe_version()'s L0 mask: uint64 [n], bit j = position j."""
        out = np.zeros(self.n, dtype=np.uint64)
        for j, s in enumerate(v.l0):
            out |= self.hit(s).astype(np.uint64) << np.uint64(j)
        return out

    def answers(self, v, resume=None):
        """Every probe form's expected answer for Version v."""
        ids, mask = self.ids(v), self.mask(v)
        order, _ = v.table_order()
        t0, V = len(v.l0), len(v.every())
        row_ord = ordinals_of(ids, order)
        out = dict(ids=ids, mask=mask, lists=lists_from_ids(ids, order),
                   vlists=version_lists_from(mask, ids, t0, order), walk=walk_from(mask, row_ord, t0))
        out["walk_lists"] = lists_from_ord(out["walk"][1], V)
        if resume is not None:
            out["walk_from"] = walk_from(mask, row_ord, t0, resume)
            out["walk_from_lists"] = lists_from_ord(out["walk_from"][1], V)
        return out

    def texture(self, v):
        """What makes a verification of v more than zeros: row hits, keys in
        range of a table and rejected by its filter, false positives, keys
        with two or more L0 bits."""
        hits = rejected = false_pos = 0
        for s in v.every():
            may, inr, mem = self.columns(s)
            if s not in v.l0:
                hits += int((may & inr).sum())
            rejected += int((inr & ~may).sum())
            false_pos += int((inr & may & ~mem).sum())
        m = self.mask(v)
        two = int(sum(1 for x in m if bin(int(x)).count("1") >= 2))
        return dict(row_hits=hits, rejected=rejected, false_positives=false_pos, two_l0_bits=two)


def resume_for(rng, n, W):
    """Resume steps over [0, W + 2], steps past the last one included, with LSMB_LSET_NONE mixed in."""
    resume = rng.integers(0, W + 3, n).astype(np.uint32)
    resume[rng.random(n) < 0.1] = NONE
    return resume


# -------------------------------------------------- filter-set slot churn

def fset_script(seed, prefill, steps=40):
    """(ops): ("add" | "add_checked" | "add_filter", Spec) or ("remove", j),
    j the position of the table among the live ones in arrival order.  The
    first `prefill` ops are adds; then about `steps` ops climb to the 64-slot
    limit (or as far as they get) and come back down."""
    rng = np.random.default_rng(seed)
    ops, live = [], 0
    geoms = [g for g in GEOMS if g[0] <= 16385]

    def add():
        ncell = int(rng.integers(1, 4))
        g = geoms[int(rng.integers(len(geoms)))]
        spec = Spec(len(ops) + 1, int(rng.integers(0, NCELL - ncell + 1)), ncell, g[0], g[1], bool(rng.random() < 0.125
                                                                                                    and ncell == 1), 40)
        return (("add", "add_checked", "add_filter")[int(rng.integers(3))], spec)

    for _ in range(prefill):
        ops.append(add())
        live += 1
    for j in range(steps):
        p_add = 0.9 if j < steps // 2 else 0.2
        if live < 64 and (live == 0 or rng.random() < p_add):
            ops.append(add())
            live += 1
        else:
            ops.append(("remove", int(rng.integers(live))))
            live -= 1
    return ops
