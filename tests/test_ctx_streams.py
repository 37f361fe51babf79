"""One context, several streams: the device entry points of lsmb_ctx take the
caller's stream, and all of them share the context's build workspace (ws_*),
its probe descriptor array (filt_desc) and the two staging slots of the batched
builds and the compaction calls (slots).  What keeps one stream's kernels from
reading or overwriting what another stream's kernels still use is host-side
bookkeeping (the table in csrc/ctx.hpp): ws_done / ws_stream, desc_done /
desc_stream and slots.done / slots.stream.  A mistake there raises no error; it
gives a filter with wrong words
or a probe with wrong answers, and only when two streams overlap.

Two kinds of test:

 * black box: builds / probes / batches alternate between streams with no host
   synchronisation, and every result equals the CPU oracle's;
 * gated: one stream is made busy for a known while (the gate), the call under
   test is queued behind it, and the test looks at what a call on a second
   stream does meanwhile.  A call that shares the buffer must not complete
   while the gate holds; a call that shares nothing must complete.

A gated test cannot pass vacuously:
 - independence control: before the call under test, a trivial op on the second
   stream must complete while the gate holds.  Two streams on one hardware
   queue would make every "B waited for A" hold for the wrong reason; the test
   then FAILS as inconclusive (streams are taken from torch, four candidates
   at the most per stream);
 - the gate must still hold after the observation, or the test FAILS with
   "gate too short".
The gate is torch.cuda._sleep (a chain of matrix products where torch has none),
never a kernel that spins on a host flag: the library may block the host on an
event queued behind the gate.  Its length is not fixed in advance: the ungated
sequence of each test is timed once (host time to enqueue, and to completion),
a unit of the gate is timed with events, and the gate is max(100 ms, 20 x the
sequence's time to completion), which is at least 20 x its enqueue time.  A
"must not complete" observation polls for 3 x the ungated time to completion
(5 ms at least), so the call had the time to complete had nothing held it back.  Both figures
are printed (pytest -s).
"""
import math
import time

import numpy as np
import pytest

import keygen
import lsmbloom
import sst_support as ss
from test_compact_sst import merge_model

pytestmark = pytest.mark.gpu

MIN_GATE_MS = 100.0   # the gate's least length
GATE_FACTOR = 20      # ... and its least multiple of the ungated sequence's time
MIN_POLL_MS = 5.0     # a "must not complete" observation lasts this long at least (1/20 of the least gate)
MAX_GATE_MS = 4000.0  # a sequence that would need more does not belong in a gated test
CANDIDATES = 4        # streams tried for one independent of the gated stream
GARBAGE = 0x5A5A5A5A5A5A5A5A  # what output-only words hold before a fresh build

_G = {}  # module state: the gate's unit, the streams, the control tensor


def _seed(tag):
    """keygen.key16 seeds of distinct key sets: key i of seed s is key i + 1 of
    seed s - 2, so nearby seeds give nearly the same keys; these are 2^32 apart."""
    return tag << 32


def _dev():
    import torch
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ctx():
    c = lsmbloom.Context(0)
    yield c
    c.close()


def _host(w):
    return w.cpu().numpy().view(np.uint64)


def _cmp(a, b, what=""):
    assert a.shape == b.shape, what
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, "%s: %d words differ from the oracle's, first at %s" % (what, bad.size, bad[:8])


class _synced:
    """Every stream is synchronised before the test goes on or returns, also on
    an assertion failure: no gate outlives its test."""

    def __init__(self, *streams):
        self.streams = streams

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for s in self.streams:
            s.synchronize()
        return False


# ---------------------------------------------------------------- the gate

def _gate_unit():
    """(enqueue one unit of the gate on the current stream, its length in ms):
    torch.cuda._sleep(c) for the smallest c = 10^6 * 4^i that takes 5 ms, timed
    with events; a 4096^2 matrix product where torch has no _sleep."""
    if "unit" in _G:
        return _G["unit"]
    import torch
    s = _streams(1)[0]  # (the stream the tests gate: no stream of its own)
    _G["ctl"] = torch.zeros(64, dtype=torch.int32, device=_dev())  # the control's tensor (_touch)
    torch.cuda.synchronize()

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            fn()  # (the first call loads the kernel)
            t0.record(s)
            fn()
            t1.record(s)
        t1.synchronize()
        return t0.elapsed_time(t1)

    if hasattr(torch.cuda, "_sleep"):
        c = 1_000_000
        ms = timed(lambda: torch.cuda._sleep(c))
        while ms < 5.0 and c < (1 << 40):
            c *= 4
            ms = timed(lambda: torch.cuda._sleep(c))
        fn, what = (lambda: torch.cuda._sleep(c)), "torch.cuda._sleep(%d)" % c
    else:
        a = torch.ones((4096, 4096), dtype=torch.float32, device=_dev())
        _G["mm"] = (a, torch.empty_like(a))
        fn, what = (lambda: torch.mm(a, a, out=_G["mm"][1])), "torch.mm of 4096^2 fp32"
        ms = timed(fn)
    assert ms > 0.0, "the gate's unit (%s) took no measurable time" % what
    print("[ctx_streams] gate unit: %s = %.3f ms" % (what, ms))
    _G["unit"] = (fn, ms)
    return _G["unit"]


def _touch(s):
    """The trivial op of the independence control, on stream s -> its event."""
    import torch
    with torch.cuda.stream(s):
        _G["ctl"].add_(1)
    ev = torch.cuda.Event()
    ev.record(s)
    return ev


class _Gate:
    """Makes `stream` busy for max(MIN_GATE_MS, GATE_FACTOR * run_ms) from now
    on; `end` is recorded right after it."""

    def __init__(self, stream, enq_ms, run_ms, label):
        import torch
        fn, unit_ms = _gate_unit()
        self.ms = max(MIN_GATE_MS, GATE_FACTOR * max(run_ms, enq_ms))
        self.poll_s = max(3.0 * run_ms, MIN_POLL_MS) / 1e3
        self.label = label
        print("[ctx_streams] %s: ungated enqueue %.3f ms, to completion %.3f ms -> gate %.1f ms"
              % (label, enq_ms, run_ms, self.ms))
        if self.ms > MAX_GATE_MS:
            pytest.fail("%s: a gate of %.0f ms is past the %.0f ms a gated test may take" % (label, self.ms, MAX_GATE_MS))
        with torch.cuda.stream(stream):
            for _ in range(int(math.ceil(self.ms / unit_ms))):
                fn()
        self.end = torch.cuda.Event()
        self.end.record(stream)

    def still_closed(self, when):
        if self.end.query():
            pytest.fail("%s: gate too short: its %.0f ms had passed %s, so nothing was observed"
                        % (self.label, self.ms, when))

    def control(self, other):
        """Independence control: a trivial op on `other` completes while the gate holds."""
        _touch(other).synchronize()
        if self.end.query():
            pytest.fail("%s: inconclusive: a trivial op on the second stream completed only after the gate, "
                        "the two streams are not independent (one hardware queue?)" % self.label)

    def completed_early(self, ev):
        """For a call that must wait for the gated stream: polls ev for 3 x the
        ungated sequence's time to completion (MIN_POLL_MS at least).  Returns whether it completed; the
        gate must still hold after the last look."""
        t_end = time.perf_counter() + self.poll_s
        done = ev.query()
        while not done and time.perf_counter() < t_end:
            done = ev.query()
        self.still_closed("after the observation")
        return done

    def completes(self, ev, what):
        """For a call that shares nothing with the gated stream: it completes while the gate holds."""
        ev.synchronize()
        if self.end.query():
            pytest.fail("%s: %s completed only after the gate of %.0f ms (>= %d x the ungated sequence): it waited "
                        "for the gated stream" % (self.label, what, self.ms, GATE_FACTOR))


def _independent(s1, cand):
    import torch
    fn, unit_ms = _gate_unit()
    with torch.cuda.stream(s1):
        for _ in range(int(math.ceil(MIN_GATE_MS / unit_ms))):
            fn()
    end = torch.cuda.Event()
    end.record(s1)
    _touch(cand).synchronize()
    ok = not end.query()
    s1.synchronize()
    return ok


def _streams(n):
    """n user streams (at most three): [0] is the one the tests gate, each of the
    others was seen to run while [0] was gated.  Each test asserts that again
    with its own gate (_Gate.control)."""
    import torch
    assert n <= 3
    st = _G.setdefault("streams", [])
    if not st:
        st.append(torch.cuda.Stream())
    while len(st) < n:
        for _ in range(CANDIDATES):
            cand = torch.cuda.Stream()
            _G.setdefault("rejected", []).append(cand)  # (kept alive: a freed stream's queue would be handed out again)
            if _independent(st[0], cand):
                st.append(cand)
                break
        else:
            pytest.fail("inconclusive: none of %d torch streams runs while another one is busy "
                        "(they share a hardware queue): stream ordering cannot be observed" % CANDIDATES)
    return st[:n]


def _time_ungated(enqueue, streams):
    """The sequence once cold, then timed: host ms to enqueue, and to completion."""
    import torch
    enqueue()
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    enqueue()
    t1 = time.perf_counter()
    for s in streams:
        s.synchronize()
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t0) * 1e3


# ---------------------------------------------------------------- builds (ws_done)

class _Job:
    """One device build: its keys on the device, its own output words, the oracle's filter.
    kind: acc (lsmb_build_fixed_dev into zeroed words), new / var_new / sweep_new
    (the fresh entry points, into garbage)."""

    def __init__(self, kind, n, filter_keys, seed, strategy, keys_h=None, sweep=None):
        import torch
        self.kind, self.n, self.sweep = kind, n, sweep
        self.nb, self.k = lsmbloom.params(filter_keys, 0.01)
        assert lsmbloom.build_strategy(self.nb, n, self.k) == strategy
        if kind == "var_new":
            self.data_h, self.offs_h = keygen.varlen(n, first=seed)  # (seed: the first key of the global stream)
            self.data = torch.from_numpy(self.data_h).to(_dev())
            self.offs = torch.from_numpy(self.offs_h.view(np.int64)).to(_dev())
        else:
            self.keys_h = keygen.key16(_seed(seed), 0, n) if keys_h is None else keys_h
            self.keys = torch.from_numpy(self.keys_h).to(_dev())
        self.w = torch.empty(lsmbloom.num_words(self.nb), dtype=torch.int64, device=_dev())
        self.reset()

    def other_sweep(self, sweep):
        """The same build's other sweep: same keys, same words."""
        import copy
        j = copy.copy(self)
        j.sweep = sweep
        return j

    def reset(self):
        self.w.fill_(0 if self.kind == "acc" else GARBAGE)

    def enqueue(self, ctx, s):
        st = s.cuda_stream
        if self.kind == "acc":
            ctx.build_fixed_dev(self.keys, 16, self.n, self.nb, self.k, self.w, stream=st)
        elif self.kind == "new":
            ctx.build_fixed_dev_new(self.keys, 16, self.n, self.nb, self.k, self.w, stream=st)
        elif self.kind == "var_new":
            ctx.build_var_dev_new(self.data, self.offs, self.n, self.nb, self.k, self.w, stream=st)
        else:
            ctx.build_fixed_dev_sweep_new(self.keys, 16, self.n, self.nb, self.k, self.w, self.sweep, stream=st)

    def check(self, oracle, what):
        if self.kind == "var_new":
            ref = oracle.build_var_mt(self.data_h, self.offs_h, self.nb, self.k, 16)
        else:
            ref = oracle.build_fixed_mt(self.keys_h, 16, self.nb, self.k, 16)
        _cmp(_host(self.w), ref, what)


# The builds that use the shared workspace, each at the smallest shape that takes
# its path: (kind, n, filter sized for, strategy).  tiled: prehash records in
# ws_hashes.  partition: 95.67 M bits, 92 bins of 2^20 bits, one sweep; acc is
# pass A into regions, new the LIST pass A (ws_ovl / ws_ovn), var_new k_hash_var
# and the walk records in ws_hashes.
WS_CASES = {
    "tiled": ("acc", 150_000, 150_000, "tiled"),
    "partition": ("acc", 200_000, 10_000_000, "partition"),
    "partition-new": ("new", 200_000, 10_000_000, "partition"),
    "partition-var-new": ("var_new", 200_000, 10_000_000, "partition"),
}
# Two sweeps: new(10^9, 0.01) saturates at 2^32 - 1 bits (512 MiB).  The planner
# takes few keys into a big filter to scattered atomics (n * k < nw32 / 16, here
# below 1 198 373 keys: one sweep), so the smallest round n with two sweeps is
# past that; 4 M is the suite's bound for this file.
SWEEP_CASE = ("sweep_new", 4_000_000, 10**9, "partition")


def _jobs(case, count):
    if case == "sweep":
        kind, n, fk, strat = SWEEP_CASE
        a = _Job(kind, n, fk, 0xC5A0, strat, sweep=0)
        assert lsmbloom.build_sweeps(a.nb, n, a.k) == 2
        return [a, a.other_sweep(1)]
    kind, n, fk, strat = WS_CASES[case]
    if kind == "var_new":
        return [_Job(kind, n, fk, i * n, strat) for i in range(count)]
    return [_Job(kind, n, fk, 0xC5A0 + i, strat) for i in range(count)]


def _gated_builds(ctx, oracle, label, jobs, streams):
    """jobs[i] goes on streams[i]; streams[0] is gated, jobs[1] (on another
    stream) must not complete while the gate holds; every filter equals the oracle's."""
    import torch
    distinct = list(dict.fromkeys(streams))

    def enqueue():
        for j, s in zip(jobs, streams):
            j.enqueue(ctx, s)

    with _synced(*distinct):
        enq_ms, run_ms = _time_ungated(enqueue, distinct)
        for j in jobs:
            j.reset()
        torch.cuda.synchronize()
        gate = _Gate(streams[0], enq_ms, run_ms, label)
        jobs[0].enqueue(ctx, streams[0])
        gate.control(streams[1])
        jobs[1].enqueue(ctx, streams[1])
        ev_b = torch.cuda.Event()
        ev_b.record(streams[1])
        for j, s in zip(jobs[2:], streams[2:]):
            j.enqueue(ctx, s)
        early = gate.completed_early(ev_b)
    seen = set()
    for i, j in enumerate(jobs):
        if id(j.w) not in seen:  # (the two sweeps share their words)
            seen.add(id(j.w))
            j.check(oracle, "%s: build %d" % (label, i))
    assert not early, ("%s: the second stream's build completed while the first stream's build was still queued "
                       "behind the gate: nothing ordered it after the workspace's last user" % label)


@pytest.mark.parametrize("case", list(WS_CASES) + ["sweep"])
def test_ws_build_on_second_stream_waits_for_the_first(ctx, oracle, case):
    s1, s2 = _streams(2)
    _gated_builds(ctx, oracle, "ws %s" % case, _jobs(case, 2), [s1, s2])


def test_ws_roles_reversed(ctx, oracle):
    s1, s2 = _streams(2)
    _gated_builds(ctx, oracle, "ws partition, A on the second stream", _jobs("partition", 2), [s2, s1])


def test_ws_three_call_chain(ctx, oracle):
    s1, s2 = _streams(2)
    _gated_builds(ctx, oracle, "ws partition-new, chain s1 s2 s1", _jobs("partition-new", 3), [s1, s2, s1])


def test_ws_ungated_interleave_six_builds(oracle):
    """Six builds alternate between two streams with no host synchronisation:
    the shapes above, one that grows the workspace while the other stream's
    build is in flight (a context of its own, so it does grow), and an lds and
    an atomic build, which take no workspace and must not be disturbed."""
    import torch
    s1, s2 = _streams(2)
    c = lsmbloom.Context(0)
    try:
        jobs = [
            _Job("acc", 200_000, 10_000_000, 0x1A00, "partition"),
            _Job("new", 4_000_000, 10_000_000, 0x1B00, "partition"),  # grows regions, counts, lists
            _Job("acc", 50_000, 50_000, 0x1C00, "lds"),
            _Job("acc", 150_000, 150_000, 0x1D00, "tiled"),
            _Job("acc", 1000, 10_000_000, 0x1E00, "atomic"),
            _Job("var_new", 200_000, 10_000_000, 0, "partition"),
        ]
        torch.cuda.synchronize()
        with _synced(s1, s2):
            for i, j in enumerate(jobs):
                j.enqueue(c, (s1, s2)[i & 1])
        for i, j in enumerate(jobs):
            j.check(oracle, "interleave: build %d (%s)" % (i, j.kind))
    finally:
        c.close()


def test_ws_no_stale_overflow_across_streams(ctx, oracle):
    """Duplicate-heavy keys (the pattern of test_fresh_overflow_side_buffer at
    1 M keys) spill rings into the overflow words on one stream; a clean fresh
    build on the other stream follows with no host synchronisation and must see
    them all-zero again."""
    import torch
    s1, s2 = _streams(2)
    n = 1_000_000
    keys_h = keygen.key16(0xD00D, 0, n)
    keys_h[:n // 5] = keys_h[0]
    keys_h[n // 5:3 * n // 10] = keys_h[n // 2]
    dup = _Job("new", n, 10_000_000, 0, "partition", keys_h=keys_h)
    clean = _Job("new", 200_000, 10_000_000, 0xC1EA, "partition")
    torch.cuda.synchronize()
    with _synced(s1, s2):
        dup.enqueue(ctx, s1)
        clean.enqueue(ctx, s2)
    dup.check(oracle, "duplicate-heavy fresh build")
    clean.check(oracle, "clean fresh build after it, other stream")


def test_ws_host_build_after_device_build(ctx, oracle):
    """lsmb_build_fixed_dev on a user stream, not synchronised, then at once the
    synchronous host-memory build (the context's own stream) into a
    partition-sized filter: it must wait for the workspace too."""
    import torch
    (s1,) = _streams(1)
    a = _Job("acc", 200_000, 10_000_000, 0x2A00, "partition")
    keys_b = keygen.key16(_seed(0x2B00), 0, 200_000)
    assert keys_b.shape[0] > lsmbloom.host_max_keys()
    torch.cuda.synchronize()
    with _synced(s1):
        a.enqueue(ctx, s1)
        got_b = ctx.build_fixed(keys_b, 16, a.nb, a.k)
    a.check(oracle, "device build on the user stream")
    _cmp(got_b, oracle.build_fixed_mt(keys_b, 16, a.nb, a.k, 16), "host-memory build after it")


# ---------------------------------------------------------------- probes (desc_done)

NQ = 20_000
GENERIC_SETS = (  # (keys, fpr) per filter: mixed (num_bits, k), so k_probe_generic reads filt_desc
    ((1000, 0.01), (5000, 0.001), (30_000, 0.05), (200, 0.5)),
    ((2000, 0.01), (4000, 0.001), (20_000, 0.05), (300, 0.5)),
    ((1500, 0.01), (6000, 0.001), (25_000, 0.05), (100, 0.5)),
)
SLICED_SETS = (((1000, 0.01),) * 8,) * 3  # eight SSTable filters: the bit-sliced kernel, no descriptors


class _ProbeSets:
    """Three filter sets of one filter count (host and device), 20 000 16-byte
    queries of which half are members of the second set, the oracle's answers
    per set.  Every device tensor lives as long as this object."""

    def __init__(self, oracle, shapes, seed):
        import torch
        self.host, self.dev, members = [], [], []
        for j, shape in enumerate(shapes):
            hs = []
            for i, (n, fpr) in enumerate(shape):
                nb, k = lsmbloom.params(n, fpr)
                keys = keygen.key16(_seed(seed + 16 * j + i), 0, n)
                hs.append((oracle.build_fixed(keys, 16, nb, k), nb, k))
                if j == 1:
                    members.append(keys)
            self.host.append(hs)
            self.dev.append([(torch.from_numpy(w.view(np.int64)).to(_dev()), nb, k) for (w, nb, k) in hs])
        mem = np.concatenate(sorted(members, key=len, reverse=True))[:NQ // 2]  # (the biggest filter's keys first)
        self.q_h = np.concatenate([mem, keygen.key16(_seed(seed + 0x999), 0, NQ - mem.shape[0])])
        self.q = torch.from_numpy(self.q_h).to(_dev())
        self.ref = [oracle.probe(hs, self.q_h, key_len=16) for hs in self.host]
        self.out = [torch.zeros(self.ref[0].shape, dtype=torch.uint8, device=_dev()) for _ in range(4)]
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def generic(oracle):
    p = _ProbeSets(oracle, GENERIC_SETS, 0x7000)
    for hs in p.host:  # mixed (num_bits, k): not the bit-sliced kernel's shape
        assert len({(nb, k) for (_, nb, k) in hs}) > 1
    # a stale or overwritten descriptor array gives another set's answers: they differ in thousands of rows
    for a in range(3):
        for b in range(a + 1, 3):
            assert int((p.ref[a] != p.ref[b]).any(axis=1).sum()) > 2000, (a, b)
    return p


@pytest.fixture(scope="module")
def sliced(oracle):
    p = _ProbeSets(oracle, SLICED_SETS, 0x7800)
    for a in range(3):
        for b in range(a + 1, 3):
            assert int((p.ref[a] != p.ref[b]).any(axis=1).sum()) > 2000, (a, b)
    return p


def _probe_scenario(ctx, p, label, shares, third, with_empty=False):
    """The opening of both scenarios: set 0 on s1, synchronised; the gate on s1;
    set 1 on s1 (a generic probe's upload queues behind the gate); set 1 on s2
    into its own output.  third: then set 2 on s3 while s1's probe is still
    queued.  shares: the probes read the context's descriptor array (generic),
    so s2's probe must not complete before the gate ends; else (bit-sliced) it
    must complete while the gate holds, and so must s3's.
    Returns whether s2's probe completed while the gate held."""
    import torch
    s1, s2, s3 = _streams(3)
    used = (s1, s2, s3) if third else (s1, s2)
    o_first, o_s1, o_s2, o_s3 = p.out

    def probe(j, out, s, n=NQ):
        ctx.probe_dev(p.dev[j], p.q, n, out, key_len=16, stream=s.cuda_stream)

    def sequence(open_gate=None):
        probe(0, o_first, s1)
        s1.synchronize()
        gate = open_gate() if open_gate else None
        probe(1, o_s1, s1)
        if gate:
            gate.control(s2)
        if with_empty:
            probe(2, o_s3, s2, n=0)  # kb.n == 0: no launch, and it must leave the bookkeeping alone
        probe(1, o_s2, s2)
        ev2 = torch.cuda.Event()
        ev2.record(s2)
        ev3 = None
        if third:
            if gate:
                gate.control(s3)
                gate.still_closed("before the third set's probe was issued")
            probe(2, o_s3, s3)  # (new descriptors: the library's host wait may last as long as the gate)
            ev3 = torch.cuda.Event()
            ev3.record(s3)
        return gate, ev2, ev3

    early = None
    with _synced(*used):
        enq_ms, run_ms = _time_ungated(sequence, used)
        for o in p.out:
            o.zero_()
        torch.cuda.synchronize()
        gate, ev2, ev3 = sequence(lambda: _Gate(s1, enq_ms, run_ms, label))
        if not shares:
            gate.completes(ev2, "the second stream's bit-sliced probe")
            if third:
                gate.completes(ev3, "the third stream's bit-sliced probe")
        elif not third:
            early = gate.completed_early(ev2)
    got = [o.cpu().numpy() for o in p.out]
    return early, got


def _answers(p, got, j):
    """Which set's answers an output holds, for the failure message."""
    same = [k for k in range(3) if np.array_equal(got, p.ref[k])]
    return "set %d's answers expected, got %s" % (j, ("set %d's" % same[0]) if same else "no set's")


@pytest.mark.parametrize("with_empty", [False, True])
def test_desc_same_filters_on_second_stream_are_not_read_stale(ctx, generic, with_empty):
    """The second stream's probe takes the descriptors the first stream's probe
    uploads; that upload is still queued behind the gate.  Its kernel must run
    after the upload: right answers, and not before the gate ends."""
    p = generic
    early, got = _probe_scenario(ctx, p, "desc stale read%s" % (" + empty probe" if with_empty else ""),
                                 shares=True, third=False, with_empty=with_empty)
    assert np.array_equal(got[0], p.ref[0]), _answers(p, got[0], 0)
    assert np.array_equal(got[1], p.ref[1]), "first stream: " + _answers(p, got[1], 1)
    assert np.array_equal(got[2], p.ref[1]), "second stream: " + _answers(p, got[2], 1)
    assert not early, "the second stream's probe completed while the descriptors' upload was still queued behind the gate"


def test_desc_upload_does_not_overwrite_under_a_queued_reader(ctx, generic):
    """After probes on two streams, a third set's upload must wait for both
    readers, not for the latest launch alone: the first stream's probe is still
    queued behind the gate when the third set is probed on a third stream."""
    p = generic
    _, got = _probe_scenario(ctx, p, "desc overwrite", shares=True, third=True)
    assert np.array_equal(got[1], p.ref[1]), "first stream: " + _answers(p, got[1], 1)
    assert np.array_equal(got[2], p.ref[1]), "second stream: " + _answers(p, got[2], 1)
    assert np.array_equal(got[3], p.ref[2]), "third stream: " + _answers(p, got[3], 2)


@pytest.mark.parametrize("third", [False, True])
def test_desc_sliced_probes_stay_independent(ctx, sliced, third):
    """Control: the bit-sliced probe takes its filters in the kernel arguments,
    shares nothing, and must not be made to wait for another stream."""
    p = sliced
    _, got = _probe_scenario(ctx, p, "sliced probes%s" % (", three streams" if third else ""), shares=False,
                             third=third, with_empty=True)
    assert np.array_equal(got[1], p.ref[1]) and np.array_equal(got[2], p.ref[1])
    if third:
        assert np.array_equal(got[3], p.ref[2])


# ---------------------------------------------------------------- batched build (slots.done)

BB_COUNTS = (0, 1, 63, 64, 65, 1000)  # six SSTable filters of 0 .. 1000 keys
BB_SEG = np.concatenate([[0], np.cumsum(BB_COUNTS)]).astype(np.uint64)
BB_SST = lsmbloom.params(1000, 0.01)  # SSTableBuilder's filter


class _Batch:
    def __init__(self, seed):
        import torch
        self.n = int(BB_SEG[-1])
        self.nb, self.kk = [BB_SST[0]] * len(BB_COUNTS), [BB_SST[1]] * len(BB_COUNTS)
        self.keys_h = keygen.key16(_seed(seed), 0, self.n)
        self.data = torch.from_numpy(np.concatenate([self.keys_h.reshape(-1), np.zeros(16, np.uint8)])).to(_dev())
        self.total = int(lsmbloom.build_batch_layout(self.nb)[-1])
        self.words = torch.empty(self.total, dtype=torch.int64, device=_dev())
        self.reset()

    def reset(self):
        self.words.fill_(-1)  # output-only: every byte 0xFF

    def enqueue(self, ctx, s):
        self.woff = ctx.build_batch_dev(self.data, self.n, BB_SEG, self.nb, self.kk, self.words, key_len=16,
                                        stream=s.cuda_stream)

    def check(self, oracle, what):
        got = _host(self.words)
        nw = lsmbloom.num_words(BB_SST[0])
        for t in range(len(BB_COUNTS)):
            lo, hi = int(BB_SEG[t]), int(BB_SEG[t + 1])
            exp = oracle.build_fixed(self.keys_h[lo:hi], 16, *BB_SST) if hi > lo else np.zeros(nw, np.uint64)
            _cmp(got[int(self.woff[t]):int(self.woff[t]) + nw], exp, "%s, table %d" % (what, t))


def test_bb_five_batches_alternate_streams(ctx, oracle):
    import torch
    s1, s2 = _streams(2)
    batches = [_Batch(0xBB00 + i) for i in range(5)]
    torch.cuda.synchronize()
    with _synced(s1, s2):
        for i, b in enumerate(batches):
            b.enqueue(ctx, (s1, s2)[i & 1])
    for i, b in enumerate(batches):
        b.check(oracle, "batch %d" % i)


def test_bb_other_slot_runs_and_reused_slot_waits(ctx, oracle):
    """Batch 1 behind the gate on s1; batch 2 on s2 takes the other slot and
    completes while the gate holds; batch 3 on s2 refills batch 1's slot (the
    library waits for batch 1 first, for as long as the gate) and comes out right."""
    import torch
    s1, s2 = _streams(2)
    b1, b2, b3 = (_Batch(0xBC00 + i) for i in range(3))

    def enqueue():
        b1.enqueue(ctx, s1)
        b2.enqueue(ctx, s2)
        b3.enqueue(ctx, s2)

    with _synced(s1, s2):
        enq_ms, run_ms = _time_ungated(enqueue, (s1, s2))
        for b in (b1, b2, b3):
            b.reset()
        torch.cuda.synchronize()
        gate = _Gate(s1, enq_ms, run_ms, "bb slots")
        b1.enqueue(ctx, s1)
        gate.control(s2)
        b2.enqueue(ctx, s2)
        ev2 = torch.cuda.Event()
        ev2.record(s2)
        gate.completes(ev2, "the batch in the other slot")
        b3.enqueue(ctx, s2)
    for i, b in enumerate((b1, b2, b3)):
        b.check(oracle, "batch %d" % (i + 1))


# ---------------------------------------------------------------- the slots' three routes

class _BlocksBatch:
    """Three SSTable filters straight from seven data blocks of 1 .. 20 entries
    at odd offsets, the middle table without a block."""
    COUNTS = ((20, 1, 7), (), (13, 20, 2, 5))

    def __init__(self, tag):
        import torch
        self.tables, first = [], 0
        for counts in self.COUNTS:
            self.tables.append([])
            for c in counts:
                self.tables[-1].append(ss.encode_block([(b"%04x-%08d" % (tag, first + i), b"v" * (i % 5))
                                                        for i in range(c)]))
                first += c
        buf, self.blk_off, self.blk_len = ss.place([b for t in self.tables for b in t], odd=True)
        assert all(int(o) % 2 for o in self.blk_off)
        self.bseg = np.concatenate([[0], np.cumsum([len(t) for t in self.tables])]).astype(np.uint64)
        self.bytes = torch.from_numpy(np.array(buf, dtype=np.uint8)).to(_dev())
        self.nb, self.kk = [BB_SST[0]] * len(self.tables), [BB_SST[1]] * len(self.tables)
        self.words = torch.full((int(lsmbloom.build_batch_layout(self.nb)[-1]),), -1, dtype=torch.int64, device=_dev())
        self.ent = torch.full((len(self.blk_off),), -1, dtype=torch.int32, device=_dev())

    def enqueue(self, ctx, s):
        self.woff = ctx.build_batch_sst_dev(self.bytes, self.blk_off, self.blk_len, self.bseg, self.nb, self.kk,
                                            self.words, blk_entries=self.ent, stream=s.cuda_stream)

    def check(self, oracle, what):
        got = _host(self.words)
        nw = lsmbloom.num_words(BB_SST[0])
        for t, blocks in enumerate(self.tables):
            keys = [k for b in blocks for k in ss.parse_block(b)]
            exp = oracle.build_var(*keygen.pack(keys), *BB_SST) if keys else np.zeros(nw, np.uint64)
            _cmp(got[int(self.woff[t]):int(self.woff[t]) + nw], exp, "%s, table %d" % (what, t))
        assert [int(e) for e in self.ent.cpu().numpy()] == [c for counts in self.COUNTS for c in counts], what


class _Compaction:
    """Two sources of two blocks each, drop_tombstones = 1: key 13 is in both
    sources, key 2 is a tombstone in the newer one.  The outputs are sized from
    the model, so that the gather can follow its mark with nothing in between."""

    def __init__(self, tag):
        import torch

        def block(lo, n, tomb=None):
            return ss.encode_block([(b"%04x-%08d" % (tag, i), b"" if i == tomb else b"val") for i in range(lo, lo + n)])

        self.sources = [[block(0, 5, tomb=2), block(10, 4)], [block(5, 5), block(13, 6)]]  # newest first
        buf, self.blk_off, self.blk_len = ss.place(self.sources[0] + self.sources[1], odd=True)
        self.sseg = np.array([0, 2, 4], dtype=np.uint64)
        self.exp, self.seen, bad, _ = merge_model(self.sources, 1)
        assert len(self.exp) == 18 and self.seen == 20 and bad == 0  # 20 entries less the tombstone and the older 13
        dev = _dev()
        self.bytes = torch.from_numpy(np.array(buf, dtype=np.uint8)).to(dev)
        self.work = torch.full((lsmbloom.compact_sst_work_bytes(self.blk_len),), 0xFF, dtype=torch.uint8, device=dev)
        self.totals = torch.full((4,), -1, dtype=torch.int64, device=dev)
        self.key_data = torch.full((sum(len(k) for k in self.exp),), 0xFF, dtype=torch.uint8, device=dev)
        self.key_offs = torch.full((len(self.exp) + 1,), -1, dtype=torch.int64, device=dev)

    def mark(self, ctx, s):
        ctx.compact_sst_mark_dev(self.bytes, self.blk_off, self.blk_len, self.sseg, 1, self.work, self.totals,
                                 stream=s.cuda_stream)

    def gather(self, ctx, s):
        ctx.compact_sst_gather_dev(self.bytes, self.blk_off, self.blk_len, self.sseg, self.work, self.key_data,
                                   self.key_offs, stream=s.cuda_stream)

    def check(self, what):
        data, o = self.key_data.cpu().numpy().tobytes(), _host(self.key_offs)
        assert [int(x) for x in _host(self.totals)] == [len(self.exp), len(data), self.seen, 0], what
        assert [data[int(o[i]):int(o[i + 1])] for i in range(len(self.exp))] == self.exp, what


def test_slots_shared_by_three_routes(ctx, oracle):
    """The batched build, the build from blocks and the compaction's mark and
    gather stage their work lists through the same two slots.  Eight calls on
    two streams with no host synchronisation, each gather behind its own mark:
    each slot is refilled by another route, from another stream, than its last
    user's.  Every output starts as 0xFF and equals the oracle's filters or the
    dict merge's survivors."""
    import torch
    s1, s2 = _streams(2)
    a, b = _Batch(0xBD00), _Batch(0xBD01)
    p, q = _BlocksBatch(0xBD02), _BlocksBatch(0xBD03)
    m, n = _Compaction(0xBD04), _Compaction(0xBD05)
    torch.cuda.synchronize()
    with _synced(s1, s2):
        a.enqueue(ctx, s1)
        m.mark(ctx, s2)
        p.enqueue(ctx, s1)
        m.gather(ctx, s2)
        b.enqueue(ctx, s2)
        q.enqueue(ctx, s2)
        n.mark(ctx, s1)
        n.gather(ctx, s1)
    a.check(oracle, "call 1, batched build")
    b.check(oracle, "call 5, batched build")
    p.check(oracle, "call 3, build from blocks")
    q.check(oracle, "call 6, build from blocks")
    m.check("calls 2 and 4, compaction")
    n.check("calls 7 and 8, compaction")
