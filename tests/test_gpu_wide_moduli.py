"""GPU parity for filters of 2^31 .. 2^32-2 bits.

fits_walk32(d) is d <= 2^31: below it pass A walks with 32-bit remainders
(Walk32 / RecWalk32), the saturated 2^32-1-bit filter folds (WalkM), and every
size in between takes Walk64 / RecWalk64, Mod32::reduce with d > 2^31 and the
third branch of WalkRec::make.  These are ordinary product sizes (new(n, .01)
for 225 M < n < 448 M keys), and the planner makes choices there that no other
size takes: 2^21-bit bins with a last bin one bit wide (2^31 + 1), 72- and
56-entry rings, and 1024 bins per sweep with 32-entry rings and two keys per
lane (2^32 - 2; the plan switches that combination off for 2^32 - 1 alone).

Every word of every build and every probe answer is compared with the CPU
oracle (16 threads); nothing has a tolerance.  The oracle's words go up to the
device and are compared there, which keeps a case with three 512 MiB filters
under a second.  Each build asserts its strategy
and sweep count first, so a planner change cannot move a case onto a kernel
another test already covers.  Which k_bin instantiation (pick_k_bin,
csrc/bloom_build.hip) a case reaches is noted at the case.
"""
import warnings

import numpy as np
import pytest

import keygen
import lsmbloom
from lsmbloom import BloomFilter, FilterSet
from lset_support import check_mask_lists as check_lists, expected_masks

pytestmark = pytest.mark.gpu

NB3E8 = 2_870_145_874        # new(300_000_000, .01), k = 7
NB25E7 = 3_587_682_343       # new(250_000_000, .001), k = 10
NB = [2**31, 2**31 + 1, NB3E8, 2**32 - 2]
PRESET = 0x8000000000000001  # every 101st word of an accumulate build's starting words

_KEYS = {}
_REFS = {}


@pytest.fixture(scope="module")
def ctx():
    c = lsmbloom.Context(0)
    yield c
    c.close()


def _dev():
    import torch
    return torch.device("cuda:0")


def _to_dev(a):
    import torch
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)  # (read-only references upload as they are)
        return torch.from_numpy(a).to(_dev())


def _host(w):
    import torch
    torch.cuda.synchronize()
    return w.cpu().numpy().view(np.uint64)


def _cmp(a, b):
    assert a.shape == b.shape
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, "%d words differ, first %s" % (bad.size, bad[:8])


def _garbage(nw, seed):
    import torch
    g = torch.Generator(device=_dev()).manual_seed(seed)
    return torch.randint(-2**62, 2**62, (nw,), generator=g, dtype=torch.int64, device=_dev())


def _ones(nw):
    import torch
    return torch.full((nw,), -1, dtype=torch.int64, device=_dev())


def _preset(nw):
    """Device words with a sparse preset: the start of an accumulate build."""
    import torch
    w = torch.zeros(nw, dtype=torch.int64, device=_dev())
    w[::101] = PRESET - 2**64
    return w


def _check(w, ref, preset=False, lo=0, hi=None):
    """Every word of the device words w[lo:hi] equals ref[lo:hi] (| the preset
    of an accumulate build).  The oracle's words go up and the comparison runs
    on the device (torch.equal over int64: exact); only a mismatch brings the
    words to the host, for the report."""
    import torch
    exp = _to_dev(ref.view(np.int64))
    if preset:
        exp = exp.clone()  # (never the reference's own memory)
        exp[::101] |= PRESET - 2**64
    if torch.equal(w[lo:hi], exp[lo:hi]):
        return
    _cmp(_host(w[lo:hi]), _host(exp[lo:hi]))


def _keys(tag):
    """The shared key sets, generated once: K8 / K2 = 8 M / 2 M key16, V = 1.55 M
    var-len keys (C4's shape; builds take the first 1.5 M, probes the rest as
    non-members)."""
    if tag not in _KEYS:
        if tag == "K8":
            _KEYS[tag] = keygen.key16(0xA1D00001, 0, 8_000_000)
        elif tag == "K2":
            _KEYS[tag] = keygen.key16(0xB1D00001, 0, 2_000_000)
        elif tag == "V":
            _KEYS[tag] = keygen.varlen(1_550_000)
    return _KEYS[tag]


NV = 1_500_000


def _varlen_members():
    data, offs = _keys("V")
    return data[:int(offs[NV])], offs[:NV + 1]


def _ref(oracle, tag, nb, k):
    """The oracle's filter over a shared key set, built once per (keys, nb, k)
    and read-only from then on."""
    key = (tag, nb, k)
    if key not in _REFS:
        if tag == "V":
            data, offs = _varlen_members()
            r = oracle.build_var_mt(data, offs, nb, k, 16)
        else:
            r = oracle.build_fixed_mt(_keys(tag), 16, nb, k, 16)
        r.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


def _plan(nb, n, k, strategy, sweeps):
    assert lsmbloom.build_strategy(nb, n, k) == strategy
    assert lsmbloom.build_sweeps(nb, n, k) == sweeps


# ---------------------------------------------------------------- 1. the plans
def test_sizes_and_plans_are_the_uncovered_ones():
    """The product sizes land strictly between 2^31 and 2^32 - 1, and the
    planner gives every size here the sweeps the cases below rely on (256 CUs,
    plan knobs unset): 2 sweeps at k = 7 (2^20-bit bins at 2^31, 2^21-bit bins
    above), 3 sweeps of 2^20-bit bins for k = 5, 10, 16 at 3e9 bits, 4 at
    k = 32; k = 33 and 1000 keys are atomic builds."""
    assert lsmbloom.params(300_000_000, 0.01) == (NB3E8, 7)
    assert lsmbloom.params(250_000_000, 0.001) == (NB25E7, 10)
    assert 2**31 < NB3E8 < 2**32 - 1 and 2**31 < NB25E7 < 2**32 - 1
    for nb in NB:
        _plan(nb, 8_000_000, 7, "partition", 2)
        _plan(nb, 2_000_000, 7, "partition", 2)
    for nb in NB[1:]:  # two sweeps of 2^21-bit bins: sweep 0 ends at a multiple of 2^21 bits
        bins = (nb + 2**21 - 1) >> 21
        lo, hi = lsmbloom.sweep_words(nb, 2_000_000, 0, 7)
        assert (lo, hi) == (0, (bins + 1) // 2 * 2**15)
    assert lsmbloom.sweep_words(2**31 + 1, 2_000_000, 0, 7) == (0, 513 * 2**15)  # 513 + 512 bins, the last one bit wide
    assert lsmbloom.sweep_words(2**31, 2_000_000, 0, 7) == (0, 2**24)            # 1024 2^20-bit bins
    for k, n, sweeps in ((5, 2_000_000, 3), (16, 1_000_000, 3), (32, 600_000, 4)):
        _plan(3_000_000_000, n, k, "partition", sweeps)
    _plan(NB25E7, 2_000_000, 10, "partition", 4)
    _plan(3_000_000_000, 600_000, 33, "atomic", 1)
    _plan(NB3E8, 1000, 7, "atomic", 1)


# ---------------------------------------------------------------- 2. accumulate, steady state
@pytest.mark.parametrize("nb", NB)
def test_accumulate_fixed16_k7_steady_state(ctx, oracle, nb):
    """8 M key16 OR-accumulated onto a sparse preset, k = 7, two sweeps with two
    keys per lane: k_bin<Fixed16, Walk64, 7, true, false, 2, 21> above 2^31,
    k_bin<Fixed16, Walk32, 7, true, false, 2, 20> at 2^31 itself (the last
    Walk32 size, 2048 2^20-bit bins).

    Why 8 M: pass A runs one workgroup per CU for 2^21-bit bins (256 on an
    MI355X), and each (workgroup, bin) ring receives n k / (256 nbins)
    entries: 213 = 3.0 ring lengths at 2^31 + 1 (1025 bins, 72-entry rings,
    the widest), 159 = 2.8 at new(3e8, .01) (1369 bins, 56 entries) and
    107 = 3.3 at 2^32 - 2 (2048 bins, 32 entries).  So every ring wraps and
    every region takes more than one 24-entry segment flush: steady state, not
    the first fill.  (2^31 has two workgroups per CU and 2048 bins: 53
    entries, 1.7 lengths of its 32-entry rings, 2.2 segments.)"""
    n, k = 8_000_000, 7
    _plan(nb, n, k, "partition", 2)
    w = _preset(lsmbloom.num_words(nb))
    ctx.build_fixed_dev(_to_dev(_keys("K8")), 16, n, nb, k, w)
    _check(w, _ref(oracle, "K8", nb, k), preset=True)


# ---------------------------------------------------------------- 3. fresh builds
@pytest.mark.parametrize("nb,ones", [(2**31 + 1, True), (NB3E8, False), (2**32 - 2, False)])
def test_fresh_fixed16_k7(ctx, oracle, nb, ones):
    """build_fixed_dev_new into all-ones / garbage words: the LIST pass A,
    k_bin<Fixed16, Walk64, 7, true, false, 1, 21, true>, and the pass B that
    never reads the words."""
    n, k = 2_000_000, 7
    _plan(nb, n, k, "partition", 2)
    nw = lsmbloom.num_words(nb)
    w = _ones(nw) if ones else _garbage(nw, nb & 0xFFFF)
    ctx.build_fixed_dev_new(_to_dev(_keys("K2")), 16, n, nb, k, w)
    _check(w, _ref(oracle, "K2", nb, k))


# ---------------------------------------------------------------- 4. pinned 2^20-bit bins
def test_pinned_2_20_bit_bins(ctx, oracle, monkeypatch):
    """new(3e8, .01) with LSMB_SLICE_LOG2=20: 2738 bins in three sweeps of the
    2^20-wide kernels (913 bins, 40-entry rings, two keys per lane),
    k_bin<Fixed16, Walk64, 7, true, false, 2, 20> (accumulate) and the LIST
    form <..., 1, 20, true> (fresh)."""
    monkeypatch.setenv("LSMB_SLICE_LOG2", "20")
    n, k, nb = 2_000_000, 7, NB3E8
    _plan(nb, n, k, "partition", 3)
    keys = _to_dev(_keys("K2"))
    ref = _ref(oracle, "K2", nb, k)
    w = _preset(lsmbloom.num_words(nb))
    ctx.build_fixed_dev(keys, 16, n, nb, k, w)
    _check(w, ref, preset=True)
    w = _garbage(lsmbloom.num_words(nb), 20)
    ctx.build_fixed_dev_new(keys, 16, n, nb, k, w)
    _check(w, ref)


# ---------------------------------------------------------------- 5. generic-k classes
@pytest.mark.parametrize("nb,k,n,strategy,sweeps", [
    (3_000_000_000, 5, 2_000_000, "partition", 3),   # k_bin<Fixed16, Walk64, 8, false, false>
    (NB25E7, 10, 2_000_000, "partition", 4),         # k_bin<Fixed16, Walk64, 16, false, false>; new(2.5e8, .001)
    (3_000_000_000, 16, 1_000_000, "partition", 3),  # k_bin<Fixed16, Walk64, 16, false, false>
    (3_000_000_000, 32, 600_000, "partition", 4),    # k_bin<Fixed16, Walk64, 32, false, false>
    (3_000_000_000, 33, 600_000, "atomic", 1),       # k > 32: k_build_atomic's Walk64 (PosWalk)
])
def test_generic_k_classes(ctx, oracle, nb, k, n, strategy, sweeps):
    """k != 7 at 3e9 bits (and new(2.5e8, .001), k = 10): the size classes of
    pick_k_bin with the 64-bit walk, accumulate onto a preset and fresh (the
    memset-then-accumulate path of k != 7)."""
    _plan(nb, n, k, strategy, sweeps)
    keys_h = keygen.key16(0x51D00001 + (k << 24), 0, n)
    keys = _to_dev(keys_h)
    ref = oracle.build_fixed_mt(keys_h, 16, nb, k, 16)
    w = _preset(lsmbloom.num_words(nb))
    ctx.build_fixed_dev(keys, 16, n, nb, k, w)
    _check(w, ref, preset=True)
    w = _garbage(lsmbloom.num_words(nb), k)
    ctx.build_fixed_dev_new(keys, 16, n, nb, k, w)
    _check(w, ref)


# ---------------------------------------------------------------- 6. the record path
@pytest.mark.parametrize("nb", [NB3E8, 2**32 - 2])
def test_records_varlen(ctx, oracle, nb):
    """1.5 M var-len keys: k_hash_var writes walk records through the third
    branch of WalkRec::make (md.reduce, 2^31 < d < 2^32 - 1), replayed by
    k_bin<Recs, RecWalk64, 7, true, false, 2, 21> (accumulate) and the LIST
    form <..., 1, 21, true> (fresh)."""
    n, k = NV, 7
    _plan(nb, n, k, "partition", 2)
    data, offs = _varlen_members()
    d_data, d_offs = _to_dev(data), _to_dev(offs.view(np.int64))
    ref = _ref(oracle, "V", nb, k)
    w = _preset(lsmbloom.num_words(nb))
    ctx.build_var_dev(d_data, d_offs, n, nb, k, w)
    _check(w, ref, preset=True)
    w = _garbage(lsmbloom.num_words(nb), 61)
    ctx.build_var_dev_new(d_data, d_offs, n, nb, k, w)
    _check(w, ref)


@pytest.mark.parametrize("nb", [NB3E8, 2**32 - 2])
def test_records_24_byte_keys_fresh(ctx, oracle, nb):
    """24-B fixed keys (k_hash's records), fresh: k_bin<Recs, RecWalk64, 7, true, false, 1, 21, true>."""
    n, k, kl = 1_500_000, 7, 24
    _plan(nb, n, k, "partition", 2)
    raw = keygen.stream_bytes(0x24, n * kl)
    w = _garbage(lsmbloom.num_words(nb), 24)
    ctx.build_fixed_dev_new(_to_dev(raw), kl, n, nb, k, w)
    _check(w, oracle.build_fixed_mt(raw, kl, nb, k, 16))


@pytest.mark.parametrize("nb", [NB3E8, 2**32 - 2])
def test_records_unaligned_16_byte_keys(ctx, oracle, nb):
    """16-B keys on a base pointer offset by 3 bytes are not pass A's Fixed16:
    they are hashed into records first; k_bin<Recs, RecWalk64, 7, true, false, 2, 21>."""
    import torch
    n, k = 2_000_000, 7
    _plan(nb, n, k, "partition", 2)
    raw = torch.zeros(n * 16 + 16, dtype=torch.uint8, device=_dev())
    raw[3:3 + n * 16] = _to_dev(_keys("K2")).reshape(-1)
    assert raw[3:].data_ptr() % 16 == 3
    w = _preset(lsmbloom.num_words(nb))
    ctx.build_fixed_dev(raw[3:], 16, n, nb, k, w)
    _check(w, _ref(oracle, "K2", nb, k), preset=True)


def test_records_k32_carries(ctx, oracle):
    """k = 32 fills all 31 carry bits of a record: 600 k 20-B keys at 3e9 bits,
    k_bin<Recs, RecWalk64, 32, false, false>, accumulate and fresh."""
    n, k, kl, nb = 600_000, 32, 20, 3_000_000_000
    _plan(nb, n, k, "partition", 4)
    raw = keygen.stream_bytes(0x20, n * kl)
    keys = _to_dev(raw)
    ref = oracle.build_fixed_mt(raw, kl, nb, k, 16)
    w = _preset(lsmbloom.num_words(nb))
    ctx.build_fixed_dev(keys, kl, n, nb, k, w)
    _check(w, ref, preset=True)
    w = _garbage(lsmbloom.num_words(nb), 32)
    ctx.build_fixed_dev_new(keys, kl, n, nb, k, w)
    _check(w, ref)


# ---------------------------------------------------------------- 7. overflow levels
@pytest.mark.parametrize("nb", [2**32 - 2, 2**31 + 1])
def test_overflow_levels(ctx, oracle, nb):
    """4 M key16 of which the first million are one key: that key's 7 bins get
    ~27 k positions per pass A workgroup (1 M x 7 / 256) against kOvfListCap =
    16 384, so ring, region, overflow list and the ovf / dirty side buffer all
    engage, with 2^20-bit overflow units up to index 4095.  A fresh build on
    garbage, an accumulate build onto a preset (= ref | preset), then a clean
    fresh build on the same context: no stale overflow bits remain.

    That the tiers engage is argued here from kOvfListCap and the plans, not
    checked: tests/test_partition_stage.py::test_pass_a_overflow_tiers derives
    the claim from the plan, fails if it no longer holds, and counts the
    entries of every tier after pass A."""
    n, k = 4_000_000, 7
    _plan(nb, n, k, "partition", 2)
    keys_h = _keys("K8")[:n].copy()
    keys_h[:1_000_000] = keys_h[0]
    keys = _to_dev(keys_h)
    ref = oracle.build_fixed_mt(keys_h, 16, nb, k, 16)
    nw = lsmbloom.num_words(nb)
    w = _garbage(nw, 71)
    ctx.build_fixed_dev_new(keys, 16, n, nb, k, w)
    _check(w, ref)
    w = _preset(nw)
    ctx.build_fixed_dev(keys, 16, n, nb, k, w)
    _check(w, ref, preset=True)
    del ref
    w = _garbage(nw, 72)
    ctx.build_fixed_dev_new(_to_dev(_keys("K2")), 16, 2_000_000, nb, k, w)
    _check(w, _ref(oracle, "K2", nb, k))


# ---------------------------------------------------------------- 8. sweep entry points
def test_sweep_entry_points_at_2_31_plus_1(ctx, oracle):
    """2^31 + 1 bits: sweeps of 513 and 512 2^21-bit bins, the last bin one bit
    wide.  Sweep 0 writes exactly its word range, sweep 1 completes the filter."""
    import torch
    n, k, nb = 2_000_000, 7, 2**31 + 1
    _plan(nb, n, k, "partition", 2)
    keys = _to_dev(_keys("K2"))
    ref = _ref(oracle, "K2", nb, k)
    w = _garbage(lsmbloom.num_words(nb), 81)
    before = w.clone()
    lo, hi = lsmbloom.sweep_words(nb, n, 0, k)
    assert (lo, hi) == (0, 513 * 2**15)
    assert lsmbloom.sweep_words(nb, n, 1, k) == (hi, 2**25 + 1)
    ctx.build_fixed_dev_sweep_new(keys, 16, n, nb, k, w, 0)
    _check(w, ref, lo=lo, hi=hi)
    assert torch.equal(w[hi:], before[hi:])  # the other sweep's words untouched
    ctx.build_fixed_dev_sweep_new(keys, 16, n, nb, k, w, 1)
    _check(w, ref)


# ---------------------------------------------------------------- 9. few keys
def test_few_keys_atomic(ctx, oracle):
    """1000 keys into new(3e8, .01): k_build_atomic's Walk64, accumulate and fresh."""
    n, k, nb = 1000, 7, NB3E8
    _plan(nb, n, k, "atomic", 1)
    keys_h = keygen.key16(0xE1D00001, 0, n)
    keys = _to_dev(keys_h)
    ref = oracle.build_fixed_mt(keys_h, 16, nb, k, 16)
    w = _preset(lsmbloom.num_words(nb))
    ctx.build_fixed_dev(keys, 16, n, nb, k, w)
    _check(w, ref, preset=True)
    w = _garbage(lsmbloom.num_words(nb), 9)
    ctx.build_fixed_dev_new(keys, 16, n, nb, k, w)
    _check(w, ref)


# ---------------------------------------------------------------- 10. probes
def _probe_queries(h):
    """h members then h keys the filters never saw: (16-B keys, var-len data, offsets)."""
    q16 = np.concatenate([_keys("K8")[:h], keygen.key16(0xF1D00001, 0, h)])
    data, offs = _keys("V")
    lens = np.concatenate([offs[1:h + 1] - offs[:h], offs[NV + 1:NV + h + 1] - offs[NV:NV + h]])
    qoffs = np.zeros(2 * h + 1, np.uint64)
    qoffs[1:] = np.cumsum(lens)
    qdata = np.concatenate([data[:int(offs[h])], data[int(offs[NV]):int(offs[NV + h])]])
    assert qdata.size == int(qoffs[-1])
    return q16, qdata, qoffs


@pytest.mark.parametrize("nb", [NB3E8, 2**32 - 2])
def test_probes_over_wide_filters(ctx, oracle, nb):
    """Probes of the filters built above (8 M key16; 1.5 M var-len keys), 1 and
    3 filters, 50 k members + 50 k fresh keys, 16-B and var-len queries: every
    answer equals the oracle's and every member hits its filter."""
    import torch
    k, h = 7, 50_000
    ref16, refv = _ref(oracle, "K8", nb, k), _ref(oracle, "V", nb, k)
    d16, dv = _to_dev(ref16.view(np.int64)), _to_dev(refv.view(np.int64))
    q16, qdata, qoffs = _probe_queries(h)
    for host_f, dev_f, member_bits16, member_bitsv in (
            ([(ref16, nb, k)], [(d16, nb, k)], 1, None),
            ([(refv, nb, k)], [(dv, nb, k)], None, 1),
            ([(ref16, nb, k), (refv, nb, k), (ref16, nb, k)], [(d16, nb, k), (dv, nb, k), (d16, nb, k)], 5, 2)):
        out = torch.zeros((2 * h, 1), dtype=torch.uint8, device=_dev())
        ctx.probe_dev(dev_f, _to_dev(q16), 2 * h, out, key_len=16)
        got = _host_u8(out)
        assert np.array_equal(got, oracle.probe(host_f, q16, key_len=16))
        if member_bits16:
            assert (got[:h, 0] & member_bits16 == member_bits16).all()
        out = torch.zeros((2 * h, 1), dtype=torch.uint8, device=_dev())
        ctx.probe_dev(dev_f, _to_dev(qdata), 2 * h, out, offsets=_to_dev(qoffs.view(np.int64)))
        got = _host_u8(out)
        assert np.array_equal(got, oracle.probe(host_f, qdata, offsets=qoffs))
        if member_bitsv:
            assert (got[:h, 0] & member_bitsv == member_bitsv).all()
        assert not got[h:, 0].all()  # fresh keys are (mostly) rejected: the answers are not all-ones


def _host_u8(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---------------------------------------------------------------- 11. filter set
def test_filter_set_with_a_wide_filter(ctx, oracle):
    """One set holding the new(3e8, .01) filter (add_words) next to an
    SST-sized new(1000, .01) one, each with a key range: mask rows = the
    oracle's bloom answer AND the range check (tests/test_fset.py's
    computation), and probe_lists is their transpose."""
    k = 7
    fs = FilterSet(ctx)
    big = _keys("K8")
    small = keygen.key16(0x11D00001, 0, 1000)
    nbs, ks = lsmbloom.params(1000, 0.01)
    tables = {}
    for words, nb, kk, rows in ((_ref(oracle, "K8", NB3E8, k), NB3E8, k, sorted(bytes(r) for r in big[:4000])),
                                (oracle.build_fixed(small, 16, nbs, ks), nbs, ks, sorted(bytes(r) for r in small))):
        lo, hi = rows[len(rows) // 8], rows[-1 - len(rows) // 8]
        s = fs.add_filter(BloomFilter(words, kk, nb), lo, hi)
        tables[s] = (words, nb, kk, lo, hi)
    q = np.concatenate([big[:2000], big[4_000_000:4_001_000], small, keygen.key16(0x21D00001, 0, 5000)])
    q = np.ascontiguousarray(q[np.random.default_rng(11).permutation(q.shape[0])])
    exp = np.array(expected_masks(oracle, tables, [bytes(r) for r in q]), dtype=np.uint64)
    assert (exp & np.uint64(1)).sum() >= 1000 and (exp & np.uint64(2)).sum() >= 500
    got = fs.probe(q, key_len=16)
    assert np.array_equal(got, exp)
    check_lists(fs.probe_lists(q, key_len=16), exp, "oracle")
    fs.close()
