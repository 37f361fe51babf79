"""Pass A and pass B of the partitioned build, stage by stage
(tests/hip/partition_stage_test.hip, built as storage-engine_amd/build/partition_stage_test).

The whole-build parity tests compare filter words with the oracle: at their
~52 % fill a position pass A drops is hidden half the time by another key's
bit, nothing shows that the overflow tiers engage, and the edges of the
pass A -> pass B contract cannot be reached through hashing.
The program runs k_bin on buffers of its own and compares, per slice and as
multisets, every region, list and overflow bit with the positions the keys must
produce (hashes from the oracle, positions by literal arithmetic); it feeds
k_apply / k_ovf_apply synthetic regions at the contract's edges; and it checks
hash_records' walk records field by field.

The CPU test runs the checker's self-test: a host binning of the expected
positions is accepted, and each of nine single mutations of it is rejected.
Each gpu test runs one case group in a process of its own.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "storage-engine_amd", "build", "partition_stage_test")

TIER_FIELDS = ("region_entries", "pad_entries", "list_entries", "side_positions", "regions_at_cap", "full_lists")


def _bin():
    if not os.path.exists(BIN):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "storage-engine_amd"), "build/partition_stage_test"],
                       check=True)
    return BIN


def _run(args, group, cases):
    """Runs the program; returns (the names of its good cases, its tier lines by case name)."""
    r = subprocess.run([_bin()] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-3000:]
    m = re.search(r"^partition_stage_test \(([\w-]+)\): (\d+) cases, (\d+) bad$", r.stdout, flags=re.M)
    assert m, r.stdout[-2000:]
    assert m.group(1) == group
    assert int(m.group(3)) == 0
    good = re.findall(r"^case %s/(\S+): ok$" % re.escape(group), r.stdout, flags=re.M)
    assert int(m.group(2)) == len(good)
    assert set(good) == set(cases), sorted(set(good) ^ set(cases))
    assert len(good) == len(cases)
    tiers = {}
    for name, rest in re.findall(r"^tiers (\S+) sweep \d+: (.*)$", r.stdout, flags=re.M):
        t = dict((k, int(v)) for k, v in re.findall(r"(\w+)=(\d+)", rest))
        assert set(t) == set(TIER_FIELDS), rest
        tiers.setdefault(name, []).append(t)
    return good, tiers


FORMS = ("accumulate", "fresh")

SELFTEST_MUTATIONS = [
    "drop-entry-replaced-by-neighbour", "spurious-offset", "count-one-too-high-over-garbage", "count-one-too-low",
    "entry-under-wrong-slice", "pad-not-a-copy-of-entry-0", "list-entry-outside-sweep", "extra-ovf-bit",
    "missing-dirty-mark"]


def test_checker_selftest():
    """Host only: the checker accepts a plain host binning of the expected
    positions and rejects every listed mutation of it."""
    extra = ["accept-plan-accumulate", "accept-plan-fresh", "accept-tight-fresh", "accept-tight-fresh-sweep1",
             "accept-tight-accumulate", "tight-reaches-every-tier", "drop-entry-replaced-by-neighbour-open-segment",
             "fresh-words-touched", "guard-written"]
    _, tiers = _run(["--selftest"], "selftest", SELFTEST_MUTATIONS + extra)
    # the mutated output holds every tier, so each mutation had something to hide behind
    (t,) = tiers["selftest-tight-fresh"]
    assert t["list_entries"] and t["full_lists"] and t["side_positions"] and t["regions_at_cap"]


@pytest.mark.gpu
def test_pass_a_c2_kernel_tightest_ring_and_key_counts():
    cases = ["%s-%s" % (c, f) for f in FORMS
             for c in ["c2-kernel", "tightest-ring"] + ["keys-%d" % n for n in (1, 1023, 1024, 1025, 32768, 32769)]]
    _, tiers = _run(["--group", "passa-c2"], "passa-c2", cases)
    assert set(tiers) == set(cases)
    # 200 001 keys x 7 positions: nearly all in regions, none counted twice (an
    # overflow bit may stand for several equal positions)
    for f in FORMS:
        (t,) = tiers["c2-kernel-" + f]
        assert t["region_entries"] + t["list_entries"] + t["side_positions"] <= 200_001 * 7
        assert t["region_entries"] > 0.99 * 200_001 * 7


@pytest.mark.gpu
def test_pass_a_generic_k():
    cases = ["k-%d" % k for k in (1, 8, 9, 16, 17, 32)]
    _, tiers = _run(["--group", "passa-k"], "passa-k", cases)
    assert len(tiers["k-32"]) == 2  # two sweeps of 51 bins
    assert all(len(tiers[c]) == 1 for c in cases if c != "k-32")


@pytest.mark.gpu
def test_pass_a_wide_filters():
    cases = ["%s-%s" % (c, f) for f in FORMS for c in ("bins21-one-sweep", "2^31+1", "2^32-1", "2^32-2")]
    _, tiers = _run(["--group", "passa-wide"], "passa-wide", cases)
    for c in cases:
        assert len(tiers[c]) == (1 if c.startswith("bins21") else 2), c


@pytest.mark.gpu
def test_records_and_record_walks():
    cases = ["%s-%s-k%d" % (kind, bits, k) for kind in ("var", "fixed24", "unaligned16") for bits in ("c2", "2^31+1")
             for k in (7, 32)] + ["var-c2-k7-fresh"]
    _run(["--group", "records"], "records", cases)


@pytest.mark.gpu
def test_pass_a_overflow_tiers():
    """The first workgroup's keys are one key: the program derives from the plan
    that region, ring and list must all overflow, then requires entries in
    every tier."""
    cases = ["tiers20-fresh", "tiers20-accumulate", "tiers21-fresh"]
    _, tiers = _run(["--group", "tiers"], "tiers", cases)
    for c in cases:
        (t,) = tiers[c]
        assert t["region_entries"] > 0 and t["side_positions"] > 0 and t["regions_at_cap"] > 0, (c, t)
        if c.endswith("fresh"):
            assert t["list_entries"] > 0 and t["full_lists"] > 0, (c, t)


@pytest.mark.gpu
def test_pass_b_synthetic_regions():
    cases = []
    for sl in (20, 21):
        cases += ["sl%d-grid%d-accumulate" % (sl, g) for g in (1, 15, 16, 17, 512, 1024)]
        cases += ["sl%d-grid%d-fresh" % (sl, g) for g in (1, 17)]
        cases += ["sl%d-%s-%s" % (sl, c, f) for c in ("zero-counts", "subrange") for f in FORMS]
        cases += ["sl%d-dirty" % sl, "sl%d-lists" % sl]
    _run(["--group", "passb"], "passb", cases)
