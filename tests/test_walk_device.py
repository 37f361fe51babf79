"""The device compile of csrc/bloom_math.hpp at its arithmetic edges
(tests/hip/walk_device_test.hip, built as storage-engine_amd/build/walk_device_test).

bloom_math.hpp has three branches that exist only in the device compile (the
v_cvt_f64_u32 of f64_of_u64, __umul24 in Mod14, the add-with-carry chain that
builds WalkRec::c).  tests/cpp/reduce_test.cpp and walkrec_test.cpp run the
host compile; on the GPU the product's kernels feed those branches hashes of
random keys, which never land on x = q*d + (d-1), r + s == d, s0 + dt == d or
a 31-carry chain.  The program runs ~1.45 M such cases through one kernel and
compares every value with a literal % on uint64_t / unsigned __int128.

The CPU test runs the identical case list through the host compile (--host):
it validates the generator and the reference, and that the list still holds
every edge it is built for.  The gpu test runs the kernel in a process that
loads only the HIP runtime.
"""
import os
import re
import subprocess

import pytest

import lsmbloom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "storage-engine_amd", "build", "walk_device_test")
SRC = os.path.join(ROOT, "tests", "hip", "walk_device_test.hip")


def _bin():
    if not os.path.exists(BIN):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "storage-engine_amd"), "build/walk_device_test"],
                       check=True)
    return BIN


def _check_report(out, mode):
    m = re.search(r"walk_device_test \((\w+)\): (\d+) cases, (\d+) values, (\d+) bad", out)
    assert m, out[-2000:]
    assert m.group(1) == mode
    assert 1_000_000 <= int(m.group(2)) <= 2_100_000  # about 2 M at the most: well under a second of GPU time
    assert int(m.group(4)) == 0
    kinds = dict((k, int(n)) for k, n in re.findall(r"^(\w+)\s+(\d+) cases, 0 bad$", out, flags=re.M))
    assert set(kinds) == {"reduce", "reduce31", "mod14", "walk32", "walk14", "walk64", "walkM", "rec32", "rec64"}
    assert all(n > 1000 for n in kinds.values()), kinds
    assert kinds["mod14"] >= 40 * (2**14 - 1)  # every d < 2^14, the whole x grid each


def test_walk_edges_host_compile():
    r = subprocess.run([_bin(), "--host"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    _check_report(r.stdout, "host")
    # the list holds every edge it is built for (counted by literal arithmetic)
    edges = re.search(r"^edges: (.*)$", r.stdout, flags=re.M)
    assert edges, r.stdout[-2000:]
    counts = dict((k, int(v)) for k, v in re.findall(r"(\w+)=(\d+)", edges.group(1)))
    assert set(counts) == {"below_multiple", "s0_dt_is_d", "r_s_is_d", "carries_all", "carries_none"}
    assert all(v >= 100 for v in counts.values()), counts


def test_walk_edges_cover_the_wide_build_moduli():
    """The program's modulus list names new(3e8, .01) as a literal: it is the
    size tests/test_gpu_wide_moduli.py builds."""
    nb = lsmbloom.params(300_000_000, 0.01)[0]
    src = open(SRC).read()
    assert "%du" % nb in src
    for lit in ("0x80000000u", "0x80000001u", "3000000000u", "0xFFFFFFFEu", "0xFFFFFFFFu"):
        assert lit in src


@pytest.mark.gpu
def test_walk_edges_device_compile():
    r = subprocess.run([_bin()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    _check_report(r.stdout, "device")
