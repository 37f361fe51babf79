"""The host side of a repacking derive (lsmb_lset_derive_packed), without a
GPU: the planner and the copy items of csrc/lset_repack.hpp under ASan and
UBSan, and the new entry points' argument checks."""
import ctypes
import os
import subprocess

import numpy as np

import lsmbloom
from lsmbloom import LevelSet
from lset_support import cpp_bin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = ctypes.c_void_p


def test_repack_plan_and_items_host(tmp_path):
    """lset_repack_plan against a per-chunk recount (thresholds 0, 1, 500 000,
    1 000 000 and ALL, a chunk exactly at the threshold, an over-sized filter
    in a chunk of its own, every survivor dropped, products past 2^64, random
    chains of edits through lset_place), lset_repack_items tiling every moved
    slot exactly once in items of at most kRepackItemBytes with 16-byte
    pointers and lengths, copy_segs_ref reproducing the bytes
    (tests/cpp/lset_repack_test.cpp)."""
    exe = str(tmp_path / "lset_repack_test")
    src = os.path.join(ROOT, "tests", "cpp", "lset_repack_test.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout




def test_cpp_mirror_repack_argument_checks():
    r = subprocess.run([cpp_bin("lset_repack_mirror_test")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


def test_repack_entry_points_are_exported_and_reject_null():
    L = lsmbloom.lib()
    for name in ("lsmb_lset_derive_packed", "lsmb_copy_segs_dev"):
        assert hasattr(L, name) and name in lsmbloom.SIGNATURES
    assert callable(lsmbloom.Context.copy_segs_dev)
    assert LevelSet.derive.__code__.co_varnames[:4] == ("self", "drop_ids", "repack", "stream")
    assert lsmbloom.LSMB_LSET_REPACK_ALL == 1000001
    hdr = open(os.path.join(ROOT, "include", "lsmbloom.h")).read()
    assert "#define LSMB_LSET_REPACK_ALL 1000001u" in hdr
    h = vp(123)
    ids = np.array([1, 2], np.uint32)
    nd = np.full(1, 7, np.uint64)
    mv = np.full(2, 9, np.uint64)
    pi, pn, pm = ids.ctypes.data_as(lsmbloom.u32p), nd.ctypes.data_as(lsmbloom.u64p), mv.ctypes.data_as(lsmbloom.u64p)
    ALL = lsmbloom.LSMB_LSET_REPACK_ALL
    assert L.lsmb_lset_derive_packed(None, pi, 2, ALL, pn, pm, ctypes.byref(h), None) == lsmbloom.LSMB_EINVAL
    assert h.value is None and nd[0] == 7 and (mv == 9).all()  # *out is cleared, the counts untouched
    h = vp(123)
    assert L.lsmb_lset_derive_packed(None, None, 0, 0, None, None, ctypes.byref(h), None) == lsmbloom.LSMB_EINVAL
    assert h.value is None
    assert L.lsmb_lset_derive_packed(None, None, 0, ALL + 1, None, None, None, None) == lsmbloom.LSMB_EINVAL
    assert L.lsmb_copy_segs_dev(None, vp(16), 1, None) == lsmbloom.LSMB_EINVAL
    assert L.lsmb_copy_segs_dev(None, None, 0, None) == lsmbloom.LSMB_EINVAL
    assert "null" in lsmbloom.lib().lsmb_last_error().decode()
    assert L.lsmb_abi_version() == 6
