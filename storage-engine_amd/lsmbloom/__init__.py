"""lsmbloom — Python binding of the MI355X Bloom engine's C ABI (include/lsmbloom.h).

Mirrors the reference's Rust surface `crate::bloom` (G1DO/Storage-Engine
src/bloom/mod.rs, src/bloom/builder.rs) so tests read like the reference's own:

    bf = BloomFilter.new(100, 0.01)      # BloomFilter::new            mod.rs:38-67
    bf.insert(b"hello")                  # BloomFilter::insert         mod.rs:70-78
    bf.may_contain(b"hello")             # BloomFilter::may_contain    mod.rs:82-94
    bf.serialize() / BloomFilter.deserialize(b)                      # mod.rs:102-168
    b = BloomFilterBuilder.new(n, fpr); b.add_key(k); bf = b.build()  # builder.rs:14-28

Batched work (BloomFilterBuilder.build, probe_batch) runs on the GPU through
the C ABI; it raises if the HIP library or a gfx950 device is missing — there
is no CPU fallback.  The one host path is the library's own, size-bounded:
builds of at most host_max_keys() keys (an SST flush at the reference's
default 1 000-key sizing) run its native per-key loop and need no GPU.
Device-resident entry points take torch tensors.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LSMB_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "liblsmbloom.so")  # LSMB_LIB: instrumented builds (tools/)

LSMB_OK = 0
LSMB_EINVAL = -1
LSMB_ENODEV = -2
LSMB_EHIP = -3
LSMB_ECORRUPT = -4
LSMB_ENOMEM = -5
LSMB_LSET_MAX_LEVELS = 8
LSMB_LSET_NONE = 0xFFFFFFFF  # LevelSet.probe: no table of this row
LSMB_SST_BAD_BLOCK = 0xFFFFFFFF  # build_batch_sst_dev: a malformed data block's blk_entries
LSMB_LSET_REPACK_ALL = 1000001  # LevelSet.derive(repack="all"): every surviving table moves
LSMB_LSET_ROW_L0 = 0x80000000  # `row` of any LevelSet add: the table goes to the set's L0 part
LSMB_LSET_L0_MAX = 64

u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)
vp = ctypes.c_void_p

# name -> (restype, argtypes); the exact export list of include/lsmbloom.h
SIGNATURES = {
    "lsmb_abi_version": (ctypes.c_int, []),
    "lsmb_last_error": (ctypes.c_char_p, []),
    "lsmb_params": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_double, u32p, u32p]),
    "lsmb_fill_fpr": (ctypes.c_double, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]),
    "lsmb_fill_keys": (ctypes.c_double, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]),
    "lsmb_num_words": (ctypes.c_uint64, [ctypes.c_uint32]),
    "lsmb_serialized_size": (ctypes.c_uint64, [ctypes.c_uint32]),
    "lsmb_serialize": (ctypes.c_int, [u64p, ctypes.c_uint32, ctypes.c_uint32, u8p, ctypes.c_uint64]),
    "lsmb_deserialize_header": (ctypes.c_int, [u8p, ctypes.c_uint64, u32p, u32p, u32p]),
    "lsmb_deserialize": (ctypes.c_int, [u8p, ctypes.c_uint64, u64p, ctypes.c_uint64]),
    "lsmb_insert": (ctypes.c_int, [u64p, ctypes.c_uint32, ctypes.c_uint32, u8p, ctypes.c_uint64]),
    "lsmb_may_contain": (ctypes.c_int, [u64p, ctypes.c_uint32, ctypes.c_uint32, u8p, ctypes.c_uint64]),
    "lsmb_positions": (ctypes.c_int, [u8p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, u32p]),
    "lsmb_open": (ctypes.c_int, [ctypes.POINTER(vp), ctypes.c_int]),
    "lsmb_close": (None, [vp]),
    "lsmb_sync": (ctypes.c_int, [vp]),
    "lsmb_build_fixed": (ctypes.c_int, [vp, u8p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32,
                                        ctypes.c_uint32, u64p]),
    "lsmb_build_var": (ctypes.c_int, [vp, u8p, u64p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, u64p]),
    "lsmb_build_block": (ctypes.c_int, [vp, u8p, u64p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32,
                                        ctypes.c_uint32, u8p, ctypes.c_uint64]),
    "lsmb_build_block_crc": (ctypes.c_int, [vp, u8p, u64p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32,
                                            ctypes.c_uint32, u8p, ctypes.c_uint64, u32p]),
    "lsmb_crc32": (ctypes.c_uint32, [ctypes.c_uint32, u8p, ctypes.c_uint64]),
    "lsmb_crc32_combine": (ctypes.c_uint32, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]),
    "lsmb_crc32_dev": (ctypes.c_int, [vp, ctypes.c_uint32, vp, ctypes.c_uint64, u32p, vp]),
    "lsmb_crc32_seg_dev": (ctypes.c_int, [vp, vp, ctypes.c_uint64, vp, vp]),
    "lsmb_copy_segs_dev": (ctypes.c_int, [vp, vp, ctypes.c_uint64, vp]),
    "lsmb_popcount_segs_dev": (ctypes.c_int, [vp, vp, ctypes.c_uint64, vp, vp]),
    "lsmb_fset_add_crc": (ctypes.c_int, [vp, u8p, ctypes.c_uint64, ctypes.c_uint32, u8p, ctypes.c_uint64, u8p,
                                         ctypes.c_uint64]),
    "lsmb_probe": (ctypes.c_int, [vp, ctypes.POINTER(u64p), u32p, u32p, ctypes.c_uint32, u8p, u64p,
                                  ctypes.c_uint32, ctypes.c_uint64, u8p]),
    "lsmb_build_fixed_dev": (ctypes.c_int, [vp, vp, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32,
                                            ctypes.c_uint32, vp, vp]),
    "lsmb_build_var_dev": (ctypes.c_int, [vp, vp, vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                          vp, vp]),
    "lsmb_build_fixed_dev_new": (ctypes.c_int, [vp, vp, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32,
                                                ctypes.c_uint32, vp, vp]),
    "lsmb_build_var_dev_new": (ctypes.c_int, [vp, vp, vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                              vp, vp]),
    "lsmb_probe_dev": (ctypes.c_int, [vp, ctypes.POINTER(vp), u32p, u32p, ctypes.c_uint32, vp, vp,
                                      ctypes.c_uint32, ctypes.c_uint64, vp, vp]),
    "lsmb_or_reduce_dev": (ctypes.c_int, [vp, vp, vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64, vp]),
    "lsmb_gen_key16_dev": (ctypes.c_int, [vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, vp, vp]),
    "lsmb_gen_splitmix_dev": (ctypes.c_int, [vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                                             ctypes.c_uint32, vp, vp]),
    "lsmb_fset_open": (ctypes.c_int, [vp, ctypes.POINTER(vp)]),
    "lsmb_fset_close": (None, [vp]),
    "lsmb_fset_add": (ctypes.c_int, [vp, u8p, ctypes.c_uint64, u8p, ctypes.c_uint64, u8p, ctypes.c_uint64]),
    "lsmb_fset_add_words": (ctypes.c_int, [vp, u64p, ctypes.c_uint32, ctypes.c_uint32, u8p, ctypes.c_uint64, u8p,
                                           ctypes.c_uint64]),
    "lsmb_fset_remove": (ctypes.c_int, [vp, ctypes.c_int]),
    "lsmb_fset_live_mask": (ctypes.c_uint64, [vp]),
    "lsmb_fset_probe": (ctypes.c_int, [vp, u8p, u64p, ctypes.c_uint32, ctypes.c_uint64, u64p]),
    "lsmb_fset_probe_dev": (ctypes.c_int, [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint64, vp, vp]),
    "lsmb_fset_probe_dev_rows": (ctypes.c_int, [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint64, vp, ctypes.c_uint32, vp]),
    "lsmb_fset_probe_lists_dev": (ctypes.c_int, [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint64, vp, vp, ctypes.c_uint64,
                                                 vp]),
    "lsmb_fset_probe_lists": (ctypes.c_int, [vp, u8p, u64p, ctypes.c_uint32, ctypes.c_uint64, u64p, u32p,
                                             ctypes.c_uint64]),
    "lsmb_lset_open": (ctypes.c_int, [vp, ctypes.POINTER(vp)]),
    "lsmb_lset_close": (None, [vp]),
    "lsmb_lset_add": (ctypes.c_int, [vp, ctypes.c_uint32, ctypes.c_uint32, u8p, ctypes.c_uint64, u8p, ctypes.c_uint64,
                                     u8p, ctypes.c_uint64]),
    "lsmb_lset_add_words": (ctypes.c_int, [vp, ctypes.c_uint32, ctypes.c_uint32, u64p, ctypes.c_uint32, ctypes.c_uint32,
                                           u8p, ctypes.c_uint64, u8p, ctypes.c_uint64]),
    "lsmb_lset_seal": (ctypes.c_int, [vp]),
    "lsmb_lset_derive": (ctypes.c_int, [vp, u32p, ctypes.c_uint64, u64p, ctypes.POINTER(vp)]),
    "lsmb_lset_derive_packed": (ctypes.c_int, [vp, u32p, ctypes.c_uint64, ctypes.c_uint32, u64p, u64p,
                                               ctypes.POINTER(vp), vp]),
    "lsmb_lset_add_batch": (ctypes.c_int, [vp, ctypes.c_uint64, u32p, u32p, u8p, u64p, u32p, u8p, u64p,
                                           ctypes.POINTER(ctypes.c_int32)]),
    "lsmb_lset_add_batch_dev": (ctypes.c_int, [vp, ctypes.c_uint64, u32p, u32p, vp, u64p, u32p, u32p, u8p, u64p, vp]),
    "lsmb_lset_stats": (ctypes.c_int, [vp, u64p]),
    "lsmb_lset_rows": (ctypes.c_int, [vp]),
    "lsmb_lset_tables": (ctypes.c_uint64, [vp, ctypes.c_uint32]),
    "lsmb_lset_probe": (ctypes.c_int, [vp, u8p, u64p, ctypes.c_uint32, ctypes.c_uint64, u32p]),
    "lsmb_lset_probe_dev": (ctypes.c_int, [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint64, vp, vp]),
    "lsmb_lset_total_tables": (ctypes.c_uint64, [vp]),
    "lsmb_lset_table_order": (ctypes.c_int, [vp, u32p, u64p]),
    "lsmb_lset_lists_work_bytes": (ctypes.c_uint64, [vp, ctypes.c_uint64]),
    "lsmb_lset_probe_lists_dev": (ctypes.c_int, [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint64, vp, vp, ctypes.c_uint64,
                                                 vp, ctypes.c_uint64, vp]),
    "lsmb_lset_probe_lists": (ctypes.c_int, [vp, u8p, u64p, ctypes.c_uint32, ctypes.c_uint64, u64p, u32p,
                                             ctypes.c_uint64]),
    "lsmb_lset_l0_tables": (ctypes.c_uint64, [vp]),
    "lsmb_lset_l0_order": (ctypes.c_int, [vp, u32p]),
    "lsmb_lset_probe_version_dev": (ctypes.c_int, [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint64, vp, vp, vp]),
    "lsmb_lset_probe_version": (ctypes.c_int, [vp, u8p, u64p, ctypes.c_uint32, ctypes.c_uint64, u64p, u32p]),
    "lsmb_lset_version_tables": (ctypes.c_uint64, [vp]),
    "lsmb_lset_version_order": (ctypes.c_int, [vp, u32p, u64p]),
    "lsmb_lset_version_geometry": (ctypes.c_int, [vp, u32p, u32p]),
    "lsmb_lset_census": (ctypes.c_int, [vp, u64p, vp]),
    "lsmb_lset_version_lists_work_bytes": (ctypes.c_uint64, [vp, ctypes.c_uint64]),
    "lsmb_lset_probe_version_lists_dev": (ctypes.c_int, [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint64, vp, vp,
                                                         ctypes.c_uint64, vp, ctypes.c_uint64, vp]),
    "lsmb_lset_probe_version_lists": (ctypes.c_int, [vp, u8p, u64p, ctypes.c_uint32, ctypes.c_uint64, u64p, u32p,
                                                     ctypes.c_uint64]),
    "lsmb_lset_walk_steps": (ctypes.c_uint32, [vp]),
    "lsmb_lset_probe_walk_dev": (ctypes.c_int, [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint64, vp, vp, vp, vp]),
    "lsmb_lset_probe_walk": (ctypes.c_int, [vp, u8p, u64p, ctypes.c_uint32, ctypes.c_uint64, u32p, u32p, u32p]),
    "lsmb_lset_walk_lists_work_bytes": (ctypes.c_uint64, [vp, ctypes.c_uint64]),
    "lsmb_lset_probe_walk_lists_dev": (ctypes.c_int, [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint64, vp, vp, vp, vp,
                                                      ctypes.c_uint64, vp, ctypes.c_uint64, vp]),
    "lsmb_lset_probe_walk_lists": (ctypes.c_int, [vp, u8p, u64p, ctypes.c_uint32, ctypes.c_uint64, u32p, u32p, u64p,
                                                  u32p, ctypes.c_uint64]),
    "lsmb_build_strategy": (ctypes.c_char_p, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]),
    "lsmb_host_max_keys": (ctypes.c_uint64, []),
    "lsmb_build_sweeps": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]),
    "lsmb_sweep_words": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, u64p, u64p]),
    "lsmb_build_fixed_dev_sweep": (ctypes.c_int, [vp, vp, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32,
                                                  ctypes.c_uint32, vp, ctypes.c_int, vp]),
    "lsmb_build_fixed_dev_sweep_new": (ctypes.c_int, [vp, vp, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32,
                                                      ctypes.c_uint32, vp, ctypes.c_int, vp]),
    "lsmb_set_host_max_keys": (None, [ctypes.c_uint64]),
    "lsmb_build_batch_max_bits": (ctypes.c_uint32, []),
    "lsmb_build_batch_layout": (ctypes.c_int, [ctypes.c_uint64, u32p, u64p]),
    "lsmb_build_batch_parts": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_uint32]),
    "lsmb_build_batch_dev": (ctypes.c_int, [vp, vp, vp, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, u64p, u32p,
                                            u32p, vp, ctypes.c_uint64, vp]),
    "lsmb_build_batch_blocks": (ctypes.c_int, [vp, u8p, u64p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, u64p,
                                               u32p, u32p, u8p, ctypes.c_uint64, u64p]),
    "lsmb_build_batch_sst_parts": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]),
    "lsmb_build_batch_sst_dev": (ctypes.c_int, [vp, vp, ctypes.c_uint64, ctypes.c_uint64, u64p, u32p, ctypes.c_uint64,
                                                u64p, u32p, u32p, vp, ctypes.c_uint64, vp, vp]),
    "lsmb_build_batch_sst_blocks": (ctypes.c_int, [vp, u8p, ctypes.c_uint64, ctypes.c_uint64, u64p, u32p,
                                                   ctypes.c_uint64, u64p, u32p, u32p, u8p, ctypes.c_uint64, u64p, u64p,
                                                   ctypes.POINTER(ctypes.c_int32)]),
    "lsmb_compact_sst_work_bytes": (ctypes.c_uint64, [ctypes.c_uint64, u32p]),
    "lsmb_compact_sst_mark_dev": (ctypes.c_int, [vp, vp, ctypes.c_uint64, ctypes.c_uint64, u64p, u32p, ctypes.c_uint64,
                                                 u64p, ctypes.c_int, vp, ctypes.c_uint64, vp, vp, vp]),
    "lsmb_compact_sst_gather_dev": (ctypes.c_int, [vp, vp, ctypes.c_uint64, ctypes.c_uint64, u64p, u32p, ctypes.c_uint64,
                                                   u64p, vp, vp, ctypes.c_uint64, vp, ctypes.c_uint64, vp]),
    "lsmb_compact_sst_bloom": (ctypes.c_int, [vp, u8p, ctypes.c_uint64, ctypes.c_uint64, u64p, u32p, ctypes.c_uint64,
                                              u64p, ctypes.c_int, ctypes.c_uint64, ctypes.c_double, u8p, ctypes.c_uint64,
                                              u64p, u64p, u32p, u32p]),
    "lsmb_multi_open": (ctypes.c_int, [ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int), ctypes.c_int]),
    "lsmb_multi_close": (None, [vp]),
    "lsmb_multi_size": (ctypes.c_int, [vp]),
    "lsmb_multi_ctx": (vp, [vp, ctypes.c_int]),
    "lsmb_multi_build_fixed_dev": (ctypes.c_int, [vp, ctypes.POINTER(vp), u64p, ctypes.c_uint32, ctypes.c_uint32,
                                                  ctypes.c_uint32, ctypes.POINTER(vp)]),
    "lsmb_multi_build_block": (ctypes.c_int, [vp, u8p, u64p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32,
                                              ctypes.c_uint32, u8p, ctypes.c_uint64]),
    "lsmb_multi_last_ms": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
    "lsmb_ipc_export": (ctypes.c_int, [vp, u8p, u64p]),
    "lsmb_ipc_import": (ctypes.c_int, [vp, u8p, ctypes.POINTER(vp)]),
    "lsmb_ipc_close": (ctypes.c_int, [vp, vp]),
    "lsmb_or_gather_dev": (ctypes.c_int, [vp, vp, ctypes.POINTER(vp), ctypes.c_uint32, ctypes.c_uint64, vp, vp]),
    "lsmb_copy_slices_dev": (ctypes.c_int, [vp, vp, ctypes.POINTER(vp), ctypes.c_uint32, ctypes.c_uint64,
                                            ctypes.c_uint64, vp, vp]),
    "lsmb_poison_fill_dev": (ctypes.c_int, [vp, vp, ctypes.c_uint64, vp, vp]),
    "lsmb_flag_signal_dev": (ctypes.c_int, [vp, vp, ctypes.c_uint32, vp]),
    "lsmb_flag_wait_dev": (ctypes.c_int, [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.c_uint32, ctypes.c_uint32,
                                          ctypes.c_uint32, vp, vp]),
    "lsmb_merge_status": (ctypes.c_int, [vp, vp, vp, u32p]),
    "lsmb_stream_open": (ctypes.c_int, [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(vp)]),
    "lsmb_stream_reset": (ctypes.c_int, [vp, ctypes.c_uint32, ctypes.c_uint32]),
    "lsmb_stream_close": (None, [vp]),
    "lsmb_stream_add": (ctypes.c_int, [vp, u8p, ctypes.c_uint64]),
    "lsmb_stream_add_batch": (ctypes.c_int, [vp, u8p, u64p, ctypes.c_uint64]),
    "lsmb_stream_count": (ctypes.c_uint64, [vp]),
    "lsmb_stream_finish_block": (ctypes.c_int, [vp, u8p, ctypes.c_uint64]),
    "lsmb_stream_finish_words": (ctypes.c_int, [vp, u64p]),
    "lsmb_last_build_ms": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_float)]),
    "lsmb_set_timing": (ctypes.c_int, [vp, ctypes.c_int]),
}

_lib = None


class LsmbError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("lsmb error %d: %s" % (code, msg))
        self.code = code


class Corruption(LsmbError):
    """Error::Corruption(String) of the reference (src/error.rs:12)."""


def lib():
    """Loads liblsmbloom.so; raises if the HIP library was not built (no fallback)."""
    global _lib
    if _lib is None:
        # Load torch's HIP runtime FIRST when torch is present: liblsmbloom.so
        # needs libamdhip64.so.7, and torch ships its own copy under the same
        # SONAME, so the loader then binds us to torch's runtime.  One runtime
        # per process means torch tensors, torch streams and RCCL share device
        # state with our kernels (loading ours first would start a second
        # runtime and break torch's CUDA init).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise ImportError("liblsmbloom.so not built (%s); run `make -C storage-engine_amd`" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            if os.environ.get("LSMB_LIB") and not hasattr(L, name):
                continue  # an older library for an A/B run (tools/): entry points it predates stay unbound
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc):
    if rc < 0:
        msg = lib().lsmb_last_error().decode(errors="replace")
        if rc == LSMB_ECORRUPT:
            raise Corruption(rc, msg)
        if rc == LSMB_EINVAL:
            raise ValueError(msg)
        raise LsmbError(rc, msg)
    return rc


def _p(a, t):
    return a.ctypes.data_as(t)


def _key(b):
    b = bytes(b)
    a = np.frombuffer(b + b"\0", dtype=np.uint8)
    return a, len(b)


def _host_keys(data, offsets, key_len):
    """Packed host keys -> (data, n, offsets pointer) as the C ABI takes them:
    var-length by offsets (n + 1 u64) or fixed-length by key_len (offsets
    None, a NULL pointer); empty data becomes one zero byte, so that the
    pointer is never NULL."""
    data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n, op = offsets.size - 1, _p(offsets, u64p)
    else:
        n, op = (data.size // key_len if key_len else 0), None
    if data.size == 0:
        data = np.zeros(1, np.uint8)
    return data, n, op


def _pack_keys(keys):
    """list of bytes -> (data uint8, offsets uint64[len(keys) + 1])."""
    lens = np.array([len(k) for k in keys], dtype=np.uint64)
    offs = np.zeros(len(keys) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offs[1:])
    return np.frombuffer(b"".join(bytes(k) for k in keys), dtype=np.uint8), offs


def _pack_ranges(ranges):
    """list of (min_key, max_key) -> (bytes uint8, never empty; offsets
    uint64[2 * len(ranges) + 1]): table t's bounds at offsets[2t .. 2t + 2]."""
    flat = [bytes(k) for lo_hi in ranges for k in lo_hi]
    koff = np.zeros(2 * len(ranges) + 1, dtype=np.uint64)
    np.cumsum([len(k) for k in flat], out=koff[1:])
    return np.frombuffer(b"".join(flat) + b"\0", dtype=np.uint8), koff


def params(expected_items, false_positive_rate):
    """BloomFilter::new sizing -> (num_bits, num_hashes); ValueError where the reference panics."""
    nb, k = ctypes.c_uint32(), ctypes.c_uint32()
    _check(lib().lsmb_params(int(expected_items), float(false_positive_rate), ctypes.byref(nb), ctypes.byref(k)))
    return nb.value, k.value


def fill_fpr(num_bits, num_hashes, set_bits):
    """(set_bits / num_bits) ** num_hashes, the false-positive rate a filter's fill predicts (lsmb_fill_fpr)."""
    return float(lib().lsmb_fill_fpr(int(num_bits), int(num_hashes), int(set_bits)))


def fill_keys(num_bits, num_hashes, set_bits):
    """-(m / k) ln(1 - X / m), the distinct keys a filter of that fill holds (lsmb_fill_keys)."""
    return float(lib().lsmb_fill_keys(int(num_bits), int(num_hashes), int(set_bits)))


def ipc_export(t):
    """(handle bytes, byte offset) of the device allocation holding tensor t's
    storage (lsmb_ipc_export), for another process's Context.ipc_import."""
    h = np.zeros(64, dtype=np.uint8)
    off = ctypes.c_uint64()
    _check(lib().lsmb_ipc_export(vp(t.data_ptr()), _p(h, u8p), ctypes.byref(off)))
    return h.tobytes(), off.value


def num_words(num_bits):
    return int(lib().lsmb_num_words(num_bits))


def serialized_size(num_bits):
    return int(lib().lsmb_serialized_size(num_bits))


def positions(key, num_bits, k):
    a, n = _key(key)
    out = np.zeros(max(k, 1), dtype=np.uint32)
    _check(lib().lsmb_positions(_p(a, u8p), n, num_bits, k, _p(out, u32p)))
    return [int(x) for x in out[:k]]


# ------------------------------------------------------------------ GPU context
class Context:
    """One GPU: stream + scratch arenas (lsmb_ctx).  Raises if no gfx950 device."""

    def __init__(self, device=-1):
        h = vp()
        _check(lib().lsmb_open(ctypes.byref(h), int(device)))
        self.h = h

    def close(self):
        if self.h:
            lib().lsmb_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _check(lib().lsmb_sync(self.h))

    # host-memory entry points -------------------------------------------------
    def build_fixed(self, keys, key_len, num_bits, k, words=None):
        keys = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1)
        n = keys.size // key_len if key_len else 0
        if words is None:
            words = np.zeros(num_words(num_bits), dtype=np.uint64)
        if keys.size == 0:
            keys = np.zeros(1, np.uint8)
        _check(lib().lsmb_build_fixed(self.h, _p(keys, u8p), key_len, n, num_bits, k, _p(words, u64p)))
        return words

    def build_var(self, data, offsets, num_bits, k, words=None):
        data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if words is None:
            words = np.zeros(num_words(num_bits), dtype=np.uint64)
        if data.size == 0:
            data = np.zeros(1, np.uint8)
        _check(lib().lsmb_build_var(self.h, _p(data, u8p), _p(offsets, u64p), offsets.size - 1, num_bits, k,
                                    _p(words, u64p)))
        return words

    def build_block(self, data, num_bits, k, offsets=None, key_len=0, out=None):
        """The serialized bloom block (BloomFilter::serialize of a fresh filter over
        the keys, src/bloom/mod.rs:102-115) in one call: lsmb_build_block.  Keys are
        fixed-length (key_len) or var-length (offsets, n+1 u64).  `out` may be a
        preallocated uint8 array (e.g. the SST write buffer); returns the array."""
        data, n, op = _host_keys(data, offsets, key_len)
        size = serialized_size(num_bits)
        if out is None:
            out = np.empty(size, dtype=np.uint8)
        _check(lib().lsmb_build_block(self.h, _p(data, u8p), op, key_len, n, num_bits, k, _p(out, u8p), out.size))
        return out

    def build_block_crc(self, data, num_bits, k, offsets=None, key_len=0, out=None):
        """build_block + the block's CRC-32 (lsmb_build_block_crc) -> (block, crc)."""
        data, n, op = _host_keys(data, offsets, key_len)
        if out is None:
            out = np.empty(serialized_size(num_bits), dtype=np.uint8)
        crc = ctypes.c_uint32()
        _check(lib().lsmb_build_block_crc(self.h, _p(data, u8p), op, key_len, n, num_bits, k, _p(out, u8p),
                                          out.size, ctypes.byref(crc)))
        return out, crc.value

    def crc32_dev(self, t, nbytes=None, crc=0, stream=None):
        """CRC-32 of a device tensor's bytes (lsmb_crc32_dev), appended to crc."""
        n = t.numel() * t.element_size() if nbytes is None else nbytes
        out = ctypes.c_uint32()
        _check(lib().lsmb_crc32_dev(self.h, crc, vp(t.data_ptr()), n, ctypes.byref(out), self._stream(stream)))
        return out.value

    def crc32_seg_dev(self, segs, nseg, out, stream=None):
        """CRC-32 of nseg device segments in one launch (lsmb_crc32_seg_dev):
        segs an int64 / uint64 device tensor of (pointer, byte length) pairs,
        out an int32 / uint32 device tensor of nseg; asynchronous on stream."""
        _check(lib().lsmb_crc32_seg_dev(self.h, vp(segs.data_ptr()), int(nseg), vp(out.data_ptr()),
                                        self._stream(stream)))

    def copy_segs_dev(self, segs, nseg, stream=None):
        """nseg device-to-device copies in one launch (lsmb_copy_segs_dev):
        segs an int64 / uint64 device tensor of (source pointer, destination
        pointer, byte length) triples, pointers 16-byte aligned, lengths
        multiples of 16, ranges disjoint; asynchronous on stream."""
        _check(lib().lsmb_copy_segs_dev(self.h, vp(segs.data_ptr()), int(nseg), self._stream(stream)))

    def popcount_segs_dev(self, segs, nseg, out, stream=None):
        """The set bits of nseg device segments in one launch
        (lsmb_popcount_segs_dev): segs an int64 / uint64 device tensor of
        (words pointer, bit count) pairs, pointers 16-byte aligned, out an
        int64 / uint64 device tensor of nseg; bits at or above a segment's bit
        count do not count, and nothing past its last word is read;
        asynchronous on stream."""
        _check(lib().lsmb_popcount_segs_dev(self.h, vp(segs.data_ptr()), int(nseg), vp(out.data_ptr()),
                                            self._stream(stream)))

    def probe(self, filters, data, offsets=None, key_len=0):
        """filters: [(words uint64 array, num_bits, k)] -> uint8 [n, ceil(F/8)] mask."""
        F = len(filters)
        ws = [np.ascontiguousarray(f[0], dtype=np.uint64) for f in filters]
        arr = (u64p * F)(*[_p(w, u64p) for w in ws])
        nb = np.array([f[1] for f in filters], dtype=np.uint32)
        kk = np.array([f[2] for f in filters], dtype=np.uint32)
        data, n, op = _host_keys(data, offsets, key_len)
        out = np.zeros((n, (F + 7) // 8), dtype=np.uint8)
        _check(lib().lsmb_probe(self.h, arr, _p(nb, u32p), _p(kk, u32p), F, _p(data, u8p), op, key_len, n,
                                _p(out, u8p)))
        return out

    # device-resident entry points (torch tensors) ------------------------------
    @staticmethod
    def _stream(stream):
        if stream is None:
            import torch
            return vp(torch.cuda.current_stream().cuda_stream)
        return vp(stream)

    def build_fixed_dev(self, keys, key_len, n, num_bits, k, words, stream=None):
        _check(lib().lsmb_build_fixed_dev(self.h, vp(keys.data_ptr()), key_len, n, num_bits, k,
                                          vp(words.data_ptr()), self._stream(stream)))

    def build_fixed_dev_sweep(self, keys, key_len, n, num_bits, k, words, sweep, stream=None):
        """One sweep of a partitioned build (lsmb_build_fixed_dev_sweep)."""
        _check(lib().lsmb_build_fixed_dev_sweep(self.h, vp(keys.data_ptr()), key_len, n, num_bits, k,
                                                vp(words.data_ptr()), int(sweep), self._stream(stream)))

    def build_var_dev(self, data, offsets, n, num_bits, k, words, stream=None):
        _check(lib().lsmb_build_var_dev(self.h, vp(data.data_ptr()), vp(offsets.data_ptr()), n, num_bits, k,
                                        vp(words.data_ptr()), self._stream(stream)))

    # BloomFilterBuilder::{new, add_key, build} (src/bloom/builder.rs:14-28):
    # `words` is output-only, every word of the filter (of the sweep's range)
    # is written; no zeroing pass, no read of the old words.
    def build_fixed_dev_new(self, keys, key_len, n, num_bits, k, words, stream=None):
        _check(lib().lsmb_build_fixed_dev_new(self.h, vp(keys.data_ptr() if n else 0), key_len, n, num_bits, k,
                                              vp(words.data_ptr()), self._stream(stream)))

    def build_fixed_dev_sweep_new(self, keys, key_len, n, num_bits, k, words, sweep, stream=None):
        _check(lib().lsmb_build_fixed_dev_sweep_new(self.h, vp(keys.data_ptr() if n else 0), key_len, n, num_bits,
                                                    k, vp(words.data_ptr()), int(sweep), self._stream(stream)))

    def build_var_dev_new(self, data, offsets, n, num_bits, k, words, stream=None):
        _check(lib().lsmb_build_var_dev_new(self.h, vp(data.data_ptr()), vp(offsets.data_ptr() if n else 0), n,
                                            num_bits, k, vp(words.data_ptr()), self._stream(stream)))

    # Many SSTable filters from one key run (src/sstable/builder.rs:74,93,177-182
    # for every output table of src/compaction/scheduler.rs:147-177): table t =
    # BloomFilter::new + insert of keys [seg[t], seg[t+1]) of the run.
    @staticmethod
    def _table_args(who, seg, seg_name, num_bits, num_hashes):
        # -> num_bits as an array and the C arguments ntab, seg, num_bits, num_hashes of every batched build
        seg = np.ascontiguousarray(seg, dtype=np.uint64)
        nb = np.ascontiguousarray(num_bits, dtype=np.uint32)
        kk = np.ascontiguousarray(num_hashes, dtype=np.uint32)
        if seg.size != nb.size + 1 or kk.size != nb.size:
            raise ValueError("%s: %s needs ntab + 1 entries, num_hashes ntab" % (who, seg_name))
        return nb, (nb.size, _p(seg, u64p), _p(nb, u32p) if nb.size else None, _p(kk, u32p) if nb.size else None)

    def build_batch_dev(self, data, n, seg, num_bits, num_hashes, words, offsets=None, key_len=0, stream=None):
        """lsmb_build_batch_dev: data (and offsets, n + 1 int64, for var-len
        keys) device tensors; seg (ntab + 1), num_bits and num_hashes (ntab)
        host sequences; words a 16-byte-aligned int64 device tensor of at least
        build_batch_layout(num_bits)[-1] words, output-only, in that layout.
        Asynchronous on stream.  Returns the layout (word_off, uint64)."""
        nb, tabs = self._table_args("build_batch_dev", seg, "seg", num_bits, num_hashes)
        _check(lib().lsmb_build_batch_dev(self.h, vp(data.data_ptr()) if data is not None else None,
                                          vp(offsets.data_ptr()) if offsets is not None else None, key_len, int(n),
                                          *tabs, vp(words.data_ptr()), words.numel() * words.element_size() // 8,
                                          self._stream(stream)))
        return build_batch_layout(nb)

    def build_batch_blocks(self, data, seg, num_bits, num_hashes, offsets=None, key_len=0):
        """lsmb_build_batch_blocks: packed host keys (as build_block) ->
        (blocks, block_off): the tables' serialized bloom blocks back to back
        (uint8) and their ntab + 1 offsets (uint64), the form
        lsmb_lset_add_batch takes.  Runs on the GPU whatever the key count."""
        data, n, op = _host_keys(data, offsets, key_len)
        nb, tabs = self._table_args("build_batch_blocks", seg, "seg", num_bits, num_hashes)
        boff = np.zeros(nb.size + 1, dtype=np.uint64)
        blocks = np.empty(max(sum(serialized_size(int(b)) for b in nb), 1), dtype=np.uint8)
        _check(lib().lsmb_build_batch_blocks(self.h, _p(data, u8p), op, key_len, n, *tabs, _p(blocks, u8p), blocks.size,
                                             _p(boff, u64p)))
        return blocks[:int(boff[nb.size])], boff

    # The same filters straight from the tables' data blocks (src/sstable/block/builder.rs:40-76):
    # block b = bytes[blk_off[b] .. blk_off[b] + blk_len[b]), table t = blocks [bseg[t], bseg[t+1]).
    @staticmethod
    def _block_args(who, bytes, blk_off, blk_len, seg, seg_name):
        # -> blk_off, blk_len and seg as arrays, and the five leading C arguments of every call on blocks;
        # bytes is a device tensor, host bytes (empty ones become one zero byte, never a NULL pointer) or None
        bo = np.ascontiguousarray(blk_off, dtype=np.uint64)
        bl = np.ascontiguousarray(blk_len, dtype=np.uint32)
        seg = np.ascontiguousarray(seg, dtype=np.uint64)
        if bo.size != bl.size:
            raise ValueError("%s: blk_off and blk_len differ in length" % who)
        if seg_name == "sseg" and seg.size < 1:  # (bseg is measured against num_bits, _table_args)
            raise ValueError("%s: sseg needs nsrc + 1 entries" % who)
        ptr, nbytes = None, 0
        if hasattr(bytes, "data_ptr"):
            ptr, nbytes = vp(bytes.data_ptr()), bytes.numel() * bytes.element_size()
        elif bytes is not None:
            data = bytes if isinstance(bytes, np.ndarray) else np.frombuffer(bytes, dtype=np.uint8)
            data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
            ptr, nbytes = _p(data if data.size else np.zeros(1, np.uint8), u8p), data.size  # (ptr keeps the array)
        nblk = bo.size
        return bo, bl, seg, (ptr, nbytes, nblk, _p(bo, u64p) if nblk else None, _p(bl, u32p) if nblk else None)

    def build_batch_sst_dev(self, bytes, blk_off, blk_len, bseg, num_bits, num_hashes, words, blk_entries=None,
                            stream=None):
        """lsmb_build_batch_sst_dev: bytes a uint8 device tensor holding the
        blocks; blk_off, blk_len (nblk), bseg (ntab + 1), num_bits and
        num_hashes (ntab) host sequences; words as build_batch_dev's;
        blk_entries an int32 device tensor of nblk entries or None (entry b =
        block b's entry count, LSMB_SST_BAD_BLOCK for a malformed block).
        Asynchronous on stream.  Returns the layout (word_off, uint64)."""
        bo, bl, bseg, head = self._block_args("build_batch_sst_dev", bytes, blk_off, blk_len, bseg, "bseg")
        nb, tabs = self._table_args("build_batch_sst_dev", bseg, "bseg", num_bits, num_hashes)
        if blk_entries is not None and blk_entries.numel() * blk_entries.element_size() < 4 * bo.size:
            raise ValueError("build_batch_sst_dev: blk_entries needs one uint32 per block")
        _check(lib().lsmb_build_batch_sst_dev(
            self.h, *head, *tabs, vp(words.data_ptr()), words.numel() * words.element_size() // 8,
            vp(blk_entries.data_ptr()) if blk_entries is not None else None, self._stream(stream)))
        return build_batch_layout(nb)

    def build_batch_sst_blocks(self, bytes, blk_off, blk_len, bseg, num_bits, num_hashes):
        """lsmb_build_batch_sst_blocks: host bytes holding the data blocks ->
        (blooms, bloom_off, entries, status): the tables' serialized bloom
        blocks back to back (uint8), their ntab + 1 offsets (uint64), each
        table's entry count (uint64) and LSMB_OK or LSMB_ECORRUPT per table
        (int32).  A malformed block is not raised: it is its table's status
        (that table's bloom bytes are unspecified, every other table's exact),
        and lsmb_last_error() names the first such table and block.  Runs on
        the GPU whatever the block count."""
        bo, bl, bseg, head = self._block_args("build_batch_sst_blocks", bytes, blk_off, blk_len, bseg, "bseg")
        nb, tabs = self._table_args("build_batch_sst_blocks", bseg, "bseg", num_bits, num_hashes)
        ntab = nb.size
        boff = np.zeros(ntab + 1, dtype=np.uint64)
        blooms = np.empty(max(sum(serialized_size(int(b)) for b in nb), 1), dtype=np.uint8)
        entries = np.zeros(ntab, dtype=np.uint64)
        status = np.zeros(ntab, dtype=np.int32)
        rc = lib().lsmb_build_batch_sst_blocks(
            self.h, *head, *tabs, _p(blooms, u8p), blooms.size, _p(boff, u64p), _p(entries, u64p) if ntab else None,
            _p(status, ctypes.POINTER(ctypes.c_int32)) if ntab else None)
        if rc != LSMB_ECORRUPT:
            _check(rc)
        return blooms[:int(boff[ntab])], boff, entries, status

    # The surviving keys of a compaction's merged data blocks (src/iterator/merge.rs:98-121,
    # src/compaction/scheduler.rs:147-158): the blocks as above, cut into sources, source s = the
    # blocks [sseg[s], sseg[s+1]), source 0 the newest.
    def compact_sst_mark_dev(self, bytes, blk_off, blk_len, sseg, drop_tombstones, work, totals, blk_entries=None,
                             stream=None):
        """lsmb_compact_sst_mark_dev: bytes a uint8 device tensor holding the
        blocks; blk_off, blk_len (nblk) and sseg (nsrc + 1) host sequences;
        work a device tensor of at least compact_sst_work_bytes(blk_len)
        bytes, 16-byte aligned; totals a device tensor of 4 int64 (survivors,
        their key bytes, entries seen, bad blocks); blk_entries as
        build_batch_sst_dev's.  Asynchronous on stream."""
        bo, bl, sseg, head = self._block_args("compact_sst_mark_dev", bytes, blk_off, blk_len, sseg, "sseg")
        if totals.numel() * totals.element_size() < 32:
            raise ValueError("compact_sst_mark_dev: totals needs four uint64")
        if blk_entries is not None and blk_entries.numel() * blk_entries.element_size() < 4 * bo.size:
            raise ValueError("compact_sst_mark_dev: blk_entries needs one uint32 per block")
        _check(lib().lsmb_compact_sst_mark_dev(
            self.h, *head, sseg.size - 1, _p(sseg, u64p), int(bool(drop_tombstones)),
            vp(work.data_ptr()), work.numel() * work.element_size(),
            vp(blk_entries.data_ptr()) if blk_entries is not None else None, vp(totals.data_ptr()),
            self._stream(stream)))

    def compact_sst_gather_dev(self, bytes, blk_off, blk_len, sseg, work, key_data, key_offsets, stream=None):
        """lsmb_compact_sst_gather_dev after a mark of the same arguments on
        the same stream: the survivors' keys into key_data (uint8 device
        tensor, at least totals[1] bytes) and survivors + 1 offsets into
        key_offsets (int64 device tensor).  Capacities below the mark's totals
        truncate the run: nothing is written past them."""
        bo, bl, sseg, head = self._block_args("compact_sst_gather_dev", bytes, blk_off, blk_len, sseg, "sseg")
        _check(lib().lsmb_compact_sst_gather_dev(
            self.h, *head, sseg.size - 1, _p(sseg, u64p), vp(work.data_ptr()),
            vp(key_data.data_ptr()) if key_data is not None and key_data.numel() else None,
            key_data.numel() * key_data.element_size() if key_data is not None else 0,
            vp(key_offsets.data_ptr()) if key_offsets is not None and key_offsets.numel() else None,
            key_offsets.numel() * key_offsets.element_size() // 8 if key_offsets is not None else 0,
            self._stream(stream)))

    def compact_sst_bloom(self, bytes, blk_off, blk_len, sseg, drop_tombstones, expected_items=0, fpr=0.01):
        """lsmb_compact_sst_bloom: host bytes holding the input tables' data
        blocks -> (bloom block bytes, num_bits, k, entry_count) of the
        compaction's output table.  expected_items = 0 sizes the filter for the
        survivors; 1000 with fpr = 0.01 is the store's own block.  Corruption
        for a malformed or empty block.  Runs on the GPU whatever the size."""
        bo, bl, sseg, head = self._block_args("compact_sst_bloom", bytes, blk_off, blk_len, sseg, "sseg")
        # a first size: the filter asked for, or one for every entry the blocks can hold without overlap
        guess = int(expected_items) or max(int(bl.sum()) // 6, 1)
        cap = serialized_size(params(guess, fpr)[0])
        blen, count = ctypes.c_uint64(0), ctypes.c_uint64(0)
        nb, k = ctypes.c_uint32(0), ctypes.c_uint32(0)
        for _ in range(2):
            bloom = np.empty(cap, dtype=np.uint8)
            rc = lib().lsmb_compact_sst_bloom(
                self.h, *head, sseg.size - 1, _p(sseg, u64p), int(bool(drop_tombstones)), int(expected_items), float(fpr),
                _p(bloom, u8p), cap, ctypes.byref(blen), ctypes.byref(count), ctypes.byref(nb), ctypes.byref(k))
            if rc != LSMB_EINVAL or blen.value <= cap:
                break
            cap = blen.value  # the block is larger than the guess (overlapping entries): once more
        _check(rc)
        return bloom[:blen.value].tobytes(), nb.value, k.value, count.value

    def probe_dev(self, filters, data, n, out, offsets=None, key_len=0, stream=None):
        """filters: [(words tensor on device, num_bits, k)]."""
        F = len(filters)
        arr = (vp * F)(*[vp(f[0].data_ptr()) for f in filters])
        nb = np.array([f[1] for f in filters], dtype=np.uint32)
        kk = np.array([f[2] for f in filters], dtype=np.uint32)
        _check(lib().lsmb_probe_dev(self.h, arr, _p(nb, u32p), _p(kk, u32p), F, vp(data.data_ptr()),
                                    vp(offsets.data_ptr()) if offsets is not None else None, key_len, n,
                                    vp(out.data_ptr()), self._stream(stream)))

    def or_reduce_dev(self, dst, src, nwords, nsrc, stride_words, stream=None):
        _check(lib().lsmb_or_reduce_dev(self.h, vp(dst.data_ptr()), vp(src.data_ptr()), nwords, nsrc,
                                        stride_words, self._stream(stream)))

    def or_gather_dev(self, dst_ptr, src_ptrs, nwords, stream=None, status_ptr=0):
        """dst[i] = OR of src_j[i] over the raw device pointers src_ptrs (own or
        IPC-mapped peer memory), nwords u64 words (lsmb_or_gather_dev); with a
        merge's status words (status_ptr) a poisoned merge writes all-ones."""
        arr = (vp * len(src_ptrs))(*[vp(int(p)) for p in src_ptrs])
        _check(lib().lsmb_or_gather_dev(self.h, vp(int(dst_ptr)), arr, len(src_ptrs), int(nwords),
                                        vp(int(status_ptr or 0)), self._stream(stream)))

    def copy_slices_dev(self, dst_ptr, src_ptrs, slice_words, nwords, stream=None, status_ptr=0):
        """dst slice r = src_ptrs[r]'s slice r (u64 words) for every r whose source is
        not None/0: the merge's all-gather in one kernel (lsmb_copy_slices_dev)."""
        arr = (vp * len(src_ptrs))(*[vp(int(p or 0)) for p in src_ptrs])
        _check(lib().lsmb_copy_slices_dev(self.h, vp(int(dst_ptr)), arr, len(src_ptrs), int(slice_words), int(nwords),
                                          vp(int(status_ptr or 0)), vp(stream or 0)))

    def poison_fill_dev(self, words_ptr, nwords, status_ptr, stream=None):
        """The merge's last step: all-ones over nwords words if the merge is
        poisoned (lsmb_poison_fill_dev)."""
        _check(lib().lsmb_poison_fill_dev(self.h, vp(int(words_ptr)), int(nwords), vp(int(status_ptr)),
                                          vp(stream or 0)))

    def flag_signal_dev(self, flag_ptr, value, stream=None):
        """After the stream's prior work: *flag = value, system-scope release (lsmb_flag_signal_dev)."""
        _check(lib().lsmb_flag_signal_dev(self.h, vp(int(flag_ptr)), int(value) & 0xFFFFFFFF, vp(stream or 0)))

    def flag_wait_dev(self, flag_ptrs, value, status_ptr, timeout_ms=20000, poison_ptrs=None, stream=None):
        """Later work on the stream waits until every flag >= value; a timeout or
        a set poison word ends the wait and poisons the merge's status words
        (lsmb_flag_wait_dev)."""
        arr = (vp * len(flag_ptrs))(*[vp(int(p)) for p in flag_ptrs])
        parr = (vp * len(flag_ptrs))(*[vp(int(p)) for p in poison_ptrs]) if poison_ptrs else None
        if poison_ptrs and len(poison_ptrs) != len(flag_ptrs):
            raise ValueError("one poison word per flag")
        _check(lib().lsmb_flag_wait_dev(self.h, arr, parr, len(flag_ptrs), int(value) & 0xFFFFFFFF, int(timeout_ms),
                                        vp(int(status_ptr)), vp(stream or 0)))

    def merge_status(self, status_ptr, stream=None):
        """(poisoned, timed-out waits) of a merge's status words, after the
        stream's pending work (lsmb_merge_status: synchronises the stream)."""
        out = (ctypes.c_uint32 * 2)()
        _check(lib().lsmb_merge_status(self.h, vp(int(status_ptr)), vp(stream or 0), out))
        return int(out[0]), int(out[1])

    def ipc_import(self, handle):
        """Maps another process's device allocation (lsmb_ipc_import) -> base pointer (int)."""
        h = np.frombuffer(bytes(handle), dtype=np.uint8).copy()
        base = vp()
        _check(lib().lsmb_ipc_import(self.h, _p(h, u8p), ctypes.byref(base)))
        return int(base.value)

    def ipc_close(self, base):
        _check(lib().lsmb_ipc_close(self.h, vp(int(base))))

    def gen_key16_dev(self, seed, first, n, out, stream=None):
        _check(lib().lsmb_gen_key16_dev(self.h, seed, first, n, vp(out.data_ptr()), self._stream(stream)))

    def gen_splitmix_dev(self, seed, first, n, out, mod=0, add=0, stream=None):
        _check(lib().lsmb_gen_splitmix_dev(self.h, seed, first, n, mod, add, out.data_ptr(), self._stream(stream)))

    def gen_varlen_dev(self, n, first=0, device=None):
        """C4 keys [first, first+n) of tests/keygen.varlen on the device ->
        (data uint8 tensor, offsets int64 tensor [n+1], rebased to 0)."""
        import torch
        dev = device or torch.device("cuda", torch.cuda.current_device())
        lens = torch.empty(first + n, dtype=torch.int64, device=dev)
        self.gen_splitmix_dev(0x5EED0003, 0, first + n, lens, mod=249, add=8)
        offs = torch.zeros(first + n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=offs[1:])
        del lens
        o0, o1 = int(offs[first].item()), int(offs[first + n].item())
        w0, w1 = o0 // 8, (o1 + 7) // 8
        words = torch.empty(max(w1 - w0, 1), dtype=torch.int64, device=dev)
        self.gen_splitmix_dev(0x5EED0004, w0, w1 - w0, words)
        data = words.view(torch.uint8)[o0 - 8 * w0: o0 - 8 * w0 + (o1 - o0)]
        return data, (offs[first:] - o0).contiguous()

    def set_timing(self, on):
        """Per-build HIP events (lsmb_last_build_ms) on/off."""
        _check(lib().lsmb_set_timing(self.h, 1 if on else 0))

    def last_build_ms(self):
        a = (ctypes.c_float * 3)()
        _check(lib().lsmb_last_build_ms(self.h, a))
        return tuple(a)


class KeyStream:
    """Streaming ingestion (lsmb_stream): the flush's add_key loop
    (src/db/mod.rs:379-383 -> SSTableBuilder::add -> BloomFilterBuilder::add_key)
    with full staging chunks uploaded and built while keys keep arriving.
    finish_block() == BloomFilter::new(..) + inserts, serialized."""

    def __init__(self, ctx, num_bits, k):
        """ctx None: host-only (runs of at most host_max_keys() keys)."""
        h = vp()
        _check(lib().lsmb_stream_open(ctx.h if ctx else None, num_bits, k, ctypes.byref(h)))
        self.h, self.ctx, self.num_bits, self.k = h, ctx, num_bits, k

    def close(self):
        if self.h:
            lib().lsmb_stream_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, num_bits, k):
        _check(lib().lsmb_stream_reset(self.h, num_bits, k))
        self.num_bits, self.k = num_bits, k

    def add(self, key):
        a, n = _key(key)
        _check(lib().lsmb_stream_add(self.h, _p(a, u8p), n))

    def add_batch(self, data, offsets):
        data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if data.size == 0:
            data = np.zeros(1, np.uint8)
        _check(lib().lsmb_stream_add_batch(self.h, _p(data, u8p), _p(offsets, u64p), offsets.size - 1))

    def count(self):
        return int(lib().lsmb_stream_count(self.h))

    def finish_block(self, out=None):
        if out is None:
            out = np.empty(serialized_size(self.num_bits), dtype=np.uint8)
        _check(lib().lsmb_stream_finish_block(self.h, _p(out, u8p), out.size))
        return out

    def finish_words(self):
        w = np.zeros(max(num_words(self.num_bits), 1), dtype=np.uint64)
        _check(lib().lsmb_stream_finish_words(self.h, _p(w, u64p)))
        return w[: num_words(self.num_bits)]


class FilterSet:
    """Device-resident SSTable filters with key ranges (lsmb_fset): the batched
    form of SSTable::get's range + bloom pre-check (src/sstable/reader.rs:192-199).

    probe(keys)[i] bit s = (min_s <= key_i <= max_s) and may_contain(filter s, key_i).
    """

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        h = vp()
        _check(lib().lsmb_fset_open(self.ctx.h, ctypes.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib().lsmb_fset_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, block, min_key, max_key):
        """block: serialized filter bytes (BloomFilter::serialize) -> slot."""
        b, n = _key(block)
        lo, nlo = _key(min_key)
        hi, nhi = _key(max_key)
        return _check(lib().lsmb_fset_add(self.h, _p(b, u8p), n, _p(lo, u8p), nlo, _p(hi, u8p), nhi))

    def add_checked(self, block, crc, min_key, max_key):
        """add() that checks the block's CRC-32 on the device copy (lsmb_fset_add_crc)."""
        b, n = _key(block)
        lo, nlo = _key(min_key)
        hi, nhi = _key(max_key)
        return _check(lib().lsmb_fset_add_crc(self.h, _p(b, u8p), n, crc, _p(lo, u8p), nlo, _p(hi, u8p), nhi))

    def add_filter(self, filt, min_key, max_key):
        """filt: BloomFilter -> slot."""
        w = np.ascontiguousarray(filt.bits, dtype=np.uint64)
        if w.size == 0:
            w = np.zeros(1, np.uint64)
        lo, nlo = _key(min_key)
        hi, nhi = _key(max_key)
        return _check(lib().lsmb_fset_add_words(self.h, _p(w, u64p), filt.num_bits(), filt.num_hashes(),
                                                _p(lo, u8p), nlo, _p(hi, u8p), nhi))

    def remove(self, slot):
        _check(lib().lsmb_fset_remove(self.h, int(slot)))

    def live_mask(self):
        return int(lib().lsmb_fset_live_mask(self.h))

    def probe(self, data, offsets=None, key_len=0):
        """Packed host keys (as Context.probe) -> uint64 mask per key."""
        data, n, op = _host_keys(data, offsets, key_len)
        out = np.zeros(n, dtype=np.uint64)
        _check(lib().lsmb_fset_probe(self.h, _p(data, u8p), op, key_len, n, _p(out if n else np.zeros(1, np.uint64),
                                                                                u64p)))
        return out

    def probe_keys(self, keys):
        """list of bytes -> uint64 mask per key."""
        return self.probe(*_pack_keys(keys))

    def probe_dev(self, data, n, out, offsets=None, key_len=0, stream=None, row_bytes=8):
        """Device keys -> device answer rows: u64 per key (lsmb_fset_probe_dev),
        or row_bytes = 1 / 2 / 4 per key when every live slot fits them
        (lsmb_fset_probe_dev_rows)."""
        offs = vp(offsets.data_ptr()) if offsets is not None else None
        if row_bytes == 8:
            _check(lib().lsmb_fset_probe_dev(self.h, vp(data.data_ptr()), offs, key_len, n, vp(out.data_ptr()),
                                             Context._stream(stream)))
        else:
            _check(lib().lsmb_fset_probe_dev_rows(self.h, vp(data.data_ptr()), offs, key_len, n, vp(out.data_ptr()),
                                                  int(row_bytes), Context._stream(stream)))

    def probe_lists(self, data, offsets=None, key_len=0, cap=None):
        """Packed host keys (as probe) -> (starts uint64[65], index uint32[total]):
        index[starts[s]:starts[s+1]] = the ascending indices of the keys with
        bit s set in probe()'s mask (lsmb_fset_probe_lists).  cap (default n)
        sizes the first call; a longer answer takes one more with cap = total."""
        data, n, op = _host_keys(data, offsets, key_len)
        starts = np.zeros(65, dtype=np.uint64)
        cap = n if cap is None else int(cap)
        while True:
            index = np.empty(max(cap, 1), dtype=np.uint32)
            _check(lib().lsmb_fset_probe_lists(self.h, _p(data, u8p), op, key_len, n, _p(starts, u64p),
                                               _p(index, u32p), cap))
            total = int(starts[64])
            if total <= cap:
                return starts, index[:total]
            cap = total

    def probe_lists_keys(self, keys):
        """list of bytes -> (starts, index) as probe_lists."""
        return self.probe_lists(*_pack_keys(keys))

    def probe_lists_dev(self, data, n, starts, index, offsets=None, key_len=0, stream=None):
        """Device keys -> device lists (lsmb_fset_probe_lists_dev): starts an
        int64 / uint64 tensor of 65, index an int32 / uint32 tensor whose
        length is the capacity (None: a counting call).  starts is always
        exact; entries at positions at and past the capacity are not written."""
        offs = vp(offsets.data_ptr()) if offsets is not None else None
        cap = int(index.numel()) if index is not None else 0
        _check(lib().lsmb_fset_probe_lists_dev(self.h, vp(data.data_ptr()), offs, key_len, n, vp(starts.data_ptr()),
                                               vp(index.data_ptr()) if cap else None, cap, Context._stream(stream)))


class LevelSet:
    """Device-resident snapshot of the store's non-overlapping levels (lsmb_lset),
    one per Version: rows of tables with pairwise disjoint key ranges, any
    number per row.  add / add_filter in any order, then seal(), then probe:

    probe(keys)[r, i] = table_id of the one table t of row r with
    min_t <= key_i <= max_t and may_contain(filter t, key_i), else LSMB_LSET_NONE.

    Every add also takes row=LSMB_LSET_ROW_L0: the table goes to the set's L0
    part (up to LSMB_LSET_L0_MAX tables, overlapping ranges, position = order
    of arrival), and probe_version answers L0 and the rows together, so one
    sealed set is one Version; a flush or a compaction is derive + add + seal.
    """

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        h = vp()
        _check(lib().lsmb_lset_open(self.ctx.h, ctypes.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib().lsmb_lset_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, row, table_id, block, min_key, max_key):
        """block: serialized filter bytes (BloomFilter::serialize)."""
        b, n = _key(block)
        lo, nlo = _key(min_key)
        hi, nhi = _key(max_key)
        _check(lib().lsmb_lset_add(self.h, int(row), int(table_id), _p(b, u8p), n, _p(lo, u8p), nlo, _p(hi, u8p), nhi))

    def add_filter(self, row, table_id, filt, min_key, max_key):
        """filt: BloomFilter."""
        w = np.ascontiguousarray(filt.bits, dtype=np.uint64)
        if w.size == 0:
            w = np.zeros(1, np.uint64)
        lo, nlo = _key(min_key)
        hi, nhi = _key(max_key)
        _check(lib().lsmb_lset_add_words(self.h, int(row), int(table_id), _p(w, u64p), filt.num_bits(),
                                         filt.num_hashes(), _p(lo, u8p), nlo, _p(hi, u8p), nhi))

    def seal(self):
        _check(lib().lsmb_lset_seal(self.h))

    def derive(self, drop_ids=(), repack=None, stream=None):
        """Version edit (lsmb_lset_derive): a new, unsealed LevelSet holding
        every table of this sealed set whose id is not in drop_ids, sharing
        the device filter words (nothing is uploaded).  Then add / add_many /
        seal; this set and the new one are closed in either order.  The
        number of tables left out is the new set's `dropped`.

        repack (lsmb_lset_derive_packed): a fraction in (0, 1] moves the
        survivors of every chunk of this set whose live share is below it into
        a chunk of the new set's own, device to device on stream (one launch,
        one wait), and the new set's next add continues there; "all" moves
        every survivor; 0 moves nothing.  The new set's `moved` is (tables
        moved, their slot bytes); (0, 0) without repack."""
        ids = np.ascontiguousarray(list(drop_ids), dtype=np.uint32)
        h = vp()
        nd = ctypes.c_uint64()
        mv = np.zeros(2, dtype=np.uint64)
        if repack is None:
            _check(lib().lsmb_lset_derive(self.h, _p(ids, u32p) if ids.size else None, ids.size,
                                          ctypes.cast(ctypes.byref(nd), u64p), ctypes.byref(h)))
        else:
            if isinstance(repack, str):
                if repack != "all":
                    raise ValueError('derive: repack is None, a fraction in [0, 1] or "all"')
                ppm = LSMB_LSET_REPACK_ALL
            else:
                if not 0 <= repack <= 1:
                    raise ValueError('derive: repack is None, a fraction in [0, 1] or "all"')
                ppm = int(round(repack * 1_000_000))
            _check(lib().lsmb_lset_derive_packed(self.h, _p(ids, u32p) if ids.size else None, ids.size, ppm,
                                                 ctypes.cast(ctypes.byref(nd), u64p), _p(mv, u64p), ctypes.byref(h),
                                                 Context._stream(stream)))
        child = LevelSet.__new__(LevelSet)
        child.ctx = self.ctx
        child.h = h
        child.dropped = int(nd.value)
        child.moved = (int(mv[0]), int(mv[1]))
        return child

    def add_many(self, rows, ids, blocks, ranges, crcs=None):
        """Many tables in one call (lsmb_lset_add_batch): rows and ids per
        table, blocks a list of serialized filters, ranges a list of
        (min_key, max_key), crcs (optional) each block's CRC-32, checked on
        the device copy.  All or nothing: raises as add does (Corruption,
        ValueError) for the first failing table, the exception's `status`
        holding every table's own code, and the set is unchanged; else
        returns the status array (all LSMB_OK)."""
        n = len(blocks)
        if not (len(rows) == len(ids) == len(ranges) == n) or (crcs is not None and len(crcs) != n):
            raise ValueError("add_many: rows, ids, blocks, ranges and crcs differ in length")
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        boff = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([len(b) for b in blocks], out=boff[1:])
        bb = np.frombuffer(b"".join(bytes(b) for b in blocks) + b"\0", dtype=np.uint8)
        kb, koff = _pack_ranges(ranges)
        cc = None if crcs is None else np.ascontiguousarray(crcs, dtype=np.uint32)
        status = np.zeros(max(n, 1), dtype=np.int32)
        rc = lib().lsmb_lset_add_batch(self.h, n, _p(rows, u32p) if n else None, _p(ids, u32p) if n else None,
                                       _p(bb, u8p), _p(boff, u64p), None if cc is None or not n else _p(cc, u32p),
                                       _p(kb, u8p), _p(koff, u64p), _p(status, ctypes.POINTER(ctypes.c_int32)))
        try:
            _check(rc)
        except (LsmbError, ValueError) as e:
            e.status = status[:n]
            raise
        return status[:n]

    def add_built(self, rows, ids, words, num_bits, num_hashes, ranges, stream=None):
        """Tables whose filters Context.build_batch_dev left on this set's
        device (lsmb_lset_add_batch_dev): words the int64 device tensor in the
        layout of build_batch_layout(num_bits), rows / ids / num_bits /
        num_hashes per table, ranges a list of (min_key, max_key).  The words
        move device to device on stream, which is synchronised once: on return
        `words` is free and the set is ready for seal.  All or nothing."""
        n = len(ranges)
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        nb = np.ascontiguousarray(num_bits, dtype=np.uint32)
        kk = np.ascontiguousarray(num_hashes, dtype=np.uint32)
        if not (rows.size == ids.size == nb.size == kk.size == n):
            raise ValueError("add_built: rows, ids, num_bits, num_hashes and ranges differ in length")
        woff = build_batch_layout(nb)
        if words.numel() * words.element_size() < 8 * int(woff[n]):
            raise ValueError("add_built: words is smaller than the layout of num_bits")
        kb, koff = _pack_ranges(ranges)
        _check(lib().lsmb_lset_add_batch_dev(self.h, n, _p(rows, u32p) if n else None, _p(ids, u32p) if n else None,
                                             vp(words.data_ptr()), _p(woff, u64p), _p(nb, u32p) if n else None,
                                             _p(kk, u32p) if n else None, _p(kb, u8p), _p(koff, u64p),
                                             Context._stream(stream)))

    def stats(self):
        """lsmb_lset_stats: tables, inherited (by derive), uploaded_bytes and
        upload_copies (this set's own filter uploads), chunk_bytes (device
        bytes of the arena chunks it keeps alive, shared ones included),
        filter_bytes (of its tables); occupancy = filter_bytes / chunk_bytes."""
        out = np.zeros(6, dtype=np.uint64)
        _check(lib().lsmb_lset_stats(self.h, _p(out, u64p)))
        d = dict(zip(("tables", "inherited", "uploaded_bytes", "upload_copies", "chunk_bytes", "filter_bytes"),
                     (int(x) for x in out)))
        d["occupancy"] = d["filter_bytes"] / d["chunk_bytes"] if d["chunk_bytes"] else 0.0
        return d

    def rows(self):
        return int(lib().lsmb_lset_rows(self.h))

    def tables(self, row):
        return int(lib().lsmb_lset_tables(self.h, int(row)))

    def probe(self, data, offsets=None, key_len=0):
        """Packed host keys (as Context.probe) -> uint32 table ids, shape (rows(), n)."""
        data, n, op = _host_keys(data, offsets, key_len)
        out = np.empty((self.rows(), n), dtype=np.uint32)
        _check(lib().lsmb_lset_probe(self.h, _p(data, u8p), op, key_len, n,
                                     _p(out if out.size else np.zeros(1, np.uint32), u32p)))
        return out

    def probe_keys(self, keys):
        """list of bytes -> uint32 table ids, shape (rows(), len(keys))."""
        return self.probe(*_pack_keys(keys))

    def probe_dev(self, data, n, out, offsets=None, key_len=0, stream=None):
        """Device keys -> device table ids (lsmb_lset_probe_dev): out an int32 /
        uint32 tensor of rows() * n, row r's answers at out[r * n : (r + 1) * n]."""
        offs = vp(offsets.data_ptr()) if offsets is not None else None
        _check(lib().lsmb_lset_probe_dev(self.h, vp(data.data_ptr()), offs, key_len, n, vp(out.data_ptr()),
                                         Context._stream(stream)))

    def l0_tables(self):
        """Tables of the L0 part (lsmb_lset_l0_tables)."""
        return int(lib().lsmb_lset_l0_tables(self.h))

    def l0_order(self):
        """-> uint32[l0_tables()]: the L0 tables' ids in position order,
        oldest first (bit j of probe_version's mask is position j)."""
        ids = np.zeros(max(self.l0_tables(), 1), dtype=np.uint32)
        _check(lib().lsmb_lset_l0_order(self.h, _p(ids, u32p)))
        return ids[:self.l0_tables()]

    def probe_version(self, data, offsets=None, key_len=0):
        """Packed host keys (as probe) -> (mask uint64[n], ids uint32[rows(), n])
        from one hash per key (lsmb_lset_probe_version): mask[i] bit j =
        min_j <= key_i <= max_j and may_contain(filter j, key_i) for the L0
        table at position j (a reader visits set bits from the highest down),
        ids exactly probe()'s."""
        data, n, op = _host_keys(data, offsets, key_len)
        mask = np.zeros(n, dtype=np.uint64)
        out = np.empty((self.rows(), n), dtype=np.uint32)
        _check(lib().lsmb_lset_probe_version(self.h, _p(data, u8p), op, key_len, n,
                                             _p(mask if n else np.zeros(1, np.uint64), u64p),
                                             _p(out, u32p) if out.size else None))
        return mask, out

    def probe_version_keys(self, keys):
        """list of bytes -> (mask, ids) as probe_version."""
        return self.probe_version(*_pack_keys(keys))

    def probe_version_dev(self, data, n, mask, out, offsets=None, key_len=0, stream=None):
        """Device keys -> device answers (lsmb_lset_probe_version_dev): mask an
        int64 / uint64 tensor of n, out an int32 / uint32 tensor of rows() * n
        as probe_dev's (None when the set has no row)."""
        offs = vp(offsets.data_ptr()) if offsets is not None else None
        _check(lib().lsmb_lset_probe_version_dev(self.h, vp(data.data_ptr()), offs, key_len, n, vp(mask.data_ptr()),
                                                 vp(out.data_ptr()) if out is not None else None,
                                                 Context._stream(stream)))

    def total_tables(self):
        """Tables of all rows (0 before seal): the lists' ordinals are 0 .. total_tables() - 1."""
        return int(lib().lsmb_lset_total_tables(self.h))

    def table_order(self):
        """-> (ids uint32[G], row_base uint64[rows() + 1]): table j of row r in
        the row's sealed order (ascending min_key) has the ordinal
        row_base[r] + j and the table id ids[row_base[r] + j]."""
        ids = np.zeros(max(self.total_tables(), 1), dtype=np.uint32)
        base = np.zeros(self.rows() + 1, dtype=np.uint64)
        _check(lib().lsmb_lset_table_order(self.h, _p(ids, u32p), _p(base, u64p)))
        return ids[:self.total_tables()], base

    def _lists(self, fn, total, data, offsets, key_len, cap):
        """probe_lists and probe_version_lists: fn the C entry point, total its table count."""
        data, n, op = _host_keys(data, offsets, key_len)
        starts = np.zeros(total + 1, dtype=np.uint64)
        if cap is None:
            _check(fn(self.h, _p(data, u8p), op, key_len, n, _p(starts, u64p), None, 0))
            cap = int(starts[-1])
            if cap == 0:
                return starts, np.zeros(0, dtype=np.uint32)
        cap = int(cap)
        index = np.empty(max(cap, 1), dtype=np.uint32)
        _check(fn(self.h, _p(data, u8p), op, key_len, n, _p(starts, u64p), _p(index, u32p) if cap else None, cap))
        return starts, index[:min(int(starts[-1]), cap)]

    def _lists_dev(self, fn, data, n, starts, index, work, offsets, key_len, stream):
        """probe_lists_dev and probe_version_lists_dev: fn the C entry point."""
        offs = vp(offsets.data_ptr()) if offsets is not None else None
        cap = int(index.numel()) if index is not None else 0
        wb = int(work.numel() * work.element_size()) if work is not None else 0
        _check(fn(self.h, vp(data.data_ptr()), offs, key_len, n, vp(starts.data_ptr()),
                  vp(index.data_ptr()) if cap else None, cap, vp(work.data_ptr()) if wb else None, wb,
                  Context._stream(stream)))

    def lists_work_bytes(self, n):
        """Bytes of device workspace probe_lists_dev needs for n keys."""
        return int(lib().lsmb_lset_lists_work_bytes(self.h, int(n)))

    def probe_lists(self, data, offsets=None, key_len=0, cap=None):
        """Packed host keys (as probe) -> (starts uint64[G + 1], index
        uint32[min(total, cap)]): index[starts[g]:starts[g+1]] = the ascending
        indices of the keys for which probe() answers the table of ordinal g
        (table_order()) in g's row (lsmb_lset_probe_lists).  cap=None sizes
        index from a counting call."""
        return self._lists(lib().lsmb_lset_probe_lists, self.total_tables(), data, offsets, key_len, cap)

    def probe_lists_keys(self, keys):
        """list of bytes -> (starts, index) as probe_lists."""
        return self.probe_lists(*_pack_keys(keys))

    def probe_lists_dev(self, data, n, starts, index, work, offsets=None, key_len=0, stream=None):
        """Device keys -> device lists (lsmb_lset_probe_lists_dev): starts an
        int64 / uint64 tensor of total_tables() + 1, index an int32 / uint32
        tensor whose length is the capacity (None: a counting call), work a
        uint8 tensor of at least lists_work_bytes(n) bytes — the probe's only
        scratch, so probes on different streams take different tensors.  starts
        is always exact; entries at and past the capacity are not written."""
        self._lists_dev(lib().lsmb_lset_probe_lists_dev, data, n, starts, index, work, offsets, key_len, stream)

    def version_tables(self):
        """L0 tables + tables of all rows (0 before seal): the Version lists'
        ordinals are 0 .. version_tables() - 1, L0 positions first."""
        return int(lib().lsmb_lset_version_tables(self.h))

    def version_order(self):
        """-> (ids uint32[V], part_base uint64[rows() + 2]): l0_order()'s ids
        then table_order()'s; part_base = 0, T0, T0 + row_base[1], ..., V."""
        ids = np.zeros(max(self.version_tables(), 1), dtype=np.uint32)
        base = np.zeros(self.rows() + 2, dtype=np.uint64)
        _check(lib().lsmb_lset_version_order(self.h, _p(ids, u32p), _p(base, u64p)))
        return ids[:self.version_tables()], base

    def version_geometry(self):
        """-> (num_bits uint32[V], num_hashes uint32[V]): every table's filter
        geometry in version_order()'s order (lsmb_lset_version_geometry)."""
        V = self.version_tables()
        nb = np.zeros(max(V, 1), dtype=np.uint32)
        kk = np.zeros(max(V, 1), dtype=np.uint32)
        _check(lib().lsmb_lset_version_geometry(self.h, _p(nb, u32p), _p(kk, u32p)))
        return nb[:V], kk[:V]

    def census(self, stream=None):
        """The fill of every table's resident filter (lsmb_lset_census: one
        launch on stream, one wait) -> (ids uint32[V], num_bits uint32[V],
        num_hashes uint32[V], set_bits uint64[V], fpr float64[V], keys
        float64[V]) in version_order()'s order: fpr the false-positive rate
        the fill predicts (fill_fpr), keys the distinct keys a filter of that
        fill holds (fill_keys), to set against the estimate the table's
        filter was sized for.  Not cached: a sealed set is immutable, so call
        it once per Version."""
        ids, _ = self.version_order()
        nb, kk = self.version_geometry()
        V = ids.size
        sb = np.zeros(max(V, 1), dtype=np.uint64)
        _check(lib().lsmb_lset_census(self.h, _p(sb, u64p), Context._stream(stream)))
        sb = sb[:V]
        L = lib()
        fpr = np.array([L.lsmb_fill_fpr(int(m), int(k), int(x)) for m, k, x in zip(nb, kk, sb)], dtype=np.float64)
        keys = np.array([L.lsmb_fill_keys(int(m), int(k), int(x)) for m, k, x in zip(nb, kk, sb)], dtype=np.float64)
        return ids, nb, kk, sb, fpr, keys

    def version_lists_work_bytes(self, n):
        """Bytes of device workspace probe_version_lists_dev needs for n keys."""
        return int(lib().lsmb_lset_version_lists_work_bytes(self.h, int(n)))

    def probe_version_lists(self, data, offsets=None, key_len=0, cap=None):
        """Packed host keys (as probe) -> (starts uint64[V + 1], index
        uint32[min(total, cap)]) over Version ordinals (version_order()):
        index[starts[v]:starts[v+1]] = the ascending indices of the keys with
        bit v of probe_version()'s mask set (v < l0_tables()), or for which
        probe() answers the row table of ordinal v - l0_tables(), from one
        hash per key (lsmb_lset_probe_version_lists).  cap=None sizes index
        from a counting call."""
        return self._lists(lib().lsmb_lset_probe_version_lists, self.version_tables(), data, offsets, key_len, cap)

    def probe_version_lists_keys(self, keys):
        """list of bytes -> (starts, index) as probe_version_lists."""
        return self.probe_version_lists(*_pack_keys(keys))

    def probe_version_lists_dev(self, data, n, starts, index, work, offsets=None, key_len=0, stream=None):
        """Device keys -> device lists (lsmb_lset_probe_version_lists_dev):
        starts an int64 / uint64 tensor of version_tables() + 1, index an int32
        / uint32 tensor whose length is the capacity (None: a counting call),
        work a uint8 tensor of at least version_lists_work_bytes(n) bytes — the
        probe's only scratch, so probes on different streams take different
        tensors.  starts is always exact; entries at and past the capacity are
        not written."""
        self._lists_dev(lib().lsmb_lset_probe_version_lists_dev, data, n, starts, index, work, offsets, key_len,
                        stream)

    def walk_steps(self):
        """W = l0_tables() + rows() (0 before seal): the steps of DB::get's
        walk.  Step w < l0_tables() consults the L0 table at position
        l0_tables() - 1 - w (step 0 the newest), step l0_tables() + r row r."""
        return int(lib().lsmb_lset_walk_steps(self.h))

    @staticmethod
    def _resume(resume, n):
        """A walk's resume steps (None: all zero) -> contiguous uint32[n] or None."""
        if resume is None:
            return None
        resume = np.ascontiguousarray(resume, dtype=np.uint32)
        if resume.shape != (n,):
            raise ValueError("resume: one step per key")
        return resume

    def probe_walk(self, data, offsets=None, key_len=0, resume=None):
        """Packed host keys (as probe) -> (step uint32[n], ord uint32[n]) from
        one hash per key (lsmb_lset_probe_walk): step[i] = the first walk step
        w >= resume[i] (None: 0) at which key i has a candidate (a set bit of
        probe_version()'s mask, or a table answered by probe() in that row),
        ord[i] that table's Version ordinal (version_order()); LSMB_LSET_NONE
        in both when there is none or resume[i] >= walk_steps()."""
        data, n, op = _host_keys(data, offsets, key_len)
        resume = self._resume(resume, n)
        step = np.empty(max(n, 1), dtype=np.uint32)
        ord_ = np.empty(max(n, 1), dtype=np.uint32)
        _check(lib().lsmb_lset_probe_walk(self.h, _p(data, u8p), op, key_len, n,
                                          _p(resume, u32p) if resume is not None and n else None, _p(step, u32p),
                                          _p(ord_, u32p)))
        return step[:n], ord_[:n]

    def probe_walk_keys(self, keys, resume=None):
        """list of bytes -> (step, ord) as probe_walk."""
        data, offs = _pack_keys(keys)
        return self.probe_walk(data, offs, resume=resume)

    def probe_walk_dev(self, data, n, ord, step=None, resume=None, offsets=None, key_len=0, stream=None):
        """Device keys -> device answers (lsmb_lset_probe_walk_dev): ord and
        step (optional) int32 / uint32 tensors of n, resume (optional) a tensor
        of n resume steps; step may be the resume tensor itself."""
        offs = vp(offsets.data_ptr()) if offsets is not None else None
        _check(lib().lsmb_lset_probe_walk_dev(self.h, vp(data.data_ptr()), offs, key_len, n,
                                              vp(resume.data_ptr()) if resume is not None else None,
                                              vp(step.data_ptr()) if step is not None else None,
                                              vp(ord.data_ptr()) if ord is not None else None, Context._stream(stream)))

    def walk_lists_work_bytes(self, n):
        """Bytes of device workspace probe_walk_lists_dev needs for n keys."""
        return int(lib().lsmb_lset_walk_lists_work_bytes(self.h, int(n)))

    def probe_walk_lists(self, data, offsets=None, key_len=0, cap=None, resume=None):
        """Packed host keys (as probe) -> (starts uint64[V + 1], index
        uint32[min(total, cap)], step uint32[n]) over Version ordinals:
        index[starts[v]:starts[v+1]] = the ascending indices of the keys whose
        first candidate at or after resume[i] is table v, so a key is in at
        most one list (lsmb_lset_probe_walk_lists); step as probe_walk's.
        cap=None sizes index from a counting call."""
        n = _host_keys(data, offsets, key_len)[1]
        resume = self._resume(resume, n)
        step = np.empty(max(n, 1), dtype=np.uint32)
        fn = lib().lsmb_lset_probe_walk_lists

        def walk(h, p_data, op, klen, m, p_starts, p_index, c):
            return fn(h, p_data, op, klen, m, _p(resume, u32p) if resume is not None and m else None, _p(step, u32p),
                      p_starts, p_index, c)

        starts, index = self._lists(walk, self.version_tables(), data, offsets, key_len, cap)
        return starts, index, step[:n]

    def probe_walk_lists_keys(self, keys, resume=None):
        """list of bytes -> (starts, index, step) as probe_walk_lists."""
        data, offs = _pack_keys(keys)
        return self.probe_walk_lists(data, offs, resume=resume)

    def probe_walk_lists_dev(self, data, n, starts, index, work, step=None, resume=None, offsets=None, key_len=0,
                             stream=None):
        """Device keys -> device lists (lsmb_lset_probe_walk_lists_dev): starts,
        index and work as probe_version_lists_dev's, work of at least
        walk_lists_work_bytes(n) bytes; step (optional) and resume (optional)
        as probe_walk_dev's."""
        fn = lib().lsmb_lset_probe_walk_lists_dev

        def walk(h, d_data, offs, klen, m, d_starts, d_index, cap, d_work, wb, st):
            return fn(h, d_data, offs, klen, m, vp(resume.data_ptr()) if resume is not None else None,
                      vp(step.data_ptr()) if step is not None else None, d_starts, d_index, cap, d_work, wb, st)

        self._lists_dev(walk, data, n, starts, index, work, offsets, key_len, stream)


def build_strategy(num_bits, n, k=7):
    """Device build strategy for (num_bits, k, n): lds / tiled / partition / atomic."""
    return lib().lsmb_build_strategy(num_bits, k, n).decode()


def build_batch_max_bits():
    """Largest num_bits a table of a batched build may have (lsmb_build_batch_max_bits)."""
    return int(lib().lsmb_build_batch_max_bits())


def build_batch_layout(num_bits):
    """Packed layout of a batched build (lsmb_build_batch_layout): word_off,
    uint64 of len(num_bits) + 1; table t's u64 words start at word_off[t],
    word_off[-1] is the words of the whole buffer."""
    nb = np.ascontiguousarray(num_bits, dtype=np.uint32)
    woff = np.zeros(nb.size + 1, dtype=np.uint64)
    _check(lib().lsmb_build_batch_layout(nb.size, _p(nb, u32p) if nb.size else None, _p(woff, u64p)))
    return woff


def build_batch_parts(keys, num_bits):
    """Work items a batched build gives one table of this shape (lsmb_build_batch_parts)."""
    return int(lib().lsmb_build_batch_parts(int(keys), int(num_bits)))


def build_batch_sst_parts(blocks, nbytes, num_bits):
    """Work items a batched build from data blocks gives one table of this shape (lsmb_build_batch_sst_parts)."""
    return int(lib().lsmb_build_batch_sst_parts(int(blocks), int(nbytes), int(num_bits)))


def compact_sst_work_bytes(blk_len):
    """Bytes of device work buffer compact_sst_mark_dev / compact_sst_gather_dev need for blocks of these lengths
    (lsmb_compact_sst_work_bytes)."""
    bl = np.ascontiguousarray(blk_len, dtype=np.uint32)
    return int(lib().lsmb_compact_sst_work_bytes(bl.size, _p(bl, u32p) if bl.size else None))


def crc32(data, crc=0):
    """CRC-32 of host bytes (lsmb_crc32; == zlib.crc32 == crc32fast::hash)."""
    a, n = _key(data)
    return int(lib().lsmb_crc32(crc, _p(a, u8p), n))


def crc32_combine(crc_a, crc_b, len_b):
    return int(lib().lsmb_crc32_combine(crc_a, crc_b, len_b))


def build_sweeps(num_bits, n, k=7):
    """Sweeps of the device build of n keys (1 unless partitioned in several)."""
    return int(lib().lsmb_build_sweeps(num_bits, k, n))


def sweep_words(num_bits, n, sweep, k=7):
    """[word_lo, word_hi): the filter words whose bits sweep `sweep` completes."""
    lo, hi = ctypes.c_uint64(), ctypes.c_uint64()
    _check(lib().lsmb_sweep_words(num_bits, k, n, int(sweep), ctypes.byref(lo), ctypes.byref(hi)))
    return lo.value, hi.value


def host_max_keys():
    """Host-memory builds of at most this many keys run the library's host loop."""
    return int(lib().lsmb_host_max_keys())


def set_host_max_keys(n):
    lib().lsmb_set_host_max_keys(int(n))


class Multi:
    """One process, several GPUs (lsmb_multi): a sharded build merged by an
    OR reduce-scatter over xGMI peer loads.  `devices` may repeat."""

    def __init__(self, devices):
        devices = list(devices)
        h = vp()
        arr = (ctypes.c_int * len(devices))(*devices)
        _check(lib().lsmb_multi_open(ctypes.byref(h), arr, len(devices)))
        self.h = h
        self.devices = devices

    def close(self):
        if self.h:
            lib().lsmb_multi_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        return int(lib().lsmb_multi_size(self.h))

    def build_fixed_dev(self, keys, key_len, num_bits, k, words):
        """keys / words: per-shard torch tensors on the shards' devices; every
        words[g] ends holding the merged filter."""
        G = len(keys)
        karr = (vp * G)(*[vp(t.data_ptr()) for t in keys])
        warr = (vp * G)(*[vp(t.data_ptr()) for t in words])
        n = np.array([t.numel() // key_len if key_len else t.shape[0] for t in keys], dtype=np.uint64)
        _check(lib().lsmb_multi_build_fixed_dev(self.h, karr, _p(n, u64p), key_len, num_bits, k, warr))

    def build_block(self, data, num_bits, k, offsets=None, key_len=0, out=None):
        data, n, op = _host_keys(data, offsets, key_len)
        if out is None:
            out = np.empty(serialized_size(num_bits), dtype=np.uint8)
        _check(lib().lsmb_multi_build_block(self.h, _p(data, u8p), op, key_len, n, num_bits, k, _p(out, u8p),
                                            out.size))
        return out

    def last_ms(self):
        a = (ctypes.c_float * 3)()
        _check(lib().lsmb_multi_last_ms(self.h, a))
        return tuple(a)


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(-1)
    return _default_ctx


# ------------------------------------------------------------------ reference surface
class BloomFilter:
    """Mirror of `pub struct BloomFilter` (src/bloom/mod.rs:23-27): words + num_hashes + num_bits."""

    __slots__ = ("bits", "_k", "_nb")

    def __init__(self, bits, num_hashes, num_bits):
        self.bits = bits
        self._k = num_hashes
        self._nb = num_bits

    @classmethod
    def new(cls, expected_items, false_positive_rate):
        nb, k = params(expected_items, false_positive_rate)
        return cls(np.zeros(num_words(nb), dtype=np.uint64), k, nb)

    def insert(self, key):
        a, n = _key(key)
        _check(lib().lsmb_insert(_p(self.bits, u64p), self._nb, self._k, _p(a, u8p), n))

    def may_contain(self, key):
        a, n = _key(key)
        return bool(_check(lib().lsmb_may_contain(_p(self.bits, u64p), self._nb, self._k, _p(a, u8p), n)))

    def serialize(self):
        size = int(lib().lsmb_serialized_size(self._nb))
        out = np.zeros(size, dtype=np.uint8)
        _check(lib().lsmb_serialize(_p(self.bits, u64p), self._nb, self._k, _p(out, u8p), size))
        return out.tobytes()

    @classmethod
    def deserialize(cls, data):
        a, n = _key(data)
        k, nb, nw = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        _check(lib().lsmb_deserialize_header(_p(a, u8p), n, ctypes.byref(k), ctypes.byref(nb), ctypes.byref(nw)))
        words = np.zeros(nw.value, dtype=np.uint64)
        _check(lib().lsmb_deserialize(_p(a, u8p), n, _p(words, u64p), nw.value))
        return cls(words, k.value, nb.value)

    def num_hashes(self):
        return self._k

    def num_bits(self):
        return self._nb

    # additive batched API (the reference has no multi-get)
    @staticmethod
    def may_contain_batch(filters, keys, ctx=None):
        """keys: list of bytes.  Returns uint8 [len(keys), ceil(F/8)] mask (GPU)."""
        ctx = ctx or default_context()
        offs = np.zeros(len(keys) + 1, dtype=np.uint64)
        if keys:
            offs[1:] = np.cumsum([len(k) for k in keys])
        data = np.frombuffer(b"".join(bytes(k) for k in keys), dtype=np.uint8)
        return ctx.probe([(f.bits, f._nb, f._k) for f in filters], data, offs)


class BloomFilterBuilder:
    """Mirror of `BloomFilterBuilder` (src/bloom/builder.rs:8-28).

    The reference inserts on the fly (builder.rs:21-23); this one buffers the
    run's keys in a packed arena and builds the whole filter in one GPU batch
    at `build()`.  The bits are identical.
    """

    def __init__(self, filt, ctx=None):
        self._filter = filt
        self._data = bytearray()
        self._offs = [0]
        self._ctx = ctx

    @classmethod
    def new(cls, estimated_keys, false_positive_rate, ctx=None):
        return cls(BloomFilter.new(estimated_keys, false_positive_rate), ctx)

    def add_key(self, key):
        self._data += bytes(key)
        self._offs.append(len(self._data))

    def _ctx_for(self, n):
        """The device context a build of n keys needs: None at or below the
        library's host threshold (SST-sized flushes stay on the host, no GPU
        required), else the GPU context (raises without a gfx950 device)."""
        if n <= host_max_keys():
            return None
        return self._ctx or default_context()

    def build(self):
        f = self._filter
        n = len(self._offs) - 1
        if n:
            ctx = self._ctx_for(n)
            offs = np.array(self._offs, dtype=np.uint64)
            data = np.frombuffer(bytes(self._data) or b"\0", dtype=np.uint8)
            _check(lib().lsmb_build_var(ctx.h if ctx else None, _p(data, u8p), _p(offs, u64p), n, f._nb, f._k,
                                        _p(f.bits, u64p)))
        return f

    def build_serialized(self):
        """build().serialize() in one call (lsmb_build_block): the bloom block
        SSTableBuilder::finish writes (src/sstable/builder.rs:177-179)."""
        f = self._filter
        n = len(self._offs) - 1
        ctx = self._ctx_for(n)
        offs = np.array(self._offs, dtype=np.uint64)
        data = np.frombuffer(bytes(self._data) or b"\0", dtype=np.uint8)
        out = np.empty(serialized_size(f._nb), dtype=np.uint8)
        _check(lib().lsmb_build_block(ctx.h if ctx else None, _p(data, u8p), _p(offs, u64p), 0, n, f._nb, f._k,
                                      _p(out, u8p), out.size))
        return out.tobytes()
