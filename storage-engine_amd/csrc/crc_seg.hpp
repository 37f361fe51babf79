// crc_seg.hpp — the arithmetic of the CRC-32 kernels (crc32.hip), free of HIP
// so that tests/cpp/crc_seg_test.cpp can drive it on a CPU: the GF(2)[x] mod P
// products behind crc32_combine, the slicing-by-4 step over a piece, the piece
// geometry of the segmented kernel (k_crc32_seg: one wave per segment) and
// crc_seg_ref, a serial walk over the same pieces and the same combine tree as
// the kernel's 64 lanes.  Internal.
#pragma once

#include <stdint.h>
#include <string.h>

#ifndef LSMB_HD
#if defined(__HIPCC__)  // in the library: as xxh3.hpp has it
#include <hip/hip_runtime.h>
#define LSMB_HD __host__ __device__ __forceinline__
#else
#define LSMB_HD inline
#endif
#endif

namespace lsmb {

// CRC-32 (IEEE 802.3, reflected, poly 0xEDB88320, init and xorout 0xFFFFFFFF):
// `crc32fast::hash` of the store (src/wal/record.rs:96,122).
constexpr uint32_t kCrcPoly = 0xEDB88320u;

// a·b mod P, reflected bit order (bit 31 = x^0).
LSMB_HD uint32_t multmodp(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m && a; m >>= 1) {
        if (a & m) {
            p ^= b;
            a ^= m;
        }
        b = (b & 1) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}

// x^(8 n) mod P: square-and-multiply over x^(8·2^k) (x^8 = bit 31 - 8).
LSMB_HD uint32_t x8nmodp(uint64_t n) {
    uint32_t x2k = 1u << 23;  // x^8
    uint32_t p = 1u << 31;    // x^0
    while (n) {
        if (n & 1) p = multmodp(x2k, p);
        n >>= 1;
        x2k = multmodp(x2k, x2k);
    }
    return p;
}

// CRC(A‖B) from CRC(A), CRC(B) and |B| (standard, pre/post-inverted CRCs).
LSMB_HD uint32_t crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
    return multmodp(x8nmodp(len_b), crc_a) ^ crc_b;
}

// Slicing-by-4 tables: t[0] the byte table, t[s][i] = t[0][i] advanced s bytes.
struct CrcTables {
    uint32_t t[4][256];
};

inline void crc_make_tables(CrcTables& T) {
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i;
        for (int j = 0; j < 8; j++) c = (c & 1) ? (c >> 1) ^ kCrcPoly : c >> 1;
        T.t[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; i++)
        for (int s = 1; s < 4; s++) T.t[s][i] = (T.t[s - 1][i] >> 8) ^ T.t[0][T.t[s - 1][i] & 0xFF];
}

inline const CrcTables& crc_tables() {
    static const CrcTables T = [] {
        CrcTables t;
        crc_make_tables(t);
        return t;
    }();
    return T;
}

LSMB_HD uint32_t crc_step4(const uint32_t (*t)[256], uint32_t c, uint32_t w) {
    const uint32_t x = c ^ w;
    return t[3][x & 0xFF] ^ t[2][(x >> 8) & 0xFF] ^ t[1][(x >> 16) & 0xFF] ^ t[0][x >> 24];
}

// The standard CRC-32 of the n bytes at p (0 for none), over tables t (LDS in
// the kernel).  aligned16: p is 16-byte aligned, so whole 16-byte groups are
// read as one 16-byte load; else byte by byte.
LSMB_HD uint32_t crc_piece(const uint32_t (*t)[256], const uint8_t* p, uint64_t n, bool aligned16) {
    uint32_t c = 0xFFFFFFFFu;
    uint64_t i = 0;
    if (aligned16)
        for (; i + 16 <= n; i += 16) {
            uint32_t v[4];
            memcpy(v, __builtin_assume_aligned(p + i, 16), 16);
            c = crc_step4(t, c, v[0]);
            c = crc_step4(t, c, v[1]);
            c = crc_step4(t, c, v[2]);
            c = crc_step4(t, c, v[3]);
        }
    for (; i < n; i++) c = t[0][(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

// ---- the segmented kernel's geometry ----------------------------------------
// One wave of kCrcSegLanes lanes per segment.  The segment is cut into pieces
// of P bytes from its start, P = the smallest multiple of 16 with 64·P >= len
// (16 for an empty segment): nfull whole pieces, then a tail of fewer than P
// bytes.  Every piece starts 16-byte aligned when the segment does.
//
// The whole pieces sit RIGHT-justified in the wave: piece j on lane
// 64 - nfull + j, the lanes before them empty.  CRC(empty) = 0 and
// CRC(A‖B) = CRC(A)·x^(8|B|) ⊕ CRC(B) holds for any factor when A is empty, so
// in the tree every right-hand run is complete and one factor per level serves
// all lanes: x^(8·P·2^l), each the square of the one before.  The tail is
// CRC'd by the lane before the first whole piece (free unless nfull == 64, and
// then there is no tail), kept out of the tree and appended at the end with
// the segment's only length-dependent factor, x^(8·tail).
// Segments up to kCrcSegWaveMax bytes (P <= 2048) are the kernel's design
// range; a longer one is still exact, on one wave.
constexpr uint32_t kCrcSegLanes = 64;
constexpr uint32_t kCrcSegLevels = 6;                    // log2(kCrcSegLanes)
constexpr uint32_t kCrcSegPerBlock = 4;                  // waves, so segments, per workgroup
constexpr uint64_t kCrcSegWaveMax = 128u << 10;          // above: k_crc32, a workgroup per 128 KiB

struct CrcSeg {
    const uint8_t* p;  // 16-byte aligned for the wide loads (any alignment is exact)
    uint64_t len;
};

struct CrcSegGeom {
    uint64_t P;       // bytes per whole piece
    uint32_t nfull;   // whole pieces, <= 64
    uint64_t tail;    // len - nfull·P, < P
};

LSMB_HD CrcSegGeom crc_seg_geom(uint64_t len) {
    CrcSegGeom g;
    g.P = ((len + kCrcSegLanes - 1) / kCrcSegLanes + 15) & ~(uint64_t)15;
    if (g.P == 0) g.P = 16;
    g.nfull = (uint32_t)(len / g.P);
    g.tail = len - (uint64_t)g.nfull * g.P;
    return g;
}

// Lane `lane`'s bytes: [*off, *off + n) of the segment; n == 0 for an empty lane.
LSMB_HD uint64_t crc_seg_lane(const CrcSegGeom& g, uint32_t lane, uint64_t* off) {
    const uint32_t first = kCrcSegLanes - g.nfull;  // the first whole piece's lane
    *off = 0;
    if (lane >= first) {
        *off = (uint64_t)(lane - first) * g.P;
        return g.P;
    }
    if (g.tail && lane + 1 == first) {
        *off = (uint64_t)g.nfull * g.P;
        return g.tail;
    }
    return 0;
}
LSMB_HD bool crc_seg_is_tail_lane(const CrcSegGeom& g, uint32_t lane) {
    return g.tail && lane + 1 == kCrcSegLanes - g.nfull;
}

// One step of the wave's tree: `mine` is the CRC of a lane's run of 2^l
// pieces (or of nothing), `right` that of the complete run after it,
// pw = x^(8·P·2^l).
LSMB_HD uint32_t crc_seg_merge(uint32_t mine, uint32_t right, uint32_t pw) { return multmodp(pw, mine) ^ right; }

// The tree's result and the tail's CRC -> the segment's.
LSMB_HD uint32_t crc_seg_finish(const CrcSegGeom& g, uint32_t whole, uint32_t tail_crc) {
    return g.tail ? multmodp(x8nmodp(g.tail), whole) ^ tail_crc : whole;
}

// The kernel, serially: the 64 lanes' CRCs, the tail's taken out, then the
// tree level by level (lane j with j % 2^(l+1) == 0 merges with lane j + 2^l).
// Equals crc32 of the segment.
inline uint32_t crc_seg_ref(const uint8_t* p, uint64_t len) {
    const CrcTables& T = crc_tables();
    const CrcSegGeom g = crc_seg_geom(len);
    const bool al = (reinterpret_cast<uintptr_t>(p) & 15) == 0;
    uint32_t part[kCrcSegLanes], tail_crc = 0;
    for (uint32_t lane = 0; lane < kCrcSegLanes; lane++) {
        uint64_t off;
        const uint64_t n = crc_seg_lane(g, lane, &off);
        part[lane] = crc_piece(T.t, p + off, n, al);
        if (crc_seg_is_tail_lane(g, lane)) {
            tail_crc = part[lane];
            part[lane] = 0;
        }
    }
    uint32_t pw = x8nmodp(g.P);
    for (uint32_t l = 0; l < kCrcSegLevels; l++) {
        const uint32_t step = 1u << l;
        for (uint32_t lane = 0; lane < kCrcSegLanes; lane += 2 * step)
            part[lane] = crc_seg_merge(part[lane], part[lane + step], pw);
        pw = multmodp(pw, pw);
    }
    return crc_seg_finish(g, part[0], tail_crc);
}

}  // namespace lsmb
