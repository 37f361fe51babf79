// crc32.hip — CRC-32 (IEEE 802.3, reflected, poly 0xEDB88320, init and
// xorout 0xFFFFFFFF) of bloom blocks: the checksum the store already uses for
// its WAL records and manifest (`crc32fast::hash`, src/wal/record.rs:96,122,
// src/manifest/mod.rs:5), here as the optional integrity check of the
// serialized filter that SURVEY.md §8 f4 lists (the reference's bloom block
// carries none).
//
// Device: each lane CRCs a 512-B piece with slicing-by-4 tables in LDS; the
// workgroup combines its 256 pieces in a tree (CRC(A‖B) = CRC(A)·x^(8|B|) ⊕
// CRC(B) in GF(2)[x] mod P, the combine of zlib's crc32_combine); the host
// combines the workgroups' CRCs in order.  A 120 MB C2 block is 915 workgroups.
//
// Many small blocks (a level set's SSTable filters, ~1 KB each): k_crc32_seg,
// one wave per segment and four segments per workgroup, the wave's 64 pieces
// combined in a shuffle tree, every segment's CRC from one launch.  The
// products, the piece geometry and a serial statement of the tree are in
// crc_seg.hpp, where a CPU test drives them.
#include <string.h>

#include <vector>

#include "crc_seg.hpp"
#include "ctx.hpp"

namespace lsmb {
namespace {

constexpr uint32_t kCrcLanes = 256, kCrcPiece = 512;         // bytes per lane
constexpr uint64_t kCrcBlock = (uint64_t)kCrcLanes * kCrcPiece;  // bytes per workgroup
static_assert(kCrcBlock == kCrcSegWaveMax, "segments past k_crc32_seg's range are whole k_crc32 blocks");

// The x^(8·512·2^l) factors of the workgroup tree (l = 0..7), for full pieces.
struct TreePowers {
    uint32_t p[8];
};

TreePowers tree_powers() {
    TreePowers tp;
    for (int l = 0; l < 8; l++) tp.p[l] = x8nmodp((uint64_t)kCrcPiece << l);
    return tp;
}

// Workgroup w: CRC of bytes [w·128 KiB, min((w+1)·128 KiB, len)).
__global__ __launch_bounds__(kCrcLanes) void k_crc32(const uint8_t* __restrict__ d, uint64_t len, TreePowers tp,
                                                     uint32_t* __restrict__ out) {
    __shared__ uint32_t t[4][256];
    __shared__ uint32_t part[kCrcLanes];
    const uint32_t lane = threadIdx.x;
    {  // slicing-by-4 tables, one entry per lane
        uint32_t c0 = lane;
        for (int j = 0; j < 8; j++) c0 = (c0 & 1) ? (c0 >> 1) ^ kCrcPoly : c0 >> 1;
        t[0][lane] = c0;
        __syncthreads();
        for (int s = 1; s < 4; s++) {
            t[s][lane] = (t[s - 1][lane] >> 8) ^ t[0][t[s - 1][lane] & 0xFF];
            __syncthreads();
        }
    }
    const uint64_t base = (uint64_t)blockIdx.x * kCrcBlock;
    const uint64_t a = base + (uint64_t)lane * kCrcPiece;
    const uint64_t e = a + kCrcPiece < len ? a + kCrcPiece : len;
    uint32_t c = 0xFFFFFFFFu;
    uint64_t i = a;
    if (a < e) {
        // 4 bytes per step (slicing-by-4); the piece start is 512-B aligned
        // from d: 16-B loads where d is 16-B aligned, dword loads where it is
        // only 4-B aligned (a uint4 access must be 16-B aligned), else the
        // byte loop
        auto step4 = [&](uint32_t w) {
            const uint32_t x = c ^ w;
            c = t[3][x & 0xFF] ^ t[2][(x >> 8) & 0xFF] ^ t[1][(x >> 16) & 0xFF] ^ t[0][x >> 24];
        };
        const uintptr_t al = reinterpret_cast<uintptr_t>(d);
        if ((al & 15) == 0) {
            for (; i + 16 <= e; i += 16) {
                const uint4 v = *reinterpret_cast<const uint4*>(d + i);
                step4(v.x), step4(v.y), step4(v.z), step4(v.w);
            }
        } else if ((al & 3) == 0) {
            for (; i + 16 <= e; i += 16) {
                const uint32_t* q = reinterpret_cast<const uint32_t*>(d + i);
                const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
                step4(w0), step4(w1), step4(w2), step4(w3);
            }
        }
        for (; i < e; i++) c = t[0][(c ^ d[i]) & 0xFF] ^ (c >> 8);
    }
    part[lane] = c ^ 0xFFFFFFFFu;
    __syncthreads();
    // tree: at level l, lane j (j % 2^(l+1) == 0) combines its run with the
    // run starting 2^l pieces later (length: full, or the tail's actual bytes)
    for (uint32_t l = 0; (1u << l) < kCrcLanes; l++) {
        const uint32_t step = 1u << l;
        if ((lane & (2 * step - 1)) == 0 && lane + step < kCrcLanes) {
            const uint64_t rb = a + (uint64_t)step * kCrcPiece;  // right run's first byte
            if (rb < len) {
                const uint64_t re = rb + (uint64_t)step * kCrcPiece;
                const uint64_t rlen = (re < len ? re : len) - rb;
                const uint32_t f = rlen == ((uint64_t)kCrcPiece << l) ? tp.p[l] : x8nmodp(rlen);
                part[lane] = multmodp(f, part[lane]) ^ part[lane + step];
            }
        }
        __syncthreads();
    }
    if (lane == 0) out[blockIdx.x] = part[0];
}

// Wave w of workgroup b: out[s] = CRC-32 of segment s = 4 b + w (crc_seg.hpp:
// the whole pieces right-justified on the lanes, six shuffle levels with one
// factor each, the tail appended last; crc_seg_ref is this, serially).
__global__ __launch_bounds__(kCrcSegLanes* kCrcSegPerBlock) void k_crc32_seg(const CrcSeg* __restrict__ segs,
                                                                              uint64_t nseg,
                                                                              uint32_t* __restrict__ out) {
    __shared__ uint32_t t[4][256];
    static_assert(kCrcSegLanes * kCrcSegPerBlock == 256, "one table entry per lane");
    {  // slicing-by-4 tables, one entry per lane
        const uint32_t i = threadIdx.x;
        uint32_t c0 = i;
        for (int j = 0; j < 8; j++) c0 = (c0 & 1) ? (c0 >> 1) ^ kCrcPoly : c0 >> 1;
        t[0][i] = c0;
        __syncthreads();
        for (int s = 1; s < 4; s++) {
            t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 0xFF];
            __syncthreads();
        }
    }
    const uint32_t lane = threadIdx.x % kCrcSegLanes;
    const uint64_t s = (uint64_t)blockIdx.x * kCrcSegPerBlock + threadIdx.x / kCrcSegLanes;
    if (s >= nseg) return;  // whole waves, after the last barrier
    const CrcSeg sg = segs[s];
    const CrcSegGeom g = crc_seg_geom(sg.len);
    uint64_t off;
    const uint64_t n = crc_seg_lane(g, lane, &off);
    const bool al = (reinterpret_cast<uintptr_t>(sg.p) & 15) == 0;
    uint32_t c = crc_piece(t, sg.p + off, n, al);
    // the tail's CRC to every lane and out of the tree (lane 0 when there is none: unused)
    const uint32_t tail_crc = __shfl(c, g.tail ? (int)(kCrcSegLanes - g.nfull - 1) : 0);
    if (crc_seg_is_tail_lane(g, lane)) c = 0;
    uint32_t pw = x8nmodp(g.P);
    for (uint32_t l = 0; l < kCrcSegLevels; l++) {
        const uint32_t step = 1u << l;
        const uint32_t right = __shfl_down(c, step);  // all 64 lanes take part
        if ((lane & (2 * step - 1)) == 0) c = crc_seg_merge(c, right, pw);
        if (l + 1 < kCrcSegLevels) pw = multmodp(pw, pw);
    }
    if (lane == 0) out[s] = crc_seg_finish(g, c, tail_crc);
}

}  // namespace

// out[s] = CRC-32 of the device bytes segs[s] (segs and out in device memory),
// one launch on st; nothing is synchronised.
int crc32_seg_dev(const CrcSeg* d_segs, uint64_t nseg, uint32_t* d_out, hipStream_t st) {
    if (nseg == 0) return LSMB_OK;
    const uint64_t nwg = (nseg + kCrcSegPerBlock - 1) / kCrcSegPerBlock;
    if (nwg > 0x7FFFFFFFull) return fail(LSMB_EINVAL, "crc32: %llu segments are too many", (unsigned long long)nseg);
    k_crc32_seg<<<dim3((uint32_t)nwg), dim3(kCrcSegLanes * kCrcSegPerBlock), 0, st>>>(d_segs, nseg, d_out);
    HIP_TRY(hipGetLastError());
    return LSMB_OK;
}

uint32_t crc32_host(const uint8_t* p, uint64_t len, uint32_t crc) {
    const CrcTables& T = crc_tables();
    uint32_t c = ~crc;
    uint64_t i = 0;
    for (; i + 4 <= len; i += 4) {
        uint32_t w;
        memcpy(&w, p + i, 4);
        const uint32_t x = c ^ w;
        c = T.t[3][x & 0xFF] ^ T.t[2][(x >> 8) & 0xFF] ^ T.t[1][(x >> 16) & 0xFF] ^ T.t[0][x >> 24];
    }
    for (; i < len; i++) c = T.t[0][(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return ~c;
}

uint32_t crc32_combine_host(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return crc_combine(crc_a, crc_b, len_b); }

// CRC-32 of device bytes, appended to `crc` (the CRC of the bytes before them;
// 0 for none).  Enqueued on st, then synchronised (the partials come back).
int crc32_dev(lsmb_ctx* c, const uint8_t* d, uint64_t len, uint32_t crc, hipStream_t st, uint32_t* out) {
    if (len == 0) {
        *out = crc;
        return LSMB_OK;
    }
    const uint64_t nwg = (len + kCrcBlock - 1) / kCrcBlock;
    if (nwg > 0x7FFFFFFFull) return fail(LSMB_EINVAL, "crc32: %llu bytes is too long", (unsigned long long)len);
    HIP_TRY(c->crc_parts.ensure(nwg * 4));
    static const TreePowers tp = tree_powers();
    k_crc32<<<dim3((uint32_t)nwg), dim3(kCrcLanes), 0, st>>>(d, len, tp, (uint32_t*)c->crc_parts.p);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> parts(nwg);
    HIP_TRY(hipMemcpyAsync(parts.data(), c->crc_parts.p, nwg * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    static const uint32_t full = x8nmodp(kCrcBlock);
    uint32_t r = crc;
    for (uint64_t w = 0; w < nwg; w++) {
        const uint64_t blen = w + 1 < nwg ? kCrcBlock : len - w * kCrcBlock;
        r = multmodp(blen == kCrcBlock ? full : x8nmodp(blen), r) ^ parts[w];
    }
    *out = r;
    return LSMB_OK;
}

}  // namespace lsmb

using namespace lsmb;

extern "C" {

uint32_t lsmb_crc32(uint32_t crc, const uint8_t* data, uint64_t len) {
    if (!data || !len) return crc;
    return crc32_host(data, len, crc);
}

uint32_t lsmb_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return crc32_combine_host(crc_a, crc_b, len_b); }

int lsmb_crc32_dev(lsmb_ctx* c, uint32_t crc, const void* d_data, uint64_t len, uint32_t* out, void* stream) {
    if (!c || !out) return fail(LSMB_EINVAL, "null argument");
    if (len && !d_data) return fail(LSMB_EINVAL, "null device pointer");
    DevGuard g(c->dev);
    return crc32_dev(c, (const uint8_t*)d_data, len, crc, stream ? (hipStream_t)stream : c->st, out);
}

int lsmb_crc32_seg_dev(lsmb_ctx* c, const void* d_segs, uint64_t nseg, void* d_out, void* stream) {
    static_assert(sizeof(CrcSeg) == 16, "the ABI's (pointer, length) pairs");
    if (!c) return fail(LSMB_EINVAL, "null argument");
    if (nseg && (!d_segs || !d_out)) return fail(LSMB_EINVAL, "null device pointer");
    DevGuard g(c->dev);
    return crc32_seg_dev((const CrcSeg*)d_segs, nseg, (uint32_t*)d_out, stream ? (hipStream_t)stream : c->st);
}

}  // extern "C"
