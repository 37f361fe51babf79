// lset_arena_test.cpp — the level set's arena placement
// (storage-engine_amd/csrc/lset_arena.hpp): lset_place, which plans a whole
// batch without touching anything, against the bump allocator it replaced,
// restated here as it was: one table at a time, mutating its arena.  Every
// result is also held against what an arena must guarantee (aligned, disjoint
// slots inside their chunks; spans that tile the tables; packed offsets equal
// to the batched build's layout) and against arena_chunks of
// tests/test_lset_versions.py, restated.  No HIP: a stand-alone host program
// (tests/test_lset_versions.py builds it with -fsanitize=address,undefined and
// runs it).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../storage-engine_amd/csrc/lset_arena.hpp"

using namespace lsmb;

static int g_fail = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            g_fail++;                                                       \
        }                                                                   \
    } while (0)

constexpr size_t CHUNK = 4u << 20;
constexpr uint64_t kChunkWords = CHUNK / 8;  // 524 288

static size_t slot_of(uint64_t nw) { return (std::max<size_t>(nw * 8, 8) + 15) / 16 * 16; }

// The arena as the add paths used to drive it: a slot per call, a chunk
// allocated the moment a slot does not fit.
struct RefArena {
    size_t chunks = 0, used = 0, cap = 0;
    bool own_tail = false;
    std::vector<size_t> allocated;  // capacities of the chunks these calls allocated
    explicit RefArena(const LsetArenaState& s) : chunks(s.chunks), used(s.used), cap(s.cap), own_tail(s.own_tail) {}
    bool alloc(uint64_t nw, uint32_t* chunk, size_t* off) {
        const size_t bytes = slot_of(nw);
        if (!own_tail || used + bytes > cap) {
            if (chunks >= UINT32_MAX) return false;  // "level set arena is full"
            cap = std::max(bytes, CHUNK);
            allocated.push_back(cap);
            chunks++;
            used = 0;
            own_tail = true;
        }
        *chunk = (uint32_t)(chunks - 1);
        *off = used;
        used += bytes;
        return true;
    }
};

// arena_chunks of tests/test_lset_versions.py: chunks a fresh set touches.
static size_t arena_chunks(const std::vector<uint64_t>& nwords) {
    size_t chunks = 0, used = 0, cap = 0;
    for (uint64_t nw : nwords) {
        const size_t b = slot_of(nw);
        if (chunks == 0 || used + b > cap) {
            chunks++;
            used = 0;
            cap = std::max(b, CHUNK);
        }
        used += b;
    }
    return chunks;
}

// bb_layout of build_batch_plan.hpp over word counts: max(nw, 1) words rounded up to an even count.
static std::vector<uint64_t> layout_words(const std::vector<uint64_t>& nw) {
    std::vector<uint64_t> off(nw.size() + 1, 0);
    for (size_t t = 0; t < nw.size(); t++) off[t + 1] = off[t] + ((std::max<uint64_t>(nw[t], 1) + 1) & ~(uint64_t)1);
    return off;
}

static bool same(const LsetArenaState& a, const LsetArenaState& b) {
    return a.chunks == b.chunks && a.own_tail == b.own_tail && a.used == b.used && a.cap == b.cap;
}

// One batch from state s: lset_place against the reference loop, then every
// invariant, then the same tables as single placements.  Returns the state
// after (s itself when the arena refuses the batch); *placed says which.
static LsetArenaState check_batch(const LsetArenaState& s, const std::vector<uint64_t>& nw, bool* placed = nullptr) {
    const size_t ntab = nw.size();
    RefArena ref(s);
    std::vector<uint32_t> rchunk(ntab);
    std::vector<size_t> roff(ntab);
    bool fits = true;
    for (size_t t = 0; t < ntab && fits; t++) fits = ref.alloc(nw[t], &rchunk[t], &roff[t]);

    static LsetPlacement pl;  // as the library keeps it: the last call's result must not show in this one
    const LsetArenaState s0 = s;
    const bool ok = lset_place(s, nw.data(), ntab, &pl);
    CHECK(same(s, s0));
    CHECK(ok == fits);
    if (placed) *placed = ok;
    if (!ok || !fits) return s;  // a refused batch: *out is of no use, the state is the caller's to keep

    // the reference's decisions, exactly
    CHECK(pl.slot.size() == ntab);
    for (size_t t = 0; t < ntab && t < pl.slot.size(); t++)
        CHECK(pl.slot[t].chunk == rchunk[t] && pl.slot[t].off == roff[t]);
    CHECK(pl.new_chunks == ref.allocated);
    CHECK(pl.after.chunks == ref.chunks && pl.after.used == ref.used && pl.after.own_tail == ref.own_tail);
    CHECK(pl.after.cap == ref.cap);
    if (ntab == 0) CHECK(same(pl.after, s) && pl.packed_bytes() == 0 && pl.spans.empty());
    if (pl.slot.size() != ntab) return pl.after;

    // slots: 16-byte aligned, inside their chunk, disjoint (bump order), never in an inherited tail
    auto chunk_cap = [&](uint32_t c) -> size_t {
        if (c >= s.chunks) return c - s.chunks < pl.new_chunks.size() ? pl.new_chunks[c - s.chunks] : 0;
        return s.cap;  // only the tail is ever written
    };
    for (size_t t = 0; t < ntab; t++) {
        const LsetSlot& sl = pl.slot[t];
        const size_t bytes = slot_of(nw[t]);
        CHECK(bytes == lset_slot_bytes(nw[t]) && bytes % 16 == 0 && bytes >= nw[t] * 8 && bytes >= 16);
        CHECK(sl.off % 16 == 0);
        CHECK(sl.off + bytes <= chunk_cap(sl.chunk));
        if (sl.chunk < s.chunks) {
            CHECK(s.own_tail && sl.chunk == s.chunks - 1 && sl.off >= s.used);
        } else if (sl.off == 0) {  // opens a new chunk: 4 MiB, or exactly its own slot when that is larger
            CHECK(chunk_cap(sl.chunk) == std::max(bytes, CHUNK));
        }
        if (t == 0) continue;
        const LsetSlot& pv = pl.slot[t - 1];
        if (sl.chunk == pv.chunk)
            CHECK(sl.off == pv.off + slot_of(nw[t - 1]));
        else
            CHECK(sl.chunk == pv.chunk + 1 && sl.off == 0);
    }
    for (size_t c = 0; c < pl.new_chunks.size(); c++) CHECK(pl.new_chunks[c] >= CHUNK);

    // spans: maximal runs that tile the tables in order; bytes = their slots; src = the packed offset
    const std::vector<uint64_t> woff = layout_words(nw);
    size_t t = 0, packed = 0;
    for (size_t i = 0; i < pl.spans.size(); i++) {
        const LsetSpan& sp = pl.spans[i];
        CHECK(t < ntab);
        if (t >= ntab) break;
        CHECK(sp.chunk == pl.slot[t].chunk && sp.off == pl.slot[t].off);
        CHECK(sp.src == packed && sp.src == woff[t] * 8);
        if (i) CHECK(sp.chunk != pl.spans[i - 1].chunk);
        size_t bytes = 0;
        while (t < ntab && pl.slot[t].chunk == sp.chunk) {
            CHECK(packed == woff[t] * 8);
            bytes += slot_of(nw[t]);
            packed += slot_of(nw[t]);
            t++;
        }
        CHECK(sp.bytes == bytes && sp.bytes > 0);
    }
    CHECK(t == ntab);
    CHECK(pl.packed_bytes() == packed && packed == woff[ntab] * 8);

    // the chunks of the batch, counted as the Python tests count them
    // (a set with no chunk of its own yet; chains of batches are counted in test_random)
    if (!s.own_tail) CHECK(pl.after.chunks == s.chunks + arena_chunks(nw));

    // the same tables one placement at a time
    LsetArenaState one = s;
    std::vector<size_t> one_chunks;
    for (size_t u = 0; u < ntab; u++) {
        LsetPlacement p1;
        const bool ok1 = lset_place(one, &nw[u], 1, &p1);
        CHECK(ok1);
        if (!ok1) break;
        CHECK(p1.slot.size() == 1 && p1.slot[0].chunk == pl.slot[u].chunk && p1.slot[0].off == pl.slot[u].off);
        CHECK(p1.spans.size() == 1 && p1.spans[0].src == 0 && p1.spans[0].bytes == slot_of(nw[u]));
        one_chunks.insert(one_chunks.end(), p1.new_chunks.begin(), p1.new_chunks.end());
        one = p1.after;
    }
    CHECK(same(one, pl.after) && one_chunks == pl.new_chunks);
    return pl.after;
}

static const LsetArenaState kFresh{};

static void test_small() {
    check_batch(kFresh, {});  // a batch of none
    LsetArenaState a = check_batch(kFresh, {0});
    CHECK(a.chunks == 1 && a.own_tail && a.used == 16 && a.cap == CHUNK);  // no words: a 16-byte slot
    a = check_batch(kFresh, {1, 2, 3});
    CHECK(a.chunks == 1 && a.used == 16 + 16 + 32);
    a = check_batch(a, {});
    CHECK(a.chunks == 1 && a.used == 64);
    a = check_batch(a, {3, 0, 1});
    CHECK(a.chunks == 1 && a.used == 64 + 32 + 16 + 16);
    CHECK(lset_slot_bytes(0) == 16 && lset_slot_bytes(1) == 16 && lset_slot_bytes(2) == 16 && lset_slot_bytes(3) == 32);
}

static void test_chunk_end() {
    // a run that ends exactly on the 4 MiB boundary still fits; one word more takes the next chunk
    LsetArenaState a = check_batch(kFresh, {kChunkWords / 2, kChunkWords / 2});
    CHECK(a.chunks == 1 && a.used == CHUNK);
    a = check_batch(kFresh, {kChunkWords / 2, kChunkWords / 2, 1});
    CHECK(a.chunks == 2 && a.used == 16);
    a = check_batch(kFresh, {kChunkWords / 2, kChunkWords / 2 - 1});  // the padding reaches the boundary
    CHECK(a.chunks == 1 && a.used == CHUNK);
    a = check_batch(kFresh, {kChunkWords / 2, kChunkWords / 2 - 1, 0});
    CHECK(a.chunks == 2 && a.used == 16);
    a = check_batch(kFresh, {kChunkWords / 2, kChunkWords / 2 + 1});
    CHECK(a.chunks == 2 && a.used == CHUNK / 2 + 16);
    std::vector<uint64_t> many(CHUNK / 16, 2);  // 262 144 slots of 16 bytes
    a = check_batch(kFresh, many);
    CHECK(a.chunks == 1 && a.used == CHUNK);
    many.push_back(1);
    a = check_batch(kFresh, many);
    CHECK(a.chunks == 2 && a.used == 16);
    // the same across calls
    a = check_batch(check_batch(kFresh, {kChunkWords / 2}), {kChunkWords / 2});
    CHECK(a.chunks == 1 && a.used == CHUNK);
    a = check_batch(a, {0});
    CHECK(a.chunks == 2 && a.used == 16);
}

static void test_large() {
    const uint64_t big[2] = {kChunkWords, kChunkWords + 1};  // exactly 4 MiB, and a chunk of its own size
    for (uint64_t b : big) {
        const size_t bytes = slot_of(b);
        LsetPlacement pl;
        // first
        CHECK(lset_place(kFresh, std::vector<uint64_t>{b, 1, 1}.data(), 3, &pl));
        CHECK(pl.new_chunks == (std::vector<size_t>{bytes, CHUNK}) && pl.slot[1].chunk == 1 && pl.slot[2].off == 16);
        LsetArenaState a = check_batch(kFresh, {b, 1, 1});
        CHECK(a.chunks == 2 && a.cap == CHUNK);
        // last
        CHECK(lset_place(kFresh, std::vector<uint64_t>{1, 1, b}.data(), 3, &pl));
        CHECK(pl.new_chunks == (std::vector<size_t>{CHUNK, bytes}) && pl.slot[2].chunk == 1 && pl.slot[2].off == 0);
        a = check_batch(kFresh, {1, 1, b});
        CHECK(a.chunks == 2 && a.cap == bytes && a.used == bytes);
        a = check_batch(a, {0});  // a full chunk of its own: the next slot opens another
        CHECK(a.chunks == 3 && a.cap == CHUNK);
        // in the middle
        CHECK(lset_place(kFresh, std::vector<uint64_t>{1, b, 1}.data(), 3, &pl));
        CHECK(pl.new_chunks == (std::vector<size_t>{CHUNK, bytes, CHUNK}) && pl.spans.size() == 3);
        a = check_batch(kFresh, {1, b, 1});
        CHECK(a.chunks == 3);
        // alone, and twice
        a = check_batch(kFresh, {b});
        CHECK(a.chunks == 1 && a.cap == bytes);
        a = check_batch(kFresh, {b, b});
        CHECK(a.chunks == 2);
    }
    CHECK(slot_of(kChunkWords) == CHUNK && slot_of(kChunkWords + 1) == CHUNK + 16);
}

static void test_inherited_tail() {
    // a derived set: three chunks of its parent's, the last half used; it is never written
    LsetArenaState s;
    s.chunks = 3;
    s.own_tail = false;
    s.used = CHUNK / 2;
    s.cap = CHUNK;
    LsetPlacement pl;
    const uint64_t one = 1;
    CHECK(lset_place(s, &one, 1, &pl));
    CHECK(pl.slot[0].chunk == 3 && pl.slot[0].off == 0 && pl.new_chunks == std::vector<size_t>{CHUNK});
    LsetArenaState a = check_batch(s, {1, 2, 3});
    CHECK(a.chunks == 4 && a.own_tail && a.used == 64 && a.cap == CHUNK);
    a = check_batch(s, {});
    CHECK(same(a, s));
    a = check_batch(s, {kChunkWords + 1, 0});
    CHECK(a.chunks == 5);
    s.chunks = 0;  // a child that kept no table of its parent's
    s.used = 0;
    s.cap = 0;
    a = check_batch(s, {0});
    CHECK(a.chunks == 1);
}

static void test_full() {
    LsetArenaState s;
    s.chunks = UINT32_MAX;
    s.own_tail = true;
    s.used = CHUNK - 32;
    s.cap = CHUNK;
    bool placed = false;
    check_batch(s, {}, &placed);
    CHECK(placed);
    LsetArenaState a = check_batch(s, {1, 1}, &placed);  // room in the tail: no chunk asked for
    CHECK(placed && a.chunks == UINT32_MAX && a.used == CHUNK);
    a = check_batch(s, {1, 1, 1}, &placed);
    CHECK(!placed && same(a, s));
    a = check_batch(s, {3}, &placed);
    CHECK(placed && a.used == CHUNK);
    check_batch(s, {3, 1}, &placed);
    CHECK(!placed);
    a = check_batch(s, {kChunkWords}, &placed);
    CHECK(!placed);
    s.own_tail = false;
    check_batch(s, {}, &placed);
    CHECK(placed);
    check_batch(s, {0}, &placed);
    CHECK(!placed);
    s.chunks = UINT32_MAX - 1;  // one more chunk, not two
    a = check_batch(s, {1, 1}, &placed);
    CHECK(placed && a.chunks == UINT32_MAX);
    check_batch(s, {1, kChunkWords}, &placed);
    CHECK(!placed);
}

static void test_random() {
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&](uint64_t m) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        return (x >> 11) % m;
    };
    const uint64_t sizes[] = {0, 1, 2, 3, 150, 1196, kChunkWords / 2 - 1, kChunkWords / 2, kChunkWords / 2 + 1,
                              kChunkWords / 4, kChunkWords, kChunkWords + 1};
    const size_t nsizes = sizeof sizes / sizeof sizes[0];
    LsetArenaState s;
    std::vector<uint64_t> all;  // every table of the chain so far
    size_t base = 0;            // inherited chunks at the chain's start
    for (int it = 0; it < 4000; it++) {
        if (it % 50 == 0) {  // a new chain: a fresh set, or a derived one with some inherited tail
            s = LsetArenaState{};
            if (rnd(2)) {
                s.chunks = 1 + rnd(5);
                s.used = 16 * rnd(CHUNK / 16 + 1);
                s.cap = CHUNK;
            }
            base = s.chunks;
            all.clear();
        }
        std::vector<uint64_t> nw(rnd(13));
        for (auto& w : nw) w = rnd(4) ? sizes[rnd(4 + rnd(2) * (nsizes - 4))] : 1 + rnd(2000);
        bool placed = false;
        s = check_batch(s, nw, &placed);
        CHECK(placed);
        all.insert(all.end(), nw.begin(), nw.end());
        CHECK(s.chunks == base + arena_chunks(all));
    }
}

int main() {
    test_small();
    test_chunk_end();
    test_large();
    test_inherited_tail();
    test_full();
    test_random();
    if (g_fail) {
        printf("%d check(s) FAILED\n", g_fail);
        return 1;
    }
    printf("lset_arena_test: all passed\n");
    return 0;
}
