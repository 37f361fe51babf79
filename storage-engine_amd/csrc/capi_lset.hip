// capi_lset.hip — the C ABI of the level set (lsmb_lset_*, include/lsmbloom.h).
// Host-side plumbing only; the placement of filters in the arena is planned in
// lset_arena.hpp, a repacking derive in lset_repack.hpp; the kernels are in
// lset.hip, lset_lists.hip, lset_version.hip, lset_version_lists.hip,
// lset_walk_first.hip, lset_repack.hip, lset_census.hip and crc32.hip.  Every add stages, copies
// and commits through lset_stage / lset_commit (a repacking derive through
// lset_commit_arena); the six lists entry points describe their flavour
// (LsetListsProbe) and run one device path (lset_lists_dev) or one host path
// (lset_lists_host, whose copy-back is ctx.hpp's lists_to_host).
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "crc_seg.hpp"
#include "ctx.hpp"
#include "fset_plan.hpp"
#include "lset_arena.hpp"
#include "lset_lists_plan.hpp"
#include "lset_order.hpp"
#include "lset_repack.hpp"
#include "lset_vlists_plan.hpp"
#include "lset_walk_plan.hpp"
#include "popcount_seg.hpp"

using namespace lsmb;

extern "C" {

// ---------------------------------------------------------------- level sets
// An immutable, device-resident snapshot of the store's non-overlapping
// levels (one per Version, src/db/mod.rs:255-267): rows of tables with
// pairwise disjoint key ranges, any number per row.  Tables are added in any
// order, each filter copied into a device arena as it arrives; seal sorts the
// rows, checks them (lset_order.hpp) and uploads the descriptors.  A sealed
// set is only read, so its probes need no scratch and no ordering.
//
// A Version edit (src/compaction/scheduler.rs:163-177) derives the next set
// from a sealed one: the child holds the surviving tables with their device
// words where they are, so the arena chunks are reference-counted (the counts
// are shared_ptr's, atomic: a parent may be probed while a child is derived)
// and a chunk goes when the last set holding one of its tables is closed.  A
// set bump-allocates only in chunks it allocated itself (own_tail), never in
// the tail of an inherited one: two children of one parent would collide
// there, and a sealed set's memory stays read-only for probes in flight.
// Left alone, a chain of edits therefore holds a chunk per edit for one small
// filter each; lsmb_lset_derive_packed moves the survivors of sparse chunks
// into a chunk of the child's own (k_copy_segs, device to device) and leaves
// the bump pointer there for the edit's add.
//
// The L0 part (row LSMB_LSET_ROW_L0 of any add): up to LSMB_LSET_L0_MAX tables
// whose ranges may overlap in any way, kept in order of arrival (a flush is
// new_levels[0].push(meta), src/db/mod.rs:402; a derived set keeps the
// parent's survivors in order, then its own adds: Vec::retain then push,
// src/compaction/scheduler.rs:171-174).  Their words live in the same arena;
// seal plans them as a filter set plans its slots (fset_plan.hpp), and
// lsmb_lset_probe_version answers L0 and the rows from one hash per key, so
// one sealed set is one Version (src/db/mod.rs:238-267).
namespace lsmb {
struct LsetChunk {
    int dev = 0;
    DevBuf buf;
    ~LsetChunk() {  // the last set holding the chunk closes (or a failed add gives its chunks back)
        DevGuard g(dev);
        buf.release();
    }
};

// Steps 2 and 3 of an add (below): where the filters go, and the chunks that
// do not exist yet.
struct LsetStaged {
    LsetPlacement pl;
    std::vector<std::shared_ptr<LsetChunk>> fresh;  // pl.new_chunks, allocated
    std::vector<uint8_t*> words;                    // per table: the device address of its slot
};
}  // namespace lsmb

struct lsmb_lset {
    lsmb_ctx* c = nullptr;
    struct Table {
        uint32_t id = 0, num_bits = 0, k = 0;
        uint32_t chunk = 0;               // index into chunks
        const uint32_t* words = nullptr;  // in the arena
        std::vector<uint8_t> lo, hi;
    };
    std::vector<Table> row[kLsetMaxRows];
    uint32_t nrows = 0;  // 1 + highest row added
    std::vector<Table> l0;  // position order
    std::vector<Table>& tables_of(uint32_t r) { return r == LSMB_LSET_ROW_L0 ? l0 : row[r]; }
    const std::vector<Table>& tables_of(uint32_t r) const { return r == LSMB_LSET_ROW_L0 ? l0 : row[r]; }
    bool sealed = false;
    // filter words: bump-allocated from chunks that are never reallocated;
    // a derived set's inherited chunks come first.  arena is the bump state
    // over them (lset_arena.hpp), arena.chunks == chunks.size()
    std::vector<std::shared_ptr<LsetChunk>> chunks;
    LsetArenaState arena;
    // the add in progress; between adds it holds nothing but its vectors'
    // capacity, so that a loop of single adds does not allocate for each
    LsetStaged staged;
    // lsmb_lset_stats: tables taken over by derive, filter bytes and copy calls of this set's uploads
    uint64_t inherited = 0, up_bytes = 0, up_copies = 0;
    // lsmb_lset_add_batch: pinned staging (words in the arena's layout, CRC
    // segments and results) and the device side of the CRC check
    uint8_t* pin = nullptr;
    uint64_t pin_cap = 0;
    PinnedPool pin_retired;
    DevBuf segs;
    DevBuf bounds, desc, pfx;  // seal: the bound keys' bytes, LsetTable[], prefix pairs
    LsetRows rows{};
    // seal: the table id of every ordinal (row by row, each in its sealed
    // order) and the first ordinal of every row, base[nrows] = all tables
    std::vector<uint32_t> ids;
    uint64_t base[kLsetMaxRows + 1] = {0};
    // seal: the filter of every ordinal, where it lives in the arena
    // (lsmb_lset_version_geometry, lsmb_lset_census)
    struct Geom {
        const uint32_t* words;
        uint32_t num_bits, k;
    };
    std::vector<Geom> geom;
    // seal, the L0 part: the boundary points' bytes, FsetPoint[] then the
    // region masks, RangedFilter[] (descriptor j = position j), and what the
    // kernels take by value
    DevBuf l0_bounds, l0_points, l0_desc;
    FsetRanges l0_rg{};
    FsetClasses l0_cl{};
    uint32_t l0_shared_nb = 0, l0_shared_k = 0;
    hipStream_t ust = nullptr;  // uploads
};

namespace {

// Every add (lset_add_common, lsmb_lset_add_batch, lsmb_lset_add_batch_dev)
// runs the same five steps: the host checks, the placement (lset_place), this
// call's new chunks, the copies and their wait, the commit.  The set is not
// touched before the commit (ls->staged is the add's own scratch), so a refused
// or failed add has nothing to undo.

// Device address of byte `off` of chunk `chunk`: one of the set's, or one of
// the staged add's new chunks after them.
uint8_t* lset_at(const lsmb_lset* ls, uint32_t chunk, size_t off) {
    const size_t held = ls->chunks.size();
    return (uint8_t*)(chunk < held ? ls->chunks[chunk] : ls->staged.fresh[chunk - held])->buf.p + off;
}

// Steps 2 and 3 into ls->staged.
int lset_stage(lsmb_lset* ls, const uint64_t* nw, uint64_t ntab) {
    LsetStaged& sg = ls->staged;
    if (!lset_place(ls->arena, nw, ntab, &sg.pl)) return fail(LSMB_EINVAL, "level set arena is full");
    for (const size_t bytes : sg.pl.new_chunks) {
        auto ch = std::make_shared<LsetChunk>();
        ch->dev = ls->c->dev;
        const hipError_t e = ch->buf.ensure(bytes);
        if (e != hipSuccess) return hip_fail(e, "ch->buf.ensure(std::max(bytes, kLsetChunkBytes))");
        sg.fresh.push_back(std::move(ch));
    }
    sg.words.resize(ntab);
    for (uint64_t t = 0; t < ntab; t++) sg.words[t] = lset_at(ls, sg.pl.slot[t].chunk, sg.pl.slot[t].off);
    return LSMB_OK;
}

// A failed add gives its chunks back: the stream first (~LsetChunk frees, and a
// copy may still be in flight), last_error() kept across the wait.
int lset_abandon(lsmb_lset* ls, hipStream_t st, int rc) {
    const std::string msg = last_error();
    (void)hipStreamSynchronize(st);
    ls->staged.fresh.clear();
    set_last_error(msg);
    return rc;
}

// Step 5, after every copy has completed.  The arena's half: the set adopts the
// staged chunks and takes the bump state after the placement.
void lset_commit_arena(lsmb_lset* ls) {
    LsetStaged& sg = ls->staged;
    for (auto& ch : sg.fresh) ls->chunks.push_back(std::move(ch));
    sg.fresh.clear();
    ls->arena = sg.pl.after;
}

// Table t of the staged placement has its slot.
void lset_commit_slot(const lsmb_lset* ls, uint64_t t, lsmb_lset::Table* T) {
    T->chunk = ls->staged.pl.slot[t].chunk;
    T->words = (const uint32_t*)ls->staged.words[t];
}

// All of step 5: the arena, the tables (tabs[t] into rows[t]) and the stats.
void lset_commit(lsmb_lset* ls, const uint32_t* rows, lsmb_lset::Table* tabs, uint64_t ntab, uint64_t up_bytes,
                 uint64_t up_copies) {
    lset_commit_arena(ls);
    for (uint64_t t = 0; t < ntab; t++) {
        lset_commit_slot(ls, t, &tabs[t]);
        ls->tables_of(rows[t]).push_back(std::move(tabs[t]));
        if (rows[t] != LSMB_LSET_ROW_L0) ls->nrows = std::max(ls->nrows, rows[t] + 1);
    }
    ls->up_bytes += up_bytes;
    ls->up_copies += up_copies;
}

// A table's key range as every add checks it.
int lset_range_check(const uint8_t* min_key, uint64_t min_len, const uint8_t* max_key, uint64_t max_len) {
    if ((min_len && !min_key) || (max_len && !max_key)) return fail(LSMB_EINVAL, "null key range");
    if (min_len > UINT32_MAX || max_len > UINT32_MAX) return fail(LSMB_EINVAL, "range key too long");
    return LSMB_OK;
}

// Room for `more` tables in `row`, `l0_before` of them L0 tables that come
// earlier in the same batch.
int lset_room_check(const lsmb_lset* ls, uint32_t row, uint64_t more, uint64_t l0_before) {
    if (row == LSMB_LSET_ROW_L0) {
        if (ls->l0.size() + l0_before >= LSMB_LSET_L0_MAX)
            return fail(LSMB_EINVAL, "level set L0 is full (%u tables)", (unsigned)LSMB_LSET_L0_MAX);
        return LSMB_OK;
    }
    if (ls->row[row].size() + more >= UINT32_MAX) return fail(LSMB_EINVAL, "level set row %u is full", row);
    return LSMB_OK;
}

int lset_add_common(lsmb_lset* ls, uint32_t row, uint32_t table_id, const uint8_t* words_le, uint32_t num_bits,
                    uint32_t k, const uint8_t* min_key, uint64_t min_len, const uint8_t* max_key, uint64_t max_len) {
    if (int rc = check_filter(num_bits, k)) return rc;
    if (int rc = lset_range_check(min_key, min_len, max_key, max_len)) return rc;
    if (int rc = lset_room_check(ls, row, 0, 0)) return rc;
    DevGuard g(ls->c->dev);
    const uint64_t nw = nwords64(num_bits);
    lsmb_lset::Table tab;
    tab.id = table_id;
    tab.num_bits = num_bits;
    tab.k = k;
    tab.lo.assign(min_key, min_key + min_len);
    tab.hi.assign(max_key, max_key + max_len);
    auto upload = [&]() -> int {
        if (int rc = lset_stage(ls, &nw, 1)) return rc;
        if (nw) {
            HIP_TRY(hipMemcpyAsync(ls->staged.words[0], words_le, nw * 8, hipMemcpyHostToDevice, ls->ust));
            HIP_TRY(hipStreamSynchronize(ls->ust));  // the caller's block is free to go
        }
        return LSMB_OK;
    };
    if (int rc = upload()) return lset_abandon(ls, ls->ust, rc);
    lset_commit(ls, &row, &tab, 1, nw * 8, nw ? 1 : 0);
    return LSMB_OK;
}

int lset_add_check(const lsmb_lset* ls, uint32_t row, uint32_t table_id) {
    if (!ls) return fail(LSMB_EINVAL, "null level set");
    if (ls->sealed) return fail(LSMB_EINVAL, "level set is sealed: a new Version takes a new set");
    if (row >= kLsetMaxRows && row != LSMB_LSET_ROW_L0)
        return fail(LSMB_EINVAL, "row %u: a level set has %u rows (and LSMB_LSET_ROW_L0)", row, kLsetMaxRows);
    if (table_id == LSMB_LSET_NONE) return fail(LSMB_EINVAL, "table id 0xFFFFFFFF is the probe's 'no table' answer");
    return LSMB_OK;
}

int lset_probe_check(const lsmb_lset* ls) {
    if (!ls) return fail(LSMB_EINVAL, "null level set");
    if (!ls->sealed) return fail(LSMB_EINVAL, "level set not sealed");
    return LSMB_OK;
}

}  // namespace

int lsmb_lset_open(lsmb_ctx* c, lsmb_lset** out) {
    if (!c || !out) return fail(LSMB_EINVAL, "null argument");
    *out = nullptr;
    DevGuard g(c->dev);
    lsmb_lset* ls = new lsmb_lset;
    ls->c = c;
    if (hipStreamCreateWithFlags(&ls->ust, hipStreamNonBlocking) != hipSuccess) {
        delete ls;
        return fail(LSMB_EHIP, "level set: stream creation failed");
    }
    *out = ls;
    return LSMB_OK;
}

void lsmb_lset_close(lsmb_lset* ls) {
    if (!ls) return;
    {
        DevGuard g(ls->c->dev);
        if (ls->ust) hipStreamSynchronize(ls->ust), hipStreamDestroy(ls->ust);
        ls->chunks.clear();  // each chunk goes with the last set holding it
        ls->segs.release();
        if (ls->pin) (void)hipHostFree(ls->pin);  // teardown
        ls->pin_retired.release();
        ls->bounds.release();
        ls->desc.release();
        ls->pfx.release();
        ls->l0_bounds.release();
        ls->l0_points.release();
        ls->l0_desc.release();
    }
    delete ls;
}

int lsmb_lset_add(lsmb_lset* ls, uint32_t row, uint32_t table_id, const uint8_t* block, uint64_t len,
                  const uint8_t* min_key, uint64_t min_len, const uint8_t* max_key, uint64_t max_len) {
    if (int rc = lset_add_check(ls, row, table_id)) return rc;
    uint32_t k, nb, nw;
    if (int rc = lsmb_deserialize_header(block, len, &k, &nb, &nw)) return rc;
    return lset_add_common(ls, row, table_id, block + 12, nb, k, min_key, min_len, max_key, max_len);
}

int lsmb_lset_add_words(lsmb_lset* ls, uint32_t row, uint32_t table_id, const uint64_t* words, uint32_t num_bits,
                        uint32_t num_hashes, const uint8_t* min_key, uint64_t min_len, const uint8_t* max_key,
                        uint64_t max_len) {
    if (int rc = lset_add_check(ls, row, table_id)) return rc;
    if (!words && nwords64(num_bits)) return fail(LSMB_EINVAL, "null words");
    return lset_add_common(ls, row, table_id, (const uint8_t*)words, num_bits, num_hashes, min_key, min_len, max_key,
                           max_len);
}

namespace {

// The survivors the plan (lset_repack.hpp) moved, already in the child's rows
// with the parent's addresses: their slots in chunks of the child's own, one
// k_copy_segs launch on st (NULL: the child's upload stream) and its wait, then
// the commit's arena half and the new slots.  The items cross through the
// child's pinned staging.
int lset_repack_moved(lsmb_lset* ls, const std::vector<lsmb_lset::Table*>& mv, void* stream, uint64_t* moved_bytes) {
    DevGuard g(ls->c->dev);
    const hipStream_t st = stream ? (hipStream_t)stream : ls->ust;
    std::vector<uint64_t> nw(mv.size());
    std::vector<const uint8_t*> src(mv.size());
    for (size_t m = 0; m < mv.size(); m++) {
        nw[m] = nwords64(mv[m]->num_bits);
        src[m] = (const uint8_t*)mv[m]->words;
        *moved_bytes += lset_slot_bytes(nw[m]);
    }
    auto copy = [&]() -> int {
        if (int rc = lset_stage(ls, nw.data(), nw.size())) return rc;
        LsetStaged& sg = ls->staged;
        std::vector<uint8_t*> fresh;
        for (const auto& ch : sg.fresh) fresh.push_back((uint8_t*)ch->buf.p);
        std::vector<CopySeg> items;
        lset_repack_items(sg.pl, ls->chunks.size(), fresh.data(), src.data(), nw.data(), &items);
        const size_t bytes = items.size() * sizeof(CopySeg);
        if (int rc = pinned_ensure(ls->pin_retired, &ls->pin, &ls->pin_cap, bytes, "level set")) return rc;
        memcpy(ls->pin, items.data(), bytes);
        HIP_TRY(ls->segs.ensure(bytes));
        HIP_TRY(hipMemcpyAsync(ls->segs.p, ls->pin, bytes, hipMemcpyHostToDevice, st));
        if (int rc = copy_segs_dev((const CopySeg*)ls->segs.p, items.size(), st)) return rc;
        HIP_TRY(hipStreamSynchronize(st));  // the edit's one wait: the parent may be closed
        return LSMB_OK;
    };
    if (int rc = copy()) return lset_abandon(ls, st, rc);
    lset_commit_arena(ls);  // own_tail: the edit's own add lands in the same chunk
    for (size_t m = 0; m < mv.size(); m++) lset_commit_slot(ls, m, mv[m]);
    return LSMB_OK;
}

// lsmb_lset_derive (min_ppm == 0: nothing moves, nothing is launched) and
// lsmb_lset_derive_packed.
int lset_derive(const lsmb_lset* parent, const uint32_t* drop_ids, uint64_t ndrop, uint32_t min_ppm, uint64_t* dropped,
                uint64_t* moved, lsmb_lset** out, void* stream) {
    if (out) *out = nullptr;
    if (!parent || !out) return fail(LSMB_EINVAL, "null argument");
    if (!parent->sealed) return fail(LSMB_EINVAL, "derive from an unsealed level set");
    if (ndrop && !drop_ids) return fail(LSMB_EINVAL, "null drop_ids");
    if (min_ppm > LSMB_LSET_REPACK_ALL)
        return fail(LSMB_EINVAL, "min_ppm %u: at most 1000000, or LSMB_LSET_REPACK_ALL", min_ppm);
    std::vector<uint32_t> drop(drop_ids, drop_ids + ndrop);
    std::sort(drop.begin(), drop.end());
    // the surviving tables in derive order: rows 0 .. R-1, then L0 by position
    std::vector<std::pair<uint32_t, const lsmb_lset::Table*>> surv;
    uint64_t nd = 0;
    auto take = [&](uint32_t r, const std::vector<lsmb_lset::Table>& tabs) {
        for (const auto& T : tabs) {
            if (std::binary_search(drop.begin(), drop.end(), T.id))
                nd++;
            else
                surv.emplace_back(r, &T);
        }
    };
    for (uint32_t r = 0; r < parent->nrows; r++) take(r, parent->row[r]);
    take(LSMB_LSET_ROW_L0, parent->l0);
    // which of them leave their chunk (lset_repack.hpp)
    std::vector<uint8_t> move(surv.size(), 0), evac;
    if (min_ppm) {
        std::vector<RepackTable> rt(surv.size());
        for (size_t t = 0; t < surv.size(); t++)
            rt[t] = RepackTable{surv[t].second->chunk, lset_slot_bytes(nwords64(surv[t].second->num_bits))};
        std::vector<size_t> cap(parent->chunks.size());
        for (size_t c = 0; c < cap.size(); c++) cap[c] = parent->chunks[c]->buf.bytes;
        lset_repack_plan(rt.data(), rt.size(), cap.data(), cap.size(), min_ppm, &move, &evac);
    }
    lsmb_lset* ls = nullptr;
    if (int rc = lsmb_lset_open(parent->c, &ls)) return rc;
    // each survivor in its row (L0: in its relative order), and only the chunks
    // that hold one that stays
    std::vector<uint32_t> remap(parent->chunks.size(), UINT32_MAX);
    for (uint32_t r = 0; r < parent->nrows; r++) ls->row[r].reserve(parent->row[r].size());
    ls->l0.reserve(parent->l0.size());
    std::vector<lsmb_lset::Table*> mv;  // into the reserved rows: no push below reallocates
    for (size_t t = 0; t < surv.size(); t++) {
        const lsmb_lset::Table& T = *surv[t].second;
        std::vector<lsmb_lset::Table>& into = ls->tables_of(surv[t].first);
        into.push_back(T);
        ls->inherited++;
        if (move[t]) {
            mv.push_back(&into.back());
            continue;
        }
        if (remap[T.chunk] == UINT32_MAX) {
            remap[T.chunk] = (uint32_t)ls->chunks.size();
            ls->chunks.push_back(parent->chunks[T.chunk]);
        }
        into.back().chunk = remap[T.chunk];
    }
    ls->arena.chunks = ls->chunks.size();  // none of them the child's own: its first add takes a new chunk
    ls->nrows = parent->nrows;
    uint64_t moved_bytes = 0;
    if (!mv.empty())
        if (int rc = lset_repack_moved(ls, mv, stream, &moved_bytes)) {
            const std::string msg = last_error();
            lsmb_lset_close(ls);  // all or nothing: the parent is as it was
            set_last_error(msg);
            return rc;
        }
    if (dropped) *dropped = nd;
    if (moved) moved[0] = mv.size(), moved[1] = moved_bytes;
    *out = ls;
    return LSMB_OK;
}

}  // namespace

int lsmb_lset_derive(const lsmb_lset* parent, const uint32_t* drop_ids, uint64_t ndrop, uint64_t* dropped,
                     lsmb_lset** out) {
    return lset_derive(parent, drop_ids, ndrop, 0, dropped, nullptr, out, nullptr);
}

// A derive that also moves the survivors of sparse parent chunks into a chunk
// of the child's own, device to device (k_copy_segs): a chain of edits
// (src/compaction/scheduler.rs:163-177, src/db/mod.rs:402) then holds a chunk
// per edit no longer.
int lsmb_lset_derive_packed(const lsmb_lset* parent, const uint32_t* drop_ids, uint64_t ndrop, uint32_t min_ppm,
                            uint64_t* dropped, uint64_t moved[2], lsmb_lset** out, void* stream) {
    return lset_derive(parent, drop_ids, ndrop, min_ppm, dropped, moved, out, stream);
}

namespace {

// Table t of a batch, its bounds at ko[0 .. 2] in keys; its slot comes with the commit.
void lset_batch_table(lsmb_lset::Table* T, uint32_t id, uint32_t num_bits, uint32_t k, const uint8_t* keys,
                      const uint64_t* ko) {
    T->id = id;
    T->num_bits = num_bits;
    T->k = k;
    if (ko[1] > ko[0]) T->lo.assign(keys + ko[0], keys + ko[1]);
    if (ko[2] > ko[1]) T->hi.assign(keys + ko[1], keys + ko[2]);
}

// What both batches check of a table once its filter is known.
int lset_batch_table_check(const lsmb_lset* ls, uint64_t ntab, uint64_t l0_before, uint32_t row, uint32_t num_bits,
                           uint32_t k, const uint8_t* keys, const uint64_t* koff) {
    if (int rc = check_filter(num_bits, k)) return rc;
    if (koff[1] < koff[0] || koff[2] < koff[1]) return fail(LSMB_EINVAL, "key offsets descend");
    if (int rc = lset_range_check(keys, koff[1] - koff[0], keys, koff[2] - koff[1])) return rc;
    return lset_room_check(ls, row, ntab, l0_before);
}

// One table of lsmb_lset_add_batch: its host-side checks, then *T.
int lset_batch_check_one(const lsmb_lset* ls, uint64_t ntab, uint64_t l0_before, uint32_t row, uint32_t id,
                         const uint8_t* blocks,
                         const uint64_t* boff, const uint8_t* keys, const uint64_t* koff, lsmb_lset::Table* T) {
    if (int rc = lset_add_check(ls, row, id)) return rc;
    if (boff[1] < boff[0]) return fail(LSMB_EINVAL, "block offsets descend");
    uint32_t k = 0, nb = 0, nw32 = 0;
    if (int rc = lsmb_deserialize_header(blocks ? blocks + boff[0] : nullptr, boff[1] - boff[0], &k, &nb, &nw32))
        return rc;
    if (int rc = lset_batch_table_check(ls, ntab, l0_before, row, nb, k, keys, koff)) return rc;
    lset_batch_table(T, id, nb, k, keys, koff);
    return LSMB_OK;
}

// What both batches check before any table: the set, then (an empty batch is
// done) the arrays (`arrays`: none of them null) and the count.
int lset_batch_check(const lsmb_lset* ls, uint64_t ntab, bool arrays) {
    if (!ls) return fail(LSMB_EINVAL, "null level set");
    if (ls->sealed) return fail(LSMB_EINVAL, "level set is sealed: a new Version takes a new set");
    if (ntab == 0) return LSMB_OK;
    if (!arrays) return fail(LSMB_EINVAL, "null argument");
    if (ntab >= UINT32_MAX) return fail(LSMB_EINVAL, "more than 2^32-2 tables in one batch");
    return LSMB_OK;
}

// Slots, staging, copies and the CRC check of a batch whose headers passed
// (nw[t]: table t's u64 words).
int lset_batch_upload(lsmb_lset* ls, uint64_t ntab, const uint64_t* nw, const uint32_t* ids, const uint8_t* blocks,
                      const uint64_t* boff, const uint32_t* crcs, int32_t* status) {
    // slots in the arena, 16-B aligned, and the runs they form per chunk
    if (int rc = lset_stage(ls, nw, ntab)) return rc;
    const LsetStaged* sg = &ls->staged;
    const size_t stage = sg->pl.packed_bytes();
    // the CRC segments (up to 128 KiB each: one wave per segment) and their results after the words
    std::vector<uint64_t> seg_of;
    if (crcs)
        for (uint64_t t = 0; t < ntab; t++)
            if (nw[t] * 8 <= kCrcSegWaveMax) seg_of.push_back(t);
    const size_t nseg = seg_of.size();
    const size_t seg_at = stage, out_at = seg_at + nseg * sizeof(CrcSeg);
    if (int rc = pinned_ensure(ls->pin_retired, &ls->pin, &ls->pin_cap, out_at + nseg * 4 + 16, "level set")) return rc;
    size_t at = 0;  // table t's words in the pinned staging: the slots back to back
    for (uint64_t t = 0; t < ntab; t++) {
        const size_t slot = lset_slot_bytes(nw[t]);
        if (nw[t]) memcpy(ls->pin + at, blocks + boff[t] + 12, nw[t] * 8);
        memset(ls->pin + at + nw[t] * 8, 0, slot - nw[t] * 8);
        at += slot;
    }
    for (const LsetSpan& sp : sg->pl.spans)  // one copy per chunk touched
        HIP_TRY(hipMemcpyAsync(lset_at(ls, sp.chunk, sp.off), ls->pin + sp.src, sp.bytes, hipMemcpyHostToDevice, ls->ust));
    if (nseg) {
        CrcSeg* hs = (CrcSeg*)(ls->pin + seg_at);
        for (size_t s = 0; s < nseg; s++) hs[s] = CrcSeg{sg->words[seg_of[s]], nw[seg_of[s]] * 8};
        HIP_TRY(ls->segs.ensure(nseg * (sizeof(CrcSeg) + 4)));
        uint8_t* ds = (uint8_t*)ls->segs.p;
        uint32_t* dout = (uint32_t*)(ds + nseg * sizeof(CrcSeg));
        HIP_TRY(hipMemcpyAsync(ds, hs, nseg * sizeof(CrcSeg), hipMemcpyHostToDevice, ls->ust));
        if (int rc = crc32_seg_dev((const CrcSeg*)ds, nseg, dout, ls->ust)) return rc;
        HIP_TRY(hipMemcpyAsync(ls->pin + out_at, dout, nseg * 4, hipMemcpyDeviceToHost, ls->ust));
    }
    HIP_TRY(hipStreamSynchronize(ls->ust));  // the batch's one wait: the caller's blocks are free to go
    if (!crcs) return LSMB_OK;
    // the copies now in HBM, not the host bytes, are what probes will read
    std::vector<uint32_t> words_crc(ntab, 0);
    const uint32_t* hout = (const uint32_t*)(ls->pin + out_at);
    for (size_t s = 0; s < nseg; s++) words_crc[seg_of[s]] = hout[s];
    for (uint64_t t = 0; t < ntab; t++)
        if (nw[t] * 8 > kCrcSegWaveMax)
            if (int rc = crc32_dev(ls->c, sg->words[t], nw[t] * 8, 0, ls->ust, &words_crc[t])) return rc;
    int first = LSMB_OK;
    uint64_t f_len = 0;
    uint32_t f = 1u << 31;  // x^(8·f_len): the tables of a store mostly share one size
    for (uint64_t t = 0; t < ntab; t++) {
        if (nw[t] * 8 != f_len) f = x8nmodp(f_len = nw[t] * 8);
        const uint32_t got = multmodp(f, crc32_host(blocks + boff[t], 12, 0)) ^ words_crc[t];  // header ‖ words
        if (got == crcs[t]) continue;
        if (status) status[t] = LSMB_ECORRUPT;
        if (first == LSMB_OK)
            first = fail(LSMB_ECORRUPT,
                         "table %llu of the batch (id %u): bloom block CRC-32 mismatch: expected %08x, device copy %08x",
                         (unsigned long long)t, ids[t], crcs[t], got);
    }
    return first;
}

}  // namespace

int lsmb_lset_add_batch(lsmb_lset* ls, uint64_t ntab, const uint32_t* rows, const uint32_t* table_ids,
                        const uint8_t* blocks, const uint64_t* block_off, const uint32_t* crcs, const uint8_t* keys,
                        const uint64_t* key_off, int32_t* status) {
    if (int rc = lset_batch_check(ls, ntab, rows && table_ids && block_off && key_off)) return rc;
    if (ntab == 0) return LSMB_OK;
    // every header on the host first: nothing is allocated or uploaded for a batch that fails here
    std::vector<lsmb_lset::Table> tabs(ntab);
    int first_rc = LSMB_OK;
    uint64_t first_t = 0;
    std::string first_msg;
    uint64_t l0_before = 0;  // L0 tables of the batch before table t: the 65th of the set is refused
    for (uint64_t t = 0; t < ntab; t++) {
        const int rc = lset_batch_check_one(ls, ntab, l0_before, rows[t], table_ids[t], blocks, block_off + t, keys,
                                            key_off + 2 * t, &tabs[t]);
        l0_before += rows[t] == LSMB_LSET_ROW_L0;
        if (status) status[t] = rc;
        if (rc && first_rc == LSMB_OK) {
            first_rc = rc;
            first_t = t;
            first_msg = last_error();
        }
    }
    if (first_rc)
        return fail(first_rc, "table %llu of the batch (id %u): %s", (unsigned long long)first_t, table_ids[first_t],
                    first_msg.c_str());
    DevGuard g(ls->c->dev);
    std::vector<uint64_t> nw(ntab);
    uint64_t up_bytes = 0;
    for (uint64_t t = 0; t < ntab; t++) up_bytes += (nw[t] = nwords64(tabs[t].num_bits)) * 8;
    if (int rc = lset_batch_upload(ls, ntab, nw.data(), table_ids, blocks, block_off, crcs, status))
        return lset_abandon(ls, ls->ust, rc);  // all or nothing
    lset_commit(ls, rows, tabs.data(), ntab, up_bytes, ls->staged.pl.spans.size());
    return LSMB_OK;
}

// Filters a batched build left on the set's device (lsmb_build_batch_dev: the
// outputs of src/compaction/scheduler.rs:147-177 pushed into the next Version
// without a trip through the host): the slots of the packed buffer are the
// arena's slots, so each run of tables landing in one chunk is one
// device-to-device copy.
int lsmb_lset_add_batch_dev(lsmb_lset* ls, uint64_t ntab, const uint32_t* rows, const uint32_t* table_ids,
                            const void* d_words, const uint64_t* word_off, const uint32_t* num_bits,
                            const uint32_t* num_hashes, const uint8_t* keys, const uint64_t* key_off, void* stream) {
    if (int rc = lset_batch_check(ls, ntab, rows && table_ids && d_words && word_off && num_bits && num_hashes && key_off))
        return rc;
    if (ntab == 0) return LSMB_OK;
    if (reinterpret_cast<uintptr_t>(d_words) & 15) return fail(LSMB_EINVAL, "d_words is not 16-byte aligned");
    // every table on the host first: nothing is allocated or copied for a batch that fails here
    uint64_t at = 0;  // the layout's word_off[t]: the slots back to back, the spans' packed source
    auto off_check = [&](uint64_t t) {
        if (word_off[t] == at) return LSMB_OK;
        return fail(LSMB_EINVAL, "word_off[%llu] = %llu, lsmb_build_batch_layout gives %llu", (unsigned long long)t,
                    (unsigned long long)word_off[t], (unsigned long long)at);
    };
    std::vector<uint64_t> nw(ntab);
    uint64_t l0_before = 0;
    for (uint64_t t = 0; t < ntab; t++) {
        int rc = off_check(t);
        if (!rc) rc = lset_add_check(ls, rows[t], table_ids[t]);
        if (!rc)
            rc = lset_batch_table_check(ls, ntab, l0_before, rows[t], num_bits[t], num_hashes[t], keys, key_off + 2 * t);
        l0_before += rows[t] == LSMB_LSET_ROW_L0;
        if (rc) {
            const std::string msg = last_error();
            return fail(rc, "table %llu of the batch (id %u): %s", (unsigned long long)t, table_ids[t], msg.c_str());
        }
        nw[t] = nwords64(num_bits[t]);
        at += lset_slot_bytes(nw[t]) / 8;
    }
    if (int rc = off_check(ntab)) return rc;
    DevGuard g(ls->c->dev);
    hipStream_t st = pick_stream(ls->c, stream);
    std::vector<lsmb_lset::Table> tabs(ntab);
    for (uint64_t t = 0; t < ntab; t++)
        lset_batch_table(&tabs[t], table_ids[t], num_bits[t], num_hashes[t], keys, key_off + 2 * t);
    auto copy = [&]() -> int {
        if (int rc = lset_stage(ls, nw.data(), ntab)) return rc;
        for (const LsetSpan& sp : ls->staged.pl.spans)  // one device-to-device copy per chunk touched
            HIP_TRY(hipMemcpyAsync(lset_at(ls, sp.chunk, sp.off), (const uint8_t*)d_words + sp.src, sp.bytes,
                                   hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));  // the batch's one wait: the source buffer is free to go
        return LSMB_OK;
    };
    if (int rc = copy()) return lset_abandon(ls, st, rc);  // all or nothing
    lset_commit(ls, rows, tabs.data(), ntab, 0, 0);  // nothing crossed from the host
    return LSMB_OK;
}

int lsmb_lset_stats(const lsmb_lset* ls, uint64_t out[6]) {
    if (!ls || !out) return fail(LSMB_EINVAL, "null argument");
    uint64_t ntab = 0, fbytes = 0, cbytes = 0;
    for (uint32_t r = 0; r < ls->nrows; r++) {
        ntab += ls->row[r].size();
        for (const auto& T : ls->row[r]) fbytes += nwords64(T.num_bits) * 8;
    }
    ntab += ls->l0.size();
    for (const auto& T : ls->l0) fbytes += nwords64(T.num_bits) * 8;
    for (const auto& ch : ls->chunks) cbytes += ch->buf.bytes;
    out[0] = ntab;
    out[1] = ls->inherited;
    out[2] = ls->up_bytes;
    out[3] = ls->up_copies;
    out[4] = cbytes;
    out[5] = fbytes;
    return LSMB_OK;
}

int lsmb_lset_seal(lsmb_lset* ls) {
    if (!ls) return fail(LSMB_EINVAL, "null level set");
    if (ls->sealed) return LSMB_OK;
    // per row: sorted by min_key, ranges disjoint
    std::vector<uint32_t> order[kLsetMaxRows];
    uint64_t ntab = 0;
    for (uint32_t r = 0; r < ls->nrows; r++) {
        const auto& T = ls->row[r];
        std::vector<LsetRange> rg(T.size());
        for (size_t j = 0; j < T.size(); j++)
            rg[j] = LsetRange{T[j].lo.data(), T[j].lo.size(), T[j].hi.data(), T[j].hi.size(), T[j].id};
        LsetOrderError err;
        if (!lset_order_row(rg.data(), (uint32_t)rg.size(), &order[r], &err)) {
            if (err.inverted) return fail(LSMB_EINVAL, "level set row %u: table %u has min_key > max_key", r, err.id_a);
            return fail(LSMB_EINVAL, "level set row %u: tables %u and %u overlap (max_key of %u >= min_key of %u)", r,
                        err.id_a, err.id_b, err.id_a, err.id_b);
        }
        ntab += T.size();
    }
    // L0: any overlap goes, no order to find; a table still has min_key <= max_key
    for (const auto& T : ls->l0)
        if (bytes_cmp(T.lo.data(), T.lo.size(), T.hi.data(), T.hi.size()) > 0)
            return fail(LSMB_EINVAL, "level set L0: table %u has min_key > max_key", T.id);
    // the bound keys' bytes, the descriptors and the search prefixes, each row's
    // tables in sorted order, rows back to back
    std::vector<uint8_t> blob;
    std::vector<LsetTable> d;
    std::vector<ulonglong2> px;
    d.reserve(ntab);
    px.reserve(ntab);
    for (uint32_t r = 0; r < ls->nrows; r++)
        for (uint32_t j : order[r]) {
            const auto& S = ls->row[r][j];
            LsetTable t;
            memset(&t, 0, sizeof t);
            t.words32 = S.words;
            t.lo = (const uint8_t*)(uintptr_t)blob.size();  // offsets until the blob has its address
            blob.insert(blob.end(), S.lo.begin(), S.lo.end());
            t.hi = (const uint8_t*)(uintptr_t)blob.size();
            blob.insert(blob.end(), S.hi.begin(), S.hi.end());
            const HostPfx16 pl = host_prefix16(S.lo.data(), S.lo.size()), ph = host_prefix16(S.hi.data(), S.hi.size());
            t.lo_w0 = pl.w0;
            t.lo_w1 = pl.w1;
            t.md = Mod32::make(S.num_bits ? S.num_bits : 1);
            t.lo_len = (uint32_t)S.lo.size();
            t.hi_len = (uint32_t)S.hi.size();
            t.num_bits = S.num_bits;
            t.k = S.k;
            t.id = S.id;
            d.push_back(t);
            ulonglong2 q;
            q.x = ph.w0;
            q.y = ph.w1;
            px.push_back(q);
        }
    DevGuard g(ls->c->dev);
    HIP_TRY(ls->bounds.ensure(blob.size() + 16));
    HIP_TRY(ls->desc.ensure(std::max<size_t>(d.size(), 1) * sizeof(LsetTable)));
    HIP_TRY(ls->pfx.ensure(std::max<size_t>(px.size(), 1) * sizeof(ulonglong2)));
    const uint8_t* base = (const uint8_t*)ls->bounds.p;
    for (auto& t : d) {
        t.lo = base + (uintptr_t)t.lo;
        t.hi = base + (uintptr_t)t.hi;
    }
    if (!blob.empty()) HIP_TRY(hipMemcpyAsync(ls->bounds.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ls->ust));
    if (!d.empty()) {
        HIP_TRY(hipMemcpyAsync(ls->desc.p, d.data(), d.size() * sizeof(LsetTable), hipMemcpyHostToDevice, ls->ust));
        HIP_TRY(hipMemcpyAsync(ls->pfx.p, px.data(), px.size() * sizeof(ulonglong2), hipMemcpyHostToDevice, ls->ust));
    }
    // the L0 part as a filter set's (fset_plan.hpp): descriptor j = position j = answer bit j
    FsetPlan pl;
    std::vector<uint8_t> pbuf;
    std::vector<RangedFilter> l0d;
    if (!ls->l0.empty()) {
        std::vector<FsetPlanTable> pt;
        for (const auto& T : ls->l0)
            pt.push_back(FsetPlanTable{T.lo.data(), T.lo.size(), T.hi.data(), T.hi.size(), T.num_bits, T.k});
        fset_plan(pt.data(), (uint32_t)pt.size(), &pl);
        const uint32_t m = (uint32_t)pl.points.size();
        HIP_TRY(ls->l0_bounds.ensure(pl.blob.size() + 16));
        pbuf.resize(sizeof(FsetPoint) * m + 8 * pl.regmask.size());
        FsetPoint* fp = (FsetPoint*)pbuf.data();
        for (uint32_t j = 0; j < m; j++) {
            fp[j] = pl.points[j];
            fp[j].p = (const uint8_t*)ls->l0_bounds.p + (uintptr_t)pl.points[j].p;
        }
        memcpy(pbuf.data() + sizeof(FsetPoint) * m, pl.regmask.data(), 8 * pl.regmask.size());
        for (uint32_t j = 0; j < ls->l0.size(); j++)
            l0d.push_back(fset_plan_desc(ls->l0[j].words, ls->l0[j].num_bits, ls->l0[j].k, j));
        HIP_TRY(ls->l0_points.ensure(pbuf.size()));
        HIP_TRY(ls->l0_desc.ensure(l0d.size() * sizeof(RangedFilter)));
        if (!pl.blob.empty())
            HIP_TRY(hipMemcpyAsync(ls->l0_bounds.p, pl.blob.data(), pl.blob.size(), hipMemcpyHostToDevice, ls->ust));
        HIP_TRY(hipMemcpyAsync(ls->l0_points.p, pbuf.data(), pbuf.size(), hipMemcpyHostToDevice, ls->ust));
        HIP_TRY(hipMemcpyAsync(ls->l0_desc.p, l0d.data(), l0d.size() * sizeof(RangedFilter), hipMemcpyHostToDevice,
                               ls->ust));
        ls->l0_rg.pts = (const FsetPoint*)ls->l0_points.p;
        ls->l0_rg.regmask = (const uint64_t*)((const uint8_t*)ls->l0_points.p + sizeof(FsetPoint) * m);
        ls->l0_rg.npts = m;
        ls->l0_cl = pl.cl;
        ls->l0_shared_nb = pl.shared_nb;
        ls->l0_shared_k = pl.shared_k;
    }
    HIP_TRY(hipStreamSynchronize(ls->ust));  // blob, d, px, pl, pbuf and l0d are host temporaries
    memset(&ls->rows, 0, sizeof ls->rows);
    ls->rows.nrows = ls->nrows;
    uint64_t at = 0;
    for (uint32_t r = 0; r < ls->nrows; r++) {
        const uint32_t m = (uint32_t)ls->row[r].size();
        if (m) {
            ls->rows.row[r].hi_pfx = (const ulonglong2*)ls->pfx.p + at;
            ls->rows.row[r].tab = (const LsetTable*)ls->desc.p + at;
        }
        ls->rows.row[r].ntab = m;
        ls->base[r] = at;
        at += m;
    }
    for (uint32_t r = ls->nrows; r <= kLsetMaxRows; r++) ls->base[r] = at;
    ls->ids.resize(d.size());
    ls->geom.resize(d.size());
    for (size_t g = 0; g < d.size(); g++) {
        ls->ids[g] = d[g].id;
        ls->geom[g] = lsmb_lset::Geom{d[g].words32, d[g].num_bits, d[g].k};
    }
    ls->sealed = true;
    return LSMB_OK;
}

int lsmb_lset_rows(const lsmb_lset* ls) { return ls ? (int)ls->nrows : 0; }

uint64_t lsmb_lset_tables(const lsmb_lset* ls, uint32_t row) {
    if (ls && row == LSMB_LSET_ROW_L0) return (uint64_t)ls->l0.size();
    return ls && row < kLsetMaxRows ? (uint64_t)ls->row[row].size() : 0;
}

uint64_t lsmb_lset_l0_tables(const lsmb_lset* ls) { return ls ? (uint64_t)ls->l0.size() : 0; }

int lsmb_lset_l0_order(const lsmb_lset* ls, uint32_t* ids) {
    if (int rc = lset_probe_check(ls)) return rc;
    if (!ids && !ls->l0.empty()) return fail(LSMB_EINVAL, "null ids");
    for (size_t j = 0; j < ls->l0.size(); j++) ids[j] = ls->l0[j].id;
    return LSMB_OK;
}

int lsmb_lset_probe_dev(lsmb_lset* ls, const void* d_data, const void* d_offsets, uint32_t key_len, uint64_t n,
                        void* d_out, void* stream) {
    if (int rc = lset_probe_check(ls)) return rc;
    if (n == 0 || ls->nrows == 0) return LSMB_OK;
    if (!d_out || !d_data) return fail(LSMB_EINVAL, "null keys or output");
    DevGuard g(ls->c->dev);
    KeyBatch kb{(const uint8_t*)d_data, (const uint64_t*)d_offsets, key_len, n};
    HIP_TRY(launch_lset_probe(kb, ls->rows, (uint32_t*)d_out, ls->c->num_cus, pick_stream(ls->c, stream)));
    return LSMB_OK;
}

int lsmb_lset_probe(lsmb_lset* ls, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                    uint32_t* out) {
    if (int rc = lset_probe_check(ls)) return rc;
    if (n == 0 || ls->nrows == 0) return LSMB_OK;
    if (!out || host_keys_null(data, offsets, key_len, n)) return fail(LSMB_EINVAL, "null keys or output");
    lsmb_ctx* c = ls->c;
    DevGuard g(c->dev);
    const uint64_t obytes = (uint64_t)ls->nrows * n * 4;
    HIP_TRY(c->out.ensure(obytes));
    KeyBatch kb;
    if (int rc = stage_host_keys(c, data, offsets, key_len, n, &kb)) return rc;
    HIP_TRY(launch_lset_probe(kb, ls->rows, (uint32_t*)c->out.p, c->num_cus, c->st));
    HIP_TRY(hipMemcpyAsync(out, c->out.p, obytes, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    return LSMB_OK;
}

// The Version probe of kb on st: d_mask (n u64) and d_out (nrows * n u32,
// unused when the set has no row).  Without L0 tables the rows' own kernel and
// a cleared mask; else the fused kernel (lset_version.hip).
static int lset_version_launch(lsmb_lset* ls, const KeyBatch& kb, uint64_t* d_mask, uint32_t* d_out, hipStream_t st) {
    if (ls->l0.empty()) {
        HIP_TRY(hipMemsetAsync(d_mask, 0, kb.n * 8, st));
        if (ls->nrows) HIP_TRY(launch_lset_probe(kb, ls->rows, d_out, ls->c->num_cus, st));
        return LSMB_OK;
    }
    HIP_TRY(launch_lset_version(kb, ls->rows, (const RangedFilter*)ls->l0_desc.p, (uint32_t)ls->l0.size(), ls->l0_rg,
                                ls->l0_cl, d_mask, d_out, ls->c->num_cus, st));
    return LSMB_OK;
}

int lsmb_lset_probe_version_dev(lsmb_lset* ls, const void* d_data, const void* d_offsets, uint32_t key_len, uint64_t n,
                                void* d_l0_mask, void* d_out, void* stream) {
    if (int rc = lset_probe_check(ls)) return rc;
    if (n == 0) return LSMB_OK;
    if (!d_l0_mask || !d_data) return fail(LSMB_EINVAL, "null keys or L0 mask");
    if (!d_out && ls->nrows) return fail(LSMB_EINVAL, "null output for a set with rows");
    DevGuard g(ls->c->dev);
    KeyBatch kb{(const uint8_t*)d_data, (const uint64_t*)d_offsets, key_len, n};
    return lset_version_launch(ls, kb, (uint64_t*)d_l0_mask, (uint32_t*)d_out, pick_stream(ls->c, stream));
}

int lsmb_lset_probe_version(lsmb_lset* ls, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                            uint64_t* l0_mask, uint32_t* out) {
    if (int rc = lset_probe_check(ls)) return rc;
    if (n == 0) return LSMB_OK;
    if (!l0_mask || host_keys_null(data, offsets, key_len, n)) return fail(LSMB_EINVAL, "null keys or L0 mask");
    if (!out && ls->nrows) return fail(LSMB_EINVAL, "null output for a set with rows");
    lsmb_ctx* c = ls->c;
    DevGuard g(c->dev);
    // the context's output scratch: the masks, then the rows' ids
    const uint64_t mbytes = n * 8, obytes = (uint64_t)ls->nrows * n * 4;
    HIP_TRY(c->out.ensure(mbytes + obytes));
    uint64_t* d_mask = (uint64_t*)c->out.p;
    uint32_t* d_out = (uint32_t*)((uint8_t*)c->out.p + mbytes);
    KeyBatch kb;
    if (int rc = stage_host_keys(c, data, offsets, key_len, n, &kb)) return rc;
    if (int rc = lset_version_launch(ls, kb, d_mask, d_out, c->st)) return rc;
    HIP_TRY(hipMemcpyAsync(l0_mask, d_mask, mbytes, hipMemcpyDeviceToHost, c->st));
    if (obytes) HIP_TRY(hipMemcpyAsync(out, d_out, obytes, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    return LSMB_OK;
}

uint64_t lsmb_lset_total_tables(const lsmb_lset* ls) { return ls && ls->sealed ? ls->base[ls->nrows] : 0; }

int lsmb_lset_table_order(const lsmb_lset* ls, uint32_t* ids, uint64_t* row_base) {
    if (int rc = lset_probe_check(ls)) return rc;
    if (ids && !ls->ids.empty()) memcpy(ids, ls->ids.data(), ls->ids.size() * sizeof(uint32_t));
    if (row_base) memcpy(row_base, ls->base, ((size_t)ls->nrows + 1) * sizeof(uint64_t));
    return LSMB_OK;
}

uint64_t lsmb_lset_lists_work_bytes(const lsmb_lset* ls, uint64_t n) {
    if (!ls || !ls->sealed || n > UINT32_MAX) return 0;
    return lset_lists_plan(n, ls->nrows, ls->base[ls->nrows]).work_bytes;
}

// A lists probe over this sealed set, the rows' (lsmb_lset_probe_lists*), the
// whole Version's (lsmb_lset_probe_version_lists*) or the walk's
// (lsmb_lset_probe_walk_lists*): what the flavours differ in.  A Version
// without L0 tables is the rows' probe, byte for byte.
enum class LsetLists { Rows, Version, Walk };
struct LsetListsProbe {
    uint64_t total = 0;       // tables: the starts have total + 1 entries
    uint64_t work_bytes = 0;  // the workspace of n keys
    uint64_t bound = 0;       // no more list entries than this
    const char* sizer = "";   // the public function that reports work_bytes
    // the walk only: every key's resume step (null: all zero) and, coming back
    // next to the lists, its step (null: not wanted); the caller's pointers,
    // device memory on the device path, host memory on the host path
    const uint32_t* from = nullptr;
    uint32_t* step = nullptr;
    hipError_t (*launch)(lsmb_lset* ls, const KeyBatch& kb, const uint32_t* d_from, uint32_t* d_step, uint64_t* d_starts,
                         uint32_t* d_index, uint64_t cap, void* d_work, uint64_t work_bytes, hipStream_t st) = nullptr;
};

// The argument checks shared by all six lists entry points, then *lp.
static int lset_lists_desc(const lsmb_lset* ls, LsetLists kind, uint64_t n, const void* starts, const void* index,
                           uint64_t cap, LsetListsProbe* lp) {
    if (int rc = lset_probe_check(ls)) return rc;
    if (n > UINT32_MAX) return fail(LSMB_EINVAL, "more than 2^32-1 keys (the lists hold 32-bit indices)");
    const uint64_t G = ls->base[ls->nrows], T0 = kind == LsetLists::Rows ? 0 : ls->l0.size();
    if (T0 + G > UINT32_MAX) return fail(LSMB_EINVAL, "more than 2^32-1 tables");
    if (!starts || (cap && !index)) return fail(LSMB_EINVAL, "null output");
    lp->total = T0 + G;
    if (kind == LsetLists::Walk) {
        lp->work_bytes = lset_walk_lists_plan(n, T0 + G).work_bytes;
        lp->bound = n;  // a key is in at most one list
        lp->sizer = "lsmb_lset_walk_lists_work_bytes";
        lp->launch = [](lsmb_lset* ls, const KeyBatch& kb, const uint32_t* d_from, uint32_t* d_step, uint64_t* d_starts,
                        uint32_t* d_index, uint64_t cap, void* d_work, uint64_t work_bytes, hipStream_t st) {
            return launch_lset_walk_lists(kb, ls->rows, ls->base[ls->nrows], (const RangedFilter*)ls->l0_desc.p,
                                          (uint32_t)ls->l0.size(), ls->l0_rg, ls->l0_cl, d_from, d_step, d_starts,
                                          d_index, cap, d_work, work_bytes, ls->c->num_cus, st);
        };
        return LSMB_OK;
    }
    if (T0 == 0) {
        const LsetListsPlan pl = lset_lists_plan(n, ls->nrows, G);
        lp->work_bytes = pl.work_bytes;
        lp->bound = pl.pairs;  // one per row and key
        lp->sizer = "lsmb_lset_lists_work_bytes";
        lp->launch = [](lsmb_lset* ls, const KeyBatch& kb, const uint32_t*, uint32_t*, uint64_t* d_starts,
                        uint32_t* d_index, uint64_t cap, void* d_work, uint64_t work_bytes, hipStream_t st) {
            return launch_lset_lists(kb, ls->rows, ls->base[ls->nrows], d_starts, d_index, cap, d_work, work_bytes,
                                     ls->c->num_cus, st);
        };
        return LSMB_OK;
    }
    const LsetVlistsPlan pl = lset_vlists_plan(n, (uint32_t)T0, ls->nrows, G);
    lp->work_bytes = pl.work_bytes;
    lp->bound = pl.entries;  // one per L0 table, row and key
    lp->sizer = "lsmb_lset_version_lists_work_bytes";
    lp->launch = [](lsmb_lset* ls, const KeyBatch& kb, const uint32_t*, uint32_t*, uint64_t* d_starts,
                    uint32_t* d_index, uint64_t cap, void* d_work, uint64_t work_bytes, hipStream_t st) {
        return launch_lset_version_lists(kb, ls->rows, ls->base[ls->nrows], (const RangedFilter*)ls->l0_desc.p,
                                         (uint32_t)ls->l0.size(), ls->l0_rg, ls->l0_cl, d_starts, d_index, cap, d_work,
                                         work_bytes, ls->c->num_cus, st);
    };
    return LSMB_OK;
}

// The device entry path.  Nothing to probe (no key, or no table): the starts are
// cleared on the stream (and a walk's steps, when wanted, all answer "none").
static int lset_lists_dev(lsmb_lset* ls, const LsetListsProbe& lp, const void* d_data, const void* d_offsets,
                          uint32_t key_len, uint64_t n, void* d_starts, void* d_index, uint64_t cap, void* d_work,
                          uint64_t work_bytes, void* stream) {
    const bool idle = n == 0 || lp.total == 0;
    if (!idle) {
        if (!d_data) return fail(LSMB_EINVAL, "null keys");
        if (!d_work || (reinterpret_cast<uintptr_t>(d_work) & 15))
            return fail(LSMB_EINVAL, "null or misaligned workspace (16-byte alignment)");
        if (work_bytes < lp.work_bytes)
            return fail(LSMB_EINVAL, "workspace of %llu bytes, %s asks for %llu", (unsigned long long)work_bytes,
                        lp.sizer, (unsigned long long)lp.work_bytes);
    }
    DevGuard g(ls->c->dev);
    const hipStream_t st = pick_stream(ls->c, stream);
    if (idle) {
        HIP_TRY(hipMemsetAsync(d_starts, 0, (lp.total + 1) * 8, st));
        if (lp.step && n) HIP_TRY(hipMemsetAsync(lp.step, 0xFF, n * 4, st));
        return LSMB_OK;
    }
    KeyBatch kb{(const uint8_t*)d_data, (const uint64_t*)d_offsets, key_len, n};
    HIP_TRY(lp.launch(ls, kb, lp.from, lp.step, (uint64_t*)d_starts, (uint32_t*)d_index, cap, d_work, work_bytes, st));
    return LSMB_OK;
}

// The host entry path, on the context's stream and output scratch.
static int lset_lists_host(lsmb_lset* ls, const LsetListsProbe& lp, const uint8_t* data, const uint64_t* offsets,
                           uint32_t key_len, uint64_t n, uint64_t* starts, uint32_t* index, uint64_t cap) {
    if (n && host_keys_null(data, offsets, key_len, n)) return fail(LSMB_EINVAL, "null keys");
    memset(starts, 0, (lp.total + 1) * 8);
    if (n == 0 || lp.total == 0) {
        if (lp.step) std::fill(lp.step, lp.step + n, LSMB_LSET_NONE);
        return LSMB_OK;
    }
    lsmb_ctx* c = ls->c;
    DevGuard g(c->dev);
    // the scratch, carved: workspace | starts | a walk's resume points, then (in place) its steps | index
    const uint64_t dcap = std::min<uint64_t>(cap, lp.bound);
    const uint64_t sbytes = ((lp.total + 1) * 8 + kLlAlign - 1) / kLlAlign * kLlAlign;
    const uint64_t fbytes = lp.from || lp.step ? (n * 4 + kLlAlign - 1) / kLlAlign * kLlAlign : 0;
    HIP_TRY(c->out.ensure(lp.work_bytes + sbytes + fbytes + std::max<uint64_t>(dcap, 1) * 4));
    uint8_t* w = (uint8_t*)c->out.p;
    uint64_t* d_starts = (uint64_t*)(w + lp.work_bytes);
    uint32_t* d_fs = (uint32_t*)(w + lp.work_bytes + sbytes);
    uint32_t* d_index = (uint32_t*)(w + lp.work_bytes + sbytes + fbytes);
    KeyBatch kb;
    if (int rc = stage_host_keys(c, data, offsets, key_len, n, &kb)) return rc;
    if (lp.from) HIP_TRY(hipMemcpyAsync(d_fs, lp.from, n * 4, hipMemcpyHostToDevice, c->st));
    HIP_TRY(lp.launch(ls, kb, lp.from ? d_fs : nullptr, lp.step ? d_fs : nullptr, d_starts, d_index, dcap, w,
                      lp.work_bytes, c->st));
    if (lp.step) HIP_TRY(hipMemcpyAsync(lp.step, d_fs, n * 4, hipMemcpyDeviceToHost, c->st));  // lists_to_host waits
    return lists_to_host(starts, d_starts, lp.total, index, d_index, dcap, c->st);
}

int lsmb_lset_probe_lists_dev(lsmb_lset* ls, const void* d_data, const void* d_offsets, uint32_t key_len, uint64_t n,
                              void* d_starts, void* d_index, uint64_t cap, void* d_work, uint64_t work_bytes,
                              void* stream) {
    LsetListsProbe lp;
    if (int rc = lset_lists_desc(ls, LsetLists::Rows, n, d_starts, d_index, cap, &lp)) return rc;
    return lset_lists_dev(ls, lp, d_data, d_offsets, key_len, n, d_starts, d_index, cap, d_work, work_bytes, stream);
}

int lsmb_lset_probe_lists(lsmb_lset* ls, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                          uint64_t* starts, uint32_t* index, uint64_t cap) {
    LsetListsProbe lp;
    if (int rc = lset_lists_desc(ls, LsetLists::Rows, n, starts, index, cap, &lp)) return rc;
    return lset_lists_host(ls, lp, data, offsets, key_len, n, starts, index, cap);
}

// ------------------------------------------------- a whole Version per table
// The lists over Version ordinals (src/db/mod.rs:238-267): v < T0 the L0 table
// at position v, v >= T0 the rows' ordinal v - T0; V = T0 + G.
uint64_t lsmb_lset_version_tables(const lsmb_lset* ls) {
    return ls && ls->sealed ? (uint64_t)ls->l0.size() + ls->base[ls->nrows] : 0;
}

int lsmb_lset_version_order(const lsmb_lset* ls, uint32_t* ids, uint64_t* part_base) {
    if (int rc = lset_probe_check(ls)) return rc;
    const uint64_t T0 = ls->l0.size();
    if (ids) {
        for (uint64_t j = 0; j < T0; j++) ids[j] = ls->l0[j].id;
        if (!ls->ids.empty()) memcpy(ids + T0, ls->ids.data(), ls->ids.size() * sizeof(uint32_t));
    }
    if (part_base) {
        part_base[0] = 0;
        for (uint32_t r = 0; r <= ls->nrows; r++) part_base[1 + r] = T0 + ls->base[r];
    }
    return LSMB_OK;
}

uint64_t lsmb_lset_version_lists_work_bytes(const lsmb_lset* ls, uint64_t n) {
    if (!ls || !ls->sealed || n > UINT32_MAX) return 0;
    return lset_vlists_plan(n, (uint32_t)ls->l0.size(), ls->nrows, ls->base[ls->nrows]).work_bytes;
}

int lsmb_lset_probe_version_lists_dev(lsmb_lset* ls, const void* d_data, const void* d_offsets, uint32_t key_len,
                                      uint64_t n, void* d_starts, void* d_index, uint64_t cap, void* d_work,
                                      uint64_t work_bytes, void* stream) {
    LsetListsProbe lp;
    if (int rc = lset_lists_desc(ls, LsetLists::Version, n, d_starts, d_index, cap, &lp)) return rc;
    return lset_lists_dev(ls, lp, d_data, d_offsets, key_len, n, d_starts, d_index, cap, d_work, work_bytes, stream);
}

int lsmb_lset_probe_version_lists(lsmb_lset* ls, const uint8_t* data, const uint64_t* offsets, uint32_t key_len,
                                  uint64_t n, uint64_t* starts, uint32_t* index, uint64_t cap) {
    LsetListsProbe lp;
    if (int rc = lset_lists_desc(ls, LsetLists::Version, n, starts, index, cap, &lp)) return rc;
    return lset_lists_host(ls, lp, data, offsets, key_len, n, starts, index, cap);
}

// ------------------------------------------------- the walk's first candidate
// DB::get and Snapshot::get stop at the first table that holds the key
// (src/db/mod.rs:243-267, src/db/snapshot.rs:40-69).  Walk step w < T0 consults
// the L0 table at position T0-1-w (version.level(0).iter().rev()), step T0 + r
// row r; per key, the first step at or after its resume point whose table
// passes src/sstable/reader.rs:192-199's check (lset_walk_plan.hpp).
uint32_t lsmb_lset_walk_steps(const lsmb_lset* ls) {
    return ls && ls->sealed ? lset_walk_steps((uint32_t)ls->l0.size(), ls->nrows) : 0;
}

// The per-key walk probe of kb on st (d_from and d_step may be null, or one buffer).
static int lset_walk_launch(lsmb_lset* ls, const KeyBatch& kb, const uint32_t* d_from, uint32_t* d_step, uint32_t* d_ord,
                            hipStream_t st) {
    HIP_TRY(launch_lset_walk_first(kb, ls->rows, (const RangedFilter*)ls->l0_desc.p, (uint32_t)ls->l0.size(), ls->l0_rg,
                                   ls->l0_cl, d_from, d_step, d_ord, ls->c->num_cus, st));
    return LSMB_OK;
}

// What both per-key forms check before anything else.
static int lset_walk_check(const lsmb_lset* ls, uint64_t n, const void* ord) {
    if (int rc = lset_probe_check(ls)) return rc;
    if (ls->l0.size() + ls->base[ls->nrows] >= UINT32_MAX)
        return fail(LSMB_EINVAL, "more than 2^32-2 tables (0xFFFFFFFF is the 'no candidate' ordinal)");
    if (n && !ord) return fail(LSMB_EINVAL, "null ord output");
    return LSMB_OK;
}

int lsmb_lset_probe_walk_dev(lsmb_lset* ls, const void* d_data, const void* d_offsets, uint32_t key_len, uint64_t n,
                             const void* d_from, void* d_step, void* d_ord, void* stream) {
    if (int rc = lset_walk_check(ls, n, d_ord)) return rc;
    if (n == 0) return LSMB_OK;
    if (!d_data) return fail(LSMB_EINVAL, "null keys");
    DevGuard g(ls->c->dev);
    KeyBatch kb{(const uint8_t*)d_data, (const uint64_t*)d_offsets, key_len, n};
    return lset_walk_launch(ls, kb, (const uint32_t*)d_from, (uint32_t*)d_step, (uint32_t*)d_ord,
                            pick_stream(ls->c, stream));
}

int lsmb_lset_probe_walk(lsmb_lset* ls, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                         const uint32_t* from, uint32_t* step, uint32_t* ord) {
    if (int rc = lset_walk_check(ls, n, ord)) return rc;
    if (n == 0) return LSMB_OK;
    if (host_keys_null(data, offsets, key_len, n)) return fail(LSMB_EINVAL, "null keys");
    lsmb_ctx* c = ls->c;
    DevGuard g(c->dev);
    // the context's output scratch: the resume points, then (in place) the steps | the ordinals
    HIP_TRY(c->out.ensure(2 * n * 4));
    uint32_t* d_fs = (uint32_t*)c->out.p;
    uint32_t* d_ord = d_fs + n;
    KeyBatch kb;
    if (int rc = stage_host_keys(c, data, offsets, key_len, n, &kb)) return rc;
    if (from) HIP_TRY(hipMemcpyAsync(d_fs, from, n * 4, hipMemcpyHostToDevice, c->st));
    if (int rc = lset_walk_launch(ls, kb, from ? d_fs : nullptr, step ? d_fs : nullptr, d_ord, c->st)) return rc;
    if (step) HIP_TRY(hipMemcpyAsync(step, d_fs, n * 4, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipMemcpyAsync(ord, d_ord, n * 4, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    return LSMB_OK;
}

uint64_t lsmb_lset_walk_lists_work_bytes(const lsmb_lset* ls, uint64_t n) {
    if (!ls || !ls->sealed || n > UINT32_MAX) return 0;
    return lset_walk_lists_plan(n, (uint64_t)ls->l0.size() + ls->base[ls->nrows]).work_bytes;
}

int lsmb_lset_probe_walk_lists_dev(lsmb_lset* ls, const void* d_data, const void* d_offsets, uint32_t key_len,
                                   uint64_t n, const void* d_from, void* d_step, void* d_starts, void* d_index,
                                   uint64_t cap, void* d_work, uint64_t work_bytes, void* stream) {
    LsetListsProbe lp;
    if (int rc = lset_lists_desc(ls, LsetLists::Walk, n, d_starts, d_index, cap, &lp)) return rc;
    lp.from = (const uint32_t*)d_from;
    lp.step = (uint32_t*)d_step;
    return lset_lists_dev(ls, lp, d_data, d_offsets, key_len, n, d_starts, d_index, cap, d_work, work_bytes, stream);
}

int lsmb_lset_probe_walk_lists(lsmb_lset* ls, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                               const uint32_t* from, uint32_t* step, uint64_t* starts, uint32_t* index, uint64_t cap) {
    LsetListsProbe lp;
    if (int rc = lset_lists_desc(ls, LsetLists::Walk, n, starts, index, cap, &lp)) return rc;
    lp.from = from;
    lp.step = step;
    return lset_lists_host(ls, lp, data, offsets, key_len, n, starts, index, cap);
}

// ------------------------------------------------- the fill census of a Version
// SSTableBuilder sizes a table's filter from an estimate of its keys
// (src/sstable/builder.rs:74), so a sealed set may hold filters that are mostly
// ones; their words live only in the arena.  The census counts every table's
// set bits there, in Version ordinals.
int lsmb_lset_version_geometry(const lsmb_lset* ls, uint32_t* num_bits, uint32_t* num_hashes) {
    if (int rc = lset_probe_check(ls)) return rc;
    const uint64_t T0 = ls->l0.size();
    for (uint64_t j = 0; j < T0; j++) {
        if (num_bits) num_bits[j] = ls->l0[j].num_bits;
        if (num_hashes) num_hashes[j] = ls->l0[j].k;
    }
    for (size_t g = 0; g < ls->geom.size(); g++) {
        if (num_bits) num_bits[T0 + g] = ls->geom[g].num_bits;
        if (num_hashes) num_hashes[T0 + g] = ls->geom[g].k;
    }
    return LSMB_OK;
}

// The items (popcount_seg.hpp) cross through the set's pinned staging, idle
// since its last add; their counts come back next to them.
int lsmb_lset_census(lsmb_lset* ls, uint64_t* set_bits, void* stream) {
    if (int rc = lset_probe_check(ls)) return rc;
    const uint64_t T0 = ls->l0.size(), V = T0 + ls->geom.size();
    if (V == 0) return LSMB_OK;
    if (!set_bits) return fail(LSMB_EINVAL, "null output");
    std::vector<const void*> words(V);
    std::vector<uint64_t> nbits(V);
    for (uint64_t j = 0; j < T0; j++) words[j] = ls->l0[j].words, nbits[j] = ls->l0[j].num_bits;
    for (size_t g = 0; g < ls->geom.size(); g++) words[T0 + g] = ls->geom[g].words, nbits[T0 + g] = ls->geom[g].num_bits;
    std::vector<PopSeg> items;
    std::vector<uint32_t> table_of;
    popcount_items(words.data(), nbits.data(), V, &items, &table_of);
    const size_t nit = items.size();
    if (nit == 0) {  // no table has a bit
        std::fill(set_bits, set_bits + V, (uint64_t)0);
        return LSMB_OK;
    }
    DevGuard g(ls->c->dev);
    const hipStream_t st = stream ? (hipStream_t)stream : ls->ust;
    const size_t ibytes = nit * sizeof(PopSeg), cbytes = nit * sizeof(uint64_t);
    if (int rc = pinned_ensure(ls->pin_retired, &ls->pin, &ls->pin_cap, ibytes + cbytes, "level set")) return rc;
    memcpy(ls->pin, items.data(), ibytes);
    HIP_TRY(ls->segs.ensure(ibytes + cbytes));
    uint8_t* ds = (uint8_t*)ls->segs.p;
    HIP_TRY(hipMemcpyAsync(ds, ls->pin, ibytes, hipMemcpyHostToDevice, st));
    if (int rc = popcount_segs_dev((const PopSeg*)ds, nit, (uint64_t*)(ds + ibytes), st)) return rc;
    HIP_TRY(hipMemcpyAsync(ls->pin + ibytes, ds + ibytes, cbytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // the census' one wait
    popcount_fold((const uint64_t*)(ls->pin + ibytes), table_of.data(), nit, V, set_bits);
    return LSMB_OK;
}

}  // extern "C"
