// lsm_bloom.hpp — C++ host mirror of the reference's `crate::bloom` surface
// (G1DO/Storage-Engine src/bloom/mod.rs, src/bloom/builder.rs) over the C ABI
// in include/lsmbloom.h.  Header-only; link against liblsmbloom.
//
// Rust (reference)                                C++ (this header)
//   BloomFilter::new(n, fpr)        mod.rs:38-67    BloomFilter(n, fpr)
//   bf.insert(key)                  mod.rs:70-78    bf.insert(key)
//   bf.may_contain(key)             mod.rs:82-94    bf.may_contain(key)
//   bf.serialize()                  mod.rs:102-115  bf.serialize()
//   BloomFilter::deserialize(data)  mod.rs:123-168  BloomFilter::deserialize(data)   (throws Corruption)
//   bf.num_hashes() / num_bits()    mod.rs:171-178  same
//   BloomFilterBuilder::new(n, fpr) builder.rs:14   BloomFilterBuilder(n, fpr)
//   b.add_key(key)                  builder.rs:21   b.add_key(key)    (buffers the key)
//   b.build()                       builder.rs:26   b.build()         (one GPU batch)
// Reference panics (assert!, % by zero) become std::invalid_argument;
// Err(Error::Corruption(msg)) (src/error.rs:12) becomes lsm::bloom::Corruption.
// The batched build/probe run on the GPU: without a gfx950 device they throw
// (no CPU fallback), except builds of at most lsmb_host_max_keys() keys, which
// run the library's own host loop (same bits, no device round trip).
#pragma once

#include <stdint.h>

#include <array>
#include <memory>
#include <stdexcept>
#include <string>
#include <string_view>
#include <vector>

#include "../../include/lsmbloom.h"

namespace lsm::bloom {

struct Corruption : std::runtime_error {
    using std::runtime_error::runtime_error;
};
struct GpuError : std::runtime_error {
    int code;
    GpuError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

inline int check(int rc) {
    if (rc >= 0) return rc;
    const std::string msg = lsmb_last_error();
    if (rc == LSMB_ECORRUPT) throw Corruption(msg);
    if (rc == LSMB_EINVAL) throw std::invalid_argument(msg);
    throw GpuError(rc, msg);
}

namespace detail {

// Keys back to back and their keys.size() + 1 offsets: the C ABI's var-length batch.
struct PackedKeys {
    std::string data;
    std::vector<uint64_t> offs;
    const uint8_t* bytes() const { return reinterpret_cast<const uint8_t*>(data.data()); }
};
inline PackedKeys pack_keys(const std::vector<std::string>& keys) {
    PackedKeys p;
    p.offs.assign(keys.size() + 1, 0);
    for (size_t i = 0; i < keys.size(); i++) {
        p.data += keys[i];
        p.offs[i + 1] = p.data.size();
    }
    return p;
}

// Table t's min_key and max_key at koff[2t .. 2t + 2] of kb (never empty), as the batch adds take them.
template <class Range>
void pack_ranges(const std::vector<Range>& ranges, std::vector<uint8_t>* kb, std::vector<uint64_t>* koff) {
    koff->assign(2 * ranges.size() + 1, 0);
    for (size_t t = 0; t < ranges.size(); t++) {
        kb->insert(kb->end(), ranges[t].min_key.begin(), ranges[t].min_key.end());
        (*koff)[2 * t + 1] = kb->size();
        kb->insert(kb->end(), ranges[t].max_key.begin(), ranges[t].max_key.end());
        (*koff)[2 * t + 2] = kb->size();
    }
    kb->push_back(0);
}

}  // namespace detail

// One GPU (lsmb_ctx).  Movable, not copyable.
class Context {
   public:
    explicit Context(int device = -1) { check(lsmb_open(&c_, device)); }
    ~Context() { lsmb_close(c_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    Context(Context&& o) noexcept : c_(o.c_) { o.c_ = nullptr; }
    lsmb_ctx* get() const { return c_; }

    // Default context of the calling thread, opened on first use.  A context
    // is used by one thread at a time (lsmbloom.h), and the store builds from
    // more than one thread at once (flush + the background compaction thread,
    // src/compaction/scheduler.rs:37), so each thread gets its own — the same
    // choice as the Rust shim's thread_local CTX.
    static Context& shared() {
        thread_local Context ctx(-1);
        return ctx;
    }

    // Many SSTable filters from one key run (lsmb_build_batch_blocks;
    // src/sstable/builder.rs:74,93,177-182 for every output table of
    // src/compaction/scheduler.rs:147-177): table t = BloomFilterBuilder over
    // keys[seg[t] .. seg[t+1]) in a filter of (num_bits[t], num_hashes[t]);
    // returns each table's serialized block.  Always on the GPU.
    std::vector<std::vector<uint8_t>> build_batch_blocks(const std::vector<std::string>& keys,
                                                         const std::vector<uint64_t>& seg,
                                                         const std::vector<uint32_t>& num_bits,
                                                         const std::vector<uint32_t>& num_hashes) {
        const size_t ntab = num_bits.size();
        if (seg.size() != ntab + 1 || num_hashes.size() != ntab)
            throw std::invalid_argument("build_batch_blocks: seg needs ntab + 1 entries, num_hashes ntab");
        std::vector<uint64_t> boff(ntab + 1, 0);
        detail::PackedKeys pk = detail::pack_keys(keys);
        pk.data.push_back('\0');
        uint64_t total = 0;
        for (uint32_t nb : num_bits) total += lsmb_serialized_size(nb);
        std::vector<uint8_t> flat(total + 1);
        check(lsmb_build_batch_blocks(c_, pk.bytes(), pk.offs.data(), 0, keys.size(), ntab, seg.data(), num_bits.data(),
                                      num_hashes.data(), flat.data(), total, boff.data()));
        std::vector<std::vector<uint8_t>> blocks(ntab);
        for (size_t t = 0; t < ntab; t++) blocks[t].assign(flat.begin() + boff[t], flat.begin() + boff[t + 1]);
        return blocks;
    }

    // The same filters straight from written tables' data blocks
    // (lsmb_build_batch_sst_blocks; src/sstable/block/builder.rs:40-76's
    // format, src/sstable/builder.rs:93 for every key in them): block b =
    // bytes[blk_off[b] .. blk_off[b] + blk_len[b]), table t = the blocks
    // [bseg[t], bseg[t+1]).  Returns each table's serialized bloom block;
    // entries (optional) receives each table's entry count.  A table with a
    // malformed block throws Corruption naming it.  Always on the GPU.
    std::vector<std::vector<uint8_t>> build_batch_sst_blocks(const std::vector<uint8_t>& bytes,
                                                             const std::vector<uint64_t>& blk_off,
                                                             const std::vector<uint32_t>& blk_len,
                                                             const std::vector<uint64_t>& bseg,
                                                             const std::vector<uint32_t>& num_bits,
                                                             const std::vector<uint32_t>& num_hashes,
                                                             std::vector<uint64_t>* entries = nullptr) {
        const size_t ntab = num_bits.size();
        if (bseg.size() != ntab + 1 || num_hashes.size() != ntab || blk_off.size() != blk_len.size())
            throw std::invalid_argument(
                "build_batch_sst_blocks: bseg needs ntab + 1 entries, num_hashes ntab, blk_off and blk_len one per block");
        std::vector<uint64_t> boff(ntab + 1, 0), ent(ntab, 0);
        uint64_t total = 0;
        for (uint32_t nb : num_bits) total += lsmb_serialized_size(nb);
        std::vector<uint8_t> flat(total + 1);
        const uint8_t none = 0;
        check(lsmb_build_batch_sst_blocks(c_, bytes.empty() ? &none : bytes.data(), bytes.size(), blk_off.size(),
                                          blk_off.data(), blk_len.data(), ntab, bseg.data(), num_bits.data(),
                                          num_hashes.data(), flat.data(), total, boff.data(), ent.data(), nullptr));
        if (entries) *entries = ent;
        std::vector<std::vector<uint8_t>> blocks(ntab);
        for (size_t t = 0; t < ntab; t++) blocks[t].assign(flat.begin() + boff[t], flat.begin() + boff[t + 1]);
        return blocks;
    }

    // The bloom block of the table a compaction of these data blocks writes
    // (lsmb_compact_sst_bloom; run_compaction, src/compaction/scheduler.rs:
    // 91-103,147-158): the blocks as above cut into sources, source s = the
    // blocks [sseg[s], sseg[s+1]), source 0 the newest
    // (src/iterator/merge.rs:15).  The newest version of each key survives,
    // and with drop_tombstones (the task's is_bottommost) not the keys whose
    // newest version is a tombstone.  expected_items = 0 sizes the filter for
    // the survivors; 1000 with fpr 0.01 is SSTableBuilder's own
    // (src/sstable/builder.rs:74).  A malformed or empty block throws
    // Corruption naming it.  Always on the GPU.
    struct CompactedFilter {
        std::vector<uint8_t> bloom;  // BloomFilter::serialize's bytes
        uint32_t num_bits = 0, num_hashes = 0;
        uint64_t entry_count = 0;    // the meta block's (builder.rs:139-162)
    };
    CompactedFilter compact_sst_bloom(const std::vector<uint8_t>& bytes, const std::vector<uint64_t>& blk_off,
                                      const std::vector<uint32_t>& blk_len, const std::vector<uint64_t>& sseg,
                                      bool drop_tombstones, uint64_t expected_items = 0, double fpr = 0.01) {
        if (sseg.empty() || blk_off.size() != blk_len.size())
            throw std::invalid_argument("compact_sst_bloom: sseg needs nsrc + 1 entries, blk_off and blk_len one per block");
        // a first size: the filter asked for, or one for every entry the blocks can hold without overlap
        uint64_t guess = expected_items;
        if (!guess) {
            for (uint32_t l : blk_len) guess += l;
            guess = guess / 6 ? guess / 6 : 1;
        }
        uint32_t nb = 0, k = 0;
        check(lsmb_params(guess, fpr, &nb, &k));
        CompactedFilter out;
        uint64_t cap = lsmb_serialized_size(nb), len = 0;
        const uint8_t none = 0;
        int rc = LSMB_OK;
        for (int pass = 0; pass < 2; pass++) {
            out.bloom.assign(cap, 0);
            rc = lsmb_compact_sst_bloom(c_, bytes.empty() ? &none : bytes.data(), bytes.size(), blk_off.size(), blk_off.data(),
                                        blk_len.data(), sseg.size() - 1, sseg.data(), drop_tombstones ? 1 : 0,
                                        expected_items, fpr, out.bloom.data(), cap, &len, &out.entry_count, &out.num_bits,
                                        &out.num_hashes);
            if (rc != LSMB_EINVAL || len <= cap) break;
            cap = len;  // the block is larger than the guess (overlapping entries): once more
        }
        check(rc);
        out.bloom.resize(len);
        return out;
    }

   private:
    lsmb_ctx* c_ = nullptr;
};

class BloomFilter {
   public:
    BloomFilter(size_t expected_items, double false_positive_rate) {
        check(lsmb_params(expected_items, false_positive_rate, &num_bits_, &num_hashes_));
        bits_.assign(lsmb_num_words(num_bits_), 0);
    }

    void insert(std::string_view key) { insert(key.data(), key.size()); }
    void insert(const void* key, size_t len) {
        check(lsmb_insert(bits_.data(), num_bits_, num_hashes_, static_cast<const uint8_t*>(key), len));
    }
    bool may_contain(std::string_view key) const { return may_contain(key.data(), key.size()); }
    bool may_contain(const void* key, size_t len) const {
        return check(lsmb_may_contain(bits_.data(), num_bits_, num_hashes_, static_cast<const uint8_t*>(key),
                                      len)) == 1;
    }

    std::vector<uint8_t> serialize() const {
        std::vector<uint8_t> out(lsmb_serialized_size(num_bits_));
        check(lsmb_serialize(bits_.data(), num_bits_, num_hashes_, out.data(), out.size()));
        return out;
    }
    static BloomFilter deserialize(const std::vector<uint8_t>& data) { return deserialize(data.data(), data.size()); }
    static BloomFilter deserialize(const uint8_t* data, size_t len) {
        uint32_t k = 0, nb = 0, nw = 0;
        check(lsmb_deserialize_header(data, len, &k, &nb, &nw));
        BloomFilter f;
        f.num_hashes_ = k;
        f.num_bits_ = nb;
        f.bits_.assign(nw, 0);
        check(lsmb_deserialize(data, len, f.bits_.data(), nw));
        return f;
    }

    uint32_t num_hashes() const { return num_hashes_; }
    uint32_t num_bits() const { return num_bits_; }
    const std::vector<uint64_t>& words() const { return bits_; }
    std::vector<uint64_t>& words() { return bits_; }

    // Additive batched probe (the reference has no multi-get): for each key,
    // a bitmask row over `filters` (bit f = may_contain(filters[f], key)).
    static std::vector<uint8_t> may_contain_batch(const std::vector<const BloomFilter*>& filters,
                                                  const std::vector<std::string>& keys,
                                                  Context& ctx = Context::shared()) {
        const uint32_t nf = static_cast<uint32_t>(filters.size());
        std::vector<const uint64_t*> w(nf);
        std::vector<uint32_t> nb(nf), kk(nf);
        for (uint32_t f = 0; f < nf; f++) {
            w[f] = filters[f]->bits_.data();
            nb[f] = filters[f]->num_bits_;
            kk[f] = filters[f]->num_hashes_;
        }
        const detail::PackedKeys pk = detail::pack_keys(keys);
        std::vector<uint8_t> out(keys.size() * ((nf + 7) / 8));
        check(lsmb_probe(ctx.get(), w.data(), nb.data(), kk.data(), nf, pk.bytes(), pk.offs.data(), 0, keys.size(),
                         out.data()));
        return out;
    }

   private:
    BloomFilter() = default;
    friend class BloomFilterBuilder;
    std::vector<uint64_t> bits_;
    uint32_t num_hashes_ = 0;
    uint32_t num_bits_ = 0;
};

// Buffers the run's keys in a packed arena and builds the whole filter in one
// GPU batch at build() (the reference inserts on the fly, builder.rs:5-7, 21-23);
// the bits are identical.
class BloomFilterBuilder {
   public:
    BloomFilterBuilder(size_t estimated_keys, double false_positive_rate, Context* ctx = nullptr)
        : filter_(estimated_keys, false_positive_rate), ctx_(ctx) {
        offsets_.push_back(0);
    }
    void add_key(std::string_view key) { add_key(key.data(), key.size()); }
    void add_key(const void* key, size_t len) {
        const uint8_t* p = static_cast<const uint8_t*>(key);
        data_.insert(data_.end(), p, p + len);
        offsets_.push_back(data_.size());
    }
    BloomFilter build() {
        if (offsets_.size() > 1) {
            check(lsmb_build_var(ctx_for(offsets_.size() - 1), data_.data(), offsets_.data(), offsets_.size() - 1,
                                 filter_.num_bits_, filter_.num_hashes_, filter_.bits_.data()));
        }
        return std::move(filter_);
    }
    // build().serialize() in one call (lsmb_build_block): the bloom block
    // SSTableBuilder::finish writes (src/sstable/builder.rs:177-179), with the
    // words copied device -> block directly.
    std::vector<uint8_t> build_serialized() {
        std::vector<uint8_t> block(lsmb_serialized_size(filter_.num_bits_));
        check(lsmb_build_block(ctx_for(offsets_.size() - 1), data_.empty() ? nullptr : data_.data(), offsets_.data(),
                               0, offsets_.size() - 1, filter_.num_bits_, filter_.num_hashes_, block.data(),
                               block.size()));
        return block;
    }

   private:
    // Builds of at most lsmb_host_max_keys() keys (an SST flush at the
    // reference's default 1 000-key sizing) run the library's host loop and
    // need no GPU; bigger ones take the GPU context (throws without one).
    lsmb_ctx* ctx_for(size_t n) {
        if (n <= lsmb_host_max_keys()) return nullptr;
        return (ctx_ ? *ctx_ : Context::shared()).get();
    }
    BloomFilter filter_;
    Context* ctx_;
    std::vector<uint8_t> data_;
    std::vector<uint64_t> offsets_;
};

// Device-resident SSTable filters with key ranges (lsmb_fset): probe(keys)[i]
// bit s = (min_s <= key i <= max_s) && may_contain(filter s, key i), the
// checks SSTable::get makes before reading the index (reader.rs:192-199).
class FilterSet {
   public:
    explicit FilterSet(Context& ctx = Context::shared()) { check(lsmb_fset_open(ctx.get(), &fs_)); }
    ~FilterSet() { lsmb_fset_close(fs_); }
    FilterSet(const FilterSet&) = delete;
    FilterSet& operator=(const FilterSet&) = delete;

    // From a serialized bloom block (throws Corruption like deserialize); returns the slot.
    int add(const std::vector<uint8_t>& block, std::string_view min_key, std::string_view max_key) {
        return check(lsmb_fset_add(fs_, block.data(), block.size(), u8(min_key), min_key.size(), u8(max_key),
                                   max_key.size()));
    }
    int add(const BloomFilter& f, std::string_view min_key, std::string_view max_key) {
        return check(lsmb_fset_add_words(fs_, f.words().data(), f.num_bits(), f.num_hashes(), u8(min_key),
                                         min_key.size(), u8(max_key), max_key.size()));
    }
    void remove(int slot) { check(lsmb_fset_remove(fs_, slot)); }
    uint64_t live_mask() const { return lsmb_fset_live_mask(fs_); }

    std::vector<uint64_t> probe(const std::vector<std::string>& keys) {
        const detail::PackedKeys pk = detail::pack_keys(keys);
        std::vector<uint64_t> out(keys.size());
        check(lsmb_fset_probe(fs_, pk.bytes(), pk.offs.data(), 0, keys.size(), out.data()));
        return out;
    }

    // The answer per table (lsmb_fset_probe_lists): index[starts[s] ..
    // starts[s+1]) = the ascending indices of the keys with bit s set in
    // probe()'s mask.  Sized for one entry per key; a longer answer takes one
    // more call with the size the first one reported.
    struct Lists {
        std::array<uint64_t, 65> starts;
        std::vector<uint32_t> index;
    };
    Lists probe_lists(const std::vector<std::string>& keys) {
        const detail::PackedKeys pk = detail::pack_keys(keys);
        Lists out;
        out.index.resize(keys.size());
        for (;;) {
            const uint64_t cap = out.index.size();
            check(lsmb_fset_probe_lists(fs_, pk.bytes(), pk.offs.data(), 0, keys.size(), out.starts.data(),
                                        out.index.data(), cap));
            out.index.resize(out.starts[64]);
            if (out.starts[64] <= cap) return out;
        }
    }

   private:
    static const uint8_t* u8(std::string_view s) { return reinterpret_cast<const uint8_t*>(s.data()); }
    lsmb_fset* fs_ = nullptr;
};

// Device-resident snapshot of the store's non-overlapping levels (lsmb_lset),
// one per Version: rows of tables with pairwise disjoint key ranges, any
// number per row.  add in any order, seal(), then probe(keys)[r * n + i] =
// the table_id of the one table t of row r with min_t <= key i <= max_t &&
// may_contain(filter t, key i), else LSMB_LSET_NONE (the walk of L1 and below
// in DB::get, src/db/mod.rs:255-267).
class LevelSet {
   public:
    explicit LevelSet(Context& ctx = Context::shared()) { check(lsmb_lset_open(ctx.get(), &ls_)); }
    ~LevelSet() { lsmb_lset_close(ls_); }
    LevelSet(const LevelSet&) = delete;
    LevelSet& operator=(const LevelSet&) = delete;

    // From a serialized bloom block (throws Corruption like deserialize).
    void add(uint32_t row, uint32_t table_id, const std::vector<uint8_t>& block, std::string_view min_key,
             std::string_view max_key) {
        check(lsmb_lset_add(ls_, row, table_id, block.data(), block.size(), u8(min_key), min_key.size(), u8(max_key),
                            max_key.size()));
    }
    void add(uint32_t row, uint32_t table_id, const BloomFilter& f, std::string_view min_key, std::string_view max_key) {
        check(lsmb_lset_add_words(ls_, row, table_id, f.words().data(), f.num_bits(), f.num_hashes(), u8(min_key),
                                  min_key.size(), u8(max_key), max_key.size()));
    }
    // Sorts and checks the rows (std::invalid_argument naming two overlapping tables).
    void seal() { check(lsmb_lset_seal(ls_)); }

    // Version edit (lsmb_lset_derive, src/compaction/scheduler.rs:163-177): a
    // new, unsealed set holding every table of this sealed one whose id is not
    // in drop_ids, sharing the device filter words.  Then add / add_many /
    // seal; the two sets are destroyed in either order.
    std::unique_ptr<LevelSet> derive(const std::vector<uint32_t>& drop_ids, uint64_t* dropped = nullptr) const {
        lsmb_lset* h = nullptr;
        check(lsmb_lset_derive(ls_, drop_ids.data(), drop_ids.size(), dropped, &h));
        return std::unique_ptr<LevelSet>(new LevelSet(h));
    }
    // derive that also repacks sparse arena chunks on the device
    // (lsmb_lset_derive_packed; src/compaction/scheduler.rs:163-177,
    // src/db/mod.rs:402): the survivors of every chunk of this set whose live
    // share is below min_ppm millionths (LSMB_LSET_REPACK_ALL: every survivor)
    // move into a chunk of the new set's own, device to device on stream, and
    // the new set's next add continues there.  moved: {tables, slot bytes}.
    std::unique_ptr<LevelSet> derive_packed(const std::vector<uint32_t>& drop_ids, uint32_t min_ppm,
                                            uint64_t* dropped = nullptr, std::array<uint64_t, 2>* moved = nullptr,
                                            void* stream = nullptr) const {
        lsmb_lset* h = nullptr;
        check(lsmb_lset_derive_packed(ls_, drop_ids.data(), drop_ids.size(), min_ppm, dropped,
                                      moved ? moved->data() : nullptr, &h, stream));
        return std::unique_ptr<LevelSet>(new LevelSet(h));
    }
    // Many tables in one call (lsmb_lset_add_batch): all or nothing; crcs
    // (optional) are checked on the device copies.  Throws as add does for the
    // first failing table; status (optional) receives every table's own code.
    struct TableRange {
        std::string min_key, max_key;
    };
    void add_many(const std::vector<uint32_t>& rows, const std::vector<uint32_t>& table_ids,
                  const std::vector<std::vector<uint8_t>>& blocks, const std::vector<TableRange>& ranges,
                  const std::vector<uint32_t>* crcs = nullptr, std::vector<int32_t>* status = nullptr) {
        const size_t n = blocks.size();
        if (rows.size() != n || table_ids.size() != n || ranges.size() != n || (crcs && crcs->size() != n))
            throw std::invalid_argument("add_many: rows, table_ids, blocks, ranges and crcs differ in length");
        std::vector<uint8_t> bb, kb;
        std::vector<uint64_t> boff(n + 1, 0), koff;
        for (size_t t = 0; t < n; t++) {
            bb.insert(bb.end(), blocks[t].begin(), blocks[t].end());
            boff[t + 1] = bb.size();
        }
        bb.push_back(0);
        detail::pack_ranges(ranges, &kb, &koff);
        if (status) status->assign(n, 0);
        check(lsmb_lset_add_batch(ls_, n, rows.data(), table_ids.data(), bb.data(), boff.data(),
                                  crcs ? crcs->data() : nullptr, kb.data(), koff.data(),
                                  status && n ? status->data() : nullptr));
    }
    // Tables whose filter words lsmb_build_batch_dev left on this set's device
    // (lsmb_lset_add_batch_dev): d_words in the layout of
    // lsmb_build_batch_layout(num_bits).  The words move device to device on
    // `stream`, which is synchronised once; all or nothing.
    void add_built(const std::vector<uint32_t>& rows, const std::vector<uint32_t>& table_ids, const void* d_words,
                   const std::vector<uint32_t>& num_bits, const std::vector<uint32_t>& num_hashes,
                   const std::vector<TableRange>& ranges, void* stream = nullptr) {
        const size_t n = ranges.size();
        if (rows.size() != n || table_ids.size() != n || num_bits.size() != n || num_hashes.size() != n)
            throw std::invalid_argument("add_built: rows, table_ids, num_bits, num_hashes and ranges differ in length");
        std::vector<uint64_t> woff(n + 1, 0), koff;
        check(lsmb_build_batch_layout(n, num_bits.data(), woff.data()));
        std::vector<uint8_t> kb;
        detail::pack_ranges(ranges, &kb, &koff);
        check(lsmb_lset_add_batch_dev(ls_, n, rows.data(), table_ids.data(), d_words, woff.data(), num_bits.data(),
                                      num_hashes.data(), kb.data(), koff.data(), stream));
    }
    // lsmb_lset_stats: [0] tables, [1] inherited by derive, [2] filter bytes
    // and [3] copy calls of this set's own uploads, [4] device bytes of the
    // arena chunks it keeps alive, [5] filter bytes of its tables.
    std::array<uint64_t, 6> stats() const {
        std::array<uint64_t, 6> s{};
        check(lsmb_lset_stats(ls_, s.data()));
        return s;
    }
    int rows() const { return lsmb_lset_rows(ls_); }
    uint64_t tables(uint32_t row) const { return lsmb_lset_tables(ls_, row); }

    std::vector<uint32_t> probe(const std::vector<std::string>& keys) {
        const detail::PackedKeys pk = detail::pack_keys(keys);
        std::vector<uint32_t> out(static_cast<size_t>(rows()) * keys.size());
        check(lsmb_lset_probe(ls_, pk.bytes(), pk.offs.data(), 0, keys.size(), out.data()));
        return out;
    }
    // Device keys and output (rows() * n uint32_t), asynchronous on `stream`.
    void probe_dev(const void* d_data, const void* d_offsets, uint32_t key_len, uint64_t n, void* d_out,
                   void* stream = nullptr) {
        check(lsmb_lset_probe_dev(ls_, d_data, d_offsets, key_len, n, d_out, stream));
    }

    // The L0 part (every add takes row = LSMB_LSET_ROW_L0): up to
    // LSMB_LSET_L0_MAX tables with overlapping ranges, position = order of
    // arrival, survivors of derive first.  With it one sealed set is one
    // Version (src/db/mod.rs:238-267); a flush or a compaction is derive + add
    // + seal.
    uint64_t l0_tables() const { return lsmb_lset_l0_tables(ls_); }
    std::vector<uint32_t> l0_order() const {
        std::vector<uint32_t> ids(l0_tables());
        uint32_t none = 0;
        check(lsmb_lset_l0_order(ls_, ids.empty() ? &none : ids.data()));
        return ids;
    }
    // mask[i] bit j = min_j <= key i <= max_j && may_contain(filter j, key i)
    // for the L0 table at position j (read the set bits from the highest
    // down); ids = probe()'s answer, from the same hash.
    struct VersionAnswer {
        std::vector<uint64_t> mask;  // keys.size()
        std::vector<uint32_t> ids;   // rows() * keys.size()
    };
    VersionAnswer probe_version(const std::vector<std::string>& keys) {
        const detail::PackedKeys pk = detail::pack_keys(keys);
        VersionAnswer a;
        a.mask.assign(keys.size(), 0);
        a.ids.resize(static_cast<size_t>(rows()) * keys.size());
        check(lsmb_lset_probe_version(ls_, pk.bytes(), pk.offs.data(), 0, keys.size(), a.mask.data(),
                                      a.ids.empty() ? nullptr : a.ids.data()));
        return a;
    }
    // Device keys and outputs (d_l0_mask: n uint64_t, d_out: rows() * n
    // uint32_t, null when the set has no row), asynchronous on `stream`.
    void probe_version_dev(const void* d_data, const void* d_offsets, uint32_t key_len, uint64_t n, void* d_l0_mask,
                           void* d_out, void* stream = nullptr) {
        check(lsmb_lset_probe_version_dev(ls_, d_data, d_offsets, key_len, n, d_l0_mask, d_out, stream));
    }

    // The answer per table (lsmb_lset_probe_lists), keyed by ordinal: table j
    // of row r in the row's sealed order (ascending min_key) is ordinal
    // row_base[r] + j, ids[g] its table id.
    uint64_t total_tables() const { return lsmb_lset_total_tables(ls_); }
    struct TableOrder {
        std::vector<uint32_t> ids;       // total_tables()
        std::vector<uint64_t> row_base;  // rows() + 1
    };
    TableOrder table_order() const {
        TableOrder o;
        o.ids.resize(total_tables());
        o.row_base.resize(static_cast<size_t>(rows()) + 1);
        check(lsmb_lset_table_order(ls_, o.ids.data(), o.row_base.data()));
        return o;
    }
    // index[starts[g] .. starts[g+1]) = the ascending indices of the keys for
    // which probe() answers table g in g's row; starts has total_tables() + 1
    // entries.  A counting call sizes the index.
    struct Lists {
        std::vector<uint64_t> starts;
        std::vector<uint32_t> index;
    };
    Lists probe_lists(const std::vector<std::string>& keys) {
        return lists_via(lsmb_lset_probe_lists, total_tables(), keys);
    }
    // Device keys, outputs (d_starts: total_tables() + 1 uint64_t, d_index: cap
    // uint32_t) and workspace (lists_work_bytes(n) bytes), asynchronous on `stream`.
    uint64_t lists_work_bytes(uint64_t n) const { return lsmb_lset_lists_work_bytes(ls_, n); }
    void probe_lists_dev(const void* d_data, const void* d_offsets, uint32_t key_len, uint64_t n, void* d_starts,
                         void* d_index, uint64_t cap, void* d_work, uint64_t work_bytes, void* stream = nullptr) {
        check(lsmb_lset_probe_lists_dev(ls_, d_data, d_offsets, key_len, n, d_starts, d_index, cap, d_work, work_bytes,
                                        stream));
    }

    // The whole Version per table (lsmb_lset_probe_version_lists), keyed by
    // Version ordinal: v < l0_tables() is the L0 table at position v (walk
    // them from the highest down for newest first, src/db/mod.rs:243), v >=
    // l0_tables() the rows' ordinal v - l0_tables().
    uint64_t version_tables() const { return lsmb_lset_version_tables(ls_); }
    struct VersionOrder {
        std::vector<uint32_t> ids;        // version_tables(): l0_order(), then table_order().ids
        std::vector<uint64_t> part_base;  // rows() + 2: 0, T0, T0 + row_base[1], ..., version_tables()
    };
    VersionOrder version_order() const {
        VersionOrder o;
        o.ids.resize(version_tables());
        o.part_base.resize(static_cast<size_t>(rows()) + 2);
        check(lsmb_lset_version_order(ls_, o.ids.data(), o.part_base.data()));
        return o;
    }
    // Every table's filter geometry in version_order()'s order
    // (lsmb_lset_version_geometry; src/bloom/mod.rs:38-68).
    struct VersionGeometry {
        std::vector<uint32_t> num_bits, num_hashes;  // version_tables() each
    };
    VersionGeometry version_geometry() const {
        VersionGeometry g;
        g.num_bits.resize(version_tables());
        g.num_hashes.resize(version_tables());
        check(lsmb_lset_version_geometry(ls_, g.num_bits.data(), g.num_hashes.data()));
        return g;
    }
    // The fill of every table's resident filter (lsmb_lset_census: one launch
    // on `stream`, one wait), in version_order()'s order: set_bits below
    // num_bits, fpr = lsmb_fill_fpr (the false-positive rate the fill
    // predicts), keys = lsmb_fill_keys (the distinct keys a filter of that
    // fill holds, against src/sstable/builder.rs:74's estimate).  Not cached:
    // a sealed set is immutable, so call it once per Version.
    struct Census {
        std::vector<uint32_t> ids, num_bits, num_hashes;
        std::vector<uint64_t> set_bits;
        std::vector<double> fpr, keys;
    };
    Census census(void* stream = nullptr) {
        Census c;
        c.ids = version_order().ids;
        VersionGeometry g = version_geometry();
        c.num_bits = std::move(g.num_bits);
        c.num_hashes = std::move(g.num_hashes);
        const size_t V = c.ids.size();
        c.set_bits.assign(V, 0);
        check(lsmb_lset_census(ls_, c.set_bits.data(), stream));
        c.fpr.resize(V);
        c.keys.resize(V);
        for (size_t v = 0; v < V; v++) {
            c.fpr[v] = lsmb_fill_fpr(c.num_bits[v], c.num_hashes[v], c.set_bits[v]);
            c.keys[v] = lsmb_fill_keys(c.num_bits[v], c.num_hashes[v], c.set_bits[v]);
        }
        return c;
    }
    // index[starts[v] .. starts[v+1]) = the ascending indices of the keys that
    // table v answers (bit v of probe_version()'s mask, or probe()'s answer in
    // its row), from one hash per key; starts has version_tables() + 1
    // entries.  A counting call sizes the index.
    Lists probe_version_lists(const std::vector<std::string>& keys) {
        return lists_via(lsmb_lset_probe_version_lists, version_tables(), keys);
    }
    // Device keys, outputs (d_starts: version_tables() + 1 uint64_t, d_index:
    // cap uint32_t) and workspace (version_lists_work_bytes(n) bytes),
    // asynchronous on `stream`.
    uint64_t version_lists_work_bytes(uint64_t n) const { return lsmb_lset_version_lists_work_bytes(ls_, n); }
    void probe_version_lists_dev(const void* d_data, const void* d_offsets, uint32_t key_len, uint64_t n,
                                 void* d_starts, void* d_index, uint64_t cap, void* d_work, uint64_t work_bytes,
                                 void* stream = nullptr) {
        check(lsmb_lset_probe_version_lists_dev(ls_, d_data, d_offsets, key_len, n, d_starts, d_index, cap, d_work,
                                                work_bytes, stream));
    }

    // The walk itself (lsmb_lset_probe_walk): DB::get stops at the first table
    // that holds the key (src/db/mod.rs:243-267).  Step w < l0_tables()
    // consults the L0 table at position l0_tables() - 1 - w (step 0 the
    // newest), step l0_tables() + r row r; walk_steps() in all.  Per key: the
    // first step at or after its resume step (`from`, null: 0) with a
    // candidate and that table's Version ordinal, LSMB_LSET_NONE in both when
    // there is none or the resume step is >= walk_steps() (a retired key).
    // A multi-get repeats the probe with from = step + 1 for the false
    // positives and from = LSMB_LSET_NONE for the keys it found.
    uint32_t walk_steps() const { return lsmb_lset_walk_steps(ls_); }
    struct WalkAnswer {
        std::vector<uint32_t> step, ord;  // n each
    };
    // Packed host keys: offsets null selects fixed-length keys of key_len bytes.
    WalkAnswer probe_walk(const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                          const std::vector<uint32_t>* from = nullptr) {
        if (from && from->size() != n) throw std::invalid_argument("probe_walk: one resume step per key");
        WalkAnswer a;
        a.step.resize(n);
        a.ord.resize(n);
        uint32_t none = 0;
        check(lsmb_lset_probe_walk(ls_, data, offsets, key_len, n, from && n ? from->data() : nullptr,
                                   n ? a.step.data() : &none, n ? a.ord.data() : &none));
        return a;
    }
    WalkAnswer probe_walk_keys(const std::vector<std::string>& keys, const std::vector<uint32_t>* from = nullptr) {
        const detail::PackedKeys pk = detail::pack_keys(keys);
        return probe_walk(pk.bytes(), pk.offs.data(), 0, keys.size(), from);
    }
    // Device keys, resume steps (d_from, may be null) and outputs (d_step: n
    // uint32_t, may be null or d_from itself; d_ord: n uint32_t),
    // asynchronous on `stream`.
    void probe_walk_dev(const void* d_data, const void* d_offsets, uint32_t key_len, uint64_t n, const void* d_from,
                        void* d_step, void* d_ord, void* stream = nullptr) {
        check(lsmb_lset_probe_walk_dev(ls_, d_data, d_offsets, key_len, n, d_from, d_step, d_ord, stream));
    }
    // The same answer per table: index[starts[v] .. starts[v+1]) = the
    // ascending indices of the keys whose first candidate is Version ordinal
    // v; a key is in at most one list.  A counting call sizes the index.
    struct WalkLists {
        std::vector<uint64_t> starts;  // version_tables() + 1
        std::vector<uint32_t> index;
        std::vector<uint32_t> step;  // n
    };
    WalkLists probe_walk_lists(const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                               const std::vector<uint32_t>* from = nullptr) {
        if (from && from->size() != n) throw std::invalid_argument("probe_walk_lists: one resume step per key");
        WalkLists out;
        out.starts.assign(version_tables() + 1, 0);
        out.step.resize(n);
        uint32_t none = 0;
        const uint32_t* f = from && n ? from->data() : nullptr;
        uint32_t* s = n ? out.step.data() : &none;
        check(lsmb_lset_probe_walk_lists(ls_, data, offsets, key_len, n, f, s, out.starts.data(), nullptr, 0));
        out.index.resize(out.starts.back());
        if (!out.index.empty())
            check(lsmb_lset_probe_walk_lists(ls_, data, offsets, key_len, n, f, s, out.starts.data(), out.index.data(),
                                             out.index.size()));
        return out;
    }
    WalkLists probe_walk_lists_keys(const std::vector<std::string>& keys, const std::vector<uint32_t>* from = nullptr) {
        const detail::PackedKeys pk = detail::pack_keys(keys);
        return probe_walk_lists(pk.bytes(), pk.offs.data(), 0, keys.size(), from);
    }
    // Device keys, resume steps, outputs (d_step optional; d_starts:
    // version_tables() + 1 uint64_t; d_index: cap uint32_t) and workspace
    // (walk_lists_work_bytes(n) bytes), asynchronous on `stream`.
    uint64_t walk_lists_work_bytes(uint64_t n) const { return lsmb_lset_walk_lists_work_bytes(ls_, n); }
    void probe_walk_lists_dev(const void* d_data, const void* d_offsets, uint32_t key_len, uint64_t n,
                              const void* d_from, void* d_step, void* d_starts, void* d_index, uint64_t cap,
                              void* d_work, uint64_t work_bytes, void* stream = nullptr) {
        check(lsmb_lset_probe_walk_lists_dev(ls_, d_data, d_offsets, key_len, n, d_from, d_step, d_starts, d_index, cap,
                                             d_work, work_bytes, stream));
    }

   private:
    explicit LevelSet(lsmb_lset* h) : ls_(h) {}  // derive
    static const uint8_t* u8(std::string_view s) { return reinterpret_cast<const uint8_t*>(s.data()); }
    // probe_lists and probe_version_lists: fn the C entry point, total its table count.
    template <class Fn>
    Lists lists_via(Fn fn, uint64_t total, const std::vector<std::string>& keys) {
        const detail::PackedKeys pk = detail::pack_keys(keys);
        Lists out;
        out.starts.assign(total + 1, 0);
        check(fn(ls_, pk.bytes(), pk.offs.data(), 0, keys.size(), out.starts.data(), nullptr, 0));
        out.index.resize(out.starts.back());
        if (!out.index.empty())
            check(fn(ls_, pk.bytes(), pk.offs.data(), 0, keys.size(), out.starts.data(), out.index.data(),
                     out.index.size()));
        return out;
    }
    lsmb_lset* ls_ = nullptr;
};

}  // namespace lsm::bloom
