/*
 * lsmbloom.h — C ABI of the MI355X-native Bloom-filter engine.
 *
 * Drop-in boundary for G1DO/Storage-Engine `src/bloom` (Rust).  The store's
 * callers — SSTableBuilder (src/sstable/builder.rs:74,93,177-182), SSTable::open
 * (src/sstable/reader.rs:78-82), SSTable::get (src/sstable/reader.rs:197) — keep
 * calling the Rust surface `crate::bloom::{BloomFilter, BloomFilterBuilder}`;
 * a thin Rust shim forwards to the entry points below.
 *
 * Conventions
 *   - Plain pointers and sizes only; all buffers are caller-owned and the
 *     library keeps no pointer after a call returns.
 *   - Return 0 (LSMB_OK) on success, a negative LSMB_E* code otherwise; the
 *     thread-local message of the last failure is lsmb_last_error().
 *   - Where the reference panics (assert!/division by zero), the ABI returns
 *     LSMB_EINVAL; where it returns Err(Error::Corruption) (deserialize), the
 *     ABI returns LSMB_ECORRUPT (src/error.rs:12).
 *   - Filter words are the reference's `bits: Vec<u64>` (src/bloom/mod.rs:24):
 *     ceil(num_bits/64) little-endian u64, bit p = word p/64, bit p%64.
 *   - Batched build entry points OR-ACCUMULATE into `words` (existing bits are
 *     kept), so a build after insert()s, or a merge of shard partials, is exact.
 *   - Batched entry points run on the GPU.  With no usable gfx950 device,
 *     lsmb_open fails with LSMB_ENODEV: there is no silent CPU fallback.  The
 *     one host path is deliberate and size-bounded: host-memory builds of at
 *     most lsmb_host_max_keys() keys (an SST flush of the reference's default
 *     1 000-key sizing, src/sstable/builder.rs:51,74) run the library's own
 *     per-key loop, where a device round trip costs more than the whole build;
 *     for those ctx may be NULL, so the store works on a host without a GPU.
 *   - Thread safety: a context may be used from one thread at a time; distinct
 *     contexts (e.g. flush + background compaction, src/compaction/scheduler.rs:37)
 *     may run concurrently.  Stateless functions are always thread safe.
 */
#ifndef LSMBLOOM_H
#define LSMBLOOM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSMB_OK 0
#define LSMB_EINVAL (-1)   /* argument the reference rejects by panicking      */
#define LSMB_ENODEV (-2)   /* no gfx950 device / HIP initialisation failed     */
#define LSMB_EHIP (-3)     /* HIP runtime or kernel launch error               */
#define LSMB_ECORRUPT (-4) /* serialized filter fails validation               */
#define LSMB_ENOMEM (-5)   /* device or pinned-host allocation failed          */

#define LSMB_ABI_VERSION 6 /* 5: sweep builds, block CRC-32; 6: fail-safe merge status words */

typedef struct lsmb_ctx lsmb_ctx; /* one GPU: stream, events, scratch arenas */

int lsmb_abi_version(void);
const char* lsmb_last_error(void);

/* ---- sizing ------------------------------------------------------------ */

/* BloomFilter::new(expected_items, false_positive_rate) sizing
 * (src/bloom/mod.rs:38-67): num_bits = max(sat_u32(ceil(n * -1.44*log2 fpr)), 64),
 * num_hashes = max(ceil(bpk * ln 2), 1).  LSMB_EINVAL where the reference
 * panics (n == 0, fpr outside (0,1); :39-43). */
int lsmb_params(uint64_t expected_items, double false_positive_rate, uint32_t* num_bits,
                uint32_t* num_hashes);

/* The false-positive rate a filter's FILL predicts, (set_bits / num_bits)^num_hashes: the chance
 * that may_contain finds all num_hashes positions of an absent key set.  The sizing above
 * (src/bloom/mod.rs:38-68) aims the fill at 1/2 for expected_items keys; SSTableBuilder passes an
 * ESTIMATE there (src/sstable/builder.rs:74), and a table that holds several times the estimate has
 * a fill near 1 and answers true to nearly everything.  set_bits comes from lsmb_lset_census or
 * lsmb_popcount_segs_dev.  num_hashes == 0 gives 1.0 (may_contain is then always true), also with
 * num_bits == 0; set_bits > num_bits gives NaN, as does num_bits == 0 with num_hashes > 0.  Pure
 * host arithmetic in doubles. */
double lsmb_fill_fpr(uint32_t num_bits, uint32_t num_hashes, uint64_t set_bits);

/* The number of DISTINCT keys a filter of that fill holds, -(m/k) * ln(1 - X/m) with m = num_bits,
 * k = num_hashes, X = set_bits: the quantity to set against the estimated_keys the filter was sized
 * for (src/sstable/builder.rs:74, through src/bloom/mod.rs:38-68).  X == m gives +inf (the filter
 * is full: no count can be told), X == 0 gives 0; num_hashes == 0 and set_bits > num_bits give NaN. */
double lsmb_fill_keys(uint32_t num_bits, uint32_t num_hashes, uint64_t set_bits);

/* ceil(num_bits / 64): length of the words array (src/bloom/mod.rs:58). */
uint64_t lsmb_num_words(uint32_t num_bits);

/* ---- format (src/bloom/mod.rs:102-168) --------------------------------- */

/* 12 + 8 * ceil(num_bits/64)  (serialize, :102-115). */
uint64_t lsmb_serialized_size(uint32_t num_bits);

/* BloomFilter::serialize (:102-115): [num_hashes u32][num_bits u32]
 * [num_u64s u32][words u64...] little-endian.  out_len must be >= the size. */
int lsmb_serialize(const uint64_t* words, uint32_t num_bits, uint32_t num_hashes, uint8_t* out,
                   uint64_t out_len);

/* BloomFilter::deserialize validation (:123-153): len >= 12, num_u64s ==
 * ceil(num_bits/64), len == 12 + 8*num_u64s; else LSMB_ECORRUPT. */
int lsmb_deserialize_header(const uint8_t* data, uint64_t len, uint32_t* num_hashes,
                            uint32_t* num_bits, uint32_t* num_u64s);

/* Validates like lsmb_deserialize_header, then copies the words (:156-161). */
int lsmb_deserialize(const uint8_t* data, uint64_t len, uint64_t* words, uint64_t words_cap);

/* ---- single-key operations (BloomFilter::insert / may_contain) ---------- */

/* BloomFilter::insert (src/bloom/mod.rs:70-78) on host-resident words: one
 * key, so no device round trip (a launch costs ~10 us, the insert ~20 ns). */
int lsmb_insert(uint64_t* words, uint32_t num_bits, uint32_t num_hashes, const uint8_t* key,
                uint64_t key_len);

/* BloomFilter::may_contain (:82-94).  Returns 1 / 0, or < 0 on error. */
int lsmb_may_contain(const uint64_t* words, uint32_t num_bits, uint32_t num_hashes,
                     const uint8_t* key, uint64_t key_len);

/* Debug/test helper: the k bit positions of one key (hash_key + get_position,
 * src/bloom/mod.rs:181-197). */
int lsmb_positions(const uint8_t* key, uint64_t key_len, uint32_t num_bits, uint32_t num_hashes,
                   uint32_t* out_positions);

/* ---- GPU context --------------------------------------------------------- */

/* Opens `device` (HIP ordinal; -1 = current device).  LSMB_ENODEV if no
 * gfx950 device is usable. */
int lsmb_open(lsmb_ctx** out, int device);
void lsmb_close(lsmb_ctx* ctx);

/* Blocks until all work issued on the context's stream has finished. */
int lsmb_sync(lsmb_ctx* ctx);

/* ---- batched build (BloomFilterBuilder::add_key loop + build) ------------ */
/* Host-memory entry points: the keys go up in chunks through two device
 * staging slots (chunk i+1's H2D overlaps chunk i's kernels), the build runs on
 * the GPU, the words come back (OR-accumulated into `words`).  Synchronous.
 * n <= lsmb_host_max_keys(): the library's host loop builds the same bits with
 * no device round trip, and ctx may be NULL (above it, NULL is LSMB_EINVAL). */

/* Size threshold of the host path (default 2048 keys, env LSMB_HOST_MAX_KEYS;
 * 0 sends every build to the GPU).  The bits never depend on it. */
uint64_t lsmb_host_max_keys(void);
void lsmb_set_host_max_keys(uint64_t n);

/* n keys of key_len bytes each, packed back to back (key i at keys + i*key_len). */
int lsmb_build_fixed(lsmb_ctx* ctx, const uint8_t* keys, uint32_t key_len, uint64_t n,
                     uint32_t num_bits, uint32_t num_hashes, uint64_t* words);

/* n variable-length keys: key i = data[offsets[i] .. offsets[i+1]). */
int lsmb_build_var(lsmb_ctx* ctx, const uint8_t* data, const uint64_t* offsets, uint64_t n,
                   uint32_t num_bits, uint32_t num_hashes, uint64_t* words);

/* The SSTable bloom block in one call: replaces
 *     let bloom = self.bloom_builder.build();   let bloom_data = bloom.serialize();
 * of SSTableBuilder::finish (src/sstable/builder.rs:177-179).  Builds a fresh
 * filter (BloomFilter::new(..) then insert of every key, src/bloom/mod.rs:38-78)
 * from n host-memory keys — fixed-length (offsets == NULL, key i at
 * data + i*key_len) or variable-length (key i = data[offsets[i]..offsets[i+1])) —
 * and writes exactly the bytes BloomFilter::serialize returns
 * (src/bloom/mod.rs:102-115) into block[0 .. lsmb_serialized_size(num_bits)).
 * The words go device -> block directly (no host word array, no serialize
 * copy); the key H2D is chunked and overlapped with the build kernels.
 * n == 0 gives the empty filter's block.  block_len < the size: LSMB_EINVAL. */
int lsmb_build_block(lsmb_ctx* ctx, const uint8_t* data, const uint64_t* offsets, uint32_t key_len,
                     uint64_t n, uint32_t num_bits, uint32_t num_hashes, uint8_t* block,
                     uint64_t block_len);

/* ---- streaming ingestion (the flush / compaction add_key loop) ----------- */
/* The store's flush walks the frozen memtable and adds every key
 * (src/db/mod.rs:379-383 -> SSTableBuilder::add -> BloomFilterBuilder::add_key,
 * src/sstable/builder.rs:93); compaction does the same over its merged
 * entries (src/compaction/scheduler.rs:113-125,152-158).  An lsmb_stream takes
 * those keys one at a time while the walk is still going: each add is a copy
 * into pinned staging, and every full staging chunk (LSMB_STREAM_CHUNK_MB,
 * default 128) is uploaded and built asynchronously while the caller keeps
 * adding into the other chunk.  finish writes the serialized bloom block (or
 * the words) of BloomFilter::new + insert of every added key.  A run of at
 * most lsmb_host_max_keys() keys never touches the device (host loop at
 * finish); with ctx == NULL the stream is host-only and finish of a larger
 * run is LSMB_EINVAL.  One stream per thread; reusable after finish
 * (lsmb_stream_reset for another filter size). */
typedef struct lsmb_stream lsmb_stream;

int lsmb_stream_open(lsmb_ctx* ctx, uint32_t num_bits, uint32_t num_hashes, lsmb_stream** out);
int lsmb_stream_reset(lsmb_stream* s, uint32_t num_bits, uint32_t num_hashes);
void lsmb_stream_close(lsmb_stream* s);

/* BloomFilterBuilder::add_key (src/bloom/builder.rs:21-23): appends one key. */
int lsmb_stream_add(lsmb_stream* s, const uint8_t* key, uint64_t key_len);

/* Appends n keys: key i = data[offsets[i] .. offsets[i+1]). */
int lsmb_stream_add_batch(lsmb_stream* s, const uint8_t* data, const uint64_t* offsets, uint64_t n);

/* Keys added since open / the last finish. */
uint64_t lsmb_stream_count(const lsmb_stream* s);

/* Finishes the filter: the bytes BloomFilter::serialize returns
 * (src/bloom/mod.rs:102-115) into block[0 .. lsmb_serialized_size(num_bits)),
 * or the ceil(num_bits/64) words.  Synchronous; the stream then starts a new,
 * empty filter of the same size. */
int lsmb_stream_finish_block(lsmb_stream* s, uint8_t* block, uint64_t block_len);
int lsmb_stream_finish_words(lsmb_stream* s, uint64_t* words);

/* ---- batched probe (may_contain over a batch of keys x filters) --------- */
/* For key i and filter f: bit (f % 8) of out_mask[i * ceil(nfilt/8) + f / 8]
 * = may_contain(filter f, key i), exactly what SSTable::get's bloom check
 * (src/sstable/reader.rs:197) answers for that SSTable.  offsets == NULL
 * selects fixed-length keys of key_len bytes.  nfilt <= 64. */
int lsmb_probe(lsmb_ctx* ctx, const uint64_t* const* filt_words, const uint32_t* filt_bits,
               const uint32_t* filt_hashes, uint32_t nfilt, const uint8_t* data,
               const uint64_t* offsets, uint32_t key_len, uint64_t n, uint8_t* out_mask);

/* ---- device-resident entry points ---------------------------------------- */
/* All pointers are device pointers (hipMalloc).  `stream` is a hipStream_t
 * (NULL = the context's own stream).  Asynchronous: the call returns after
 * enqueueing; synchronise on the stream before reading results. */

int lsmb_build_fixed_dev(lsmb_ctx* ctx, const void* d_keys, uint32_t key_len, uint64_t n,
                         uint32_t num_bits, uint32_t num_hashes, void* d_words, void* stream);

int lsmb_build_var_dev(lsmb_ctx* ctx, const void* d_data, const void* d_offsets, uint64_t n,
                       uint32_t num_bits, uint32_t num_hashes, void* d_words, void* stream);

/* BloomFilterBuilder::{new, add_key per key, build} (src/bloom/builder.rs:14-28) into device words:
 * BloomFilter::new (src/bloom/mod.rs:38-67) + insert of every key.  Unlike the
 * entry points above, `d_words` is OUTPUT-ONLY — its old contents are ignored,
 * every word of the filter is written — so the build needs no zeroing pass and
 * never reads the old words.  n == 0 or num_hashes == 0 writes all-zero words.
 * Memory: a partitioned k = 7 build also allocates, once per context and kept
 * until lsmb_close, an overflow bitmap as large as the filter (C2: 120 MB; the
 * 2^32-1-bit C5 filter: 512 MiB), 4 bytes per 2^20 filter bits of unit marks,
 * and 64 KiB of overflow lists per pass A workgroup per sweep (C2 and C5: 32
 * MiB).  These are outside LSMB_WORKSPACE_MB, which bounds only the partition
 * regions (the key chunk size follows from it). */
int lsmb_build_fixed_dev_new(lsmb_ctx* ctx, const void* d_keys, uint32_t key_len, uint64_t n,
                             uint32_t num_bits, uint32_t num_hashes, void* d_words, void* stream);
int lsmb_build_var_dev_new(lsmb_ctx* ctx, const void* d_data, const void* d_offsets, uint64_t n,
                           uint32_t num_bits, uint32_t num_hashes, void* d_words, void* stream);

/* A partitioned build (filters above a few MiB) runs in sweeps: each re-reads
 * the keys and keeps the positions of its own range of the filter (C5's
 * 2^32-1-bit filter: 2 sweeps of 256 MiB).  lsmb_build_sweeps gives their
 * number (1 for every other strategy), lsmb_sweep_words the word range
 * [word_lo, word_hi) whose bits sweep s completes, and
 * lsmb_build_fixed_dev_sweep builds just that sweep (OR-accumulate; running
 * every sweep == lsmb_build_fixed_dev).  A sharded build can then merge sweep
 * s's word range across GPUs while sweep s+1 builds. */
int lsmb_build_sweeps(uint32_t num_bits, uint32_t num_hashes, uint64_t n);
int lsmb_sweep_words(uint32_t num_bits, uint32_t num_hashes, uint64_t n, int sweep, uint64_t* word_lo,
                     uint64_t* word_hi);
int lsmb_build_fixed_dev_sweep(lsmb_ctx* ctx, const void* d_keys, uint32_t key_len, uint64_t n,
                               uint32_t num_bits, uint32_t num_hashes, void* d_words, int sweep, void* stream);
/* Sweep s of lsmb_build_fixed_dev_new: writes every word of sweep s's range
 * [word_lo, word_hi) (output-only there), no other word.  Running every sweep
 * == lsmb_build_fixed_dev_new. */
int lsmb_build_fixed_dev_sweep_new(lsmb_ctx* ctx, const void* d_keys, uint32_t key_len, uint64_t n,
                                   uint32_t num_bits, uint32_t num_hashes, void* d_words, int sweep, void* stream);

/* ---- batched build: many SSTable filters from one key run ---------------- */
/* The store sizes every SSTable's filter new(1000, 0.01) (src/sstable/builder.rs:74), fills it
 * key by key (builder.rs:93) and serializes it at finish (builder.rs:177-182); a bulk load, a
 * level rewritten with another false-positive rate or several compactions finishing together
 * (src/compaction/scheduler.rs:147-177) produce many such tables at once.  These entry points
 * build ntab independent filters from one run of n keys: table t is BloomFilter::new +
 * insert of the keys [seg[t], seg[t+1]) of the run, in a filter of (num_bits[t],
 * num_hashes[t]).  seg is non-decreasing with seg[ntab] <= n; keys outside every segment are
 * ignored.  One kernel launch per geometry class, at most two, whatever ntab is.
 *
 * Packed layout: table t's u64 words start at word_off[t]; its slot is
 * max(ceil(num_bits[t] / 64), 1) words rounded up to an even count (16-byte-aligned slots, the
 * level set's arena rule), word_off[ntab] = the words of the whole buffer.  Every word of
 * every slot is written (zero words and the pad word included): the buffer is output-only. */

/* The largest num_bits a table of a batch may have (src/sstable/builder.rs:74 is far below it):
 * 1 310 720, the filters the "lds" strategy serves.  A larger table takes
 * lsmb_build_fixed_dev_new / lsmb_build_var_dev_new. */
uint32_t lsmb_build_batch_max_bits(void);

/* word_off[0 .. ntab] of the packed layout for these num_bits (the slots
 * src/sstable/builder.rs:177-182's filters take in device memory).  LSMB_EINVAL: NULL word_off,
 * NULL num_bits with ntab > 0. */
int lsmb_build_batch_layout(uint64_t ntab, const uint32_t* num_bits, uint64_t* word_off);

/* Work items (one wave or one workgroup each) the plan gives a table of `keys` keys and
 * num_bits bits (src/sstable/builder.rs:93 per key): >= 1, non-decreasing in keys.  1: the table's
 * words are stored once with plain stores; more: its parts OR into a slot cleared first.
 * For tests and tools, like lsmb_build_strategy.  Measurement switches read at every call
 * (tools/mb_build_batch.py's geometry A/B): LSMB_BB_WAVE_MAX_BITS (below 65 536: smaller
 * filters take the workgroup class too) and LSMB_BB_GROUP_LANES (64 .. 1024: that class's
 * workgroup).  The filter bits never depend on them. */
int lsmb_build_batch_parts(uint64_t keys, uint32_t num_bits);

/* Device keys (d_offsets == NULL: fixed key_len; else n + 1 uint64_t offsets into d_data), host
 * seg[ntab + 1], num_bits[ntab], num_hashes[ntab]; d_words: device, 16-byte aligned, words_cap
 * u64 words.  src/sstable/builder.rs:74,93 for every table of src/compaction/scheduler.rs:147-177's
 * outputs.  Asynchronous on `stream`, no host synchronisation inside (from the third batch in
 * flight on one context, the call first waits for the batch two before it: its work list
 * staging is reused).  LSMB_EINVAL, nothing written: NULL ctx, seg, num_bits, num_hashes or
 * d_words; NULL keys with a non-empty segment; seg descending or seg[ntab] > n; words_cap <
 * word_off[ntab]; d_words not 16-byte aligned; num_bits == 0 with num_hashes > 0; a table above
 * lsmb_build_batch_max_bits() (lsmb_last_error() names the table).  ntab == 0: LSMB_OK, nothing
 * written. */
int lsmb_build_batch_dev(lsmb_ctx* ctx, const void* d_data, const void* d_offsets, uint32_t key_len, uint64_t n,
                         uint64_t ntab, const uint64_t* seg, const uint32_t* num_bits, const uint32_t* num_hashes,
                         void* d_words, uint64_t words_cap, void* stream);

/* Host keys in, serialized blocks out, synchronous: blocks[block_off[t] .. block_off[t+1]) =
 * BloomFilter::serialize (src/sstable/builder.rs:177-182) of table t, back to back — the
 * blocks / block_off form lsmb_lset_add_batch takes.  block_off[ntab + 1] is always filled when
 * the other arguments pass; blocks == NULL or blocks_cap < block_off[ntab] is then LSMB_EINVAL,
 * so a first call may ask for the size.  The keys cross once, the packed words come back in one
 * copy and the host writes the 12-byte headers.  No host fallback: a NULL ctx is LSMB_EINVAL
 * whatever the key count (src/compaction/scheduler.rs:147-177 batches are the device's).
 * Other errors as lsmb_build_batch_dev, with blocks and block_off untouched. */
int lsmb_build_batch_blocks(lsmb_ctx* ctx, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                            uint64_t ntab, const uint64_t* seg, const uint32_t* num_bits, const uint32_t* num_hashes,
                            uint8_t* blocks, uint64_t blocks_cap, uint64_t* block_off);

/* ---- batched build from the tables' data blocks --------------------------- */
/* A table written long ago keeps its keys in one place only: inside its data blocks, interleaved
 * with the values,
 *   [klen u16][vlen u16][key][value] ... [off u16 ...][n u16]
 * (src/sstable/block/builder.rs:40-76; read back by Block::decode / key_at,
 * src/sstable/block/reader.rs:18-44).  These entry points take such blocks as the key source and
 * build ntab filters in one launch per geometry class, so that a filter the census finds saturated
 * (lsmb_lset_census; src/sstable/builder.rs:51,74 sizes every one new(1000, 0.01), and
 * src/compaction/scheduler.rs:147-160 writes a whole compaction into one), a bloom block that failed
 * its CRC, a level rewritten with another false-positive rate or the inputs of a compaction read
 * as whole files (scheduler.rs:91-103) are rebuilt without a host parse.  The caller uploads the
 * files' data regions as they stand and names the blocks: block b is bytes[blk_off[b] ..
 * blk_off[b] + blk_len[b]) (the index entries' offset and size, src/sstable/footer.rs:20-27), at
 * any byte alignment; table t is the blocks [bseg[t], bseg[t+1]), bseg non-decreasing with
 * bseg[ntab] <= nblk.  Blocks outside every table are ignored.
 *
 * A block is well-formed when len >= 2, with n = the u16 at len - 2: 2 + 2n <= len, and with
 * data_end = len - 2 - 2n, for every i < n, off = the u16 at data_end + 2i, klen = the u16 at off,
 * vlen = the u16 at off + 2: off + 4 <= data_end and off + 4 + klen + vlen <= data_end.  Nothing
 * else is asked: offsets need not ascend, entries may overlap, empty keys and the keys of empty
 * values (tombstones: builder.rs:93 adds the key first) count, a key present twice sets its bits
 * twice, and a single-entry block may exceed 65 535 bytes (block/builder.rs:45).  No byte outside a
 * block is read, whatever its bytes are.  A malformed block is not an error of the device call: its
 * table's words are unspecified (only that table's slot is written, every other table is exact),
 * and the block is reported as LSMB_SST_BAD_BLOCK.
 *
 * Output: the packed layout of lsmb_build_batch_dev, so lsmb_lset_add_batch_dev takes it as it is. */
#define LSMB_SST_BAD_BLOCK 0xFFFFFFFFu

/* Work items the plan gives a table of `blocks` data blocks holding `bytes` bytes in a filter of
 * num_bits (src/sstable/block/builder.rs:40-76 blocks): >= 1, non-decreasing in bytes, at most one
 * per block.  For tests and tools, like lsmb_build_batch_parts, and under the same switches plus
 * two of its own, read at every call (tools/mb_build_batch_sst.py): LSMB_SST_WAVE_BYTES and
 * LSMB_SST_GROUP_BYTES, the block bytes one item of each class walks (default 256 KiB and 1 MiB).
 * The filter bits never depend on them. */
int lsmb_build_batch_sst_parts(uint64_t blocks, uint64_t bytes, uint32_t num_bits);

/* Device bytes (nbytes of them), host blk_off[nblk], blk_len[nblk], bseg[ntab + 1], num_bits[ntab],
 * num_hashes[ntab]; d_words: device, 16-byte aligned, words_cap u64 words; d_blk_entries: device
 * uint32_t[nblk] or NULL: entry b = block b's entry count, or LSMB_SST_BAD_BLOCK, for every block
 * of a table (one plain store by the wave that owns the block; unclaimed blocks' entries are left
 * as they were).  src/sstable/builder.rs:93 for every key of src/sstable/block/builder.rs:40-76's
 * blocks.  Asynchronous on `stream`, no host synchronisation inside; the work list and the blocks'
 * descriptors are staged as lsmb_build_batch_dev stages its own.  LSMB_EINVAL, nothing written:
 * NULL ctx, bseg, num_bits, num_hashes or d_words; NULL blk_off or blk_len with nblk > 0; NULL
 * d_bytes with a non-empty claimed block; bseg descending or bseg[ntab] > nblk; a claimed block
 * with blk_off + blk_len > nbytes (checked here, so the device never sees a block that leaves the
 * buffer); words_cap < word_off[ntab]; d_words not 16-byte aligned; num_bits == 0 with num_hashes
 * > 0; a table above lsmb_build_batch_max_bits() (lsmb_last_error() names the table).  ntab == 0:
 * LSMB_OK, nothing written. */
int lsmb_build_batch_sst_dev(lsmb_ctx* ctx, const void* d_bytes, uint64_t nbytes, uint64_t nblk,
                             const uint64_t* blk_off, const uint32_t* blk_len, uint64_t ntab, const uint64_t* bseg,
                             const uint32_t* num_bits, const uint32_t* num_hashes, void* d_words, uint64_t words_cap,
                             void* d_blk_entries, void* stream);

/* Host bytes in, serialized bloom blocks out, synchronous: blooms[bloom_off[t] .. bloom_off[t+1]) =
 * BloomFilter::serialize (src/sstable/builder.rs:177-182) of table t.  bloom_off[ntab + 1] is
 * always filled when the other arguments pass; blooms == NULL or blooms_cap < bloom_off[ntab] is
 * then LSMB_EINVAL, so a first call may ask for the size (as lsmb_build_batch_blocks).  entries
 * (uint64_t[ntab], may be NULL): the sum of the table's block entry counts — what the meta block's
 * entry_count (builder.rs:139-162) says of an intact table.  status (int32_t[ntab], may be NULL):
 * LSMB_OK, or LSMB_ECORRUPT for a table with a malformed block; the return value is the first
 * status that is not LSMB_OK, and lsmb_last_error() names that table and block.  The bloom bytes of
 * a corrupt table are unspecified, every other table's are exact.  No host fallback: a NULL ctx is
 * LSMB_EINVAL.  Other errors as lsmb_build_batch_sst_dev, with every output untouched. */
int lsmb_build_batch_sst_blocks(lsmb_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, uint64_t nblk,
                                const uint64_t* blk_off, const uint32_t* blk_len, uint64_t ntab, const uint64_t* bseg,
                                const uint32_t* num_bits, const uint32_t* num_hashes, uint8_t* blooms,
                                uint64_t blooms_cap, uint64_t* bloom_off, uint64_t* entries, int32_t* status);

/* ---- compaction: the surviving keys of merged data blocks -------------------- */
/* A compaction's output table is not the union of its inputs.  MergeIterator keeps the newest version
 * of each key, the lowest source index (src/iterator/merge.rs:15,55-56,98-121), and a bottommost
 * compaction drops every key whose newest version is a tombstone (src/compaction/scheduler.rs:
 * 147-158).  These entry points resolve that on the device from the data blocks the compaction has
 * already read, and give what the rest of the engine needs of the merge: the survivor count (the
 * output table's entry_count, and the n of BloomFilter::new(n, fpr)), the survivors' keys as a device
 * key run (what lsmb_build_var_dev_new and lsmb_build_batch_dev take), and in one call the output
 * table's bloom block.
 *
 * Input: the bytes and blocks of lsmb_build_batch_sst_dev (format and well-formed rule above,
 * unchanged), cut into sources instead of tables: host sseg[nsrc + 1], non-decreasing, sseg[nsrc] <=
 * nblk; source s is the blocks [sseg[s], sseg[s+1]); source 0 is the NEWEST (the order in which
 * scheduler.rs:92-103 pushes task.inputs; merge.rs:15 "lower index = newer source").  Blocks outside
 * every source are ignored.  A source is meant to be one SSTable: keys strictly ascending in unsigned
 * byte-lexicographic order (Vec<u8>'s cmp, a proper prefix is smaller) across its entries and blocks.
 *
 * An entry e of source s SURVIVES when (1) no source s' < s holds an entry with a byte-equal key, and
 * (2) drop_tombstones == 0, or e's vlen > 0.  For ascending sources this is exactly the set
 * run_compaction hands to builder.add (scheduler.rs:152-158); drop_tombstones is its is_bottommost,
 * which the caller decides (scheduler.rs:127-145).  Survivors are reported in (block index, entry
 * index) order: the output is deterministic, no atomic decides a layout.
 *
 * The lookup in a newer source is the store's own (SSTable::get): a binary search of the source's
 * blocks by each block's last key, then a binary search inside that block through its offset array.
 * Every "shadowed" verdict rests on a byte-equal key actually found.  For sources that are not
 * ascending a search may miss but can never hit falsely: the survivor set is then a SUPERSET of the
 * right one, never a subset — extra filter bits, no false negative — and the call is still LSMB_OK.
 *
 * A claimed block that is malformed, or that holds no entries (the store never writes one,
 * src/sstable/builder.rs:112-115, and the search needs a last key), is BAD: it is reported as
 * LSMB_SST_BAD_BLOCK in d_blk_entries and counted in totals[3], holds no keys for any search (the
 * other blocks' verdicts are as if it were absent) and contributes no survivors.  No byte outside a
 * claimed block is read, whatever the bytes are, and every search terminates on any input. */

/* The bytes of device work buffer a mark and gather over any sources cut from these nblk blocks need
 * (src/compaction/scheduler.rs:91-103's inputs): per block a 24-byte descriptor, four u64 counters and
 * one flag bit per entry the block could hold (entries may overlap, so blk_len / 2 of them: about
 * blk_len / 16 bytes).  0 for NULL blk_len with nblk > 0. */
uint64_t lsmb_compact_sst_work_bytes(uint64_t nblk, const uint32_t* blk_len);

/* The mark (the merge of src/iterator/merge.rs:98-121 and the tombstone drop of src/compaction/
 * scheduler.rs:152-158, as verdicts): device bytes, host blk_off[nblk], blk_len[nblk], sseg[nsrc + 1];
 * d_work: device, 16-byte aligned, work_bytes >= lsmb_compact_sst_work_bytes of the claimed blocks;
 * d_blk_entries: device uint32_t[nblk] or NULL: entry b = block b's entry count, or
 * LSMB_SST_BAD_BLOCK, for every claimed block (unclaimed blocks' entries are left as they were);
 * d_totals: device uint64_t[4], all four written in full: {survivors, the survivors' key bytes, the
 * entries of the good claimed blocks, bad blocks}.  Asynchronous on `stream`, no host synchronisation
 * inside; the blocks' descriptors are staged as lsmb_build_batch_sst_dev stages its own.
 * LSMB_EINVAL, nothing written: NULL ctx, sseg, d_work or d_totals; NULL blk_off or blk_len with nblk
 * > 0; NULL d_bytes with a non-empty claimed block; sseg descending or sseg[nsrc] > nblk; a claimed
 * block with blk_off + blk_len > nbytes (checked here, so the device never sees a block that leaves
 * the buffer); work_bytes too small; d_work not 16-byte aligned.  nsrc == 0: LSMB_OK, totals all
 * zero. */
int lsmb_compact_sst_mark_dev(lsmb_ctx* ctx, const void* d_bytes, uint64_t nbytes, uint64_t nblk,
                              const uint64_t* blk_off, const uint32_t* blk_len, uint64_t nsrc, const uint64_t* sseg,
                              int drop_tombstones, void* d_work, uint64_t work_bytes, void* d_blk_entries,
                              void* d_totals, void* stream);

/* The gather (the keys src/compaction/scheduler.rs:152-158 hands to builder.add, src/sstable/
 * builder.rs:93, as a key run): after a mark of the same block and source arguments and the same
 * d_work on the same stream, the survivors' keys back to back into d_key_data and survivors + 1
 * uint64_t offsets into d_key_offsets (8-byte aligned), offsets[0] = 0, key i =
 * d_key_data[offsets[i] .. offsets[i+1]).  The caller sizes both from the totals it read back:
 * data_cap >= totals[1] bytes, offs_cap >= totals[0] + 1 offsets.  The mark's totals are the
 * authority: with a capacity below them nothing is written at or past it and the run is TRUNCATED
 * (offsets[j] is written iff j < offs_cap, a key byte iff its position is below data_cap; the call is
 * still LSMB_OK, being asynchronous) — a caller tells by comparing its capacities with the totals.
 * Asynchronous on `stream`, no host synchronisation inside.  LSMB_EINVAL, nothing written: the mark's
 * conditions (the work buffer's size is the mark's to check), NULL d_key_data or d_key_offsets with a
 * non-zero capacity, d_key_offsets misaligned. */
int lsmb_compact_sst_gather_dev(lsmb_ctx* ctx, const void* d_bytes, uint64_t nbytes, uint64_t nblk,
                                const uint64_t* blk_off, const uint32_t* blk_len, uint64_t nsrc, const uint64_t* sseg,
                                const void* d_work, void* d_key_data, uint64_t data_cap, void* d_key_offsets,
                                uint64_t offs_cap, void* stream);

/* The output table's bloom block in one call, synchronous: host bytes in; upload, mark, the totals
 * read back, lsmb_params(expected_items ? expected_items : max(survivors, 1), fpr), gather,
 * lsmb_build_var_dev_new, BloomFilter::serialize into bloom[0 .. *bloom_len).  Replaces the
 * MergeIterator walk of src/compaction/scheduler.rs:147-158 as far as the filter is concerned and
 * SSTableBuilder's new / add per key / finish (src/sstable/builder.rs:74,93,177-182): expected_items
 * = 1000, fpr = 0.01 reproduces the store's own block byte for byte; expected_items = 0 sizes the
 * filter for the survivors.  *entry_count (may be NULL) = the survivors, the meta block's
 * entry_count (builder.rs:90,139-162); *num_bits, *num_hashes (may be NULL) = the filter's shape.
 * A bad block: LSMB_ECORRUPT, lsmb_last_error() names the source and the block, and no output is
 * written.  Otherwise *bloom_len and the other outputs are always filled when the arguments pass;
 * bloom == NULL or bloom_cap < *bloom_len is then LSMB_EINVAL, so a first call may ask for the
 * size.  Zero survivors give the empty filter's block.  No host fallback: a NULL ctx is
 * LSMB_EINVAL.  Other errors as lsmb_compact_sst_mark_dev (and lsmb_params' for fpr), with every
 * output untouched. */
int lsmb_compact_sst_bloom(lsmb_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, uint64_t nblk,
                           const uint64_t* blk_off, const uint32_t* blk_len, uint64_t nsrc, const uint64_t* sseg,
                           int drop_tombstones, uint64_t expected_items, double false_positive_rate, uint8_t* bloom,
                           uint64_t bloom_cap, uint64_t* bloom_len, uint64_t* entry_count, uint32_t* num_bits,
                           uint32_t* num_hashes);

/* CRC-32 of bloom blocks (optional checksum; the reference's
 * bloom block has none).  The same CRC as crc32fast::hash / zlib.crc32, which
 * the store already uses for WAL records and the manifest
 * (src/wal/record.rs:96,122, src/manifest/mod.rs:5).
 *   lsmb_crc32          host bytes, appended to crc (0 to start)
 *   lsmb_crc32_combine  CRC(A||B) from CRC(A), CRC(B), |B|
 *   lsmb_crc32_dev      device bytes (parallel CRC + combine), appended to crc
 *   lsmb_build_block_crc  lsmb_build_block + the block's CRC-32, the words'
 *                         part computed on the device copy before the D2H
 *   lsmb_fset_add_crc   lsmb_fset_add that checks the block's CRC-32 on the
 *                       copy in HBM: mismatch -> LSMB_ECORRUPT, slot not added */
uint32_t lsmb_crc32(uint32_t crc, const uint8_t* data, uint64_t len);
uint32_t lsmb_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
int lsmb_crc32_dev(lsmb_ctx* ctx, uint32_t crc, const void* d_data, uint64_t len, uint32_t* out, void* stream);
/* Many device segments in one launch (the bloom blocks of the SSTables a store
 * opens, SSTable::open -> deserialize, src/sstable/reader.rs:78-82, ~1 KB
 * each): d_segs is nseg pairs {const void* data; uint64_t len} in device
 * memory, d_out[s] = the CRC-32 (src/wal/record.rs:96) of segment s, uint32_t
 * in device memory.  One wave per segment: meant for segments up to 128 KiB,
 * exact for any length; 16-byte-aligned segments take the wide loads.
 * Asynchronous on `stream`, no host synchronisation inside.  This is what
 * lsmb_lset_add_batch checks its CRCs with. */
int lsmb_crc32_seg_dev(lsmb_ctx* ctx, const void* d_segs, uint64_t nseg, void* d_out, void* stream);
/* Many small device-to-device copies in one launch (the surviving SSTable filters a Version
 * edit moves out of sparse arena chunks, src/compaction/scheduler.rs:163-177, src/db/mod.rs:402):
 * d_segs is nseg triples {const void* src; void* dst; uint64_t len} in device memory, src and
 * dst 16-byte aligned, len a multiple of 16 (0: nothing moves).  One wave per segment; cut a
 * long copy into several segments to spread it.  Segments whose ranges overlap, within one
 * segment or across segments, are undefined.  Asynchronous on `stream` (NULL: the context's), no
 * host synchronisation inside; nseg == 0 is LSMB_OK.  LSMB_EINVAL: NULL ctx, NULL d_segs with
 * nseg > 0.  This is what lsmb_lset_derive_packed moves its tables with. */
int lsmb_copy_segs_dev(lsmb_ctx* ctx, const void* d_segs, uint64_t nseg, void* stream);
/* The set bits of many small device segments in one launch (the filters of a resident Version,
 * each sized from an estimate, src/sstable/builder.rs:74, by src/bloom/mod.rs:38-68): d_segs is
 * nseg pairs {const void* words; uint64_t nbits} in device memory, words 16-byte aligned;
 * d_out[s] (uint64_t, device memory) = the number of set bits among bits 0 .. nbits-1 of the LE u64
 * words at `words`.  Exactly ceil(nbits / 64) 8-byte words are read, so the buffer may end with the
 * last of them; bits at or above nbits in that word do not count (BloomFilter::deserialize never
 * checks them, src/bloom/mod.rs:123-168, and may_contain never reads them); nbits == 0 answers 0
 * and reads nothing.  One wave per segment; cut a long filter into several segments to spread it
 * and add their counts.  Asynchronous on `stream` (NULL: the context's), no host synchronisation
 * inside; nseg == 0 is LSMB_OK.  LSMB_EINVAL: NULL ctx, NULL d_segs or d_out with nseg > 0.  This
 * is what lsmb_lset_census counts with. */
int lsmb_popcount_segs_dev(lsmb_ctx* ctx, const void* d_segs, uint64_t nseg, void* d_out, void* stream);
int lsmb_build_block_crc(lsmb_ctx* ctx, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                         uint32_t num_bits, uint32_t num_hashes, uint8_t* block, uint64_t block_len, uint32_t* crc);

/* d_filt_words: host array of nfilt DEVICE pointers. */
int lsmb_probe_dev(lsmb_ctx* ctx, const void* const* d_filt_words, const uint32_t* filt_bits,
                   const uint32_t* filt_hashes, uint32_t nfilt, const void* d_data,
                   const void* d_offsets, uint32_t key_len, uint64_t n, void* d_out_mask,
                   void* stream);

/* OR-reduce: d_dst[i] |= d_src[j*stride_words + i] for j < nsrc, i < nwords.
 * The merge step of a sharded build (partial filters -> one filter). */
int lsmb_or_reduce_dev(lsmb_ctx* ctx, void* d_dst, const void* d_src, uint64_t nwords,
                       uint32_t nsrc, uint64_t stride_words, void* stream);

/* Synthetic workload generators, device-side:
 * key16(seed, i) = LE64(splitmix64(seed+2i)) || LE64(splitmix64(seed+2i+1)),
 * for i in [first, first+n). */
int lsmb_gen_key16_dev(lsmb_ctx* ctx, uint64_t seed, uint64_t first, uint64_t n, void* d_keys,
                       void* stream);

/* u64 stream: d_out[j] = mod ? add + splitmix64(seed+first+j) % mod
 *                            : splitmix64(seed+first+j), j in [0, n).
 * The C4 var-len workload: key lengths (seed 0x5EED0003, mod 249, add 8) and
 * the packed key bytes (seed 0x5EED0004, mod 0, LE words). */
int lsmb_gen_splitmix_dev(lsmb_ctx* ctx, uint64_t seed, uint64_t first, uint64_t n, uint32_t mod,
                          uint32_t add, void* d_out, void* stream);

/* ---- one process, several GPUs (sharded build) -------------------------- */
/* When one flush / compaction run is large (src/db/mod.rs:377-383,
 * src/compaction/scheduler.rs:150-158, both feeding SSTableBuilder::add,
 * src/sstable/builder.rs:93), lsmb_multi splits its keys into G contiguous
 * shards, builds a full-size partial filter per shard on its own GPU and merges
 * the partials with a bitwise-OR reduce-scatter done by peer loads over xGMI.
 * OR is associative, commutative and idempotent: the merged words equal a
 * single-device build of all the keys, bit for bit.  Devices may repeat (the
 * shards then share a GPU).  Used from one thread at a time. */
typedef struct lsmb_multi lsmb_multi;

/* devices: ndev HIP ordinals (NULL = 0..ndev-1), 1 <= ndev <= 16.  Enables
 * peer access between every pair of distinct devices (LSMB_ENODEV if a pair
 * has no peer path). */
int lsmb_multi_open(lsmb_multi** out, const int* devices, int ndev);
void lsmb_multi_close(lsmb_multi* m);
int lsmb_multi_size(const lsmb_multi* m);

/* Shard g's single-GPU context (its device, stream and scratch), e.g. to place
 * device buffers or run other entry points on that GPU. */
lsmb_ctx* lsmb_multi_ctx(lsmb_multi* m, int shard);

/* Device-resident sharded build: shard g's n[g] keys of key_len bytes at
 * d_keys[g] and its words d_words[g] live on shard g's device.  Every shard
 * builds into its own words (OR-accumulate), then reduce-scatter + all-gather:
 * on return every d_words[g] holds the merged filter.  Synchronous. */
int lsmb_multi_build_fixed_dev(lsmb_multi* m, const void* const* d_keys, const uint64_t* n, uint32_t key_len,
                               uint32_t num_bits, uint32_t num_hashes, void* const* d_words);

/* lsmb_build_block over G GPUs: the n host-memory keys (fixed-length, or
 * var-length with offsets) are split into G contiguous shards; each GPU
 * uploads and builds its shard (G PCIe links in parallel), the partials are
 * OR-reduce-scattered over xGMI, and each GPU copies its merged word slice
 * into the block.  Writes exactly BloomFilter::serialize's bytes. */
int lsmb_multi_build_block(lsmb_multi* m, const uint8_t* data, const uint64_t* offsets, uint32_t key_len,
                           uint64_t n, uint32_t num_bits, uint32_t num_hashes, uint8_t* block,
                           uint64_t block_len);

/* Timing of the last multi build, ms: [0] total (slowest shard), [1] build
 * (slowest shard), [2] merge = [0] - [1]. */
int lsmb_multi_last_ms(lsmb_multi* m, float* out3);

/* ---- one process per GPU: cross-process peer-load merge ------------------- */
/* The same OR merge between processes (one per GPU, e.g. torch.distributed
 * ranks), without a collective library: every rank exports the device
 * allocation holding its partial words, maps the other ranks' allocations
 * (over xGMI when they sit on other GPUs of the node; the same HBM when they
 * share one), and merges with peer loads: rank g ORs word-slice g of every
 * partial into its own words (lsmb_or_gather_dev with all G sources), then
 * copies every other merged slice from its owner (one source each).  The
 * caller orders the ranks between the phases: a host barrier after each
 * rank's stream has finished, or the device flags below.  Replaces what RCCL cannot do in one call (it
 * has no bitwise-OR reduction) for the sharded flush / compaction of
 * src/db/mod.rs:377-383 and src/compaction/scheduler.rs:150-158. */
#define LSMB_IPC_HANDLE_BYTES 64

/* Handle of the device allocation holding d_ptr (hipIpcGetMemHandle) and
 * d_ptr's byte offset in it. */
int lsmb_ipc_export(const void* d_ptr, uint8_t* handle, uint64_t* offset);

/* Maps another process's allocation into this context's device
 * (hipIpcOpenMemHandle, peer access enabled lazily); *d_base = its first
 * byte here.  A handle exported by this same process is LSMB_EINVAL. */
int lsmb_ipc_import(lsmb_ctx* ctx, const uint8_t* handle, void** d_base);

/* Unmaps an allocation lsmb_ipc_import mapped (d_base as returned). */
int lsmb_ipc_close(lsmb_ctx* ctx, void* d_base);

/* Merge status words (round 6): LSMB_MERGE_STATUS_WORDS u32 in device memory,
 * zero when the merge is set up, owned by one merge (one per IpcMerge):
 *   [0] poison: set (sticky) once one of the merge's phase waits timed out or
 *       saw another rank's poison;
 *   [1] the merge's phase waits that timed out.
 * A poisoned merge never reads its peers' words again and leaves every range
 * it merges all-ones: all-ones is a superset of every partial, so the filter
 * can answer "maybe" too often but never "no" for a key that was added (a
 * false negative would make DB::get skip the SST holding the key,
 * src/sstable/reader.rs:196-199, src/db/mod.rs:243-267).  The caller learns
 * of it at its next sync point (lsmb_merge_status) and must not trust the
 * filter as exact.  The status words live in the flag allocation the peers
 * map, so that a rank's poison is visible to every peer's waits. */
#define LSMB_MERGE_STATUS_WORDS 2

/* d_dst[i] = OR over j < nsrc of d_srcs[j][i], i < nwords (u64 words; any
 * source may be d_dst itself, or mapped peer memory).  Asynchronous on
 * `stream`.  nsrc == 1 is a copy; 1 <= nsrc <= 16.  d_status (NULL: none):
 * when the merge is poisoned at kernel time, d_dst[0, nwords) = all-ones and
 * no source is read. */
int lsmb_or_gather_dev(lsmb_ctx* ctx, void* d_dst, const void* const* d_srcs, uint32_t nsrc, uint64_t nwords,
                       const uint32_t* d_status, void* stream);

/* The merge's all-gather in one call: for every slice r < nsrc with
 * d_srcs[r] != NULL, d_dst[w] = d_srcs[r][w] for w in [r slice_words,
 * min((r+1) slice_words, nwords)) (u64 words; a NULL source leaves its slice
 * alone, e.g. the caller's own).  One kernel streams every slice at once, so
 * every peer link is busy.  The sources (mapped peer memory, or other local
 * buffers) must not overlap d_dst.  Asynchronous on `stream`.  d_status as
 * above: poisoned, those slices are written all-ones. */
int lsmb_copy_slices_dev(lsmb_ctx* ctx, void* d_dst, const void* const* d_srcs, uint32_t nsrc, uint64_t slice_words,
                         uint64_t nwords, const uint32_t* d_status, void* stream);

/* The merge's last step: if the merge is poisoned once everything before this
 * on `stream` has run, d_words[0, nwords) = all-ones; otherwise nothing. */
int lsmb_poison_fill_dev(lsmb_ctx* ctx, void* d_words, uint64_t nwords, const uint32_t* d_status, void* stream);

/* Device-ordered phases for the merge above, so that no host waits inside it:
 * a flag is a u32 epoch counter in device memory (this process's own, or a
 * peer's mapped with lsmb_ipc_import).  The merge of epoch e on `stream` is
 *   signal(own flag[0], e); wait(every rank's flag[0] >= e)   partials final
 *   or_gather (reduce-scatter);  signal(flag[1], e); wait(all flag[1] >= e)
 *   copy_slices (all-gather); signal(flag[2], e); wait(all flag[2] >= e)
 *   poison_fill
 * (lsmbloom.dist.IpcMerge, lsmbloom.dist.merge_schedule).  All enqueue and
 * return at once. */

/* After everything before it on `stream`: a system-scope release store of
 * `value` into *d_flag. */
int lsmb_flag_signal_dev(lsmb_ctx* ctx, uint32_t* d_flag, uint32_t value, void* stream);

/* Later work on `stream` waits until every d_flags[j] >= value (epoch compare,
 * wrap-safe), j < nflags <= 64.  d_poison[j] (or NULL) = rank j's poison word
 * (its status word [0]; the caller's own among them).  The wait ends early,
 * and poisons this merge (d_status[0] = 1), when any poison word is set, also
 * when one is set after the flags were met; a flag still short after
 * timeout_ms counts a timeout (d_status[1] += 1), poisons the merge and ends
 * the wait: a dead peer can never hang the queue, and never yields a filter
 * with missing bits. */
int lsmb_flag_wait_dev(lsmb_ctx* ctx, const uint32_t* const* d_flags, const uint32_t* const* d_poison, uint32_t nflags,
                       uint32_t value, uint32_t timeout_ms, uint32_t* d_status, void* stream);

/* The merge's sync point: waits for `stream`, then out2 = {poison, timeouts}
 * (the status words above). */
int lsmb_merge_status(lsmb_ctx* ctx, const uint32_t* d_status, void* stream, uint32_t* out2);

/* ---- device-resident filter sets (multi-get pre-check) --------------------- */
/* An lsmb_fset keeps up to 64 SSTable filters resident in device memory, each
 * with its table's key range [min_key, max_key] (SSTable meta,
 * src/sstable/reader.rs:192).  A probe answers, per key and per filter, the two
 * checks SSTable::get makes before it touches the index (reader.rs:192-199):
 *     min_key <= key <= max_key   (byte-wise lexicographic, as Rust's [u8] Ord)
 *     && may_contain(filter, key)
 * for a whole batch of keys, so DB::get (src/db/mod.rs:243-267), which today
 * re-opens and re-deserializes every SSTable per lookup (mod.rs:245,259), can
 * keep its filters on the GPU and read only the tables a key may be in.
 * A set belongs to one context and is used from one thread at a time. */
typedef struct lsmb_fset lsmb_fset;

int lsmb_fset_open(lsmb_ctx* ctx, lsmb_fset** out);
void lsmb_fset_close(lsmb_fset* fs);

/* Adds a filter from its serialized bloom block (the bytes BloomFilter::serialize
 * wrote, src/bloom/mod.rs:102-115), validated exactly as BloomFilter::deserialize
 * (mod.rs:123-168; LSMB_ECORRUPT) and copied straight into device memory.
 * Returns the filter's slot (0..63, bit `slot` of the probe mask) or < 0. */
int lsmb_fset_add(lsmb_fset* fs, const uint8_t* block, uint64_t len, const uint8_t* min_key,
                  uint64_t min_len, const uint8_t* max_key, uint64_t max_len);

/* lsmb_fset_add that also checks the block's CRC-32 (lsmb_crc32 /
 * crc32fast::hash of all `len` bytes) on the copy in device memory. */
int lsmb_fset_add_crc(lsmb_fset* fs, const uint8_t* block, uint64_t len, uint32_t crc, const uint8_t* min_key,
                      uint64_t min_len, const uint8_t* max_key, uint64_t max_len);

/* Same from in-memory filter words (ceil(num_bits/64) LE u64). */
int lsmb_fset_add_words(lsmb_fset* fs, const uint64_t* words, uint32_t num_bits, uint32_t num_hashes,
                        const uint8_t* min_key, uint64_t min_len, const uint8_t* max_key,
                        uint64_t max_len);

/* Drops a filter (e.g. its table was compacted away); the slot is re-used. */
int lsmb_fset_remove(lsmb_fset* fs, int slot);

/* Bit s set = slot s holds a filter. */
uint64_t lsmb_fset_live_mask(const lsmb_fset* fs);

/* out_mask[i] bit s = (min_s <= key i <= max_s) && may_contain(filter s, key i).
 * offsets == NULL selects fixed-length keys of key_len bytes.  Synchronous. */
int lsmb_fset_probe(lsmb_fset* fs, const uint8_t* data, const uint64_t* offsets, uint32_t key_len,
                    uint64_t n, uint64_t* out_mask);

/* Device-memory keys and output (u64 per key); asynchronous on `stream`. */
int lsmb_fset_probe_dev(lsmb_fset* fs, const void* d_data, const void* d_offsets, uint32_t key_len,
                        uint64_t n, void* d_out_mask, void* stream);

/* lsmb_fset_probe_dev with answer rows of row_bytes = 1, 2, 4 or 8 bytes: row i
 * is the u64 mask's low row_bytes bytes (LE), so a set whose live slots are
 * all below 8 * row_bytes (e.g. 8 per-level tables in 1 byte) writes 1/8 of
 * the u64 rows' bytes.  A live slot at or above 8 * row_bytes is LSMB_EINVAL. */
int lsmb_fset_probe_dev_rows(lsmb_fset* fs, const void* d_data, const void* d_offsets, uint32_t key_len, uint64_t n,
                             void* d_out, uint32_t row_bytes, void* stream);

/* The answer per table instead of per key: what a reader that works table by
 * table wants (open table s, look up the keys that may be in it, close it).
 * For every slot s < 64: d_index[d_starts[s] .. d_starts[s+1]) = the indices i
 * (ascending) of the keys with bit s set in lsmb_fset_probe's mask, i.e.
 * (min_s <= key i <= max_s) && may_contain(filter s, key i).  d_starts is
 * uint64_t[65]; d_starts[0] = 0; d_starts[64] = total entries; a dead slot's run
 * is empty.  d_index is uint32_t[cap].  d_starts is always exact; the entry at
 * global position p is written iff p < cap, nothing else in d_index is
 * touched, so a caller whose d_starts[64] > cap learns the size it needs
 * (cap == 0 with a null d_index is a counting call).  n == 0 or an empty set
 * writes 65 zero starts.  n > 2^32-1: LSMB_EINVAL.  Asynchronous on `stream`.
 * The mask rows and per-tile counts in between live in the set's own scratch:
 * lists probes on different streams run one after the other. */
int lsmb_fset_probe_lists_dev(lsmb_fset* fs, const void* d_data, const void* d_offsets, uint32_t key_len,
                              uint64_t n, void* d_starts, void* d_index, uint64_t cap, void* stream);

/* Host keys and host outputs (starts[65], index[cap]); synchronous.  Only
 * starts and min(total, cap) entries cross PCIe on the way back. */
int lsmb_fset_probe_lists(lsmb_fset* fs, const uint8_t* data, const uint64_t* offsets, uint32_t key_len,
                          uint64_t n, uint64_t* starts, uint32_t* index, uint64_t cap);

/* ---- device-resident level sets (the non-overlapping levels) --------------- */
/* An lsmb_lset is an immutable snapshot of the store's levels below L0, one
 * per Version: up to LSMB_LSET_MAX_LEVELS rows, each holding any number of
 * SSTable filters (bounded by memory and uint32_t) whose key ranges
 * [min_key, max_key] are pairwise disjoint, as DB::get relies on for those
 * levels (src/db/mod.rs:255-267, "L1+: no overlaps, at most one SSTable
 * contains the key").  So the answer per key and row is one table or none, and
 * a probe writes a caller-chosen table id (the SST id, meta.id) instead of a
 * mask bit per table: a row of thousands of tables costs each key one binary
 * search, one range check and at most one filter walk.  Filters may have any
 * (num_bits, num_hashes), num_hashes = 0 and > 8 included.  The Version's L0,
 * whose tables overlap (src/db/mod.rs:243-252), lives in the same set as its L0
 * part (LSMB_LSET_ROW_L0, further down), so one sealed set is one Version.
 *   open -> add / add_words / add_batch (any order) -> seal -> probe ... -> close
 *   derive / derive_packed (from a sealed set, sharing its filters) -> add ... -> seal -> probe ... -> close
 * A set belongs to one context.  Adds and seal are used from one thread at a
 * time; a sealed set is only read, so probes on different streams need no
 * ordering among themselves.  Close a set once its probes have completed. */
typedef struct lsmb_lset lsmb_lset;
#define LSMB_LSET_MAX_LEVELS 8
#define LSMB_LSET_NONE 0xFFFFFFFFu /* the probe's "no table of this row" */

int lsmb_lset_open(lsmb_ctx* ctx, lsmb_lset** out);
void lsmb_lset_close(lsmb_lset* ls);

/* Adds table `table_id` to row `row` from its serialized bloom block, validated
 * exactly as lsmb_fset_add does (LSMB_ECORRUPT) and copied to device memory
 * before the call returns.  LSMB_EINVAL: row >= LSMB_LSET_MAX_LEVELS (other than
 * LSMB_LSET_ROW_L0, below: the set's L0 part), table_id
 * == LSMB_LSET_NONE, num_bits == 0 with num_hashes > 0, an add after seal. */
int lsmb_lset_add(lsmb_lset* ls, uint32_t row, uint32_t table_id, const uint8_t* block, uint64_t len,
                  const uint8_t* min_key, uint64_t min_len, const uint8_t* max_key, uint64_t max_len);

/* Same from in-memory filter words (ceil(num_bits/64) LE u64). */
int lsmb_lset_add_words(lsmb_lset* ls, uint32_t row, uint32_t table_id, const uint64_t* words, uint32_t num_bits,
                        uint32_t num_hashes, const uint8_t* min_key, uint64_t min_len, const uint8_t* max_key,
                        uint64_t max_len);

/* Sorts every row by min_key, checks min_t <= max_t for every table and
 * max_t < min_{t+1} strictly between neighbours (byte-wise, a proper prefix
 * first, as Rust's [u8] Ord) and uploads the sorted descriptors.  A row that
 * fails is LSMB_EINVAL, lsmb_last_error() naming the two offending table ids;
 * the set stays unsealed.  A set with no table seals too. */
int lsmb_lset_seal(lsmb_lset* ls);

/* Version edit (src/compaction/scheduler.rs:163-177: retain(!input_ids.contains(id)) over every
 * level, then push): a new, UNSEALED set on parent's context holding every table of the sealed
 * parent whose id is not in drop_ids (in any row; an id held by several tables drops them all;
 * an id no table has is ignored), each in its row, with its range, SHARING the parent's device
 * filter words: nothing is uploaded.  *dropped (may be NULL) = tables left out.
 * lsmb_lset_rows(child) >= lsmb_lset_rows(parent), even if the top rows end up empty.
 * Then add / add_batch / seal as for any set.  LSMB_EINVAL: NULL parent or out, unsealed parent,
 * ndrop > 0 with NULL drop_ids.
 * The shared words live in reference-counted arena chunks: a chunk is released when the last
 * set holding one of its tables is closed, so parent and child may be closed in either order
 * (each once its own probes have completed), and the parent may be probed on other threads
 * while a child is derived.  A set writes only into chunks it allocated itself. */
int lsmb_lset_derive(const lsmb_lset* parent, const uint32_t* drop_ids, uint64_t ndrop,
                     uint64_t* dropped, lsmb_lset** out);

/* lsmb_lset_derive that also REPACKS sparse arena chunks on the device, for a store that edits
 * its Version for days (a compaction, src/compaction/scheduler.rs:163-177, or a flush,
 * src/db/mod.rs:402, is derive + add + seal, and every plain derive leaves the child's add a
 * fresh chunk for one small filter while each old chunk lives as long as one table in it).
 * With live(c) = the slot bytes (filter words rounded up to 16) of the surviving tables in the
 * parent's chunk c, chunk c is EVACUATED iff live(c) > 0 and live(c) * 1e6 < min_ppm * bytes(c);
 * under min_ppm = LSMB_LSET_REPACK_ALL iff live(c) > 0.  All survivors of an evacuated chunk are
 * copied, device to device, into chunks the child allocates itself, and the child holds no
 * reference to the evacuated chunk; all other survivors stay shared as lsmb_lset_derive leaves
 * them.  A filter in a chunk of its own has live == bytes, so only LSMB_LSET_REPACK_ALL moves it;
 * min_ppm == 0 moves nothing and is lsmb_lset_derive exactly.  Tables, rows, L0 positions, ids
 * and ranges of the child are those of lsmb_lset_derive in every case.
 * The child's next add continues in the chunk the moved tables went to instead of taking a new
 * one.  moved (may be NULL): [0] tables moved, [1] their slot bytes.
 * The copy is one kernel launch (lsmb_copy_segs_dev's) on `stream` (NULL: a stream of the
 * child's own) followed by ONE synchronisation of it; on return the parent may be closed and the
 * child is ready for adds and lsmb_lset_seal.  The parent's memory is only read: its probes on
 * other streams or threads need no ordering with this call.  ALL OR NOTHING: on any failure
 * *out == NULL, the chunks the call allocated are released and the parent is as it was.
 * LSMB_EINVAL as lsmb_lset_derive, and for min_ppm > LSMB_LSET_REPACK_ALL.
 * In lsmb_lset_stats moved tables count in [0], [1], [4] and [5] and add nothing to [2] and [3]:
 * no byte crosses PCIe. */
#define LSMB_LSET_REPACK_ALL 1000001u
int lsmb_lset_derive_packed(const lsmb_lset* parent, const uint32_t* drop_ids, uint64_t ndrop,
                            uint32_t min_ppm, uint64_t* dropped, uint64_t moved[2], lsmb_lset** out,
                            void* stream);

/* ntab tables in one call (a store opening its SSTables, SSTable::open -> deserialize,
 * src/sstable/reader.rs:78-82): table t goes to rows[t] with id table_ids[t]; its serialized block is
 * blocks[block_off[t] .. block_off[t+1]), its min_key keys[key_off[2t] .. key_off[2t+1]), its
 * max_key keys[key_off[2t+1] .. key_off[2t+2]).  crcs == NULL: unchecked, as lsmb_lset_add.
 * crcs != NULL: crcs[t] is the CRC-32 (lsmb_crc32) of table t's whole block, checked on the
 * copy in device memory.  ALL OR NOTHING: if any table fails (argument, header validation as
 * lsmb_lset_add, CRC), the set is exactly as before the call, and the return is the code of the
 * first failing table.  status (may be NULL) receives every table's own code (LSMB_OK,
 * LSMB_EINVAL, LSMB_ECORRUPT), and lsmb_last_error() names the first failing index and id.
 * ntab == 0 is LSMB_OK.  The words are staged in pinned memory and cross in at most one copy
 * per arena chunk touched, with one synchronisation for the batch; CRCs are only checked
 * once every header has passed. */
int lsmb_lset_add_batch(lsmb_lset* ls, uint64_t ntab, const uint32_t* rows, const uint32_t* table_ids,
                        const uint8_t* blocks, const uint64_t* block_off, const uint32_t* crcs,
                        const uint8_t* keys, const uint64_t* key_off, int32_t* status);

/* ntab tables whose filter words are ALREADY on the set's device, in the packed layout of
 * lsmb_build_batch_layout (what lsmb_build_batch_dev leaves: the output tables of
 * src/compaction/scheduler.rs:147-177 pushed into the next Version, their filters finished by
 * src/sstable/builder.rs:177-182, without a trip through the host): table t goes to rows[t] with
 * id table_ids[t], its words are the u64 words d_words[word_off[t] ..], its filter is
 * (num_bits[t], num_hashes[t]), its range as in lsmb_lset_add_batch (keys / key_off).  word_off
 * must equal that layout for num_bits (LSMB_EINVAL otherwise), d_words must be 16-byte aligned.
 * Arena slots are reserved as in lsmb_lset_add_batch; the words move in one device-to-device
 * copy on `stream` (NULL: the context's) per run of tables landing in one arena chunk, followed by
 * ONE synchronisation of `stream`, so work enqueued on it before the call (the build) is complete
 * and, on return, d_words is free to go and the set is ready for lsmb_lset_seal.  ALL OR NOTHING
 * with the undo of lsmb_lset_add_batch; lsmb_last_error() names the first failing index and id.
 * ntab == 0 is LSMB_OK.  In lsmb_lset_stats these tables count in [0], [4] and [5] and add nothing
 * to [2] and [3]: no byte crosses PCIe. */
int lsmb_lset_add_batch_dev(lsmb_lset* ls, uint64_t ntab, const uint32_t* rows, const uint32_t* table_ids,
                            const void* d_words, const uint64_t* word_off, const uint32_t* num_bits,
                            const uint32_t* num_hashes, const uint8_t* keys, const uint64_t* key_off,
                            void* stream);

/* A set's footprint after a chain of version edits (src/compaction/scheduler.rs:163-177):
 * out[0] tables; [1] tables inherited by lsmb_lset_derive; [2] filter bytes this set uploaded;
 * [3] host-to-device copy calls this set issued for filter words; [4] device bytes of all arena
 * chunks this set keeps alive (its own and shared ones); [5] filter bytes of its tables.
 * [5]/[4] is the occupancy.  A chain of plain derives leaves it low; lsmb_lset_derive_packed
 * keeps it up on the device, without a rebuild from the host.  LSMB_EINVAL: NULL set or out. */
int lsmb_lset_stats(const lsmb_lset* ls, uint64_t out[6]);

/* 1 + the highest row added (0 when empty; 0 for NULL). */
int lsmb_lset_rows(const lsmb_lset* ls);
/* Tables of one row (0 for NULL or a row >= LSMB_LSET_MAX_LEVELS); row =
 * LSMB_LSET_ROW_L0: the tables of the L0 part. */
uint64_t lsmb_lset_tables(const lsmb_lset* ls, uint32_t row);

/* With R = lsmb_lset_rows(ls), out holds R * n values, row-major by level:
 * out[r*n + i] = table_id of the one table t of row r with
 *     min_t <= key i <= max_t && may_contain(filter t, key i),
 * else LSMB_LSET_NONE (an empty row answers LSMB_LSET_NONE everywhere).
 * n == 0 or R == 0 writes nothing.  offsets == NULL selects fixed-length keys
 * of key_len bytes.  Before seal: LSMB_EINVAL.  Host keys; synchronous. */
int lsmb_lset_probe(lsmb_lset* ls, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                    uint32_t* out);

/* Device-memory keys and output (R * n uint32_t); asynchronous on `stream`. */
int lsmb_lset_probe_dev(lsmb_lset* ls, const void* d_data, const void* d_offsets, uint32_t key_len, uint64_t n,
                        void* d_out, void* stream);

/* ---- a level set's answer per table ---------------------------------------- */
/* What a reader that works table by table wants from the levels below L0
 * (src/db/mod.rs:255-267 picks the one table per level, src/sstable/reader.rs:
 * 192-199 is the range-and-bloom check each list entry has passed): open
 * table g, look up the keys that may be in it, close it.  Table ids are the
 * caller's and need not be unique, so the lists are keyed by ORDINAL: with R =
 * lsmb_lset_rows(ls), T_r = lsmb_lset_tables(ls, r) and base_r = T_0 + ... +
 * T_{r-1}, table j of row r in the row's sealed order (ascending min_key) has
 * the ordinal g = base_r + j, and G = base_R tables have one. */

/* G (src/db/mod.rs:255-267, src/sstable/reader.rs:192-199: every table a get
 * may consult below L0).  0 for NULL or an unsealed set. */
uint64_t lsmb_lset_total_tables(const lsmb_lset* ls);

/* Host outputs: ids[G] = the table id of every ordinal, row_base[R + 1] =
 * base_0 .. base_R (the tables of src/db/mod.rs:255-267's levels in the order
 * src/sstable/reader.rs:192-199's min_key sorts them).  Either pointer may be
 * NULL.  Before seal: LSMB_EINVAL. */
int lsmb_lset_table_order(const lsmb_lset* ls, uint32_t* ids, uint64_t* row_base);

/* Bytes of device workspace a lists probe of n keys needs (the batched walk of
 * src/db/mod.rs:255-267 with src/sstable/reader.rs:192-199's checks keeps its
 * intermediate answers there).  0 for NULL, an unsealed set, n == 0, an empty
 * set or n > 2^32-1. */
uint64_t lsmb_lset_lists_work_bytes(const lsmb_lset* ls, uint64_t n);

/* d_starts is uint64_t[G + 1], d_index is uint32_t[cap].  For every ordinal g,
 * d_index[d_starts[g] .. d_starts[g+1]) = the indices i, ascending, of the
 * keys for which lsmb_lset_probe answers table g in g's row:
 *     min_g <= key i <= max_g && may_contain(filter g, key i)
 * (src/db/mod.rs:255-267, src/sstable/reader.rs:192-199).  d_starts[0] = 0,
 * d_starts[G] = the total number of entries.  d_starts is always exact; the
 * entry at global position p is written iff p < cap, nothing else in d_index
 * is touched (cap == 0 with a null d_index is a counting call), as
 * lsmb_fset_probe_lists_dev.  n == 0 or G == 0 writes G + 1 zero starts and
 * nothing else.  LSMB_EINVAL: n > 2^32-1, work_bytes below
 * lsmb_lset_lists_work_bytes(ls, n), a null (or not 16-byte-aligned) d_work
 * with n > 0 && G > 0, a call before seal; the outputs are then untouched.
 * Asynchronous on `stream`, no host synchronisation inside.  The sealed set
 * stays read-only: ALL scratch is the caller's d_work, so lists probes on
 * different streams with different workspaces need no ordering among
 * themselves (two probes sharing one workspace do).  The same keys give the
 * same bytes in d_starts and d_index on every run. */
int lsmb_lset_probe_lists_dev(lsmb_lset* ls, const void* d_data, const void* d_offsets, uint32_t key_len, uint64_t n,
                              void* d_starts, void* d_index, uint64_t cap, void* d_work, uint64_t work_bytes,
                              void* stream);

/* Host keys and host outputs (starts[G + 1], index[cap]); synchronous; the
 * lists of src/db/mod.rs:255-267's levels under src/sstable/reader.rs:192-199's
 * checks as above.  The workspace is the context's own scratch, so calls on
 * one context run one at a time, as its other host entry points.  Only starts
 * and min(total, cap) entries cross PCIe on the way back. */
int lsmb_lset_probe_lists(lsmb_lset* ls, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                          uint64_t* starts, uint32_t* index, uint64_t cap);

/* ---- a level set's L0 part: one sealed set answers a Version ---------------- */
/* DB::get and Snapshot::get walk one Version (src/db/mod.rs:238-267,
 * src/db/snapshot.rs:40-69): L0 newest first, where the tables' ranges overlap,
 * then one table per level below.  A level set holds both halves: any add path
 * called with row = LSMB_LSET_ROW_L0 puts the table into the set's L0 part
 * instead of a row.  Up to LSMB_LSET_L0_MAX tables, ranges overlapping in any
 * way; a table's POSITION is its order of arrival (call order, index order
 * within a batch: a flush is new_levels[0].push(meta), src/db/mod.rs:402).
 * lsmb_lset_derive keeps the parent's surviving L0 tables in their relative
 * order, the child's adds follow them (Vec::retain then push,
 * src/compaction/scheduler.rs:171-174), and drop_ids drops L0 tables exactly as
 * row tables, the words shared.  So a flush and a compaction are each derive +
 * add + seal, and the sealed result is the new Version.
 * The 65th L0 table is LSMB_EINVAL and leaves the set as it was; in a batch
 * status[t] is LSMB_EINVAL at the first table past the cap (all or nothing) and
 * lsmb_last_error() names its index and id.  lsmb_lset_seal neither orders nor
 * checks L0 ranges against each other; an L0 table with min_key > max_key is
 * LSMB_EINVAL naming its id.
 * lsmb_lset_rows, _total_tables, _table_order, lsmb_lset_probe* and
 * lsmb_lset_probe_lists* see the rows only (lsmb_lset_probe_version_lists*
 * below list L0 too); a set with no L0 table behaves as before.
 * lsmb_lset_tables(ls, LSMB_LSET_ROW_L0) is the L0 count, and
 * lsmb_lset_stats counts L0 tables in [0], [1], [4] and [5] like any other. */
#define LSMB_LSET_ROW_L0 0x80000000u /* `row` of any add path: the table goes to L0 */
#define LSMB_LSET_L0_MAX 64

/* T0: the L0 tables (src/db/mod.rs:243-252's version.level(0)).  0 for NULL. */
uint64_t lsmb_lset_l0_tables(const lsmb_lset* ls);

/* ids[T0] = the table ids in position order (oldest first; src/db/mod.rs:243
 * reads them in reverse).  Before seal, or NULL: LSMB_EINVAL. */
int lsmb_lset_l0_order(const lsmb_lset* ls, uint32_t* ids);

/* The whole Version from one hash per key (src/db/mod.rs:238-267,
 * src/db/snapshot.rs:40-69).  With R = lsmb_lset_rows(ls), T0 = lsmb_lset_l0_tables(ls):
 *   l0_mask[i] bit j = (min_j <= key i <= max_j) && may_contain(filter j, key i)
 * for the L0 table at position j (src/sstable/reader.rs:192-199); a reader visits
 * the set bits from the highest down (version.level(0).iter().rev());
 *   out[r*n + i] = exactly what lsmb_lset_probe writes.
 * d_l0_mask (n uint64_t) is always written for n > 0, all zero when T0 == 0;
 * NULL there is LSMB_EINVAL.  d_out (R * n uint32_t) may be NULL only when
 * R == 0.  n == 0 writes nothing.  Before seal: LSMB_EINVAL, outputs untouched.
 * Asynchronous on `stream` (NULL: the context's), no host synchronisation and no
 * scratch: the sealed set stays read-only, probes on different streams need no
 * ordering, and the same keys give the same bytes on every run. */
int lsmb_lset_probe_version_dev(lsmb_lset* ls, const void* d_data, const void* d_offsets, uint32_t key_len,
                                uint64_t n, void* d_l0_mask, void* d_out, void* stream);

/* Host keys and host outputs; synchronous, through the context's staging as
 * lsmb_lset_probe (src/db/mod.rs:238-267). */
int lsmb_lset_probe_version(lsmb_lset* ls, const uint8_t* data, const uint64_t* offsets, uint32_t key_len,
                            uint64_t n, uint64_t* l0_mask, uint32_t* out);

/* ---- a whole Version's answer per table ------------------------------------- */
/* lsmb_lset_probe_lists* see the rows only.  A reader that works table by table
 * over the whole walk of DB::get (src/db/mod.rs:238-267, src/db/snapshot.rs:40-69)
 * wants the L0 tables' lists too, from the same hash.  VERSION ORDINALS: with
 * T0 = lsmb_lset_l0_tables(ls), R = lsmb_lset_rows(ls), G =
 * lsmb_lset_total_tables(ls) and V = T0 + G,
 *   v <  T0  is the L0 table at position v, the numbering of
 *            lsmb_lset_probe_version's mask bits: a reader walks v = T0-1 .. 0
 *            for newest first, as src/db/mod.rs:243 does;
 *   v >= T0  is the rows' ordinal g = v - T0 of lsmb_lset_table_order. */

/* V (src/db/mod.rs:238-267, src/db/snapshot.rs:40-69, src/sstable/reader.rs:192-199:
 * every table a get may consult).  0 for NULL or an unsealed set. */
uint64_t lsmb_lset_version_tables(const lsmb_lset* ls);

/* Host outputs: ids[V] = lsmb_lset_l0_order's ids, then lsmb_lset_table_order's;
 * part_base[R + 2] = 0, T0, T0 + base_1, ..., T0 + base_R = V: the first
 * Version ordinal of L0, of every row, and the end (the tables of
 * src/db/mod.rs:238-267's walk, src/db/snapshot.rs:40-69; each checked as
 * src/sstable/reader.rs:192-199).  Either pointer may be NULL.  Before seal:
 * LSMB_EINVAL. */
int lsmb_lset_version_order(const lsmb_lset* ls, uint32_t* ids, uint64_t* part_base);

/* ---- a Version's fill census -------------------------------------------------- */
/* How good the filters of a resident Version are.  SSTableBuilder sizes each table's filter from an
 * ESTIMATE of its key count (src/sstable/builder.rs:74 -> BloomFilter::new, src/bloom/mod.rs:38-68),
 * and a flush or compaction output that holds several times the estimate gets a filter that is
 * mostly ones: every may_contain on it is true, every probe lists it as a candidate, and the reader
 * pays a table lookup per key for nothing.  The words of a sealed set live only in its arena
 * (tables of lsmb_lset_add_batch_dev never crossed the host), so this is where a store learns which
 * tables to rewrite with another rate, without re-reading a bloom block from disk. */

/* Host outputs, V = lsmb_lset_version_tables(ls) entries each, in lsmb_lset_version_order's order
 * (the L0 tables by position, then the rows' tables by ordinal): every table's filter geometry as
 * it was added (src/bloom/mod.rs:38-68).  Either pointer may be NULL.  LSMB_EINVAL: NULL or
 * unsealed set. */
int lsmb_lset_version_geometry(const lsmb_lset* ls, uint32_t* num_bits, uint32_t* num_hashes);

/* set_bits[v] (host, V entries, the same order) = the set bits below num_bits of table v's resident
 * words; stray ones at or above num_bits in the last word (src/bloom/mod.rs:123-168 lets them in)
 * and the arena's padding do not count.  With lsmb_lset_version_geometry it gives
 * lsmb_fill_fpr and lsmb_fill_keys per table, the latter to set against builder.rs:74's estimate.
 * The call plans the tables' words into items of at most 64 KiB on the host, stages them in pinned
 * memory, and makes one upload, ONE launch (lsmb_popcount_segs_dev's kernel), one copy back of the
 * item counts and ONE synchronisation of `stream` (NULL: a stream of the set's own), then adds the
 * counts up per table on the host.  The set's tables are only read: probes on other streams or
 * threads need no ordering with it, and tables shared with a parent (lsmb_lset_derive) or moved by
 * lsmb_lset_derive_packed count like uploaded ones; lsmb_lset_stats is unchanged by it.  The
 * staging is the set's own, so one census of a set runs at a time.  The result is NOT cached: a
 * sealed set is immutable, so a store calls this once per Version and keeps the answer.
 * V == 0 is LSMB_OK.  LSMB_EINVAL: NULL or unsealed set, NULL set_bits with V > 0. */
int lsmb_lset_census(lsmb_lset* ls, uint64_t* set_bits, void* stream);

/* Bytes of device workspace a Version lists probe of n keys needs (the batched
 * walk of src/db/mod.rs:238-267 / src/db/snapshot.rs:40-69 under
 * src/sstable/reader.rs:192-199's checks keeps its masks and intermediate
 * answers there).  0 for NULL, an unsealed set, n == 0, V == 0 or n > 2^32-1;
 * with T0 == 0 it is lsmb_lset_lists_work_bytes(ls, n). */
uint64_t lsmb_lset_version_lists_work_bytes(const lsmb_lset* ls, uint64_t n);

/* d_starts is uint64_t[V + 1], d_index is uint32_t[cap].  For every Version
 * ordinal v, d_index[d_starts[v] .. d_starts[v+1]) = the indices i, ascending,
 * of the keys with
 *     min_v <= key i <= max_v && may_contain(filter v, key i)
 * (src/db/mod.rs:238-267, src/db/snapshot.rs:40-69, src/sstable/reader.rs:192-199):
 * for v < T0 the keys whose bit v is set in lsmb_lset_probe_version's mask, for
 * v >= T0 the keys for which lsmb_lset_probe answers that table in its row; one
 * hash per key serves both.  d_starts[0] = 0, d_starts[T0] = the number of L0
 * entries, d_starts[V] = the total.  Capacity, counting calls, errors, streams,
 * scratch and determinism are lsmb_lset_probe_lists_dev's with V for G and
 * lsmb_lset_version_lists_work_bytes for the workspace: d_starts is always
 * exact; the entry at global position p is written iff p < cap and nothing else
 * in d_index is touched; n == 0 or V == 0 writes V + 1 zero starts and nothing
 * else; LSMB_EINVAL (outputs untouched) for n > 2^32-1, V > 2^32-1, a call
 * before seal, null outputs, and with n > 0 && V > 0 a null or not
 * 16-byte-aligned d_work or work_bytes below the need.  With T0 == 0 the call
 * is lsmb_lset_probe_lists_dev, byte for byte.  No atomics: the same keys give
 * the same bytes on every run. */
int lsmb_lset_probe_version_lists_dev(lsmb_lset* ls, const void* d_data, const void* d_offsets, uint32_t key_len,
                                      uint64_t n, void* d_starts, void* d_index, uint64_t cap, void* d_work,
                                      uint64_t work_bytes, void* stream);

/* Host keys and host outputs (starts[V + 1], index[cap]); synchronous; the
 * lists of src/db/mod.rs:238-267's walk (src/db/snapshot.rs:40-69) under
 * src/sstable/reader.rs:192-199's checks as above.  The workspace is the
 * context's own scratch, as lsmb_lset_probe_lists; only starts and
 * min(total, cap) entries cross PCIe on the way back. */
int lsmb_lset_probe_version_lists(lsmb_lset* ls, const uint8_t* data, const uint64_t* offsets, uint32_t key_len,
                                  uint64_t n, uint64_t* starts, uint32_t* index, uint64_t cap);

/* ---- the walk itself: each key's first candidate ---------------------------- */
/* DB::get and Snapshot::get visit the tables of a Version in one fixed order and
 * STOP at the first one that holds the key, value or tombstone
 * (src/db/mod.rs:243-267, src/db/snapshot.rs:40-69).  The lists above name every
 * table that may hold a key, so a reader working from them also reads the older
 * copies of an overwritten key, which the store itself never does.  WALK STEPS:
 * with T0 = lsmb_lset_l0_tables(ls) and R = lsmb_lset_rows(ls),
 *   step w <  T0     consults the L0 table at position T0-1-w: step 0 is the
 *                    newest arrival, the order of version.level(0).iter().rev()
 *                    (src/db/mod.rs:243);
 *   step w = T0 + r  consults row r (src/db/mod.rs:255-267);
 * W = T0 + R steps in all.  Key i has a CANDIDATE at an L0 step iff the bit of
 * that position is set in lsmb_lset_probe_version's mask, at a row step iff
 * lsmb_lset_probe answers a table in that row (src/sstable/reader.rs:192-199's
 * range-and-bloom check either way; a row emptied by derive never has one).
 * A multi-get works in rounds: probe; look the keys of each table's list up in
 * that table; a key that was found is finished (from = LSMB_LSET_NONE), a false
 * positive resumes one step later (from = step + 1); repeat until every step is
 * LSMB_LSET_NONE.  The table lookups of all rounds together are exactly the
 * SSTable::get calls DB::get would have made for those keys. */

/* W (the steps of src/db/mod.rs:243-267's walk).  0 for NULL or an unsealed set. */
uint32_t lsmb_lset_walk_steps(const lsmb_lset* ls);

/* Per key, from one hash (src/db/mod.rs:243-267, src/db/snapshot.rs:40-69,
 * src/sstable/reader.rs:192-199).  d_from is uint32_t[n], key i's resume step;
 * NULL means all zero.
 *   d_step[i]  uint32_t[n], may be NULL: the smallest step w >= d_from[i] at
 *              which key i has a candidate, else LSMB_LSET_NONE;
 *   d_ord[i]   uint32_t[n], required when n > 0: that candidate's Version
 *              ordinal in lsmb_lset_version_order's numbering (T0-1-w for an L0
 *              step, T0 + g for a row step, g the rows' ordinal), else
 *              LSMB_LSET_NONE.
 * d_from[i] >= W, LSMB_LSET_NONE included, answers LSMB_LSET_NONE in both and
 * the key is neither read nor hashed: how a caller retires a resolved key.
 * d_step may be d_from itself: a key's resume step is read before its step is
 * written.  n == 0 writes nothing; W == 0 writes LSMB_LSET_NONE everywhere.
 * LSMB_EINVAL (outputs untouched): a call before seal, a NULL d_ord or NULL
 * keys with n > 0.  Asynchronous on `stream` (NULL: the context's), no host
 * synchronisation, no scratch, no atomics: the sealed set stays read-only,
 * probes on different streams need no ordering, and the same inputs give the
 * same bytes on every run. */
int lsmb_lset_probe_walk_dev(lsmb_lset* ls, const void* d_data, const void* d_offsets, uint32_t key_len, uint64_t n,
                             const void* d_from, void* d_step, void* d_ord, void* stream);

/* Host keys, resume steps and outputs; synchronous, through the context's
 * staging as lsmb_lset_probe_version (src/db/mod.rs:243-267's walk, one round
 * of it).  from and step may be NULL as above, or one array. */
int lsmb_lset_probe_walk(lsmb_lset* ls, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                         const uint32_t* from, uint32_t* step, uint32_t* ord);

/* Bytes of device workspace a walk lists probe of n keys needs (one round of
 * src/db/mod.rs:243-267's walk under src/sstable/reader.rs:192-199's checks keeps
 * its per-key ordinals and their transposition there).  0 for NULL, an unsealed
 * set, n == 0, V == 0 or n > 2^32-1. */
uint64_t lsmb_lset_walk_lists_work_bytes(const lsmb_lset* ls, uint64_t n);

/* The same answer per table: d_starts is uint64_t[V + 1], d_index is
 * uint32_t[cap], V = lsmb_lset_version_tables(ls).  For every Version ordinal
 * v, d_index[d_starts[v] .. d_starts[v+1]) = the indices i, ascending, of the
 * keys whose first candidate at or after d_from[i] is table v (the table
 * src/db/mod.rs:243-267's walk, resumed there, reads next; checked as
 * src/sstable/reader.rs:192-199).  A key is in at most one list, so
 * d_starts[V] <= n.  d_from and d_step (optional) are lsmb_lset_probe_walk_dev's,
 * aliasing included.  Capacity, counting calls, errors, streams, scratch and
 * determinism are lsmb_lset_probe_version_lists_dev's with
 * lsmb_lset_walk_lists_work_bytes for the workspace: d_starts is always exact;
 * the entry at global position p is written iff p < cap and nothing else in
 * d_index is touched; n == 0 or V == 0 writes V + 1 zero starts (and
 * LSMB_LSET_NONE in every d_step[i] when it is given) and nothing else;
 * LSMB_EINVAL (outputs untouched) for n > 2^32-1, V > 2^32-1, a call before
 * seal, null outputs, and with n > 0 && V > 0 a null or not 16-byte-aligned
 * d_work or work_bytes below the need.  No atomics: the same inputs give the
 * same bytes on every run. */
int lsmb_lset_probe_walk_lists_dev(lsmb_lset* ls, const void* d_data, const void* d_offsets, uint32_t key_len,
                                   uint64_t n, const void* d_from, void* d_step, void* d_starts, void* d_index,
                                   uint64_t cap, void* d_work, uint64_t work_bytes, void* stream);

/* Host keys, resume steps and outputs (step[n] optional, starts[V + 1],
 * index[cap]); synchronous; one round of src/db/mod.rs:243-267's walk
 * (src/db/snapshot.rs:40-69) under src/sstable/reader.rs:192-199's checks as
 * above.  The workspace is the context's own scratch, as
 * lsmb_lset_probe_version_lists; the resume steps go up next to the keys, and
 * only starts, the steps and min(total, cap) entries cross PCIe on the way back. */
int lsmb_lset_probe_walk_lists(lsmb_lset* ls, const uint8_t* data, const uint64_t* offsets, uint32_t key_len, uint64_t n,
                               const uint32_t* from, uint32_t* step, uint64_t* starts, uint32_t* index, uint64_t cap);

/* ---- introspection ------------------------------------------------------- */

/* Name of the device build strategy the dispatcher picks for (num_bits, k, n):
 * "lds", "tiled", "partition", "atomic" (for tests and bench reporting).
 * Host-memory builds of n <= lsmb_host_max_keys() keys run on the host instead.
 * Measurement switches read at build time: LSMB_FORCE_STRATEGY=atomic,
 * LSMB_SWEEP_PER=1/2 (pass A keys per lane), LSMB_TILED_NO_PREHASH=1,
 * LSMB_H2D_CHUNK_MB, LSMB_WORKSPACE_MB.  The filter bits never depend on them. */
const char* lsmb_build_strategy(uint32_t num_bits, uint32_t num_hashes, uint64_t n);

/* Timing of the last device build on this context, in milliseconds, per phase
 * (HIP events on the build stream): [0] total, [1] pass A (hash + bin),
 * [2] pass B (apply).  Waits for the timed build to finish (on whatever
 * stream it was issued). */
int lsmb_last_build_ms(lsmb_ctx* ctx, float* out3);

/* Per-build HIP events behind lsmb_last_build_ms: on (1, the default) or off
 * (0: a build issues only its kernels, no timing markers between them). */
int lsmb_set_timing(lsmb_ctx* ctx, int enable);

#ifdef __cplusplus
}
#endif

#endif /* LSMBLOOM_H */
