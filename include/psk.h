/*
 * psk.h -- C ABI of the MI355X-native probabilistic-sketch engine (libpsk_hip.so).
 *
 * This is the drop-in boundary for ONE path of barrust/pyprobables (v0.7.0): bulk
 * insert / lookup of BloomFilter, CountingBloomFilter and CountMinSketch with the
 * default_fnv_1a hash family.  The reference is pure Python and has no FFI of its
 * own; each entry point below names the reference method(s) whose per-key loop it
 * replaces (paths relative to the reference checkout).  INTEGRATION.md shows the
 * ctypes stub a pyprobables maintainer would add to bind them.
 *
 * Conventions
 *   - threading: psk_last_error() is thread-local; a sketch handle owns scratch buffers, so one handle must not be
 *     used from two threads / two streams at the same time (different handles are independent).  Every call leaves
 *     the calling thread's current HIP device as it found it.
 *   - plain pointers and sizes only; every function returns a psk status code
 *     (PSK_OK == 0, negative on error; text via psk_last_error()); no exceptions
 *     cross the boundary.
 *   - `where` says where the caller's buffers (keys, offsets, weights, outputs) live:
 *     PSK_HOST  -> pageable/pinned host memory; the call stages through device
 *                  scratch and returns after the result is back on the host.
 *                  (That is what it promises -- not hipStreamSynchronize: a tiny batch, e.g. the
 *                  one-key calls of a per-key loop, ends as soon as its kernel has posted a
 *                  completion word in pinned memory, a few microseconds before the runtime sees
 *                  the stream idle.  Work the caller queued on `stream` EARLIER has completed by
 *                  then: the kernel ran behind it.  Option "host_poll_us" = 0 restores the wait.)
 *     PSK_DEVICE-> device memory of the sketch's GPU; the call only enqueues work on
 *                  `stream` (a hipStream_t passed as void*, NULL = default stream)
 *                  and returns immediately.
 *   - a sketch handle is externally synchronised: one in-flight batch per handle.
 *   - key batches come in four layouts (`layout` argument):
 *       PSK_KEYS_FIXED    data = uint8[n][key_len]            equal-length byte keys
 *       PSK_KEYS_VARLEN8  data = uint8 blob, offsets=uint64[n+1]   bytes / latin-1 str keys
 *       PSK_KEYS_VARLEN32 data = uint32 code points, offsets=uint64[n+1]  str keys with
 *                         code points > 255 (hashes.py:98 hashes ord(c), not UTF-8 bytes)
 *       PSK_KEYS_HASHES   data = uint64[n][key_len] pre-computed hashes (key_len = hashes
 *                         per key, >= k); the add_alt/check_alt path and the route for a
 *                         user-supplied hash_function (hashes.py:10-15 HashFuncT)
 *     For the three key layouts the engine computes default_fnv_1a(key, k)
 *     (hashes.py:71-103) inside the kernel.
 */
#ifndef PSK_H
#define PSK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct psk_sketch psk_sketch; /* opaque handle: owns (or borrows) one device-resident table */

enum psk_status {
    PSK_OK = 0,
    PSK_EINVAL = -1,    /* bad argument */
    PSK_ENODEV = -2,    /* no usable HIP device */
    PSK_ENOMEM = -3,    /* device allocation failed */
    PSK_EHIP = -4,      /* a HIP runtime call failed (see psk_last_error) */
    PSK_ECONTRACT = -5  /* batch-stream contract violated (see psk_get_counters) */
};

enum psk_where {
    PSK_HOST = 0,
    PSK_DEVICE = 1,
    /* psk_cbf_add / psk_cbf_remove / psk_cbf_update_combined: a device buffer that stays valid AND UNCHANGED until the handle's next
     * flush (any entry point that applies the waiting updates, psk_flush, psk_clear; psk_sketch_get_option "window_pending_batches"
     * tells how many of the latest batches still wait).  16-byte-aligned 16-byte fixed-length unit-weight keys that the engine defers
     * (update windows, write-combining lists) are then not copied: the flush hashes them where they lie, all waiting batches in one
     * pass (no key copy, one key read; round 5: BASELINE cfg 4 spent 22 % of its step copying keys).  Everything else -- other layouts,
     * batches applied at once -- is treated as PSK_DEVICE: nothing is kept. */
    PSK_DEVICE_BORROWED = 2
};

enum psk_layout { PSK_KEYS_FIXED = 0, PSK_KEYS_VARLEN8 = 1, PSK_KEYS_VARLEN32 = 2, PSK_KEYS_HASHES = 3 };

enum psk_query { PSK_Q_MIN = 0, PSK_Q_MEAN = 1, PSK_Q_MEANMIN = 2 }; /* countminsketch.py:429-453 */

enum psk_kind { PSK_KIND_BLOOM = 0, PSK_KIND_CBF = 1, PSK_KIND_CMS = 2 };

/* ordered-update opcode source (psk_*_update_ordered) */
enum psk_opmode { PSK_OP_ADD = 0, PSK_OP_REMOVE = 1, PSK_OP_SIGNED = 2 /* w>=0 add(w), w<0 remove(-w) */ };

/* counters kept on the device per sketch (psk_get_counters) */
enum psk_counter {
    PSK_CTR_ADDED = 0,      /* sum of weights applied by add batches */
    PSK_CTR_REMOVED = 1,    /* sum of weights actually removed (CBF: to_remove, countingbloom.py:203-207) */
    PSK_CTR_VIOLATIONS = 2, /* unordered batch ops whose result depended on order (CBF partial/underflowing remove) */
    PSK_CTR_SATURATED = 3,  /* counter updates that hit a rail (UINT32_MAX / INT32_MAX / INT32_MIN) */
    PSK_CTR_ABS_BOUND = 4,  /* upper bound on |any counter| (selects the wrap-free fast path) */
    PSK_CTR_SPILLED = 7,    /* diagnostic: probes of the last Bloom insert behind a clear that took pass 1's exact fallback (full bin / full segment) */
    PSK_CTR_COUNT = 8
};

/* ------------------------------------------------------------------ misc */
const char *psk_last_error(void);         /* thread-local text of the last failure */
int psk_version(void);
int psk_device_count(int *count);
/* Options (tunables of this engine: no reference counterpart).  psk_set_option keeps the PROCESS value; the names marked (s) can also be
 * overridden for one handle with psk_sketch_set_option (value INT64_MIN: follow the process value again).
 *
 *   name                        default  meaning
 *   "partition"                 1        0 = direct kernels only (one fabric transaction per probe), 1 = large batches take the partitioned passes
 *   "partition_min_keys" (s)    65536    Bloom inserts of at least this many keys are partitioned (4 x as many for lookups / counter updates)
 *   "partition_max_keys"        2^26     keys per partition round (bounds the scratch: ~2 GB per round at k = 7)
 *   "partition_cache_bytes"     240 MiB  cache-sized tables: a batch whose probe buffer exceeds 1.5 x this is cut into equal rounds (0 = never)
 *   "scratch_budget_bytes" (s)  0        cap on a handle's partition scratch (more, smaller rounds); 0 = none
 *   "pass1_bins"                1        pass 1 of Bloom inserts / tile-flag lookups, CBF unit updates and weighted CMS adds through fixed-capacity
 *                                        LDS bins where they fit (psk_part_bins.hpp); 0 = the counting sort everywhere (same probes, same results)
 *   "bloom_lookup" (s)          2        large Bloom lookups: 0 keyed probes, 1 return trip, 3 tile flags (batches of present keys), 4 lazy gathers
 *                                        (batches of absent keys), 2 = chosen per call from the previous lookups' miss tally
 *   "cms_small_weights"         1        weighted psk_cms_add: weights 0 .. 15 travel as 20-bit fields once the previous batches brought no
 *                                        other weight; 0 = never, 2 = always (exact either way)
 *   "cbf_lookup_shadow" (s)     1        psk_cbf_check keeps 4-bit images of an unchanged big table between lookups (cells / 2 bytes)
 *   "remove_exact" (s)          1        psk_cbf_remove replays order-dependent batches in order; 0 = tallies them as violations instead
 *   "update_window" (s)         1        small unit psk_cbf_add / _remove batches into big tables share one proven pass (psk_cbf_add below)
 *   "update_window_keys" (s)    2^27     most keys such a window holds
 *   "auto_combine" (s)          1        (update windows off) small unit add batches wait as scattered probes
 *   "combine_keys"              2^26     keys per list of psk_cbf_update_combined
 *   "merge_single_rank"         0        1: psk_merge_* run the collective path on a one-rank communicator (tests)
 *   "lazy_clear"                1        psk_clear of a Bloom table the engine alone reads is deferred (psk_clear below); 0 = sweep at once
 *   per sketch only: "table_private" (below), read-only "window_pending_batches" (batches an update window still holds: PSK_DEVICE_BORROWED
 *   buffers among them must stay as they are), read-only "bloom_lookup_misses" (the tally the handle's last finished large Bloom lookup
 *   published: probes that found their bit clear in a tile-flag or keyed lookup -- a probe pass 1 tested itself because its bin or segment was
 *   full is not among them --, keys answered absent by the return trip, gathers issued by the lazy scheme; -1 before the first.  Tile-flag
 *   lookups publish under any "bloom_lookup" value, the other schemes under 2.  The kernels write it: synchronise the call's stream first),
 *   read-only "pass1_bins_launches", "pass1_bins_tile_keys", "pass1_bins_workgroups" (test hooks: how many pass-1 launches of the handle went
 *   through the LDS bins, and the keys per tile / the workgroups of the last one).
 *
 * Also accepted -- where the engine switches between its kernel families, and test hooks (the tests steer small inputs onto the big-table paths
 * with them; not for callers): "partition_two_level_slices", "auto_combine_keys", "tile_threads", "even_tiles", "dense_walk_groups",
 * "lookup_half_slices", "remove_optimistic", "lookup_nibble_slices", "update_nibble_slices", "nibble_min_lg_lookup", "nibble_min_lg_update",
 * "update_window_tile", "update_window_wide", "update_window_force_fail", "ragged_sort", "host_poll_us" (how long a tiny PSK_HOST call
 * polls its completion mailbox before it waits for the stream; 0 = never poll); read-only counters "cbf_ordered_replays",
 * "update_window_folds", "update_window_replays", "cms_small_weights_used", "cbf_lookup_shadow_hits", "cms_running_fast",
 * "cms_running_sequential" (psk_cms_add_running calls that took the parallel passes / the one-lane kernel), "cms_update_running_fast",
 * "cms_update_running_sequential" (the same for psk_cms_update_running), "cbf_running_fast_chunks", "cbf_running_replayed_chunks",
 * "cbf_running_sequential" (psk_cbf_add_running / psk_cbf_update_running: chunks served by the parallel passes, chunks replayed in order,
 * calls that were not eligible).
 * The bench build (-DPSK_BENCH_KNOBS=1, libpsk_hip_knobs.so) has one more option, "part_debug": the ablation / phase-profile bits of the
 * measuring tools; this library answers "unknown option" to it.  The A/B switches of experiments that were measured and dropped are gone
 * with their code (NOTES.md). */
int psk_set_option(const char *name, int64_t value);
int psk_get_option(const char *name, int64_t *value);
/* Per-sketch options (round 4): "partition_min_keys", "cbf_lookup_shadow", "auto_combine", "update_window", "update_window_keys",
 * "scratch_budget_bytes", "remove_exact", "bloom_lookup" can differ between the sketches of one process -- psk_set_option keeps the
 * DEFAULT of each, psk_sketch_set_option overrides it for one handle (value INT64_MIN: follow the default again).  A call on a handle
 * works under the handle's overrides and, for the rest, the defaults as they stand when the call enters: a default another thread changes
 * meanwhile holds from the handle's next call on.  One more name exists
 * per sketch only: "table_private" = 1 declares that whoever holds the pointer of a caller-owned table (ext_table) announces EVERY write it
 * makes behind the engine's back (psk_table_info before, psk_rescan_bound after); without that promise -- and between psk_table_info(&ptr)
 * and the next psk_rescan_bound -- the engine keeps nothing derived from the table (the 4-bit images of repeated psk_cbf_check calls).
 * No reference counterpart (tunables of this engine). */
int psk_sketch_set_option(psk_sketch *s, const char *name, int64_t value);
int psk_sketch_get_option(psk_sketch *s, const char *name, int64_t *value);
/* bench-only: s_memtime totals per phase of the last partition pass 1 (option part_debug & 32) */
int psk_debug_phase_profile(psk_sketch *s, uint32_t nbuckets, uint32_t nwg, uint64_t out[12]);

/* -------------------------------------------------------------- lifecycle
 * ext_table: NULL -> the library hipMallocs (and zeroes) the table;
 *            else -> device pointer to caller-owned, zero-initialised memory of at least
 *                    psk_table_bytes(...) bytes (lets the caller keep the table in a tensor it
 *                    can hand to RCCL).
 * Replaces the array allocation of bloom.py:105, countingbloom.py:78, countminsketch.py:115. */
uint64_t psk_bloom_table_bytes(uint64_t m_bits);            /* ceil(m/8) rounded up to 16 B */
uint64_t psk_cbf_table_bytes(uint64_t m);                   /* 4*m rounded up to 16 B */
uint64_t psk_cms_table_bytes(uint64_t width, uint32_t depth); /* 4*width*depth rounded up to 16 B */
int psk_bloom_create(uint64_t m_bits, uint32_t k, int device, void *ext_table, psk_sketch **out);
int psk_cbf_create(uint64_t m, uint32_t k, int device, void *ext_table, psk_sketch **out);
int psk_cms_create(uint64_t width, uint32_t depth, int device, void *ext_table, psk_sketch **out);
int psk_destroy(psk_sketch *s);                             /* ext_table: write-combined updates still waiting are applied first (NULL stream + sync) */
/* psk_clear of a Bloom handle whose table nobody outside the engine holds (library-owned, or caller-owned with "table_private" = 1, and not
 * handed out by psk_table_info(&ptr) since the last psk_rescan_bound) and option "lazy_clear" = 1 launches nothing: the table is marked
 * clear-pending.  Every entry point that reads, writes or hands out the table, or reads the counters, runs the clear first on its own stream
 * (psk_flush does nothing else for a Bloom handle); a large insert takes it over -- its first apply stores the slices whole.  Otherwise the
 * table and the counter block are zeroed by one kernel on `stream`. */
int psk_clear(psk_sketch *s, void *stream);                 /* bloom.py:217-221, countminsketch.py:240-244 */
int psk_synchronize(psk_sketch *s, void *stream);
int psk_release_scratch(psk_sketch *s);                     /* free staging + partition buffers (regrow on demand) */
/* what the handle holds besides its table right now (round 4): bytes[0] = device scratch in all (staging, bucket buffers, values / perm,
 * write-combining segments, update-window key list and snapshots, kept 4-bit images), bytes[1] = of which the update window / write-combining
 * lists (they hold waiting updates: psk_flush applies them), bytes[2] = of which the kept 4-bit images; no stream work, no synchronisation.
 * (The scratch is an implementation detail of the path behind countingbloom.py:135-208 / bloom.py:234-272: the reference has none.) */
int psk_scratch_bytes(psk_sketch *s, uint64_t bytes[3]);
/* device pointer + padded size + logical size (the reference's array byte length).  A pending (deferred) clear runs first, on the NULL
 * stream: call psk_flush on the stream that will use the pointer before this, so that the clear is ordered there. */
int psk_table_info(psk_sketch *s, void **dev_ptr, uint64_t *padded_bytes, uint64_t *logical_bytes);
/* copy the first nbytes of the table to / from host memory in the reference's byte layout
 * (array('B') LSB-first bits, array('I') uint32 LE, array('i') int32 LE row-major by depth):
 * what export()/bytes()/frombytes() read and write (bloom.py:287-304,548-550; countminsketch.py:342-354,417-427) */
int psk_read_table(psk_sketch *s, void *dst_host, uint64_t nbytes, void *stream);
int psk_write_table(psk_sketch *s, const void *src_host, uint64_t nbytes, void *stream);
int psk_get_counters(psk_sketch *s, int64_t out[PSK_CTR_COUNT], void *stream); /* synchronises */
int psk_reset_counters(psk_sketch *s, void *stream);
/* recompute PSK_CTR_ABS_BOUND = max |counter| after the table was modified from outside the engine
 * (e.g. the RCCL all-reduce of the multi-GPU merge wrote into it) */
int psk_rescan_bound(psk_sketch *s, void *stream);

/* ------------------------------------------------------------- BloomFilter
 * add:   for each key: for i<k: bit = h_i % m; table |= bit      (bloom.py:234-250 add/add_alt)
 * check: for each key: out = AND_i bit(h_i % m)                  (bloom.py:252-272 check/check_alt)
 * check_bits: same result ballot-packed, bit (i & 63) of out_bits[i >> 6]; *hits += popcount (large batches: the partitioned lookup's
 *             answers -- n bytes of the handle's scratch -- packed by one streaming pass) */
int psk_bloom_add(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                  uint32_t key_len, int where, void *stream);
int psk_bloom_check(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                    uint32_t key_len, int where, uint8_t *out, void *stream);
int psk_bloom_check_bits(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                         uint32_t key_len, int where, uint64_t *out_bits, uint64_t *hits, void *stream);
/* Split lookup for DEVICE-resident keys: _begin hashes and partitions the batch without ever reading the table, _finish
 * probes it and writes out_dev[n] (0/1).  Everything between the two calls may still change the table -- the point is
 * to run pass 1 under a multi-GPU merge (pyprobables_amd/parallel.py) that is in flight on another stream.  The key
 * buffers must stay valid and unchanged until _finish; one pending lookup per handle.  Result == psk_bloom_check at
 * _finish time (bit-exact; an overflowing bucket segment is re-checked on the device). */
int psk_bloom_check_begin(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len,
                          void *stream);
int psk_bloom_check_finish(psk_sketch *s, uint8_t *out_dev, void *stream);
/* The ordered batch: exactly the loop  `for key in batch: seen = key in blm; blm.add(key)`  (bloom.py:234-272), every key's answer at ITS place
 * in the stream -- a key that repeats inside the batch is "seen" from its second occurrence on.  seen_out[i] = 0 / 1; *new_out (nullable) =
 * the number of keys with seen == 0, which is also what the loop `if key not in blm: blm.add(key)` adds (the two loops leave the same table
 * and the same flags).  Any key layout, any m < 2^63, both moduli.  The batch is resolved in ordered chunks of chunk_keys keys (0 = the
 * default, min(2^18, 2^20 / k)), two launches per chunk, through an open-addressing map in the handle's scratch (counted by
 * psk_scratch_bytes, freed by psk_release_scratch); the answers do not depend on the chunk.  PSK_HOST: host pointers, the call returns
 * with the results in place.  PSK_DEVICE: device pointers, enqueue only.  n == 0 launches nothing and writes *new_out = 0.  A map that
 * overflows (impossible with its sizing) is an error, never a silent answer: PSK_EHIP from this call (PSK_HOST) or from the next call of
 * this entry point on the handle (PSK_DEVICE). */
int psk_bloom_add_running(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                          uint32_t key_len, int where, uint64_t chunk_keys /* 0 = default */,
                          uint8_t *seen_out /* [n] */, uint64_t *new_out /* nullable: #keys with seen == 0 */, void *stream);

/* ----------------------------------------------------- CountingBloomFilter
 * Batches (weights: uint32[n] or NULL = all 1).  Round 4: the result of every batch equals the reference's per-key loop over it for ANY
 * stream -- adds commute (the clamp at 2^32-1 included); psk_cbf_remove is a TRANSACTION: it runs unordered (optimistic decrement, or lookup
 * -> amounts -> checked decrement) and proves on the way that the result does not depend on the order inside the batch; where it does
 * (duplicates of a key with too few inserts, a false positive among absent keys, a frozen counter) the batch is undone and replayed in
 * order on the device (k_cbf_ordered).  Option "remove_exact" = 0 restores the round-3 contract: exact for well-formed streams (no counter
 * saturates; every remove targets a key with >= num_els live inserts), anything else tallied in PSK_CTR_VIOLATIONS / PSK_CTR_SATURATED.
 * Update WINDOWS (round 4; tables of more than 2^24 counters, 16-byte keys, unit weights; options "update_window" = 0: off,
 * "update_window_keys": capacity): add / remove batches too small to pay for a pass over the table wait on the device, in arrival order, as
 * key copies (the caller's buffer is free when the call returns); the window reaches the table in ONE pass that walks it batch run by batch
 * run and proves every deferred remove (it must meet a non-zero counter at its own position of the stream: countingbloom.py:198-201);
 * a window that fails the proof is undone and replayed batch by batch through the transaction above.  Every entry point that reads the
 * table applies what is waiting first (psk_flush before using psk_table_info's pointer).
 * add:    counters[h_i % m] = min(c + w, 2^32-1) for i<k        (countingbloom.py:125-155)
 * remove: conditional decrement                                 (countingbloom.py:176-208)
 * check:  out = min_i counters[h_i % m]                         (countingbloom.py:157-174)
 * Big tables (more than 2^24 counters -- option "nibble_min_lg_update"; round 3):
 *   - unit-weight add batches too small to pay for a pass over the table (n * k < m / 8) are write-combined automatically: the
 *     batch is hashed and partitioned when it is handed over, its probes wait in persistent per-slice segments and reach the
 *     table together with their successors (adds commute, the clamp at 2^32-1 is applied all the same: exact, no opt-in;
 *     option "auto_combine" = 0 turns it off, "auto_combine_keys" sizes the segments).  Every entry point that reads the
 *     table, removes or hands out its pointer applies what is waiting first (psk_flush before using psk_table_info's pointer).
 *   - a unit-weight psk_cbf_remove of at least m / 8 probes decrements optimistically (one pass; exact whenever every counter
 *     holds what the batch takes from it, i.e. every key is present) and otherwise undoes that and takes the lookup + masked
 *     decrement path; it reads ONE 4-byte verdict back, i.e. synchronises `stream` once (option "remove_optimistic" = 0: never).
 *   - lookups of a table that is not changing (from 2^23 counters on): the partitioned psk_cbf_check squeezes the 32-bit table
 *     into 4-bit slice images on every call; from the second such call in a row on it keeps them (cells / 2 bytes, freed by
 *     psk_release_scratch) and later calls on the same stream load them instead, until any entry point that may write the
 *     table -- or psk_table_info, which hands its pointer out -- is called on the handle (option "cbf_lookup_shadow" = 0: never).
 *     Whoever writes to the table behind the engine's back must say so afterwards: psk_rescan_bound (as for the wrap-free bound). */
int psk_cbf_add(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                uint32_t key_len, const uint32_t *weights, int where, void *stream);
int psk_cbf_remove(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                   uint32_t key_len, const uint32_t *weights, int where, void *stream);
int psk_cbf_check(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                  uint32_t key_len, int where, uint32_t *out, void *stream);
/* Write-combined updates incl. REMOVES (opt-in).  The fold of a big counter table read-modify-writes the whole table whatever the batch
 * brings (1 GiB at BASELINE config 4), so small batches -- the config's 1M-key add / remove batches -- are collected on the
 * device and applied as ONE partitioned update per list once "combine_keys" keys (psk_set_option, default 2^26) are waiting:
 * first the adds (countingbloom.py:135-155), then the removes as plain decrements of every index by the key's weight
 * (countingbloom.py:203-206 with to_remove == num_els).  Exact for well-formed streams (every remove targets a key with at
 * least num_els live inserts at that point of the stream; nothing saturates) -- the contract of the unordered batch ops
 * above; a decrement below zero is tallied in PSK_CTR_VIOLATIONS.  Unlike psk_cbf_remove no per-key min is read first, so a
 * remove of an ABSENT key is a violation here, not a no-op.  Every other entry point on the handle (check, read_table,
 * get_counters, synchronize, merge ...) applies what is waiting first; psk_clear / psk_write_table drop it.  Before handing
 * the raw table pointer (psk_table_info) to anything else call psk_flush.  remove = 0: add, 1: remove. */
int psk_cbf_update_combined(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                            uint32_t key_len, const uint32_t *weights, int remove, int where, void *stream);
/* applies everything that waits in the engine on `stream`: the write-combined CBF updates above and a deferred Bloom clear (psk_clear).
 * Call it before reading or writing the table through a pointer from psk_table_info. */
int psk_flush(psk_sketch *s, void *stream);
/* Ordered (one-at-a-time, in sequence) execution of the reference semantics on the GPU, including
 * each op's return value: exact for ANY stream.  weights int64[n] or NULL (=1); opmode psk_opmode. */
int psk_cbf_update_ordered(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                           uint32_t key_len, const int64_t *weights, int opmode, int where, uint32_t *out,
                           void *stream);
/* countingbloom.py:135-208 for a whole ORDERED batch in parallel: out[i] (uint32[n]), the table and the PSK_CTR_ADDED / _REMOVED / _SATURATED /
 * _ABS_BOUND tallies end exactly as psk_cbf_update_ordered(..., PSK_OP_SIGNED, ...) leaves them for the same stream.  An op acts on each of
 * its counters as a map (a, p): x -> (x == MAX || x + p >= MAX) ? MAX : x + a, MAX = 2^32 - 1 sticky; an add is (w, w), a remove that finds
 * its key with at least w is (-w, -inf), and (a1, p1) then (a2, p2) is (a1 + a2, max(p1, a1 + p2)).  A counter's value in front of an op is
 * a segmented scan of these maps in arrival order per counter: a hash pass (probe e = i * k + s), a stable radix sort of (counter, e), the
 * scan, a per-op pass -- over ordered chunks of at most min(2^20, 2^23 / k) ops; the scratch does not grow with n.  The scan is optimistic
 * (a remove takes min(min_val, w), nothing from an absent key): the per-op pass verifies every remove and every op that hits one counter
 * twice, and the commit of a chunk waits for that verdict (one word read back per chunk).  A chunk that fails it has changed nothing and is
 * replayed in order on one lane.  Tables with k > 64 or m > 2^32 walk the whole batch on one lane.  Read-only options
 * "cbf_running_fast_chunks" / "cbf_running_replayed_chunks" count the chunks either way, "cbf_running_sequential" the calls that were not
 * eligible.  Updates that wait in the engine (write-combined lists, the update window) reach the table first.  PSK_HOST / PSK_DEVICE as for
 * psk_cms_add_running (PSK_DEVICE: out is a device pointer; the call still waits for each chunk's verdict); n == 0 runs nothing.
 * psk_cbf_add_running: weights int32[n] >= 0 or NULL (= 1).  A negative weight in a PSK_HOST batch is PSK_EINVAL before anything changes;
 * in a PSK_DEVICE batch it counts as 0 and is tallied in PSK_CTR_VIOLATIONS. */
int psk_cbf_add_running(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                        uint32_t key_len, const int32_t *weights /* NULL = 1, >= 0 */, int where, uint32_t *out, void *stream);
/* weights int32[n] or NULL (= +1): w >= 0 adds w, w < 0 removes -w; every int32 is valid (INT32_MIN removes 2^31) */
int psk_cbf_update_running(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                           uint32_t key_len, const int32_t *weights /* NULL = +1 */, int where, uint32_t *out, void *stream);

/* ---------------------------------------------------------- CountMinSketch
 * bins row-major by depth: bin = (h_i % width) + i*width, i < depth (countminsketch.py:275)
 * add:    saturating at INT32_MAX    (countminsketch.py:257-288)
 * remove: saturating at INT32_MIN    (countminsketch.py:290-321)
 * check:  min | mean (int32 out);  mean-min needs elements_added (int64 out)  (countminsketch.py:323-340,429-453)
 * Unordered batches are bit-exact with the reference whenever the final table does not depend on
 * order (same-sign weights, or no bin touching a rail). */
int psk_cms_add(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                uint32_t key_len, const int32_t *weights, int where, void *stream);
int psk_cms_remove(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                   uint32_t key_len, const int32_t *weights, int where, void *stream);
int psk_cms_check(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                  uint32_t key_len, int where, int query /* MIN or MEAN */, int32_t *out, void *stream);
int psk_cms_check_meanmin(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                          uint32_t key_len, int where, int64_t elements_added, int64_t *out, void *stream);
/* out (optional): int64[n + 1] -- the n return values, then elements_added after the batch (exact int64 clamps) */
int psk_cms_update_ordered(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                           uint32_t key_len, const int64_t *weights, int opmode, int query,
                           int64_t elements_added_in, int where, int64_t *out, void *stream);
/* countminsketch.py:267-288 for a whole ORDERED batch of adds at once: out[i] is what the reference's add(key_i, w_i) returns at its place
 * in the stream under `query` (int32[n]; int64[n] for PSK_Q_MEANMIN), the table, *els_out = elements_added and the PSK_CTR_SATURATED /
 * PSK_CTR_ABS_BOUND tallies end as the loop `for i: add(key_i, w_i)` leaves them.  weights: int32[n] >= 0 or NULL (= 1).  With w >= 0 a
 * bin's value after op i is the saturating sum of the weights that reached it so far, a segmented scan in arrival order per (row, bin): a
 * stable radix sort by bin per row, the scan, a per-op query -- a fixed number of streaming passes over ordered chunks of at most 2^20 ops
 * (the scratch does not grow with n).  Tables with depth > 64 or width > 2^32 walk the batch on one lane (psk_cms_update_ordered's kernel)
 * instead; read-only options "cms_running_fast" / "cms_running_sequential" count the calls either way.  A negative weight in a PSK_HOST
 * batch is PSK_EINVAL before the table changes; in a PSK_DEVICE batch (enqueue only: out, els_out are device pointers) it is the caller's
 * to exclude -- it counts as 0 and is tallied in PSK_CTR_VIOLATIONS. */
int psk_cms_add_running(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                        uint32_t key_len, const int32_t *weights /* NULL = 1 */, int where, int query,
                        int64_t els_in, void *out /* int32[n]; int64[n] for PSK_Q_MEANMIN */,
                        int64_t *els_out, void *stream);
/* countminsketch.py:267-321 for a whole ORDERED batch of adds AND removes: weights int32[n] or NULL (= +1), w >= 0 adds w, w < 0 removes
 * -w; every int32 is valid (INT32_MIN removes 2^31).  out[i], the table, *els_out and the PSK_CTR_SATURATED / PSK_CTR_ABS_BOUND tallies end
 * exactly as psk_cms_update_ordered(..., PSK_OP_SIGNED, ...) leaves them for the same stream.  An op on a bin is the map
 * x -> clamp(x + w, INT32_MIN, INT32_MAX); such maps compose to maps of the same form, (a, lo, hi): x -> min(hi, max(lo, x + a)), so the
 * bin's value after op i is a segmented scan of maps applied to the table -- the passes, chunks, eligibility (depth <= 64, width <= 2^32,
 * else the one-lane kernel) and the PSK_HOST / PSK_DEVICE conventions of psk_cms_add_running; n == 0 runs nothing and returns els_in.
 * Read-only options "cms_update_running_fast" / "cms_update_running_sequential" count the calls either way ("cms_running_*" are
 * psk_cms_add_running's alone). */
int psk_cms_update_running(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                           uint32_t key_len, const int32_t *weights /* NULL = +1 */, int where, int query,
                           int64_t els_in, void *out /* int32[n]; int64[n] for PSK_Q_MEANMIN */,
                           int64_t *els_out, void *stream);

/* ------------------------------------------------------------------ hashing
 * out[i*depth + j] = fnv_1a(key_i, seed=j)  (hashes.py:71-103); layout != PSK_KEYS_HASHES */
int psk_fnv1a_hash(int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len,
                   uint32_t depth, int where, uint64_t *out, int device, void *stream);
/* the digest families (hashes.py:17-40,125-150 default_md5 / default_sha256): a CHAIN, tmp = H(tmp).digest() per depth
 * step, out[i*depth + j] = LE64 of the first 8 bytes of link j.  Byte layouts only (PSK_KEYS_FIXED / PSK_KEYS_VARLEN8);
 * the reference UTF-8-encodes a str for these families (hashes.py:34), which is the caller's packing job. */
enum psk_digest { PSK_DIGEST_MD5 = 0, PSK_DIGEST_SHA256 = 1 };
int psk_digest_chain(int algo, int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len,
                     uint32_t depth, int where, uint64_t *out, int device, void *stream);

/* ------------------------------------------------------------ QuotientFilter
 * quotientfilter.py: a table of 2^q slots (3 <= q <= 31) for 32-bit hashes, quotient = h >> r, remainder = h & (2^r - 1), r = 32 - q.
 * No handle: the caller owns the four arrays (device memory) --
 *   filter        remainders, uint8 / uint16 / uint32 per slot for r <= 8 / r <= 16 / else (the reference's array type codes B / I / L)
 *   occupied, continuation, shifted   bit arrays, LSB first in 32-bit words, max(2^q / 32, 1) words each
 * The reference drops duplicates and keeps runs sorted, so its table depends only on the SET of hashes inserted; every call below
 * produces or reads exactly that table (DESIGN.md "Quotient filter").
 *   hash       out[i] = fnv_1a_32(key_i, 0) (hashes.py:106-122: add / check hash this way); `where` as everywhere (out follows the keys);
 *              PSK_KEYS_HASHES rows give the low 32 bits of their first hash
 *   build      the table of the n SORTED DISTINCT hashes (n <= 2^q; sorting and deduplicating is the caller's -- any radix sort), written
 *              over whatever the arrays held: what `for h in hashes: add_alt(h)` leaves (quotientfilter.py:154-166, :291-394) for any
 *              order and any duplicates.  scratch_dev: n / 1024 + 2 int32.  Enqueue only.
 *   check      out[i] = 0 / 1, check(key_i) (quotientfilter.py:187-206, :471-491); check_alt: the same for device uint32 hashes
 *   decode     the table's hashes in slot order (ascending up to a rotation; sort for the ascending list), two passes around the
 *              caller's prefix sums: out_dev NULL -> word_counts_dev[3][words] (int64) receives per metadata word the run starts, occupied
 *              bits and slots in use, marks_dev[0] the first slot with continuation = shifted = 0, marks_dev[1] the first empty slot
 *              (0xFFFFFFFF: full table; quotientfilter.py:215-218 starts hashes() there); the caller turns each row into INCLUSIVE
 *              prefix sums in place and calls again with out_dev (uint32[out_cap], out_cap >= the last entry of row 2: the element
 *              count) (quotientfilter.py:208-245 hashes / get_hashes).  Enqueue only.
 *   remove_alt `for h in hashes: remove_alt(h)` (quotientfilter.py:177-185, _remove_element :396-469) for n SORTED DISTINCT device hashes, on a
 *              table with at least one empty slot and q >= 5 (a smaller or a completely full table is rebuilt: decode, drop, build): the table
 *              of the remaining set, repaired in place cluster by cluster (DESIGN.md "Quotient filter: removal"); absent hashes are no-ops.
 *              scratch_dev: 2 * words + 2 + n uint32 whose first 2 * words + 2 are ZERO on entry and zero again when the call has run (one
 *              allocation serves every call on the table); *removed_dev receives the number of hashes taken out.  The reference's
 *              `_elements_added` is not decremented by a removal: that counter is the caller's.  Enqueue only.
 *   add_alt    `for h in hashes: add_alt(h)` (quotientfilter.py:154-166, _add :355-394) for n SORTED DISTINCT device hashes into a loaded table
 *              with q >= 5, auto-expansion left to the caller: the table of the union, each touched region rewritten in place (DESIGN.md
 *              "Quotient filter: insertion in place"); hashes already in the table are no-ops.  result_dev[0] receives the number added,
 *              result_dev[1] a status: 0 = the table holds the union, non-zero = the union does not fit (or fills the table so that one
 *              region comes round to its own start) and NOTHING was written: rebuild, or raise.  scratch_dev: 2 * words + 2 + n uint32 whose
 *              first 2 * words + 2 are ZERO on entry and zero again when the call has run -- remove_alt's layout: one allocation serves both.
 *              Work is proportional to the regions touched.  Enqueue only. */
int psk_qf_hash(int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len, int where, uint32_t *out,
                int device, void *stream);
int psk_qf_build(uint32_t q, const uint32_t *sorted_hashes_dev, uint64_t n, void *filter_dev, uint32_t *occupied_dev,
                 uint32_t *continuation_dev, uint32_t *shifted_dev, int32_t *scratch_dev, int device, void *stream);
int psk_qf_check(uint32_t q, const void *filter_dev, const uint32_t *occupied_dev, const uint32_t *continuation_dev,
                 const uint32_t *shifted_dev, int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len,
                 int where, uint8_t *out, int device, void *stream);
int psk_qf_check_alt(uint32_t q, const void *filter_dev, const uint32_t *occupied_dev, const uint32_t *continuation_dev,
                     const uint32_t *shifted_dev, const uint32_t *hashes_dev, uint64_t n, uint8_t *out_dev, int device, void *stream);
int psk_qf_remove_alt(uint32_t q, void *filter_dev, uint32_t *occupied_dev, uint32_t *continuation_dev, uint32_t *shifted_dev,
                      const uint32_t *sorted_hashes_dev, uint64_t n, uint32_t *scratch_dev, uint32_t *removed_dev, int device, void *stream);
int psk_qf_add_alt(uint32_t q, void *filter_dev, uint32_t *occupied_dev, uint32_t *continuation_dev, uint32_t *shifted_dev,
                   const uint32_t *sorted_hashes_dev, uint64_t n, uint32_t *scratch_dev, uint32_t *result_dev, int device, void *stream);
int psk_qf_decode(uint32_t q, const void *filter_dev, const uint32_t *occupied_dev, const uint32_t *continuation_dev,
                  const uint32_t *shifted_dev, int64_t *word_counts_dev, uint32_t *marks_dev, uint32_t *out_dev, uint64_t out_cap,
                  int device, void *stream);

/* --------------------------------------------------------- BloomFilterBank
 * Many small Bloom filters of ONE geometry (m_bits, k) in one table: `filters` rows of psk_bank_row_bytes(m_bits) =
 * psk_bloom_table_bytes(m_bits) bytes each, contiguous, bits LSB-first as in psk_bloom_add; the pad bits of a row at or beyond m_bits are
 * never set.  Row f is, byte for byte, the table of the reference's BloomFilter after add() of the keys sent to f (bloom.py:234-272).
 * No handle: the caller owns the (device) table; `data` / `offsets` / `ids` / `out` follow `where`, the table and seg / perm are device memory.
 *   add    bloom.py:241-250 per row: filter ids[i] gets key i.  ids >= filters are skipped, never written.
 *   check  out[i] = AND of the k bits of key i in row ids[i] (bloom.py:261-272); 0 for ids >= filters.
 *   build  keys grouped by filter, device keys only: filter f gets the keys at grouped positions [seg[f], seg[f+1]); position j is key
 *          perm[j] (perm == NULL: key j).  seg = uint64[filters + 1] on the device, non-decreasing, seg[filters] <= n.  One workgroup
 *          per (filter, part) sets the bits in an LDS image of the row and ORs the non-zero words into the table once.
 *          split: workgroups per filter (>= 1).  route: 0 = per part (the image unless the part is small or the row exceeds 65536 bytes),
 *          1 = always the LDS image (rows over 65536 bytes: PSK_EINVAL), 2 = atomics straight into the row.  Enqueue only.
 * PSK_KEYS_HASHES needs key_len >= k.  n < 2^32 per call. */
uint64_t psk_bank_row_bytes(uint64_t m_bits);
int psk_bank_add(void *table_dev, uint64_t filters, uint64_t m_bits, uint32_t k, int layout, const void *data, const uint64_t *offsets,
                 uint64_t n, uint32_t key_len, int where, const uint32_t *ids, int device, void *stream);
int psk_bank_check(const void *table_dev, uint64_t filters, uint64_t m_bits, uint32_t k, int layout, const void *data,
                   const uint64_t *offsets, uint64_t n, uint32_t key_len, int where, const uint32_t *ids, uint8_t *out, int device,
                   void *stream);
int psk_bank_build(void *table_dev, uint64_t filters, uint64_t m_bits, uint32_t k, int layout, const void *data, const uint64_t *offsets,
                   uint64_t n, uint32_t key_len, const uint64_t *seg_dev, const uint32_t *perm_dev, uint32_t split, int route, int device,
                   void *stream);

/* The slice image: the bank transposed, for "which filters may hold this key" (the bit-sliced signatures of BIGSI / COBS).  All filters of a
 * bank share m_bits, k and the hash family, so a key has the same k bit positions in every row; the filters that pass bloom.py:261-272 for
 * the key are the AND of k rows of the transposed table.
 *   layout  slices = uint32[m_bits][psk_bank_slice_row_bytes(filters) / 4] in device memory, owned by the caller, 16-byte aligned;
 *           psk_bank_slice_row_bytes(filters) = ceil(filters / 8) rounded up to 16 (host only).  Bit f of slice row p (word f >> 5, bit f & 31,
 *           LSB-first) == bit p of bank row f.  Columns at and beyond `filters` are zero in every row; a bank row's pad bits (p >= m_bits) have
 *           no slice row.  Byte offsets are 64-bit: m_bits * slice_row_bytes may pass 2^32.
 *   slices  STORES (not ORs) the word columns of filters [first_filter, last_filter) of every slice row from the table: a filter that was
 *           cleared is cleared in the image.  first_filter is a multiple of 32; last_filter is a multiple of 32 or == filters, and then the
 *           row's pad words behind the last filter are written (as zero) too.  Words outside the range are not touched; (0, filters) writes the
 *           whole image.  An empty range does nothing; anything else is PSK_EINVAL.  Enqueue only.
 *   match   for key i: bit f of mask_dev[i][..] (uint32[n][slice_row_bytes / 4], 16-byte aligned) is 1 exactly when all k bits of key i are set
 *           in filter f -- what psk_bank_check answers for (i, f) -- and columns >= filters are 0; count_dev[i] = the number of set bits of that
 *           row; ids_dev[out_offsets_dev[i] ...] = its set columns, ascending (out_offsets_dev = uint64[n], the exclusive prefix sums of a
 *           counts call).  The outputs are device memory whatever `where` says; each may be NULL, at least one must be given, ids_dev and
 *           out_offsets_dev go together.  Keys follow `where` (a PSK_HOST call returns when the kernel has read them).  k <= 64: the k
 *           positions of a workgroup's 256 keys live in k * 1024 bytes of LDS.  n == 0 launches nothing. */
uint64_t psk_bank_slice_row_bytes(uint64_t filters);
int psk_bank_slices(const void *table_dev, uint64_t filters, uint64_t m_bits, void *slices_dev, uint64_t first_filter, uint64_t last_filter,
                    int device, void *stream);
int psk_bank_match(const void *slices_dev, uint64_t filters, uint64_t m_bits, uint32_t k, int layout, const void *data, const uint64_t *offsets,
                   uint64_t n, uint32_t key_len, int where, uint32_t *mask_dev, uint32_t *count_dev, const uint64_t *out_offsets_dev,
                   uint32_t *ids_dev, int device, void *stream);

/* Scoring a query against every filter (the threshold queries of BIGSI / COBS).  A query is a set of keys: query q is keys
 * [query_offsets_dev[q], query_offsets_dev[q + 1]) of the batch (uint64[queries + 1], device memory, non-decreasing from 0 to n; not checked --
 * whatever it holds, no key at or beyond n is read).  The slice image and the keys are those of psk_bank_match; the per-key mask never leaves the CU.
 *   score   scores_dev[q * filters + f] (uint32[queries][filters] in device memory whatever `where` says: the row stride is `filters` words, the
 *           image's pad columns have no column, nothing is written beyond queries * filters words) = the number of keys i of query q whose k bits
 *           are all set in filter f: the sum of psk_bank_check's answers for (i, f), a repeated key counted each time.  A score is below 2^31.
 *           split (1 .. 65535): workgroups per query, each taking a contiguous part of its keys; with split > 1 the call zeroes scores_dev on
 *           `stream` and the parts add into it.  The result is the same for every split.  An empty query's row is zeros; queries == 0 launches
 *           nothing; n == 0 writes zero rows.  k <= 64 as for match.  Keys follow `where` (a PSK_HOST call returns when the kernel has read them).
 *           Element offsets are 64-bit: queries * filters may pass 2^32.  Enqueue only.  (DESIGN.md 3.13 "Scoring a query")
 *   score_select  over finished scores: count_dev[q] = the number of filters f with scores[q][f] >= thresholds_dev[q] (uint32[queries], device,
 *           every value >= 1); ids_dev[out_offsets_dev[q] ...] = those filters, ascending, and hit_scores_dev[out_offsets_dev[q] ...] = their
 *           scores beside them (out_offsets_dev = uint64[queries], the exclusive prefix sums of a counts call).  Each output may be NULL, at least
 *           one must be given; ids_dev and out_offsets_dev go together; hit_scores_dev needs ids_dev, ids_dev may come without it. */
int psk_bank_score(const void *slices_dev, uint64_t filters, uint64_t m_bits, uint32_t k, int layout, const void *data, const uint64_t *offsets,
                   uint64_t n, uint32_t key_len, int where, const uint64_t *query_offsets_dev, uint64_t queries, uint32_t split,
                   uint32_t *scores_dev, int device, void *stream);
int psk_bank_score_select(const uint32_t *scores_dev, uint64_t queries, uint64_t filters, const uint32_t *thresholds_dev, uint32_t *count_dev,
                          const uint64_t *out_offsets_dev, uint32_t *ids_dev, uint32_t *hit_scores_dev, int device, void *stream);

/* Bank statistics: the filters of a bank as sets -- what the reference answers per object, for every row (pair, group) in one launch.
 * No handle: tables, id lists, seg / members and outputs are device memory owned by the caller; tables and dst are 16-byte aligned.  Enqueue
 * only, on `stream`.  Rows are read whole (psk_bank_row_bytes): the pad bits of a row are never set.  An id at or beyond its table counts as
 * an empty row (as psk_bank_check answers 0).  Byte and element offsets are 64-bit: filters * row_bytes and na * nb may pass 2^32.
 *   popcount  out[i] = the set bits of row ids[i] (bloom.py:340-352's _cnt_number_bits_set, the input of estimate_elements); ids_dev == NULL:
 *             row i, and n == filters is required.  n == 0 launches nothing; more rows than the grid holds are walked with a stride.
 *   overlap   out[i * nb + j] = popcount(row a_ids[i] of A AND row b_ids[j] of B), uint32[na][nb] row-major: count_int of bloom.py:448-457
 *             (jaccard_index) for every pair; count_union = popcount(a) + popcount(b) - count_int.  NULL id lists mean rows 0 .. na - 1 /
 *             0 .. nb - 1, and then na <= filters_a / nb <= filters_b is required.  Ids may repeat and come in any order.  m_bits == 2^31 is
 *             accepted: the counts fit the unsigned word.  Same table, same id list (both NULL, or one pointer) and na == nb: only the tiles
 *             on or above the diagonal are computed, each stored at both places.  na, nb < 2^32.  
 *   reduce    row g of dst (`groups` rows of the table's row size) = the OR (op 0: bloom.py:401-428 union, chained) or the AND (op 1:
 *             bloom.py:371-399 intersection, chained) of the source rows members[seg[g] .. seg[g + 1]); seg = uint64[groups + 1],
 *             non-decreasing.  Rows are STORED, not ORed in.  bits_dev[g] (uint64, may be NULL) = the popcount of the stored row: what
 *             bloom.py:398 / 427 feed to estimate_elements.  An empty group stores a zero row under either op.  dst overlapping src, or
 *             any other op: PSK_EINVAL. */
int psk_bank_popcount(const void *table_dev, uint64_t filters, uint64_t m_bits, const uint32_t *ids_dev, uint64_t n, uint64_t *out_dev,
                      int device, void *stream);
int psk_bank_overlap(const void *table_a_dev, uint64_t filters_a, const uint32_t *a_ids_dev, uint64_t na, const void *table_b_dev,
                     uint64_t filters_b, const uint32_t *b_ids_dev, uint64_t nb, uint64_t m_bits, uint32_t *out_dev, int device,
                     void *stream);
int psk_bank_reduce(const void *src_dev, uint64_t filters, uint64_t m_bits, const uint64_t *seg_dev, const uint32_t *members_dev,
                    uint64_t groups, int op, void *dst_dev, uint64_t *bits_dev, int device, void *stream);

/* ------------------------------------------------------ CountMinSketchBank
 * Many small count-min sketches of ONE geometry (width, depth) in one table: `sketches` rows of psk_cms_table_bytes(width, depth) bytes each
 * (4 * width * depth rounded up to 16), contiguous; row s is int32[depth][width], row-major by depth (bin = h_i % width + i * width,
 * countminsketch.py:275); the pad ints of a row are never written.  Row s followed by the footer "IIq" (width, depth, elements_added[s]) is,
 * byte for byte, the export of the reference's CountMinSketch(width, depth) after add(key, num_els) of the ops sent to s
 * (countminsketch.py:257-288, 342-354).  Only adds enter a bank, with weights >= 0: every bin ends at min(old + the sum of the weights that
 * reached it, INT32_MAX) in any order of execution.  elements_added is the caller's (one int64 per sketch).
 * 1 <= width <= 2^31, 1 <= depth <= 64, n < 2^32 per call, PSK_KEYS_HASHES needs key_len >= depth; anything else is PSK_EINVAL.  build and reduce
 * take rows of fewer than 2^32 ints (width * depth rounded up to 4; wider rows: PSK_EINVAL before anything is enqueued -- add and the checks carry
 * 64-bit row sizes).  Byte offsets
 * are 64-bit: sketches * row bytes may pass 2^32.  No handle: the caller owns the (device, 16-byte aligned) table; `data` / `offsets` /
 * `ids` / `weights` / `out` follow `where`; the table, seg / perm / members, bound_dev, els_dev and saturated_dev are device memory.
 *   bound_dev  int64[sketches] or NULL: the caller's upper bound on the largest value any bin of sketch s can hold AFTER this call (old bound
 *          + the weights this call sends to s).  Where bound_dev[s] <= INT32_MAX an add to s is a plain no-return atomic add; otherwise, and
 *          with bound_dev == NULL, it is the clamping compare-and-swap add of psk_cms_add.  A bound that is too low lets bins wrap.
 *   saturated_dev  uint64 or NULL: raised by one for every clamping add that met the rail (a diagnostic, as PSK_CTR_SATURATED).
 *   add    countminsketch.py:267-288 per row: sketch ids[i] gets key i with weight weights[i] (NULL: 1).  ids >= sketches are skipped, never
 *          written.  A negative weight in a PSK_HOST batch is PSK_EINVAL before anything changes; in a PSK_DEVICE batch it is NOT checked and
 *          counts as 0 (the caller validates device weights, as for psk_cbf_add_running).
 *   check  out[i] = the reference's check of key i on sketch ids[i] under PSK_Q_MIN or PSK_Q_MEAN (sum // depth, Python floor), int32
 *          (countminsketch.py:429-436); check_meanmin: the mean-min query (:438-453), int64, with elements_added read from els_dev[ids[i]]
 *          on the device; width == 1 is PSK_EINVAL as for psk_cms_check_meanmin.  Both answer 0 for ids >= sketches.
 *   build  keys grouped by sketch, device keys only: sketch s gets the keys at grouped positions [seg[s], seg[s+1]); position j is key
 *          perm[j] (perm == NULL: key j) with weight weights_dev[perm[j]] (NULL: 1; negative: 0).  seg = uint64[sketches + 1] on the device,
 *          non-decreasing, seg[sketches] <= n; whatever seg and perm hold, no key at or beyond n is read and no int outside the table is
 *          written.  One workgroup per (sketch, part) counts in an LDS image of the row and adds every NON-ZERO counter to the row once --
 *          plain or clamping by the rule of bound_dev; a zero counter is never touched.  The image holds rows of
 *          width * depth <= 16384 ints.  A part takes it only where no 32-bit LDS counter can wrap: weights_dev == NULL, or
 *          bound_dev[s] <= INT32_MAX; any other part adds straight to the row, clamping.  split: workgroups per sketch (1 .. 65535).
 *          route: 0 = per part (the image unless keys * depth * 8 < the row's ints or the row is over the cap), 1 = the image wherever no
 *          counter can wrap (rows over the cap: PSK_EINVAL), 2 = atomics straight into the row.  Enqueue only.
 *   reduce row g of dst (`groups` rows of the table's row size) = the rows members[seg[g] .. seg[g + 1]) of src folded by the reference's join
 *          (countminsketch.py:380-399), a left fold in member order per bin starting from an empty sketch: an accumulator on either rail
 *          stays frozen, else acc = clamp(acc + b) computed in int64 -- exact for negative bins too.  els_out_dev[g] (int64, may be NULL) =
 *          the same clamped fold of els_dev[member] (els_dev == NULL: zeros).  A member >= sketches counts as an empty sketch, an empty group
 *          gives a zero row.  Rows are STORED.  dst overlapping src: PSK_EINVAL.  seg = uint64[groups + 1], non-decreasing; groups < 2^32;
 *          groups and row pieces beyond the grid are walked with a stride.  Enqueue only. */
int psk_cms_bank_add(void *table_dev, uint64_t sketches, uint64_t width, uint32_t depth, int layout, const void *data, const uint64_t *offsets,
                     uint64_t n, uint32_t key_len, int where, const uint32_t *ids, const int32_t *weights, const int64_t *bound_dev,
                     uint64_t *saturated_dev, int device, void *stream);
int psk_cms_bank_check(const void *table_dev, uint64_t sketches, uint64_t width, uint32_t depth, int layout, const void *data,
                       const uint64_t *offsets, uint64_t n, uint32_t key_len, int where, const uint32_t *ids, int query, int32_t *out,
                       int device, void *stream);
int psk_cms_bank_check_meanmin(const void *table_dev, uint64_t sketches, uint64_t width, uint32_t depth, int layout, const void *data,
                               const uint64_t *offsets, uint64_t n, uint32_t key_len, int where, const uint32_t *ids,
                               const int64_t *els_dev, int64_t *out, int device, void *stream);
int psk_cms_bank_build(void *table_dev, uint64_t sketches, uint64_t width, uint32_t depth, int layout, const void *data,
                       const uint64_t *offsets, uint64_t n, uint32_t key_len, const uint64_t *seg_dev, const uint32_t *perm_dev,
                       const int32_t *weights_dev, const int64_t *bound_dev, uint64_t *saturated_dev, uint32_t split, int route, int device,
                       void *stream);
int psk_cms_bank_reduce(const void *src_dev, const int64_t *els_dev, uint64_t sketches, uint64_t width, uint32_t depth,
                        const uint64_t *seg_dev, const uint32_t *members_dev, uint64_t groups, void *dst_dev, int64_t *els_out_dev, int device,
                        void *stream);

/* ------------------------------------------------------------ CuckooFilter
 * cuckoo/cuckoo.py: `capacity` buckets of `bucket_size` fingerprints of `fp_bits` bits.  No handle: the caller owns (device memory)
 *   buckets   uint32[capacity][bucket_size], every row filled from the left, its unused slots 0 (an export is this array plus the footer)
 *   fill      uint32[capacity], the fingerprints in each row (fingerprint 0 is legal, so the zeros do not say it)
 * 1 <= capacity < 2^31, bucket_size >= 1, 1 <= fp_bits <= 32.  A key is the triple fp = fnv_1a(key) & (2^fp_bits - 1),
 * idx_1 = fp % capacity, idx_2 = fnv_1a(str(fp)) % capacity (cuckoo.py:483-506); `triples` is uint32[3][n]: the fps, the idx_1s, the idx_2s.
 * Every call leaves the table exactly as the reference's loop over the same keys would (DESIGN.md "Cuckoo filter").
 *   triples      out[3][n] of the keys; PSK_KEYS_HASHES rows carry fnv_1a(key), or a fingerprint itself (the re-insert stream of
 *                _expand_logic, cuckoo.py:455-481); `where` as everywhere (out follows the keys)
 *   check        out[i] = 0 / 1, check(key_i) (cuckoo.py:306-315, :440-446), hash and lookup in one kernel
 *   present      the same for device triples
 *   place_sweep / place_apply   the part of `for t in triples: _insert_fingerprint(t)` (cuckoo.py:361-368) in front of the first key that
 *                needs a kick, for triples that are neither in the table nor repeated (the caller's job: present + any sort).
 *                claims_dev: the 2m values idx << 32 | j << 1 | which (which = 0: idx_1 of key j, 1: idx_2) in ascending order,
 *                pos_dev[which * m + j]: where that claim stands.  d_in / d_out: one byte per key, 1 / 2 = goes to idx_1 / idx_2,
 *                3 = needs a kick; start from all 1 and sweep with the two buffers swapped.  Each sweep sets marks_dev[0] to the first key
 *                whose decision changed (0xFFFFFFFF: none) and marks_dev[1] to the first key that decided 3: keys in front of marks[0]
 *                are final (the sweep that changed nothing in front of e proves [0, e): a triangular system has one fixed point).
 *                place_apply writes the keys [0, prefix) by the decisions d_dev, prefix <= min(marks) of the last sweep, and counts
 *                them into fill.  Enqueue only.
 *   insert       triples [start, end) one after the other by ONE lane: add (dedup != 0: skip a fingerprint found in its two rows,
 *                cuckoo.py:291-304) or the re-insert of an expansion (dedup = 0), kicks included (cuckoo.py:361-392).  The kicks draw from
 *                the MT19937 in mt_state_dev: the 625 words of Python's random.getstate()[1], read at the start, written back at the end,
 *                so random.setstate() with them leaves `random` where the reference would.  Stops early after `budget` steps (a key and a
 *                swap are one step each; bounds the launch, budget >= 1) or at a failed walk, whose swaps stay.  result_dev[12], in and
 *                out: [0] 0 = stopped at end / at the budget in front of key [1], 1 = the walk of key [1] failed, 2 = bad arguments in
 *                device memory (indices outside the table), 3 = the budget ran out INSIDE the walk of key [1]; [1] the first key not
 *                done, [2] the fingerprint left over, [3] fingerprints newly counted, [4] keys that began to walk, [5] steps used,
 *                [6..8] the suspended walk (fingerprint in hand, row, swaps done).  Pass [0] = 0 on entry -- or, to take a suspended walk
 *                up, the words of the launch that returned 3, with start = its [1].  Enqueue only.
 *   remove       out[i] = remove(key_i) in order (cuckoo.py:317-330) for device triples: rank_dev[i] = how many earlier requests of the batch
 *                carry the same fingerprint (any stable sort).  bucket_size <= 32.  row_marks_dev: uint32[capacity], zero on entry and
 *                zero again afterwards.  Rows are compacted to the left, vacated slots zeroed, fill lowered.  Enqueue only. */
int psk_ck_triples(uint64_t capacity, uint32_t fp_bits, int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len,
                   int where, uint32_t *out, int device, void *stream);
int psk_ck_check(uint64_t capacity, uint32_t bucket_size, uint32_t fp_bits, const uint32_t *buckets_dev, const uint32_t *fill_dev, int layout,
                 const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len, int where, uint8_t *out, int device, void *stream);
int psk_ck_present(uint64_t capacity, uint32_t bucket_size, const uint32_t *buckets_dev, const uint32_t *fill_dev,
                   const uint32_t *triples_dev, uint64_t n, uint8_t *out_dev, int device, void *stream);
int psk_ck_place_sweep(uint64_t capacity, uint32_t bucket_size, const uint32_t *fill_dev, const uint32_t *triples_dev,
                       const uint64_t *claims_dev, const uint32_t *pos_dev, uint64_t m, const uint8_t *d_in_dev, uint8_t *d_out_dev,
                       uint32_t *marks_dev, int device, void *stream);
int psk_ck_place_apply(uint64_t capacity, uint32_t bucket_size, uint32_t *buckets_dev, uint32_t *fill_dev, const uint32_t *triples_dev,
                       const uint64_t *claims_dev, const uint32_t *pos_dev, uint64_t m, const uint8_t *d_dev, uint64_t prefix, int device,
                       void *stream);
int psk_ck_insert(uint64_t capacity, uint32_t bucket_size, uint32_t max_swaps, uint32_t *buckets_dev, uint32_t *fill_dev,
                  const uint32_t *triples_dev, uint64_t n, uint64_t start, uint64_t end, int dedup, uint64_t budget,
                  uint32_t *mt_state_dev, uint32_t *result_dev, int device, void *stream);
int psk_ck_remove(uint64_t capacity, uint32_t bucket_size, uint32_t *buckets_dev, uint32_t *fill_dev, const uint32_t *triples_dev,
                  const uint32_t *rank_dev, uint64_t n, uint32_t *row_marks_dev, uint8_t *out_dev, int device, void *stream);

/* ------------------------------------------------------------ CountingCuckooFilter
 * cuckoo/countingcuckoo.py: the cuckoo filter as a multiset.  No handle: the caller owns (device memory)
 *   bins      uint32[capacity][bucket_size][2], (fingerprint, count) pairs, every row filled from the left, its unused pairs 0: the
 *             reference's export byte for byte (an export is this array plus the "II" footer)
 *   fill      uint32[capacity], the bins in each row
 * Limits, triples and the MT19937 words as for the CuckooFilter; psk_ck_triples and psk_ck_place_sweep (which reads only `fill`) serve both.
 *   check        out[i] = check(key_i) (countingcuckoo.py:175-191): the count of the first bin that holds the fingerprint, idx_1's row
 *                left to right, else idx_2's, else 0; hash and lookup in one kernel, `where` as everywhere
 *   present      0 / 1 per device triple
 *   place_apply  psk_ck_place_apply for this layout: key j is written as (fp, counts_dev[j]); counts_dev NULL: 1 for every key
 *   insert       psk_ck_insert for this layout, without its dedup (the caller hands it fingerprints that are not in the table -- the new
 *                ones of a batch -- or the re-insert stream of an expansion).  A bin placed directly takes counts_dev[i] (NULL: 1), a bin
 *                that has to walk goes in hand with count 1 WHATEVER counts_dev[i] says (countingcuckoo.py:247), a swap exchanges pairs.
 *                result_dev as there, and [9] the count of the leftover, [10] the count in hand of a suspended walk.  Enqueue only.
 *   add_counts   u DISTINCT fingerprints as triples[3][u]: weights_dev[t] is added to the first bin that holds fingerprint t (the order of
 *                check).  missed_dev[t] = 0: done, 1: no bin holds it, 2: the count would pass 2^32 - 1 and the bin is left as it is;
 *                flags_dev[0] / [1] = how many 1s / 2s.  Distinct fingerprints own distinct bins: plain stores.  Enqueue only.
 *   remove       u DISTINCT fingerprints as triples, requests_dev[t] removes of each: granted_dev[t] = min(requests, sum of the counts of
 *                its copies), taken from the copies in the order of check; bins that reach 0 leave their row (rows are compacted to the
 *                left, pairs together, vacated pairs zeroed, fill lowered) and are counted into emptied_dev[0].  bucket_size <= 32;
 *                row_marks_dev: uint32[capacity], zero on entry and zero again afterwards.  Enqueue only. */
int psk_cck_check(uint64_t capacity, uint32_t bucket_size, uint32_t fp_bits, const uint32_t *bins_dev, const uint32_t *fill_dev, int layout,
                  const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len, int where, uint32_t *out, int device, void *stream);
int psk_cck_present(uint64_t capacity, uint32_t bucket_size, const uint32_t *bins_dev, const uint32_t *fill_dev,
                    const uint32_t *triples_dev, uint64_t n, uint8_t *out_dev, int device, void *stream);
int psk_cck_place_apply(uint64_t capacity, uint32_t bucket_size, uint32_t *bins_dev, uint32_t *fill_dev, const uint32_t *triples_dev,
                        const uint64_t *claims_dev, const uint32_t *pos_dev, uint64_t m, const uint8_t *d_dev, uint64_t prefix,
                        const uint32_t *counts_dev, int device, void *stream);
int psk_cck_insert(uint64_t capacity, uint32_t bucket_size, uint32_t max_swaps, uint32_t *bins_dev, uint32_t *fill_dev,
                   const uint32_t *triples_dev, const uint32_t *counts_dev, uint64_t n, uint64_t start, uint64_t end, uint64_t budget,
                   uint32_t *mt_state_dev, uint32_t *result_dev, int device, void *stream);
int psk_cck_add_counts(uint64_t capacity, uint32_t bucket_size, uint32_t *bins_dev, uint32_t *fill_dev, const uint32_t *triples_dev,
                       const uint32_t *weights_dev, uint64_t u, uint8_t *missed_dev, uint32_t *flags_dev, int device, void *stream);
int psk_cck_remove(uint64_t capacity, uint32_t bucket_size, uint32_t *bins_dev, uint32_t *fill_dev, const uint32_t *triples_dev,
                   const uint32_t *requests_dev, uint64_t u, uint32_t *row_marks_dev, uint32_t *granted_dev, uint32_t *emptied_dev,
                   int device, void *stream);

/* ------------------------------------------------------ table algebra (device pointers)
 * Streaming kernels over whole tables; also the local half of the multi-GPU merge.
 * or/and: bloom.py:371-428 union/intersection;  popcount: bloom.py:552-557;
 * add_sat_i32: countminsketch.py:380-391 join;  add_u32: countingbloom.py:296-298 union;
 * or_reduce: dst[w] = OR_j src[j*slice_words + w] (the reduce step of allreduce(OR): RCCL has no OR op)
 * psk_table_add_sat_i32, psk_table_add_u32 and psk_cbf_intersect know nothing of handles: a caller who applies them to the table of a
 * CountMinSketch / CountingBloomFilter handle owes that handle a psk_rescan_bound afterwards.  The handle's unordered adds and removes
 * choose between wrapping atomics and the saturating path by PSK_CTR_ABS_BOUND; with a stale bound, counters that the sum has brought
 * close to a rail wrap under the next psk_cbf_add / psk_cms_add instead of stopping there. */
int psk_table_or(void *dst, const void *src, uint64_t nwords32, int device, void *stream);
int psk_table_and(void *dst, const void *src, uint64_t nwords32, int device, void *stream);
int psk_table_popcount(const void *tab, uint64_t nwords32, uint64_t *out_host, int device, void *stream);
int psk_table_nonzero_u32(const void *tab, uint64_t nwords32, uint64_t *out_host, int device, void *stream);
int psk_table_add_sat_i32(void *dst, const void *src, uint64_t n, int device, void *stream);
int psk_table_add_u32(void *dst, const void *src, uint64_t n, uint64_t *overflowed_host, int device, void *stream);
/* countingbloom.py:210-269: intersection (sum where both non-zero) and the two counts of jaccard_index */
int psk_cbf_intersect(void *dst, const void *a, const void *b, uint64_t n, uint64_t *overflowed_host, int device, void *stream);
int psk_cbf_jaccard_counts(const void *a, const void *b, uint64_t n, uint64_t out_host[2] /* union, intersection */,
                           int device, void *stream);
int psk_or_reduce_slices(void *dst, const void *src, uint32_t nslices, uint64_t slice_words32, int device,
                         void *stream);

/* ------------------------------------------------------ multi-GPU merge (SURVEY.md 8b "psk_merge_allreduce", 8e)
 * One rank per GPU holds a full-size replica fed with its own range of the key stream; ONE collective makes every replica
 * the table a single sketch fed the whole stream would hold.  `nccl_comm` is the caller's ncclComm_t (RCCL) for this rank,
 * passed as void* (ncclCommInitRank / ncclCommInitAll: one communicator per device); the handle's table is merged in
 * place on `stream`.  RCCL is looked up in the host process (no link-time dependency of libpsk_hip.so).
 *   psk_merge_or   Bloom: allreduce(OR) = grouped ncclSend/ncclRecv of the bit-range slices (slice j goes straight to rank
 *                  j), the engine's OR-reduce kernel, ncclAllGather.  bloom.py:401-428 (union is a bytewise OR).
 *                  elements_added of the merged filter is the SUM over ranks (the caller's scalar).
 *   psk_merge_sum  CMS / CBF: allreduce(SUM) of the counters -- 32-bit while the summed per-rank bounds prove that no counter
 *                  reaches a rail, else 64-bit and clamped like join (countminsketch.py:380-391; CBF at 2^32-1,
 *                  countingbloom.py:149-151); the tallies of psk_get_counters (added / removed / violations / saturated)
 *                  become global totals (cells the merge itself clamps are counted once, not once per rank).  ONE-SHOT per
 *                  stream segment: replicas and tallies are per-rank deltas going in, global totals coming out -- merging
 *                  the same replicas twice counts everything again.  Synchronises `stream` once (8-byte read-back of the
 *                  summed bound; each rank's bound is capped at 2^40 first so the sum cannot wrap).
 * One-rank communicators return at once (option "merge_single_rank" = 1 runs the collective path anyway: tests). */
int psk_merge_or(psk_sketch *s, void *nccl_comm, void *stream);
int psk_merge_sum(psk_sketch *s, void *nccl_comm, void *stream);

/* --------------------------------------------- filters whose insert depends on a lookup
 * ExpandingBloomFilter / RotatingBloomFilter (expandingbloom.py:140-170, :320-331): a key goes into the newest filter
 * unless ANY filter of the stack already reports it.  All filters share (m, k, hash): hash once, then index kernels.
 *   psk_bloom_indices        out_idx_dev[i*k + j] = hash_j(key_i) % m  (bloom.py:247; device buffer; m <= 2^32)
 *   psk_idx_test             out[i] = all k bits set (bloom.py:269-271); accumulate != 0: out[i] |= ...  (the `any`
 *                            over the filters of expandingbloom.py:147)
 *   psk_idx_resolve_ordered  flag[i] = 1 iff the sequential loop "if key not in table: table.add(key)" over the ordered
 *                            batch would insert key i (expandingbloom.py:166-170), else 0; present[i] != 0 marks keys
 *                            another filter already holds (nullable); table_dev is NOT modified.  first_dev: uint32[m]
 *                            scratch, all-ones on entry and again on exit; count_dev: uint64 scratch; *inserted_host
 *                            receives the number of inserts (NULL: no host sync)
 *   psk_idx_insert           table |= bits of the keys with flag[i] == 1 (flag NULL: all keys)  (bloom.py:247-249)
 *   psk_bytes_or             dst[i] |= src[i] */
int psk_bloom_indices(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len,
                      int where, uint32_t *out_idx_dev, void *stream);
int psk_idx_test(const void *table_dev, const uint32_t *idx_dev, uint64_t n, uint32_t k, uint8_t *out_dev, int accumulate,
                 int device, void *stream);
int psk_idx_resolve_ordered(const void *table_dev, const uint32_t *idx_dev, const uint8_t *present_dev, uint64_t n, uint32_t k,
                            uint32_t *first_dev, uint8_t *flag_dev, uint64_t *count_dev, uint64_t *inserted_host, int device,
                            void *stream);
/* the same resolution with the per-bit scratch replaced by a bounded hash map (round 4): slots_dev = uint32[2][2^lg_slots], all-ones on entry
 * and on exit, 2^lg_slots >= 2 * n * k.  The caller walks an ordered chunk in sub-chunks of n keys -- resolve, insert, next -- so the scratch
 * is a few MB whatever the filter's size (psk_idx_resolve_ordered needs 4 bytes per filter BIT).  count_dev[0] += keys to insert,
 * count_dev[1] != 0: the map overflowed (cannot happen with the sizing above).  Enqueue only: no host synchronisation.
 * Bit position 2^32 - 1 is the map's "empty" marker and must not appear in idx_dev: this entry serves filters of m <= 2^32 - 1 bits
 * (psk_idx_resolve_ordered has no such limit below m = 2^32). */
int psk_idx_resolve_ordered_hashed(const void *table_dev, const uint32_t *idx_dev, const uint8_t *present_dev, uint64_t n, uint32_t k,
                                   void *slots_dev, uint32_t lg_slots, uint8_t *flag_dev, uint64_t *count_dev, int device, void *stream);
int psk_idx_insert(void *table_dev, const uint32_t *idx_dev, const uint8_t *flag_dev, uint64_t n, uint32_t k, int device,
                   void *stream);
int psk_bytes_or(void *dst_dev, const void *src_dev, uint64_t n, int device, void *stream);

/* --------------------------------------------- synthetic streams (bench / tests)
 * key_i = LE64(sm(seed+2i)) || LE64(sm(seed+2i+1)); w_i = 1 + sm((seed^0xC0FFEE)+i) % 7 */
int psk_gen_keys16(void *dst_dev, uint64_t start, uint64_t n, uint64_t seed, int device, void *stream);
int psk_gen_weights(void *dst_dev, uint64_t start, uint64_t n, uint64_t seed, int device, void *stream);
/* GUPS-style ceiling: n uniformly random 4-byte atomic ORs (op=0), atomic adds (op=1) or loads (op=2)
 * into a table of nwords32 words; the denominator of the "random-access roofline" */
int psk_gups(void *table_dev, uint64_t nwords32, uint64_t n, int op, uint64_t seed, uint64_t *sink_dev,
             int device, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PSK_H */
