// psk_capi.hip -- the extern "C" boundary (include/psk.h), the part every sketch shares: errors, handle lifetime, the option table, clear,
// table I/O, counters and scratch accounting.  The entry points that take keys live with their sketch (psk_bloom.hip, psk_cbf.hip,
// psk_cms.hip, psk_hash.hip, psk_quotient.hip, psk_cuckoo.hip) over the staging layer of psk_stage.hpp; table algebra: psk_table_ops.hip.
#include "psk_stage.hpp"

#include <map>
#include <mutex>
#include <utility>

// ------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}


extern "C" const char *psk_last_error(void) { return g_err; }
extern "C" int psk_version(void) { return 100; }

extern "C" int psk_device_count(int *count)
{
    if (!count) return fail(PSK_EINVAL, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(PSK_ENODEV, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return PSK_OK;
}

static uint64_t round16(uint64_t b) { return (b + 15) & ~15ULL; }
extern "C" uint64_t psk_bloom_table_bytes(uint64_t m_bits) { return round16((m_bits + 7) / 8); }
extern "C" uint64_t psk_cbf_table_bytes(uint64_t m) { return round16(4 * m); }
extern "C" uint64_t psk_cms_table_bytes(uint64_t width, uint32_t depth) { return round16(4 * width * (uint64_t)depth); }

int ensure(DevBuf &b, uint64_t bytes)
{
    if (bytes <= b.cap) return PSK_OK;
    if (b.p) HIP_TRY(hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    uint64_t cap = bytes + bytes / 4 + 256;
    HIP_TRY(hipMalloc(&b.p, cap));
    b.cap = cap;
    return PSK_OK;
}


static int create_common(int kind, uint64_t m, uint32_t k, uint64_t padded, uint64_t logical, int device,
                         void *ext_table, psk_sketch **out)
{
    if (!out) return fail(PSK_EINVAL, "out handle pointer is NULL");
    *out = nullptr;
    if (m == 0 || k == 0) return fail(PSK_EINVAL, "table dimensions must be > 0 (m=%llu k=%u)", (unsigned long long)m, k);
    if (m >> 62) return fail(PSK_EINVAL, "table too large");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(PSK_ENODEV, "no HIP device available (%s)", e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(PSK_EINVAL, "device %d out of range [0,%d)", device, ndev);
    PSK_USE_DEVICE(device);
    psk_sketch *s = new (std::nothrow) psk_sketch();
    if (!s) return fail(PSK_ENOMEM, "host allocation failed");
    s->kind = kind;
    s->device = device;
    s->m = m;
    s->k = k;
    s->md = make_mod(m, &s->pow2);
    s->padded_bytes = padded;
    s->logical_bytes = logical;
    s->owns_table = ext_table == nullptr;
    s->shadow.exposed = ext_table != nullptr;  // (until the caller declares the table private to this handle: psk_sketch_set_option)
    s->table = ext_table;
    s->ctr = nullptr;
    if (s->owns_table) {
        hipError_t e2 = hipMalloc(&s->table, padded);
        if (e2 != hipSuccess) {
            delete s;
            return fail(PSK_ENOMEM, "hipMalloc(%llu bytes) for the table failed: %s", (unsigned long long)padded,
                        hipGetErrorString(e2));
        }
        e2 = hipMemset(s->table, 0, padded);
        if (e2 != hipSuccess) {
            hipFree(s->table);
            delete s;
            return fail(PSK_EHIP, "hipMemset failed: %s", hipGetErrorString(e2));
        }
    }
    hipError_t e3 = hipMalloc((void **)&s->ctr, sizeof(long long) * PSK_CTR_COUNT);
    if (e3 == hipSuccess) e3 = hipMemset(s->ctr, 0, sizeof(long long) * PSK_CTR_COUNT);
    if (e3 != hipSuccess) {
        if (s->owns_table) hipFree(s->table);
        delete s;
        return fail(PSK_ENOMEM, "counter allocation failed: %s", hipGetErrorString(e3));
    }
    *out = s;
    return PSK_OK;
}

extern "C" int psk_bloom_create(uint64_t m_bits, uint32_t k, int device, void *ext_table, psk_sketch **out)
{
    return create_common(PSK_KIND_BLOOM, m_bits, k, psk_bloom_table_bytes(m_bits), (m_bits + 7) / 8, device, ext_table, out);
}

extern "C" int psk_cbf_create(uint64_t m, uint32_t k, int device, void *ext_table, psk_sketch **out)
{
    return create_common(PSK_KIND_CBF, m, k, psk_cbf_table_bytes(m), 4 * m, device, ext_table, out);
}

extern "C" int psk_cms_create(uint64_t width, uint32_t depth, int device, void *ext_table, psk_sketch **out)
{
    return create_common(PSK_KIND_CMS, width, depth, psk_cms_table_bytes(width, depth), 4 * width * (uint64_t)depth,
                         device, ext_table, out);
}

// Every scratch buffer of a handle, each ONCE: f(buffer, waiting) -> PSK_OK to go on.  waiting: the buffer holds updates that have not reached the
// table (psk_scratch_bytes reports those apart).  psk_destroy, psk_scratch_bytes and psk_release_scratch all walk this one list.
template <class F>
static int for_each_scratch(psk_sketch *s, F &&f)
{
    for (DevBuf *b : {&s->s_keys, &s->s_offs, &s->s_w, &s->s_out, &s->s_aux, &s->s_part, &s->s_cnt, &s->s_flag, &s->s_spill, &s->s_omap, &s->s_tflag, &s->s_part2, &s->s_cnt2, &s->s_merge, &s->s_vals, &s->s_perm, &s->s_run, &s->s_tally,
                      &s->s_brw, &s->shadow.img, &s->s_wstat, &s->s_phase})
        PSK_TRY(f(*b, false));
    for (DevBuf *b : {&s->comb.add.keys, &s->comb.add.w, &s->comb.rem.keys, &s->comb.rem.w, &s->scat.add.part, &s->scat.add.cnt, &s->win.keys, &s->s_snap}) PSK_TRY(f(*b, true));
    return PSK_OK;
}

// ------------------------------------------------------------------ options
// Every process-wide option variable, defined ONCE (declared in psk_host.hpp), directly above the table that names it.
int64_t g_part_mode = 1;                   // 0 = direct kernels only, 1 = large batches take the partitioned passes
int64_t g_part_max_keys = 1 << 26;         // keys per partition round (bounds the bucket buffer: ~2 GB of scratch at k = 7)
int64_t g_part_cache_bytes = 240 << 20;    // bucket-buffer budget per round: the part of the 256 MB MALL we count on (part_round_keys)
int64_t g_part_two_level_slices = 2048;    // tables cut into more slices than this take the two-level path (0 = never)
int64_t g_part_debug = 0;                  // ablation bits for bench runs (PartGeom::dbg); 0 in production
int64_t g_part_tile_threads = 0;           // pass 1 workgroup shape for k <= 8: 0 = auto (launch_scatter), 512 / 1024 = forced
int64_t g_part_even_tiles = 1;             // pass 1 evens the tile size out over the workgroups
int64_t g_part_dense_groups = 40;          // pass 2 walks a wave's segments end to end below this many groups per segment (for_each_batch_at); 0 = never
int64_t g_part_bins = 1;                   // pass 1 through fixed-capacity bins wherever eligible (psk_part_bins.hpp); 0 = k_part_scatter everywhere
int64_t g_ragged_sort = 1;                 // pass 1 hands ragged keys to its lanes in order of length (psk_partition.hpp sort_tile); 0 = batch order
int64_t g_lookup_half = 1;                 // counter lookups into 2^26 .. 2^27 counters: 2^16-counter slices of 16-bit values
int64_t g_lookup_nibble = 1;               // CBF lookups into big tables: 4-bit slice images (psk_nibble.hpp) from cells / 16 probes on; 2 = always, 0 = never
int64_t g_update_nibble = 1;               // CBF unit adds / decrements into big tables: 4-bit delta images, one level; 0 = the two-level 32-bit path
int64_t g_nib_min_lg_lookup = 23;          // least log2(counters) of the 4-bit lookups (nib_geometry; crossovers: scripts/ab_nib_threshold.py)
int64_t g_nib_min_lg_update = 24;          // ... and the table must exceed 2^this for the 4-bit updates
int64_t g_small_weights = 1;               // weighted CMS adds in the compact probe format: 0 never, 1 by the hint (psk_sketch::wt), 2 always (tests)
int64_t g_remove_dryrun = 1;               // validated unit CBF removes into big tables: optimistic decrement first (psk_nibble.hpp)
int64_t g_combine_keys = 1 << 26;          // keys per list of psk_cbf_update_combined: 1 GiB of 16-byte keys per list
int64_t g_auto_combine_keys = 1 << 24;     // keys per list of "auto_combine" (~0.8 GB of segments for k = 7, allocated on first use)
int64_t g_window_wide = 1;                 // update windows on tables of few slices: five probe groups per lane and phase, byte-wide counts (0: three, nibbles)
int64_t g_window_tile = 0;                 // keys per pass-1 tile of an update window: 0 = by the rule in window_scatter, 2048 / 4096 = forced
int64_t g_window_force_fail = 0;           // tests: pretend a window's proof failed (exercises undo + replay on a well-formed stream)
int64_t g_merge_single_rank = 0;           // 1: psk_merge_* run the collective path even with one rank (tests)
int64_t g_lazy_clear = 1;                  // psk_clear of a Bloom table the engine alone reads is deferred; 0 = sweep at once
int64_t g_host_poll_us = 200;              // how long a tiny PSK_HOST call polls its mailbox before it waits for the stream; 0 = never poll
// read-only counters (tests, bench): calls / batches that took the path named
int64_t g_cbf_ordered_replays = 0;         // remove batches whose result depended on the order inside them: undone, replayed in order
int64_t g_window_folds = 0;                // update windows applied by the fold
int64_t g_window_replays = 0;              // ... and replayed batch by batch
int64_t g_small_weights_used = 0;          // weighted CMS adds that travelled in the compact format
int64_t g_cbf_shadow_hits = 0;             // nibble-slice lookups that loaded kept images (psk_sketch::shadow)
int64_t g_running_fast = 0;                // psk_cms_add_running calls that took the parallel passes
int64_t g_running_sequential = 0;          // ... and the one-lane kernel
int64_t g_update_running_fast = 0;         // psk_cms_update_running calls that took the parallel passes
int64_t g_update_running_sequential = 0;   // ... and the one-lane kernel
int64_t g_cbf_running_fast_chunks = 0;     // chunks of psk_cbf_add_running / _update_running the parallel passes served
int64_t g_cbf_running_replayed_chunks = 0; // ... and those whose verification failed: replayed in order on one lane
int64_t g_cbf_running_sequential = 0;      // calls of the two that were not eligible: the one-lane kernel for the whole batch
// Process DEFAULTS of the per-sketch options, in HandleOpt order.  Nothing but the option calls and resolve_options touches them: the engine
// reads psk_sketch::eff.
static int64_t g_sketch_default[HO_COUNT] = {
    1 << 16,  // partition_min_keys: least batch for the partitioned passes -- x1 for Bloom inserts, x4 for lookups / counter adds (part_wanted)
    1,        // cbf_lookup_shadow: nibble-slice lookups keep their 4-bit images while the table is unchanged (psk_sketch::shadow; cells / 2 bytes)
    1,        // auto_combine: small unit-weight add batches into big tables wait as scattered probes (adds commute: exact)
    1,        // update_window: small unit add / remove batches into big tables share one proven pass (psk_window.hpp)
    1 << 27,  // update_window_keys: most keys a window holds (16 bytes each); also capped by cells / 2 and the scratch budget
    0,        // scratch_budget_bytes: cap on a handle's partition scratch (more, smaller rounds); 0 = none
    1,        // remove_exact: order-dependent remove batches are replayed in order; 0 = clamped and tallied as violations
    2,        // bloom_lookup: 0 keyed probes + miss stores, 1 return trip, 3 tile flags, 4 lazy gathers, 2 = by the observed miss rate
};

// ONE table for every option.  Classes (include/psk.h lists the first by name):
//   supported   tunables of the shipped library a caller may have a reason to touch;
//   threshold   where the engine switches between its kernel families, and test hooks -- tests steer small inputs onto the big-table paths with them;
//   knob        "part_debug" alone, the ablation / phase-profile bits of the measuring tools: compiled in only with -DPSK_BENCH_KNOBS=1
//               (python -m pyprobables_amd.build --knobs -> libpsk_hip_knobs.so), the shipped library answers "unknown option";
//   read-only   counters tests read back.
// Per-sketch options (ho >= 0): the row points at the process default; the handle holds the override (psk_sketch::opt), and every entry
// point that takes a handle resolves the two into psk_sketch::eff on entry (resolve_options).
namespace {
enum OptClass { kOptSupported, kOptThreshold, kOptKnob, kOptReadOnly };
struct OptDesc {
    const char *name;
    int64_t *var;
    OptClass cls;
    int64_t lo;   // smallest value accepted (smaller ones are raised to it)
    int ho = -1;  // HandleOpt of a per-sketch option; -1: process-wide
};
constexpr int64_t kAny = INT64_MIN;
const OptDesc kOptions[] = {
    // supported, per sketch
    {"partition_min_keys", &g_sketch_default[HO_PART_MIN_KEYS], kOptSupported, 1, HO_PART_MIN_KEYS},
    {"cbf_lookup_shadow", &g_sketch_default[HO_CBF_SHADOW], kOptSupported, kAny, HO_CBF_SHADOW},
    {"auto_combine", &g_sketch_default[HO_AUTO_COMBINE], kOptSupported, kAny, HO_AUTO_COMBINE},
    {"update_window", &g_sketch_default[HO_WINDOW], kOptSupported, kAny, HO_WINDOW},
    {"update_window_keys", &g_sketch_default[HO_WINDOW_KEYS], kOptSupported, kAny, HO_WINDOW_KEYS},
    {"scratch_budget_bytes", &g_sketch_default[HO_SCRATCH_BUDGET], kOptSupported, kAny, HO_SCRATCH_BUDGET},
    {"remove_exact", &g_sketch_default[HO_REMOVE_EXACT], kOptSupported, kAny, HO_REMOVE_EXACT},
    {"bloom_lookup", &g_sketch_default[HO_BLOOM_LOOKUP], kOptSupported, kAny, HO_BLOOM_LOOKUP},
    // supported, process-wide
    {"partition", &g_part_mode, kOptSupported, kAny},
    {"partition_max_keys", &g_part_max_keys, kOptSupported, 1024},
    {"partition_cache_bytes", &g_part_cache_bytes, kOptSupported, kAny},
    {"combine_keys", &g_combine_keys, kOptSupported, kAny},
    {"cms_small_weights", &g_small_weights, kOptSupported, kAny},
    {"pass1_bins", &g_part_bins, kOptSupported, kAny},
    {"merge_single_rank", &g_merge_single_rank, kOptSupported, kAny},
    {"lazy_clear", &g_lazy_clear, kOptSupported, kAny},
    // thresholds of the path choice, test hooks
    {"partition_two_level_slices", &g_part_two_level_slices, kOptThreshold, kAny},
    {"auto_combine_keys", &g_auto_combine_keys, kOptThreshold, kAny},
    {"tile_threads", &g_part_tile_threads, kOptThreshold, kAny},
    {"even_tiles", &g_part_even_tiles, kOptThreshold, kAny},
    {"dense_walk_groups", &g_part_dense_groups, kOptThreshold, kAny},
    {"lookup_half_slices", &g_lookup_half, kOptThreshold, kAny},
    {"remove_optimistic", &g_remove_dryrun, kOptThreshold, kAny},
    {"lookup_nibble_slices", &g_lookup_nibble, kOptThreshold, kAny},
    {"update_nibble_slices", &g_update_nibble, kOptThreshold, kAny},
    {"nibble_min_lg_lookup", &g_nib_min_lg_lookup, kOptThreshold, 20},
    {"nibble_min_lg_update", &g_nib_min_lg_update, kOptThreshold, 20},
    {"update_window_tile", &g_window_tile, kOptThreshold, kAny},
    {"update_window_wide", &g_window_wide, kOptThreshold, kAny},
    {"update_window_force_fail", &g_window_force_fail, kOptThreshold, kAny},
    {"ragged_sort", &g_ragged_sort, kOptThreshold, kAny},
    {"host_poll_us", &g_host_poll_us, kOptThreshold, kAny},
    // read-only counters
    {"cbf_ordered_replays", &g_cbf_ordered_replays, kOptReadOnly, kAny},
    {"update_window_folds", &g_window_folds, kOptReadOnly, kAny},
    {"update_window_replays", &g_window_replays, kOptReadOnly, kAny},
    {"cms_small_weights_used", &g_small_weights_used, kOptReadOnly, kAny},
    {"cbf_lookup_shadow_hits", &g_cbf_shadow_hits, kOptReadOnly, kAny},
    {"cms_running_fast", &g_running_fast, kOptReadOnly, kAny},
    {"cms_running_sequential", &g_running_sequential, kOptReadOnly, kAny},
    {"cms_update_running_fast", &g_update_running_fast, kOptReadOnly, kAny},
    {"cms_update_running_sequential", &g_update_running_sequential, kOptReadOnly, kAny},
    {"cbf_running_fast_chunks", &g_cbf_running_fast_chunks, kOptReadOnly, kAny},
    {"cbf_running_replayed_chunks", &g_cbf_running_replayed_chunks, kOptReadOnly, kAny},
    {"cbf_running_sequential", &g_cbf_running_sequential, kOptReadOnly, kAny},
    // measuring tools (bench builds only)
    {"part_debug", &g_part_debug, kOptKnob, kAny},
};
const OptDesc *opt_find(const char *name)
{
    for (const OptDesc &d : kOptions)
        if (!strcmp(name, d.name)) return (d.cls == kOptKnob && !kBenchKnobs) ? nullptr : &d;
    return nullptr;
}
}  // namespace

// The options in force for the call that enters now: the handle's override, else the process default of this moment (another thread may
// change a default at any time; it never takes effect in the middle of a call, which asks the same question more than once).
void resolve_options(psk_sketch *s)
{
    for (int i = 0; i < HO_COUNT; ++i) s->eff[i] = s->opt[i] != kHoUnset ? s->opt[i] : __atomic_load_n(&g_sketch_default[i], __ATOMIC_RELAXED);
}

extern "C" int psk_destroy(psk_sketch *s)
{
    if (!s) return PSK_OK;
    DeviceScope scope;
    (void)scope.enter(s->device);
    if (!s->owns_table && s->table) {  // the caller's table outlives the handle: write-combined updates still waiting must reach it
        resolve_options(s);  // (psk_destroy accepts NULL, so it does not pass the handle gate)
        if (flush_combined(s, nullptr) == PSK_OK) (void)hipStreamSynchronize(nullptr);
    }
    if (s->owns_table && s->table) hipFree(s->table);
    if (s->ctr) hipFree(s->ctr);
    if (s->lk.dev) hipFree(s->lk.dev);
    if (s->lk.pin) hipHostFree((void *)s->lk.pin);
    if (s->wt.pin) hipHostFree((void *)s->wt.pin);
    (void)for_each_scratch(s, [](DevBuf &b, bool) {
        if (b.p) hipFree(b.p);
        if (b.pin) hipHostFree(b.pin);
        return (int)PSK_OK;
    });
    if (s->win.pin) hipHostFree(s->win.pin);
    if (s->mbox) hipHostFree((void *)s->mbox);
    if (s->scat.ev) hipEventDestroy(s->scat.ev);
    delete s;
    return PSK_OK;
}

// table (padded to 16 bytes) and the handle's counter block, zeroed by one kernel
// (round 4: nontemporal stores measured SLOWER for this write-only sweep -- 247 vs 215 us for the 1 GiB table of cfg 4 -- unlike the
// read-modify-write passes; plain stores stay)
static __global__ __launch_bounds__(kBlock) void k_clear(uint4 *tab, uint64_t nvec, long long *ctr)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint4 z = make_uint4(0, 0, 0, 0);
    uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    for (; i + 3 * stride < nvec; i += 4 * stride) {  // four 16-byte stores in flight per lane
        tab[i] = z;
        tab[i + stride] = z;
        tab[i + 2 * stride] = z;
        tab[i + 3 * stride] = z;
    }
    for (; i < nvec; i += stride) tab[i] = z;
    if (blockIdx.x == 0 && threadIdx.x < PSK_CTR_COUNT) ctr[threadIdx.x] = 0;
}

// one launch for the table AND the counter block (two fills are two ~5 us launches; clear sits in every bench step)
static int launch_clear(psk_sketch *s, hipStream_t st)
{
    const uint64_t nvec = s->padded_bytes / 16;
    uint64_t grid = (nvec + kBlock * 4 - 1) / (kBlock * 4);
    if (grid > 2048) grid = 2048;
    if (grid == 0) grid = 1;
    hipLaunchKernelGGL(k_clear, dim3((unsigned)grid), dim3(kBlock), 0, st, (uint4 *)s->table, nvec, s->ctr);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

int clear_materialize(psk_sketch *s, hipStream_t st)
{
    if (!s->clear_pending) return PSK_OK;
    s->clear_pending = false;
    return launch_clear(s, st);
}

extern "C" int psk_clear(psk_sketch *s, void *stream)
{
    CHECK_HANDLE(s, -1);
    hipStream_t st = (hipStream_t)stream;
    PSK_TRY(drop_pending(s, st));  // write-combined updates that have not reached the table are cleared with it
    // Bloom table that nobody outside the engine reads: the sweep is deferred.  The next entry point that reads, writes or hands out the
    // table runs it first on its own stream (clear_materialize), except a single-level partitioned insert, whose first apply STORES its
    // slices instead of read-modify-writing them (psk_part_bloom_add.hip): the 32 MiB of zeros are then neither written nor read back.
    if (s->kind == PSK_KIND_BLOOM && g_lazy_clear != 0 && !s->shadow.exposed && (s->owns_table || s->table_private)) {
        s->clear_pending = true;
        return PSK_OK;
    }
    s->clear_pending = false;
    return launch_clear(s, st);
}

extern "C" int psk_synchronize(psk_sketch *s, void *stream)
{
    CHECK_HANDLE_RO(s, -1);
    PSK_TRY(flush_combined(s, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return PSK_OK;
}

extern "C" int psk_table_info(psk_sketch *s, void **dev_ptr, uint64_t *padded_bytes, uint64_t *logical_bytes)
{
    if (!s) return fail(PSK_EINVAL, "sketch handle is NULL");
    ++s->table_version;  // the pointer leaves the engine: whoever holds it may write
    if (s->clear_pending) {  // (no stream here: a deferred clear runs on the null stream -- psk_flush on the caller's stream first avoids it)
        PSK_USE_DEVICE(s->device);
        PSK_TRY(clear_materialize(s, nullptr));
    }
    if (dev_ptr) s->shadow.exposed = true;  // ... and later, too: no kept images until the holder says it is done (psk_rescan_bound)
    if (dev_ptr) *dev_ptr = s->table;
    if (padded_bytes) *padded_bytes = s->padded_bytes;
    if (logical_bytes) *logical_bytes = s->logical_bytes;
    return PSK_OK;
}

extern "C" int psk_read_table(psk_sketch *s, void *dst_host, uint64_t nbytes, void *stream)
{
    CHECK_HANDLE_RO(s, -1);
    if (!dst_host || nbytes > s->padded_bytes) return fail(PSK_EINVAL, "bad read_table arguments");
    hipStream_t st = (hipStream_t)stream;
    PSK_TRY(flush_combined(s, st));
    HIP_TRY(hipMemcpyAsync(dst_host, s->table, nbytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PSK_OK;
}

extern "C" int psk_write_table(psk_sketch *s, const void *src_host, uint64_t nbytes, void *stream)
{
    CHECK_HANDLE(s, -1);
    if (!src_host || nbytes > s->padded_bytes) return fail(PSK_EINVAL, "bad write_table arguments");
    hipStream_t st = (hipStream_t)stream;
    PSK_TRY(drop_pending(s, st));  // the table is replaced: pending updates go with the old contents
    s->clear_pending = false;  // (the fills below do what the deferred clear would)
    HIP_TRY(hipMemsetAsync(s->table, 0, s->padded_bytes, st));
    HIP_TRY(hipMemcpyAsync(s->table, src_host, nbytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(s->ctr, 0, sizeof(long long) * PSK_CTR_COUNT, st));
    if (s->kind != PSK_KIND_BLOOM) {
        // re-seed the wrap-free bound from the loaded counters
        const uint64_t nel = s->logical_bytes / 4;
        hipLaunchKernelGGL(k_absmax, dim3(grid_for_keys(nel)), dim3(kBlock), 0, st, (const uint32_t *)s->table, nel,
                           s->kind == PSK_KIND_CMS ? 1 : 0, s->ctr);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));
    return PSK_OK;
}

extern "C" int psk_rescan_bound(psk_sketch *s, void *stream)
{
    CHECK_HANDLE(s, -1);
    // "I wrote through the pointer I hold, and I am done": kept images may be built again (a holder of a caller-owned table must have
    // promised to announce every outside write: option "table_private")
    if (s->owns_table || s->table_private) s->shadow.exposed = false;
    if (s->kind == PSK_KIND_BLOOM) return PSK_OK;
    hipStream_t st = (hipStream_t)stream;
    PSK_TRY(flush_combined(s, st));
    HIP_TRY(hipMemsetAsync(s->ctr + PSK_CTR_ABS_BOUND, 0, sizeof(long long), st));
    const uint64_t nel = s->logical_bytes / 4;
    hipLaunchKernelGGL(k_absmax, dim3(grid_for_keys(nel)), dim3(kBlock), 0, st, (const uint32_t *)s->table, nel,
                       s->kind == PSK_KIND_CMS ? 1 : 0, s->ctr);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

extern "C" int psk_get_counters(psk_sketch *s, int64_t out[PSK_CTR_COUNT], void *stream)
{
    CHECK_HANDLE_RO(s, -1);
    if (!out) return fail(PSK_EINVAL, "out is NULL");
    hipStream_t st = (hipStream_t)stream;
    PSK_TRY(flush_combined(s, st));  // the tallies describe every update handed over so far
    HIP_TRY(hipMemcpyAsync(out, s->ctr, sizeof(long long) * PSK_CTR_COUNT, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PSK_OK;
}

extern "C" int psk_reset_counters(psk_sketch *s, void *stream)
{
    CHECK_HANDLE(s, -1);
    // keep the wrap-free bound: it describes the table, not the batch history
    HIP_TRY(hipMemsetAsync(s->ctr, 0, sizeof(long long) * PSK_CTR_ABS_BOUND, (hipStream_t)stream));
    return PSK_OK;
}

int raise_dyn_lds(const void *kernel, size_t bytes)
{
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, size_t> granted;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    size_t &have = granted[{kernel, dev}];
    if (bytes > have) {
        HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        have = bytes;
    }
    return PSK_OK;
}

extern "C" int psk_set_option(const char *name, int64_t value)
{
    if (!name) return fail(PSK_EINVAL, "option name is NULL");
    const OptDesc *d = opt_find(name);
    if (!d || d->cls == kOptReadOnly) return fail(PSK_EINVAL, d ? "option %s is read-only" : "unknown option %s", name);
    if (value < d->lo) value = d->lo;
    __atomic_store_n(d->var, value, __ATOMIC_RELAXED);  // (of a per-sketch option: the default; sketches without an override follow it from their next call on)
    return PSK_OK;
}

// bench-only: phase cycle totals of the last pass-1 launch (valid when part_debug & 32); zeroes them afterwards
extern "C" int psk_debug_phase_profile(psk_sketch *s, uint32_t nbuckets, uint32_t nwg, uint64_t out[12])
{
    if (!s || !s->s_cnt.p) return fail(PSK_EINVAL, "no partition scratch yet");
    PSK_USE_DEVICE(s->device);
    HIP_TRY(hipDeviceSynchronize());
    char *p = (char *)s->s_cnt.p + (size_t)nbuckets * nwg * 4;
    HIP_TRY(hipMemcpy(out, p, 96, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(p, 0, 96));
    return PSK_OK;
}

extern "C" int psk_sketch_set_option(psk_sketch *s, const char *name, int64_t value)
{
    if (!s || !name) return fail(PSK_EINVAL, "NULL argument");
    if (!strcmp(name, "table_private")) {
        s->table_private = value != 0;
        if (s->table_private) s->shadow.exposed = false;  // (from here on the holder announces its writes)
        else if (!s->owns_table) s->shadow.exposed = true;
        if (s->shadow.exposed && s->clear_pending) {  // the holder may read its table at any time from here on (null stream: no stream here)
            PSK_USE_DEVICE(s->device);
            PSK_TRY(clear_materialize(s, nullptr));
        }
        ++s->table_version;
        return PSK_OK;
    }
    const OptDesc *d = opt_find(name);
    if (!d || d->ho < 0) return fail(PSK_EINVAL, "%s is not a per-sketch option", name);
    if (value != kHoUnset && value < d->lo) value = d->lo;
    s->opt[d->ho] = value;  // (kHoUnset = INT64_MIN: follow the process default again)
    return PSK_OK;
}

extern "C" int psk_sketch_get_option(psk_sketch *s, const char *name, int64_t *value)
{
    if (!s || !name || !value) return fail(PSK_EINVAL, "NULL argument");
    if (!strcmp(name, "table_private")) {
        *value = s->table_private ? 1 : 0;
        return PSK_OK;
    }
    if (!strcmp(name, "window_pending_batches")) {  // read-only: batches the update window still holds (borrowed ones among them must stay as they are)
        *value = s->win.n ? (int64_t)s->win.batches.size() : 0;
        return PSK_OK;
    }
    if (!strcmp(name, "bloom_lookup_misses")) {  // read-only: the miss tally the handle's last finished large lookup published (-1: none yet)
        *value = s->lk.pin && s->lk.pin[1] ? (int64_t)s->lk.pin[0] : -1;
        return PSK_OK;
    }
    // read-only: the handle's pass-1 launches through the LDS bins (k_part_bins) -- how many, and keys per tile / workgroups of the last one
    if (!strcmp(name, "pass1_bins_launches")) {
        *value = (int64_t)s->bins.launches;
        return PSK_OK;
    }
    if (!strcmp(name, "pass1_bins_tile_keys")) {
        *value = (int64_t)s->bins.tile;
        return PSK_OK;
    }
    if (!strcmp(name, "pass1_bins_workgroups")) {
        *value = (int64_t)s->bins.wgs;
        return PSK_OK;
    }
    const OptDesc *d = opt_find(name);
    if (!d || d->ho < 0) return fail(PSK_EINVAL, "%s is not a per-sketch option", name);
    *value = s->opt[d->ho] != kHoUnset ? s->opt[d->ho] : __atomic_load_n(d->var, __ATOMIC_RELAXED);
    return PSK_OK;
}

extern "C" int psk_get_option(const char *name, int64_t *value)
{
    if (!name || !value) return fail(PSK_EINVAL, "NULL argument");
    const OptDesc *d = opt_find(name);
    if (!d) return fail(PSK_EINVAL, "unknown option %s", name);
    *value = __atomic_load_n(d->var, __ATOMIC_RELAXED);
    return PSK_OK;
}

// per-handle accounting of the device scratch (the write-combining / window lists are large and allocated on first use)
extern "C" int psk_scratch_bytes(psk_sketch *s, uint64_t bytes[3])
{
    if (!s || !bytes) return fail(PSK_EINVAL, "psk_scratch_bytes: NULL argument");
    uint64_t all = 0, waiting = 0;
    (void)for_each_scratch(s, [&](DevBuf &b, bool is_waiting) {
        if (b.p) all += b.cap;
        if (b.p && is_waiting) waiting += b.cap;
        return (int)PSK_OK;
    });
    bytes[0] = all;
    bytes[1] = waiting;
    bytes[2] = s->shadow.img.p ? s->shadow.img.cap : 0;
    return PSK_OK;
}

// release the partition / staging scratch of a handle (hundreds of MB after a large batch); it regrows on demand
extern "C" int psk_release_scratch(psk_sketch *s)
{
    CHECK_HANDLE_RO(s, -1);
    if (s->pend.active) return fail(PSK_EINVAL, "a split lookup is pending: finish it before releasing the scratch buffers");
    PSK_TRY(flush_combined(s, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    PSK_TRY(for_each_scratch(s, [](DevBuf &b, bool) {  // (the pinned pages stay: psk_destroy alone frees them)
        if (b.p) HIP_TRY(hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
        return (int)PSK_OK;
    }));
    s->scat.ready = false;
    s->shadow.built = s->shadow.seen = ~0ULL;
    s->shadow.seen_count = 0;
    return PSK_OK;
}
