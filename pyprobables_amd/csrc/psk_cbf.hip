// psk_cbf.hip -- the CountingBloomFilter entry points of the C ABI (include/psk.h), and what makes small updates into big tables wait for
// a shared pass: write-combined lists, scattered probes (psk_nibble.hpp) and the update window (psk_window.hpp).
#include "psk_stage.hpp"
#include "psk_nibble.hpp"
#include "psk_window.hpp"
#include "psk_cbf_running.hpp"

// ----------------------------------------------------- CountingBloomFilter
// the direct kernels of an unordered CBF update (w = nullptr: unit weights)
static int cbf_apply_direct(psk_sketch *s, const Batch &b, const uint32_t *w, bool remove, hipStream_t st)
{
    unsigned long long *sat = (unsigned long long *)(s->ctr + PSK_CTR_SATURATED);
    return with_source(b, [&](auto src) {
        return with_pow2(s, [&](auto P) {
            if (remove) return launch_apply(src, CbfSub<P.value>{(uint32_t *)s->table, s->md, s->k, w, sat - 1}, b.n, st);
            return launch_apply(src, CbfAdd<P.value>{(uint32_t *)s->table, s->md, s->k, w, s->ctr, sat, false}, b.n, st);
        });
    });
}

// one unordered CBF update over a DEVICE-resident batch: add (countingbloom.py:135-155) or the unchecked decrement
static int cbf_apply_device(psk_sketch *s, const Batch &b, const uint32_t *w, bool remove, hipStream_t st)
{
    if (b.n == 0) return PSK_OK;
    PSK_TRY(post_acct(s, w, b.n, remove ? PSK_CTR_REMOVED : PSK_CTR_ADDED, (long long)s->k, st, !remove, false));
    bool done = false;
    PSK_TRY(remove ? cbf_remove_partitioned(s, b, w, st, &done, 0, nullptr) : cbf_add_partitioned(s, b, w, st, &done));
    PSK_TRY(settle_acct(s, w, b.n, st));
    if (done) return PSK_OK;
    return cbf_apply_direct(s, b, w, remove, st);
}

// ---- write-combined updates as scattered probes (psk_sketch::scat, psk_nibble.hpp)
// a flush (or drop) on another stream than the last append must not overtake it
// (the event is recorded only when a second stream shows up: one per append put a barrier packet -- ~5 us of dispatch bubble --
// behind every 1 M-key batch of BASELINE cfg 4, 0.45 ms per step)
static int comb_order(psk_sketch *s, hipStream_t st)
{
    if (!s->scat.appended || st == s->scat.last) return PSK_OK;
    if (!s->scat.ev) HIP_TRY(hipEventCreateWithFlags(&s->scat.ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(s->scat.ev, s->scat.last));  // the tail of the stream that appended last: behind all of its appends
    HIP_TRY(hipStreamWaitEvent(st, s->scat.ev, 0));
    s->scat.last = st;  // (what follows on `st` is ordered behind it)
    return PSK_OK;
}

static int comb_appended(psk_sketch *s, hipStream_t st)
{
    s->scat.last = st;
    s->scat.appended = true;
    return PSK_OK;
}

// does one of the mechanisms older than the update window hold updates: key lists, borrowed lists, the scattered list
static bool older_updates_pending(const psk_sketch *s)
{
    return s->comb.add.n || s->comb.rem.n || s->comb.badd.n() || s->comb.brem.n() || (s->scat.ready && s->scat.add.n);
}

static int scat_zero(psk_sketch *s, hipStream_t st)
{
    const uint64_t nseg = (uint64_t)s->scat.g.nbuckets * s->scat.g.nwg;
    if (!s->scat.add.cnt.p) return PSK_OK;
    hipLaunchKernelGGL(k_zero_u32, dim3(256), dim3(256), 0, st, (uint32_t *)s->scat.add.cnt.p, nseg);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

static int scat_drop(psk_sketch *s, hipStream_t st)
{
    if (!s->scat.ready || s->scat.add.n == 0) return PSK_OK;
    PSK_TRY(comb_order(s, st));
    PSK_TRY(scat_zero(s, st));
    s->scat.add.n = 0;
    return PSK_OK;
}

// forget every update that waits: the table is cleared or replaced, what has not reached it goes with the old contents
int drop_pending(psk_sketch *s, hipStream_t st)
{
    s->comb.add.n = s->comb.rem.n = 0;
    s->comb.add.unit = s->comb.rem.unit = true;
    s->comb.badd.clear();
    s->comb.brem.clear();
    s->win.n = s->win.copied = 0;  // (the update window too; a window's back-off is a property of the stream and stays)
    s->win.batches.clear();
    return scat_drop(s, st);
}

// apply the scattered list.  Enough probes: one pass over the table (k_nib_apply); few: a drain with atomics.
static int scat_flush(psk_sketch *s, hipStream_t st)
{
    if (!s->scat.ready || s->scat.add.n == 0) return PSK_OK;
    PSK_TRY(comb_order(s, st));
    const uint64_t na = s->scat.add.n;
    s->scat.add.n = 0;  // (cleared first: a failure must not re-apply the list on the next call)
    PartGeom g = s->scat.g;
    const uint64_t per_seg = (uint64_t)g.nbuckets * g.nwg * 6;
    g.dense = (na * s->k / per_seg) < (uint64_t)g_part_dense_groups ? 1u : 0u;
    const size_t lds = (size_t)1 << (g.shift - 1);
    unsigned long long *sat = (unsigned long long *)(s->ctr + PSK_CTR_SATURATED);
    const uint32_t direct = na * s->k >= s->m / 8 ? 0u : 1u;
    PSK_TRY(set_dyn_lds(k_nib_apply<0>, lds));
    hipLaunchKernelGGL(k_nib_apply<0>, dim3(g.nbuckets), dim3(kApplyThreads), lds, st, (uint32_t *)s->table, s->m, g, (const uint32_t *)s->scat.add.cnt.p,
                       (const uint4 *)s->scat.add.part.p, sat, direct);
    HIP_TRY(hipGetLastError());
    return scat_zero(s, st);
}

// Hand a unit-weight batch of adds over as scattered probes.  cap: keys the list holds; *done = false: not eligible (nothing was launched / changed).
static int scat_append(psk_sketch *s, const Batch &b, uint64_t cap, hipStream_t st, bool *done)
{
    *done = false;
    {   // a list must stay within what one fold's 4-bit deltas hold (nib_load_ok): ~2.5 probes per counter
        const uint64_t by_table = s->m * 5 / (2 * (uint64_t)(s->k ? s->k : 1));
        if (cap > by_table) cap = by_table;
    }
    if (s->kind != PSK_KIND_CBF || g_update_nibble == 0 || b.n == 0 || b.n > cap || s->k > 32) return PSK_OK;
    if (b.layout == PSK_KEYS_HASHES && b.key_len < s->k) return PSK_OK;
    if (!s->scat.ready || s->scat.cap != cap) {
        PartGeom g;
        if (!scat_geometry(s, cap, &g)) return PSK_OK;
        PSK_TRY(scat_flush(s, st));  // (a list sized for another capacity)
        s->scat.g = g;
        s->scat.cap = cap;
        s->scat.ready = true;
    }
    psk_sketch::ScatList &l = s->scat.add;
    if (l.n + b.n > cap) PSK_TRY(flush_combined(s, st));
    const PartGeom &g = s->scat.g;
    const uint64_t part_bytes = (uint64_t)g.nbuckets * g.nwg * g.segcap * 16 + 256, cnt_bytes = (uint64_t)g.nbuckets * g.nwg * 4 + 128;
    if (l.part.cap < part_bytes || l.cnt.cap < cnt_bytes) {  // first use (or released): allocate, counts start at zero
        if (s->eff[HO_SCRATCH_BUDGET] > 0 && (int64_t)(part_bytes + cnt_bytes) > s->eff[HO_SCRATCH_BUDGET]) return PSK_OK;  // (not taken: the direct path serves)
        if (ensure(l.part, part_bytes) != PSK_OK || ensure(l.cnt, cnt_bytes) != PSK_OK) return PSK_OK;    // out of memory costs the shortcut, not the add
        HIP_TRY(hipMemsetAsync(l.cnt.p, 0, cnt_bytes, st));
        l.n = 0;
    }
    PSK_TRY(comb_order(s, st));  // (appends are ordered among themselves too: two streams must not race on the cursors)
    bool appended = false;
    PSK_TRY(cbf_scat_append(s, b, st, &appended));
    if (!appended) return PSK_OK;  // layout without a partitioned instantiation
    l.n += b.n;
    PSK_TRY(comb_appended(s, st));
    *done = true;
    return PSK_OK;
}

// the borrowed batches of one list: their pointer / prefix tables go to the device, then ONE pass 1 over all of them + one fold
static int borrowed_flush(psk_sketch *s, psk_sketch::BorrowList &bl, bool remove, hipStream_t st)
{
    const uint64_t n = bl.n();
    if (n == 0) return PSK_OK;
    const uint32_t nb = (uint32_t)bl.base.size();
    PSK_TRY(ensure(s->s_brw, (uint64_t)(2 * nb + 2) * 8));
    const void **base_dev = (const void **)s->s_brw.p;
    uint64_t *start_dev = (uint64_t *)s->s_brw.p + nb;
    HIP_TRY(hipMemcpyAsync(base_dev, bl.base.data(), (size_t)nb * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(start_dev, bl.start.data(), (size_t)(nb + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // (the host vectors are reused from here on; a flush is milliseconds of device work anyway)
    std::vector<const void *> bases;
    std::vector<uint64_t> starts;
    bases.swap(bl.base);   // (cleared first: a failure must not re-apply the list on the next call)
    starts.swap(bl.start);
    bl.clear();
    PSK_TRY(account_weights(s, (const uint32_t *)nullptr, n, remove ? PSK_CTR_REMOVED : PSK_CTR_ADDED, (long long)s->k, st, !remove));
    bool done = false;
    PSK_TRY(cbf_unit_multi_partitioned(s, (const void *const *)base_dev, start_dev, nb, n, remove ? 1 : 0, st, &done));
    if (done) return PSK_OK;
    for (uint32_t j = 0; j < nb; ++j) {  // table not eligible after all (option changed meanwhile): batch by batch through the general path
        const Batch b{PSK_KEYS_FIXED, bases[j], nullptr, starts[j + 1] - starts[j], 16};
        PSK_TRY(cbf_apply_direct(s, b, nullptr, remove, st));
    }
    return PSK_OK;
}

// ---- update windows (psk_window.hpp): small unit-weight add / remove batches of 16-byte keys into big tables wait, in arrival order,
// as key copies; win_flush applies them in one pass over the table, proving the removes while it folds -- or replays them one by one
constexpr size_t kWinMaxBatches = 4096;

static uint64_t win_capacity(const psk_sketch *s)
{
    uint64_t cap = s->m / 2;  // (BASELINE cfg 4's whole 74.5 M-operation step is one window of the 2^28-counter table)
    if (cap < (1u << 20)) cap = 1u << 20;
    if (s->eff[HO_WINDOW_KEYS] > 0 && cap > (uint64_t)s->eff[HO_WINDOW_KEYS]) cap = (uint64_t)s->eff[HO_WINDOW_KEYS];
    cap = cap_round_by_budget(s, cap, 16.0 + (double)s->k * (16.0 / 6.0) * 1.5);  // key copy + probe groups with their padding
    return cap;
}

static bool win_eligible(const psk_sketch *s, int layout, const void *data, uint32_t key_len, const uint32_t *weights, uint64_t n)
{
    PartGeom g;
    return s->kind == PSK_KIND_CBF && s->eff[HO_WINDOW] != 0 && g_update_nibble != 0 && !weights && layout == PSK_KEYS_FIXED && key_len == 16 && data && n != 0 &&
           (int64_t)n >= s->eff[HO_PART_MIN_KEYS] && n * (uint64_t)s->k < s->m / 8 && s->k <= 32 && n <= win_capacity(s) && nib_geometry(s->m, true, &g);
}

static int cbf_remove_device(psk_sketch *s, const Batch &b, const uint32_t *w, hipStream_t st);

// every waiting batch through the per-batch paths, in arrival order (windows too small for a pass over the table, tables / options that
// rule the fold out, and the windows whose proof failed)
static int win_replay(psk_sketch *s, const void *keys, const std::vector<psk_sketch::WinBatch> &batches, hipStream_t st)
{
    __atomic_add_fetch(&g_window_replays, 1, __ATOMIC_RELAXED);
    for (const auto &wb : batches) {
        const Batch b{PSK_KEYS_FIXED, wb.ext ? wb.ext : (const void *)((const uint8_t *)keys + wb.start * 16), nullptr, wb.n, 16};
        if (wb.remove) PSK_TRY(cbf_remove_device(s, b, nullptr, st));
        else PSK_TRY(cbf_apply_device(s, b, nullptr, false, st));
    }
    return PSK_OK;
}

static int win_flush(psk_sketch *s, hipStream_t st)
{
    if (s->win.n == 0) return PSK_OK;
    PSK_TRY(comb_order(s, st));
    std::vector<psk_sketch::WinBatch> batches;
    batches.swap(s->win.batches);  // (cleared first: a failure must not re-apply the window on the next call)
    const uint64_t n = s->win.n;
    s->win.n = 0;
    s->win.copied = 0;
    const void *keys = s->win.keys.p;
    // runs of same-type batches are the fold's phases
    std::vector<WinBatchHost> wbh;
    wbh.reserve(batches.size());
    uint64_t n_add = 0, n_rem = 0;
    size_t phases = 0;
    bool borrowed = false;
    for (const auto &wb : batches) {
        phases += wbh.empty() || wbh.back().remove != wb.remove;
        wbh.push_back(WinBatchHost{wb.ext ? wb.ext : (const void *)((const uint8_t *)keys + wb.start * 16), wb.n, wb.remove});
        borrowed = borrowed || wb.ext != nullptr;
        (wb.remove ? n_rem : n_add) += wb.n;
    }
    // One phase of keys that lie end to end (copies in the list, or one borrowed batch): a plain batch (the partitioned add / the validated
    // remove take it as a whole).  Too few probes for a pass over the table, or a recent window whose proof failed: batch by batch.
    if (phases == 1 && (!borrowed || batches.size() == 1)) {
        const Batch b{PSK_KEYS_FIXED, wbh[0].keys, nullptr, n, 16};
        return wbh[0].remove ? cbf_remove_device(s, b, nullptr, st) : cbf_apply_device(s, b, nullptr, false, st);
    }
    const bool worth = n * (uint64_t)s->k >= s->m / 8 && phases <= (size_t)kWinMaxPhases;
    if (worth && s->win.backoff == 0) {
        bool launched = false, ok = false;
        PSK_TRY(cbf_window_fold(s, wbh.data(), (uint32_t)wbh.size(), st, &launched, &ok));
        if (launched && ok) {
            __atomic_add_fetch(&g_window_folds, 1, __ATOMIC_RELAXED);
            PSK_TRY(account_weights(s, (const uint32_t *)nullptr, n_add, PSK_CTR_ADDED, (long long)s->k, st, true));
            return account_weights(s, (const uint32_t *)nullptr, n_rem, PSK_CTR_REMOVED, (long long)s->k, st, false);
        }
        if (launched) s->win.backoff = 8;  // this stream removes keys that are not there: stop paying for fold + undo for a while
    } else if (s->win.backoff) {
        --s->win.backoff;
    }
    return win_replay(s, keys, batches, st);
}

// Room for `want` keys in the window's key list (16 bytes each).  The list grows in steps -- 2^22 keys (64 MiB) first, then doubling up to
// the window's capacity, the waiting keys copied over -- instead of cap x 16 bytes (2 GiB for a 2^28-counter table) on the first small
// batch.  *ok = false: the memory is not there (the HIP error is cleared): the caller takes the paths that need no list.
static int win_reserve(psk_sketch *s, uint64_t want, uint64_t cap, hipStream_t st, bool *ok)
{
    *ok = true;
    if (want * 16 <= s->win.keys.cap) return PSK_OK;
    uint64_t keys = s->win.keys.cap / 16 ? s->win.keys.cap / 16 : (1ULL << 22);
    while (keys < want) keys *= 2;
    if (keys > cap) keys = cap;
    void *p = nullptr;
    if (hipMalloc(&p, keys * 16) != hipSuccess) {
        (void)hipGetLastError();
        *ok = false;
        return PSK_OK;
    }
    if (s->win.copied) {
        // (the new list is ours until it is stored below: every failure on the way frees it)
        auto moved = [&]() -> int {
            PSK_TRY(comb_order(s, st));
            HIP_TRY(hipMemcpyAsync(p, s->win.keys.p, s->win.copied * 16, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));  // (the old list is freed below)
            return PSK_OK;
        };
        const int rc = moved();
        if (rc != PSK_OK) {
            (void)hipFree(p);
            return rc;
        }
    }
    if (s->win.keys.p) {
        const hipError_t e = hipFree(s->win.keys.p);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return fail(PSK_EHIP, "hipFree of the window's key list failed: %s", hipGetErrorString(e));
        }
    }
    s->win.keys.p = p;
    s->win.keys.cap = keys * 16;
    return PSK_OK;
}

// hand a batch over to the window (eligible: win_eligible); host batches are copied straight from the caller's buffer, PSK_DEVICE batches
// device to device, PSK_DEVICE_BORROWED ones stay where they are (the caller keeps them unchanged until the window has been applied:
// psk_flush_combined, any entry point that reads the table, or psk_sketch_get_option "window_pending_batches" back at 0).
// *taken = false: no memory for the key list -- nothing was appended, what waited has been applied, the caller applies this batch itself.
static int win_append(psk_sketch *s, const void *data, uint64_t n, bool remove, int where, hipStream_t st, bool *taken)
{
    *taken = true;
    const uint64_t cap = win_capacity(s);
    if (s->win.cap != cap && s->win.n) PSK_TRY(win_flush(s, st));
    if (s->win.n + n > cap || s->win.batches.size() >= kWinMaxBatches) PSK_TRY(win_flush(s, st));
    if (s->win.n && !s->win.batches.empty() && s->win.batches.back().remove != (remove ? 1u : 0u)) {
        size_t phases = 1;  // (a new phase: the fold holds at most kWinMaxPhases of them)
        for (size_t i = 1; i < s->win.batches.size(); ++i) phases += s->win.batches[i].remove != s->win.batches[i - 1].remove;
        if (phases >= (size_t)kWinMaxPhases) PSK_TRY(win_flush(s, st));
    }
    s->win.cap = cap;
    if (where == PSK_DEVICE_BORROWED) {  // (16-byte aligned: win_eligible's caller checked)
        s->win.batches.push_back(psk_sketch::WinBatch{0, n, remove ? 1u : 0u, data});
        s->win.n += n;
        return comb_appended(s, st);  // (a flush on another stream waits for this one: the keys may still be in the making on it)
    }
    bool room = false;
    PSK_TRY(win_reserve(s, s->win.copied + n, cap, st, &room));
    if (!room && s->win.n) {  // what waits fits what there is: apply it, then this batch may fit too
        PSK_TRY(win_flush(s, st));
        room = n * 16 <= s->win.keys.cap;
    }
    if (!room) {
        *taken = false;
        return PSK_OK;
    }
    PSK_TRY(comb_order(s, st));
    // (round 4: an own copy kernel with nontemporal loads / stores measured slower than the runtime's blit: 3.60 vs 3.55 ms per cfg-4 step)
    HIP_TRY(hipMemcpyAsync((uint8_t *)s->win.keys.p + s->win.copied * 16, data, n * 16, where == PSK_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    s->win.batches.push_back(psk_sketch::WinBatch{s->win.copied, n, remove ? 1u : 0u, nullptr});
    s->win.copied += n;
    s->win.n += n;
    PSK_TRY(comb_appended(s, st));
    if (where == PSK_HOST) HIP_TRY(hipStreamSynchronize(st));  // the caller may reuse its buffer on return
    return PSK_OK;
}

int flush_combined(psk_sketch *s, hipStream_t st)
{
    PSK_TRY(clear_materialize(s, st));  // (every caller is about to read the table or the counters, or to hand them out)
    if (s->kind != PSK_KIND_CBF) return PSK_OK;
    if (s->win.n) {  // (the window holds what arrived AFTER anything the older mechanisms below hold: see win_append's callers)
        ++s->table_version;
        if (older_updates_pending(s)) {
            std::vector<psk_sketch::WinBatch> keep;
            keep.swap(s->win.batches);
            const uint64_t wn = s->win.n, wc = s->win.copied;
            s->win.n = 0;
            PSK_TRY(flush_combined(s, st));
            s->win.batches.swap(keep);
            s->win.n = wn;
            s->win.copied = wc;
        }
        PSK_TRY(win_flush(s, st));
    }
    if (!older_updates_pending(s)) return PSK_OK;
    ++s->table_version;  // (also from the read-only entry points: what waited reaches the table now)
    PSK_TRY(comb_order(s, st));
    // adds first: a remove whose add waits in the same window must find it applied.  Two mechanisms may hold updates -- key lists
    // (weighted batches, tables below the nibble geometry; adds and removes) and scattered probes (adds only): all adds of both, then the removes.
    auto key_list = [&](int pass) {
        psk_sketch::PendList &l = pass == 0 ? s->comb.add : s->comb.rem;
        if (l.n == 0) return (int)PSK_OK;
        Batch b{PSK_KEYS_FIXED, l.keys.p, nullptr, l.n, s->comb.key_len};
        l.n = 0;  // (cleared first: a failure must not re-apply the list on the next call)
        const bool unit = l.unit;
        l.unit = true;
        return cbf_apply_device(s, b, unit ? nullptr : (const uint32_t *)l.w.p, pass == 1, st);
    };
    PSK_TRY(key_list(0));
    PSK_TRY(borrowed_flush(s, s->comb.badd, false, st));
    if (s->comb.rem.n != 0 || s->comb.brem.n() != 0) PSK_TRY(scat_flush(s, st));  // key-list removes wait: the scattered adds must land before them
    PSK_TRY(key_list(1));
    PSK_TRY(borrowed_flush(s, s->comb.brem, true, st));
    return scat_flush(s, st);
}

extern "C" int psk_flush(psk_sketch *s, void *stream)
{
    CHECK_HANDLE_RO(s, -1);
    return flush_combined(s, (hipStream_t)stream);
}

extern "C" int psk_cbf_update_combined(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                                       uint32_t key_len, const uint32_t *weights, int remove, int where, void *stream)
{
    CHECK_HANDLE(s, PSK_KIND_CBF);
    PSK_TRY(check_hashes_width(s, layout, key_len));
    if (where != PSK_HOST && where != PSK_DEVICE && where != PSK_DEVICE_BORROWED) return fail(PSK_EINVAL, "`where` must be PSK_HOST, PSK_DEVICE or PSK_DEVICE_BORROWED");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return PSK_OK;
    // Batches that wait in the update window (psk_cbf_add / psk_cbf_remove on this handle) arrived EARLIER than this one: they reach the
    // table first.  (flush_combined applies the lists below before the window: the window may only ever hold what came after them.)
    if (s->win.n) PSK_TRY(flush_combined(s, st));
    const uint64_t cap = g_combine_keys > 0 ? (uint64_t)g_combine_keys : 0;
    if (where == PSK_DEVICE_BORROWED) {
        // 16-byte unit-weight keys into a table with the nibble geometry: remember WHERE they are, nothing else.  The flush hashes all
        // borrowed batches of a list in one pass 1 where they lie (KeysFixed16Multi): no copy into a list, the keys are read once.
        PartGeom probe;
        const bool borrowable = layout == PSK_KEYS_FIXED && key_len == 16 && data && ((uintptr_t)data & 15) == 0 && !weights && cap && n <= cap &&
                                g_update_nibble != 0 && s->k <= 32 && scat_geometry(s, cap, &probe);
        if (borrowable) {
            psk_sketch::BorrowList &bl = remove ? s->comb.brem : s->comb.badd;
            const uint64_t by_table = s->m * 5 / (2 * (uint64_t)s->k);  // (what one fold's 4-bit deltas hold: nib_load_ok)
            const uint64_t capb = cap < by_table ? cap : by_table;
            if (bl.n() + n > capb || bl.base.size() >= 4096) PSK_TRY(flush_combined(s, st));
            bl.base.push_back(data);
            bl.start.push_back(bl.start.back() + n);
            return comb_appended(s, st);  // (a flush on another stream waits for this one: the keys may still be in the making on it)
        }
        where = PSK_DEVICE;  // anything else is copied as usual
    }
    const bool combinable = layout == PSK_KEYS_FIXED && key_len > 0 && data && n < cap;
    if (!combinable || (s->comb.key_len && s->comb.key_len != key_len) || (s->comb.cap && s->comb.cap != cap)) {
        PSK_TRY(flush_combined(s, st));
        if (!combinable) {  // other layouts, empty keys, batches as large as a list: applied at once (same semantics)
            Batch b;
            PSK_TRY(stage_batch(s->s_keys, s->s_offs, layout, data, offsets, n, key_len, where, st, &b));
            const uint32_t *w;
            PSK_TRY(stage_vec(s->s_w, weights, n, where, st, &w));
            PSK_TRY(cbf_apply_device(s, b, w, remove != 0, st));
            return finish(where, nullptr, st);
        }
    }
    psk_sketch::PendList &l = remove ? s->comb.rem : s->comb.add;
    if (l.n + n > cap) PSK_TRY(flush_combined(s, st));
    s->comb.key_len = key_len;
    s->comb.cap = cap;
    PSK_TRY(ensure(l.keys, cap * (uint64_t)key_len));  // full capacity at once: growing would drop the pending keys
    if (weights || !l.unit) PSK_TRY(ensure(l.w, cap * 4));  // the weight list only once a non-unit batch has arrived
    PSK_TRY(comb_order(s, st));
    const hipMemcpyKind kind = where == PSK_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    HIP_TRY(hipMemcpyAsync((uint8_t *)l.keys.p + l.n * (uint64_t)key_len, data, n * (uint64_t)key_len, kind, st));
    uint32_t *wdst = (uint32_t *)l.w.p + l.n;
    if (weights) {
        if (l.unit && l.n) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)l.w.p, 1, l.n, st));  // earlier unit batches get their 1s now
        HIP_TRY(hipMemcpyAsync(wdst, weights, n * 4, kind, st));
        l.unit = false;
    } else if (!l.unit) {
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)wdst, 1, n, st));
    }
    l.n += n;
    PSK_TRY(comb_appended(s, st));
    if (where == PSK_HOST) HIP_TRY(hipStreamSynchronize(st));  // the caller may reuse its buffers on return
    return PSK_OK;
}

extern "C" int psk_cbf_add(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                           uint32_t key_len, const uint32_t *weights, int where, void *stream)
{
    CHECK_HANDLE(s, PSK_KIND_CBF);
    PSK_TRY(check_hashes_width(s, layout, key_len));
    hipStream_t st = (hipStream_t)stream;
    if (where != PSK_HOST && where != PSK_DEVICE && where != PSK_DEVICE_BORROWED) return fail(PSK_EINVAL, "`where` must be PSK_HOST, PSK_DEVICE or PSK_DEVICE_BORROWED");
    if (win_eligible(s, layout, data, key_len, weights, n)) {
        // (what the older write-combining mechanisms hold arrived earlier: it goes first)
        if (older_updates_pending(s)) PSK_TRY(flush_combined(s, st));
        bool taken = false;
        PSK_TRY(win_append(s, data, n, false, where == PSK_DEVICE_BORROWED && ((uintptr_t)data & 15) ? PSK_DEVICE : where, st, &taken));
        if (taken) return PSK_OK;  // (else: no memory for the window's key list -- the batch goes on below like any other)
    }
    if (where == PSK_DEVICE_BORROWED) where = PSK_DEVICE;  // (applied before this call returns: nothing is kept)
    Batch b;
    PSK_TRY(stage_batch(s->s_keys, s->s_offs, layout, data, offsets, n, key_len, where, st, &b));
    // Automatic write-combining (no opt-in): a unit-weight batch too small to pay for a pass over a big table would take one
    // fabric atomic per probe.  Adds commute (countingbloom.py:135-155; the clamp at 2^32-1 is applied by the fold just the
    // same), so the batch is scattered now and folded with its successors; every entry point that reads or removes flushes first.
    // (16-byte keys wait in the update window above; the other layouts here.  An append launches min(256, tiles) workgroups and workgroup i
    // always fills segment column i: batches of fewer than 256 tiles would pile the whole list into a few columns, which overflow long before
    // the list is full -- such batches take the direct kernel, as before round 3.)
    if (!weights && s->eff[HO_AUTO_COMBINE] != 0 && s->win.n == 0 && s->comb.rem.n == 0 && s->comb.brem.n() == 0 && (int64_t)n >= s->eff[HO_PART_MIN_KEYS] &&
        n >= (256u * 2048u * 7u) / (s->k ? s->k : 1u) && n * (uint64_t)s->k < s->m / 8 && g_auto_combine_keys > 0) {
        bool taken = false;
        PSK_TRY(scat_append(s, b, (uint64_t)g_auto_combine_keys, st, &taken));
        if (taken) {
            PSK_TRY(account_weights(s, (const uint32_t *)nullptr, n, PSK_CTR_ADDED, (long long)s->k, st, true));
            return finish(where, nullptr, st);
        }
    }
    PSK_TRY(flush_combined(s, st));  // write-combined updates reach the table before anything else touches it
    const uint32_t *w;
    PSK_TRY(stage_vec(s->s_w, weights, n, where, st, &w));
    PSK_TRY(post_acct(s, w, n, PSK_CTR_ADDED, (long long)s->k, st, true, false));
    unsigned long long *sat = (unsigned long long *)(s->ctr + PSK_CTR_SATURATED);
    {
        bool done = false;
        PSK_TRY(cbf_add_partitioned(s, b, w, st, &done));
        PSK_TRY(settle_acct(s, w, n, st));
        if (done) return finish(where, nullptr, st);
    }
    return direct_apply(s, b, data, where, true, nullptr, st, [&](auto P) { return CbfAdd<P.value>{(uint32_t *)s->table, s->md, s->k, w, s->ctr, sat, false}; });
}

// countingbloom.py:198-203 for a whole batch: from the min over the key's counters (a lookup) to the amount actually removed
//   mn == 0 (absent) or mn == 2^32-1 (frozen): nothing;  else to_remove = min(mn, num_els)
// a partial removal (mn < num_els) makes the result depend on the order inside the batch: `dep` is raised
static __global__ __launch_bounds__(kBlock) void k_cbf_to_remove(const uint32_t *mins, const uint32_t *weights, uint64_t n, uint32_t *to_remove, uint32_t *dep)
{
    uint32_t partial = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const uint32_t mn = mins[i], w = weights ? weights[i] : 1u;
        uint32_t tr = 0;
        if (mn != 0 && mn != 0xFFFFFFFFu) {
            tr = mn > w ? w : mn;
            partial |= (uint32_t)(tr != w);
        }
        to_remove[i] = tr;
    }
    if (partial) *dep = 1u;
}

static __global__ void k_widen_u32(const uint32_t *w, uint64_t n, int64_t *out)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (int64_t)w[i];
}

// tmp[1] (sum of the amounts, k_weight_sum's booking slot) -> ctr[PSK_CTR_REMOVED]
static __global__ void k_book_removed(long long *ctr, const long long *tmp)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) ctr[PSK_CTR_REMOVED] += tmp[PSK_CTR_REMOVED];
}

// The validated remove (countingbloom.py:186-208) of a device-resident batch, as a TRANSACTION.  Unordered execution gives the
// reference's table whenever the result does not depend on the order inside the batch; here that is CHECKED and, where it fails, the
// batch is put back and executed in order:
//   0. unit weights into a big table: the optimistic decrement (psk_nibble.hpp) -- every key present: done in one pass over the table;
//   1. mins <- lookup of every key's k counters (the state BEFORE the batch);
//   2. amounts <- min(mn, num_els), 0 for absent / frozen keys; a partial removal (mn < num_els) raises the flag;
//   3. decrement by the amounts, wrapping, flag raised wherever a counter would go below zero or is frozen.  With T[c] >= the batch's
//      total on c for every counter, every key that step 2 found present is still present when its turn comes, whatever the order --
//      and a key found absent stays absent (removes only lower counters): the unordered result IS the sequential one;
//   4. flag up: the same amounts are added back (wrapping: the exact inverse) and the batch runs through k_cbf_ordered, one key after
//      the other -- the reference literally, for any batch (duplicates beyond their count, keys running a shared counter dry ...).
static int cbf_remove_exact(psk_sketch *s, const Batch &b, const uint32_t *w, hipStream_t st)
{
    if (b.n == 0) return PSK_OK;
    const bool big = part_wanted(s, b.n, s->k, 4);
    if (!w && big) {
        // Unit weights into a big table: decrement optimistically (psk_nibble.hpp) -- if every counter holds at least as much as the
        // batch takes from it, every key is removed and one pass 1 + ONE pass over the table did it.  The verdict is one 4-byte
        // read-back.  Otherwise the decrement is undone (exactly: wrapping arithmetic both ways) and the steps below take the batch.
        bool launched = false;
        PSK_TRY(cbf_remove_fast_begin(s, b, st, &launched));
        if (launched) {
            uint32_t flag = 1;
            HIP_TRY(hipMemcpyAsync(&flag, s->s_flag.p, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (flag == 0) return account_weights(s, (const uint32_t *)nullptr, b.n, PSK_CTR_REMOVED, (long long)s->k, st, false);
            PSK_TRY(cbf_remove_fast_undo(s, st));
        }
    }
    // s_aux: mins[n] | amounts[n] | scratch counter block | (ordered replay of a weighted batch: int64 weights[n])
    const uint64_t n4 = (b.n + 3) & ~3ULL;
    PSK_TRY(ensure(s->s_aux, n4 * 8 + 128 + (w ? b.n * 8 : 0)));
    uint32_t *mins = (uint32_t *)s->s_aux.p, *amount = mins + n4;
    long long *tmp = (long long *)(amount + n4);
    bool looked = false;
    if (big) PSK_TRY(cbf_check_partitioned(s, b, s->k, mins, st, &looked));
    if (!looked) {
        PSK_TRY(with_source(b, [&](auto src) {
            return with_pow2(s, [&](auto P) { return launch_apply(src, CbfCheck<P.value>{(const uint32_t *)s->table, s->md, s->k, mins}, b.n, st); });
        }));
    }
    PSK_TRY(ensure(s->s_flag, 8));
    uint32_t *flag = (uint32_t *)s->s_flag.p;
    HIP_TRY(hipMemsetAsync(flag, 0, 4, st));
    hipLaunchKernelGGL(k_cbf_to_remove, dim3(grid_for_keys(b.n) > 1024 ? 1024 : grid_for_keys(b.n)), dim3(kBlock), 0, st, (const uint32_t *)mins, w, b.n, amount, flag);
    HIP_TRY(hipGetLastError());
    // the amounts' sum: into a scratch block (booked once the verdict is in), and as this round's sum |w| for pass 2's wrap check
    HIP_TRY(hipMemsetAsync(tmp, 0, sizeof(long long) * PSK_CTR_COUNT, st));
    hipLaunchKernelGGL((k_weight_sum<uint32_t>), dim3(grid_for_keys(b.n) > 256 ? 256 : grid_for_keys(b.n)), dim3(kBlock), 0, st, (const uint32_t *)amount, b.n, tmp,
                       (int)PSK_CTR_REMOVED, (long long)s->k, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(s->ctr + 6, tmp + 6, sizeof(long long), hipMemcpyDeviceToDevice, st));
    s->acct.pending = false;
    auto decrement = [&](int opt, bool *partitioned) {  // opt 1: checked, 2: inverse.  The same path both times (same batch, same options)
        *partitioned = false;
        if (big) {
            s->acct.weights01 = w == nullptr;  // unit removes: every amount is 0 or 1 (masked unit probes may serve)
            const int rc = cbf_remove_partitioned(s, b, amount, st, partitioned, opt, flag);
            s->acct.weights01 = false;
            PSK_TRY(rc);
        }
        if (*partitioned) return (int)PSK_OK;
        return with_source(b, [&](auto src) {
            return with_pow2(s, [&](auto P) { return launch_apply(src, CbfSubChecked<P.value>{(uint32_t *)s->table, s->md, s->k, amount, flag, opt == 2}, b.n, st); });
        });
    };
    bool part1 = false, part2 = false;
    PSK_TRY(decrement(1, &part1));
    uint32_t verdict = 1;
    HIP_TRY(hipMemcpyAsync(&verdict, flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (verdict == 0) {
        hipLaunchKernelGGL(k_book_removed, dim3(1), dim3(1), 0, st, s->ctr, (const long long *)tmp);
        HIP_TRY(hipGetLastError());
        return PSK_OK;
    }
    PSK_TRY(decrement(2, &part2));
    if (part1 != part2) return fail(PSK_EHIP, "transactional remove: the undo took another path than the decrement");
    __atomic_add_fetch(&g_cbf_ordered_replays, 1, __ATOMIC_RELAXED);
    const int64_t *w64 = nullptr;
    if (w) {
        int64_t *dst = (int64_t *)(tmp + PSK_CTR_COUNT + 2);
        hipLaunchKernelGGL(k_widen_u32, dim3(grid_for_keys(b.n) > 1024 ? 1024 : grid_for_keys(b.n)), dim3(kBlock), 0, st, w, b.n, dst);
        HIP_TRY(hipGetLastError());
        w64 = dst;
    }
    uint64_t *wide = nullptr;  // (k beyond the ordered kernel's register arrays: index / value lists in device scratch)
    if (s->k > (uint32_t)kMaxKOrdered) {
        PSK_TRY(ensure(s->s_out, 16ULL * s->k));
        wide = (uint64_t *)s->s_out.p;
    }
    return with_source(b, [&](auto src) {
        return with_pow2(s, [&](auto P) {
            hipLaunchKernelGGL((k_cbf_ordered<decltype(src), P.value>), dim3(1), dim3(64), 0, st, src, (uint32_t *)s->table, s->md, s->k, w64, (int)PSK_OP_REMOVE, b.n,
                               (uint32_t *)nullptr, (unsigned long long *)s->ctr, wide, (uint32_t *)nullptr, 0u);
            HIP_TRY(hipGetLastError());
            return (int)PSK_OK;
        });
    });
}

// the validated remove (countingbloom.py:186-208) of a device-resident batch: composed from the partitioned pipelines when the batch is
// large enough, else the direct kernel
static int cbf_remove_device(psk_sketch *s, const Batch &b, const uint32_t *w, hipStream_t st)
{
    if (b.n == 0) return PSK_OK;
    if (s->eff[HO_REMOVE_EXACT] != 0) return cbf_remove_exact(s, b, w, st);
    // (option "remove_exact" = 0, bench A/B: the one-kernel form -- per key: read the k counters, decide, subtract; exact for
    // well-formed batches, deviations tallied in PSK_CTR_VIOLATIONS)
    return with_source(b, [&](auto src) {
        return with_pow2(s, [&](auto P) {
            hipLaunchKernelGGL((k_cbf_remove<decltype(src), P.value>), dim3(grid_for_keys(b.n)), dim3(kBlock), 0, st, src, (uint32_t *)s->table, s->md, s->k, w, b.n,
                               (unsigned long long *)s->ctr);
            HIP_TRY(hipGetLastError());
            return (int)PSK_OK;
        });
    });
}

extern "C" int psk_cbf_remove(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                              uint32_t key_len, const uint32_t *weights, int where, void *stream)
{
    CHECK_HANDLE(s, PSK_KIND_CBF);
    PSK_TRY(check_hashes_width(s, layout, key_len));
    hipStream_t st = (hipStream_t)stream;
    if (where != PSK_HOST && where != PSK_DEVICE && where != PSK_DEVICE_BORROWED) return fail(PSK_EINVAL, "`where` must be PSK_HOST, PSK_DEVICE or PSK_DEVICE_BORROWED");
    if (win_eligible(s, layout, data, key_len, weights, n)) {
        // A small batch into a big table: it waits in the update window (with the adds around it, in order) for a shared pass over
        // the table; the flush proves that it would have removed every key at this point of the stream, or replays it right here.
        if (older_updates_pending(s)) PSK_TRY(flush_combined(s, st));
        bool taken = false;
        PSK_TRY(win_append(s, data, n, true, where == PSK_DEVICE_BORROWED && ((uintptr_t)data & 15) ? PSK_DEVICE : where, st, &taken));
        if (taken) return PSK_OK;
    }
    if (where == PSK_DEVICE_BORROWED) where = PSK_DEVICE;
    PSK_TRY(flush_combined(s, st));  // write-combined updates reach the table before anything else touches it
    Batch b;
    PSK_TRY(stage_batch(s->s_keys, s->s_offs, layout, data, offsets, n, key_len, where, st, &b));
    const uint32_t *w;
    PSK_TRY(stage_vec(s->s_w, weights, n, where, st, &w));
    PSK_TRY(cbf_remove_device(s, b, w, st));
    return finish(where, nullptr, st);
}

extern "C" int psk_cbf_check(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                             uint32_t key_len, int where, uint32_t *out, void *stream)
{
    CHECK_HANDLE_RO(s, PSK_KIND_CBF);
    if (n && !out) return fail(PSK_EINVAL, "out is NULL");
    if (layout == PSK_KEYS_HASHES && key_len == 0) return fail(PSK_EINVAL, "check needs at least one hash per key");
    hipStream_t st = (hipStream_t)stream;
    PSK_TRY(flush_combined(s, st));  // write-combined updates reach the table before anything else touches it
    Batch b;
    PSK_TRY(stage_batch(s->s_keys, s->s_offs, layout, data, offsets, n, key_len, where, st, &b));
    OutBuf o;
    PSK_TRY(stage_out(s->s_out, out, n * 4, where, &o));
    // countingbloom.py:174 takes the min over ALL supplied hashes (not just the first k)
    const uint32_t kk = layout == PSK_KEYS_HASHES ? key_len : s->k;
    {
        bool done = false;
        s->shadow.allow = !s->shadow.exposed;  // (only here: a lookup INSIDE an updating entry point is followed by writes at the same table version)
        const int rc = cbf_check_partitioned(s, b, kk, (uint32_t *)o.dev, st, &done);
        s->shadow.allow = false;
        PSK_TRY(rc);
        if (done) return finish(where, &o, st);
    }
    return direct_apply(s, b, data, where, o.is_pinned, &o, st, [&](auto P) { return CbfCheck<P.value>{(const uint32_t *)s->table, s->md, kk, (uint32_t *)o.dev}; });
}

extern "C" int psk_cbf_update_ordered(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                                      uint32_t key_len, const int64_t *weights, int opmode, int where, uint32_t *out,
                                      void *stream)
{
    CHECK_HANDLE(s, PSK_KIND_CBF);
    PSK_TRY(check_hashes_width(s, layout, key_len));
    if (opmode < PSK_OP_ADD || opmode > PSK_OP_SIGNED) return fail(PSK_EINVAL, "bad opmode %d", opmode);
    hipStream_t st = (hipStream_t)stream;
    PSK_TRY(flush_combined(s, st));  // write-combined updates reach the table before anything else touches it
    Batch b;
    PSK_TRY(stage_batch(s->s_keys, s->s_offs, layout, data, offsets, n, key_len, where, st, &b));
    const int64_t *w;
    PSK_TRY(stage_vec(s->s_w, weights, n, where, st, &w));
    OutBuf o;
    PSK_TRY(stage_out(s->s_out, out, out ? n * 4 : 0, where, &o));
    uint64_t *wide = nullptr;  // k beyond the register arrays (fpr below ~1e-20): index / value lists live in device scratch
    if (s->k > (uint32_t)kMaxKOrdered) {
        PSK_TRY(ensure(s->s_aux, 16ULL * s->k));
        wide = (uint64_t *)s->s_aux.p;
    }
    Mailbox mb;
    PSK_TRY(mailbox_arm(s, where, n, out && o.is_pinned, &mb));
    if (mb.word && n == 1 && weights && weights[0] == 1) w = nullptr;  // (a null weight list means 1: no read of the pinned page for `cbf.add(key)`)
    KeysInline64 ik;
    if (n) {
        PSK_TRY(with_source_one(b, inline_key(layout, data, n, key_len, mb, &ik), [&](auto src) {
            return with_pow2(s, [&](auto P) {
                hipLaunchKernelGGL((k_cbf_ordered<decltype(src), P.value>), dim3(1), dim3(64), 0, st, src, (uint32_t *)s->table, s->md,
                                   s->k, w, opmode, n, (uint32_t *)(out ? o.dev : nullptr), (unsigned long long *)s->ctr, wide, mb.dev(), mb.seq);
                HIP_TRY(hipGetLastError());
                return (int)PSK_OK;
            });
        }));
    }
    return finish(where, &o, st, &mb);
}

// countingbloom.py:135-208 for a whole ordered batch: the table, the handle's counters and EVERY op's return value as the one-lane loop
// (k_cbf_ordered, PSK_OP_SIGNED) leaves them.  The optimistic parallel passes of psk_cbf_running.hpp chunk by chunk wherever they apply
// (k <= kMaxKOrdered, m <= 2^32); a chunk whose verification raised its flag has changed nothing and is replayed in order on one lane
// before the next chunk starts.  Anything else: the one-lane kernel for the whole call.  Read-only options "cbf_running_fast_chunks" /
// "cbf_running_replayed_chunks" / "cbf_running_sequential" count the chunks either way and the calls that were not eligible.
// ADDONLY: psk_cbf_add_running (weights >= 0 is the entry's contract).
template <bool ADDONLY>
static int cbf_running(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len, const int32_t *weights, int where,
                       uint32_t *out, void *stream)
{
    CHECK_HANDLE(s, PSK_KIND_CBF);
    PSK_TRY(check_hashes_width(s, layout, key_len));
    if (where != PSK_HOST && where != PSK_DEVICE) return fail(PSK_EINVAL, "`where` must be PSK_HOST or PSK_DEVICE");
    if (n && !out) return fail(PSK_EINVAL, "out is NULL");
    if (ADDONLY && where == PSK_HOST && weights)
        for (uint64_t i = 0; i < n; ++i)
            if (weights[i] < 0) return fail(PSK_EINVAL, "ordered add: weight %d of op %llu is negative", weights[i], (unsigned long long)i);
    hipStream_t st = (hipStream_t)stream;
    Batch b;
    if (n == 0) return stage_batch(s->s_keys, s->s_offs, layout, data, offsets, n, key_len, where, st, &b);  // (validated; nothing runs)
    PSK_TRY(flush_combined(s, st));  // write-combined and windowed updates reach the table before anything else touches it
    PSK_TRY(stage_batch(s->s_keys, s->s_offs, layout, data, offsets, n, key_len, where, st, &b));
    const int32_t *w;
    PSK_TRY(stage_vec(s->s_w, weights, n, where, st, &w));
    OutBuf o;
    PSK_TRY(stage_out(s->s_out, out, n * 4, where, &o));
    if (s->k >= 1 && s->k <= (uint32_t)kMaxKOrdered && s->m <= (1ULL << 32)) {
        CbfRunArena a;
        PSK_TRY(cbf_running_arena(s, n, &a));
        for (uint64_t base = 0; base < n; base += a.l.cap) {
            const uint32_t nc = (uint32_t)(n - base < a.l.cap ? n - base : a.l.cap);
            PSK_TRY(with_source(b, [&](auto src) {
                return with_pow2(s, [&](auto P) {
                    hipLaunchKernelGGL((k_cbfr_hash<decltype(src), P.value>), dim3(grid_for_keys(nc)), dim3(kBlock), 0, st, src, s->md, s->k, base, nc, a.bins);
                    HIP_TRY(hipGetLastError());
                    return (int)PSK_OK;
                });
            }));
            bool clean = false;
            PSK_TRY(cbf_running_chunk(s, a, w, base, nc, ADDONLY, (uint32_t *)o.dev, st, &clean));
            __atomic_add_fetch(clean ? &g_cbf_running_fast_chunks : &g_cbf_running_replayed_chunks, 1, __ATOMIC_RELAXED);
            if (clean) continue;
            PSK_TRY(with_source(b, [&](auto src) {
                return with_pow2(s, [&](auto P) {
                    hipLaunchKernelGGL((k_cbfr_replay<decltype(src), P.value, ADDONLY>), dim3(1), dim3(64), 0, st, src, (uint32_t *)s->table, s->md, s->k, w, base, nc,
                                       (uint32_t *)o.dev, (unsigned long long *)s->ctr);
                    HIP_TRY(hipGetLastError());
                    return (int)PSK_OK;
                });
            }));
        }
    } else {  // one lane, one op after the other (int64 weights: widened in front of it)
        __atomic_add_fetch(&g_cbf_running_sequential, 1, __ATOMIC_RELAXED);
        uint64_t *wide = nullptr;
        if (s->k > (uint32_t)kMaxKOrdered) {
            PSK_TRY(ensure(s->s_aux, 16ULL * s->k));
            wide = (uint64_t *)s->s_aux.p;
        }
        const int64_t *w64 = nullptr;
        if (w) {
            PSK_TRY(ensure(s->s_vals, 8 * n));
            hipLaunchKernelGGL((k_cbfr_widen<ADDONLY>), dim3(grid_for_keys(n)), dim3(kBlock), 0, st, w, n, (int64_t *)s->s_vals.p, (unsigned long long *)s->ctr);
            HIP_TRY(hipGetLastError());
            w64 = (const int64_t *)s->s_vals.p;
        }
        PSK_TRY(with_source(b, [&](auto src) {
            return with_pow2(s, [&](auto P) {
                hipLaunchKernelGGL((k_cbf_ordered<decltype(src), P.value>), dim3(1), dim3(64), 0, st, src, (uint32_t *)s->table, s->md, s->k, w64,
                                   (int)(ADDONLY ? PSK_OP_ADD : PSK_OP_SIGNED), n, (uint32_t *)o.dev, (unsigned long long *)s->ctr, wide, (uint32_t *)nullptr, 0u);
                HIP_TRY(hipGetLastError());
                return (int)PSK_OK;
            });
        }));
    }
    return finish(where, &o, st);
}

extern "C" int psk_cbf_add_running(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len,
                                   const int32_t *weights, int where, uint32_t *out, void *stream)
{
    return cbf_running<true>(s, layout, data, offsets, n, key_len, weights, where, out, stream);
}

extern "C" int psk_cbf_update_running(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len,
                                      const int32_t *weights, int where, uint32_t *out, void *stream)
{
    return cbf_running<false>(s, layout, data, offsets, n, key_len, weights, where, out, stream);
}
