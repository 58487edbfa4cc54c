// psk_cbf_running.hpp -- exact ORDERED CountingBloomFilter batches with every op's return value, in parallel (psk_cbf_add_running,
// psk_cbf_update_running).  The definition of exact is the one-lane loop cbf_ordered_loop (psk_device.hpp), i.e. countingbloom.py:135-208.
//
// What an op does to ONE counter, as a map on the counter's value x (MAX = 2^32 - 1 is sticky):
//     add w                  x -> min(x + w, MAX)
//     FULL remove of w       x -> (x == MAX ? MAX : x - w)            (a remove that found its key with at least w)
// Both are instances of (a, p): a = the signed sum, p = the largest prefix sum that ends in an add (none: -inf),
//     (a, p)(x) = (x == MAX || x + p >= MAX) ? MAX : x + a                 add = (w, w)     remove = (-w, -inf)
//     (a1, p1) then (a2, p2) = (a1 + a2, max(p1, a1 + p2))                 associative
// so the value of a counter in front of op i is a segmented EXCLUSIVE scan of maps, in arrival order per counter, applied to the table.
// A chunk has at most ~2^23 probes of |w| <= 2^31: int64 holds a and p without saturation (-inf is -2^61; it may drift by 2^54).
//
// A remove is data dependent (to_remove = min(min_val, num_els); absent keys are no-ops), so the scan is OPTIMISTIC: it is the loop's result
// only if every remove is full.  The per-op pass checks that with the values the scan produced, and k_cbfr_apply checks the ops that hit one
// counter more than once; by induction over the ops a chunk without a flag has behaved exactly as the loop.  The verdict is one word read
// back per chunk: no flag -> the commit pass stores the counters and the tallies are booked; flag -> neither has happened (the table is
// untouched: every pass before the commit only reads it) and the chunk is replayed by cbf_ordered_loop on one lane.
//
// Passes over one chunk of n ops, E = n * k probes, probe e = i * k + s (op-major: e is arrival order, op = e / k):
//   k_cbfr_hash        bins[e] = h_s(key_i) % m
//   segscan_sort       (psk_segscan.hpp) stable LSD radix sort of (bin, e): ONE row of E elements, ceil(lg m / 8) passes
//   k_cbfr_reduce / k_seg_carry / k_cbfr_apply   segmented scan of maps, reduce-then-scan with a single-workgroup second level; _apply stores
//                      the counter's value in front of the OP at before[e] and the value behind a counter's last probe at fin[j]
//   k_cbfr_perop       per op: its k before-values -> out[i], the verification flag, the chunk's tallies
//   k_cbfr_commit      the last element of every segment stores fin[j] into the table          (only after a clean verdict)
//   k_cbfr_book        the chunk's tallies -> the handle's counters
//   k_cbfr_replay      ops [base, base + n) through cbf_ordered_loop                           (only after a flag)
#pragma once
#include "psk_running.hpp"

namespace psk {

constexpr long long kCbfNoAdd = -(1LL << 61);
constexpr uint32_t kCbfMax = 0xFFFFFFFFu;

// One stretch of the sorted run as a map (the contract of a scan value: psk_segscan.hpp)
struct CbfMap {
    long long a, p;
    uint32_t head;
    static __host__ __device__ __forceinline__ CbfMap identity() { return CbfMap{0, kCbfNoAdd, 0u}; }
    // an op of signed weight w that probes the counter c times (c > 1: only exact for the ops k_cbfr_apply does not flag)
    static __host__ __device__ __forceinline__ CbfMap of(int32_t w, uint32_t c, bool head)
    {
        const long long a = (long long)w * (long long)c;
        return CbfMap{a, w >= 0 ? a : kCbfNoAdd, head ? 1u : 0u};
    }
    __host__ __device__ __forceinline__ uint32_t operator()(uint32_t x) const
    {
        return (x == kCbfMax || (long long)x + p >= (long long)kCbfMax) ? kCbfMax : (uint32_t)((long long)x + a);
    }
    // b follows a
    static __host__ __device__ __forceinline__ CbfMap combine(const CbfMap &a, const CbfMap &b)
    {
        if (b.head) return CbfMap{b.a, b.p, 1u};
        const long long q = a.a + b.p;
        return CbfMap{a.a + b.a, a.p > q ? a.p : q, a.head};
    }
};
__device__ __forceinline__ CbfMap seg_shfl_up(const CbfMap &x, int o) { return CbfMap{__shfl_up(x.a, o), __shfl_up(x.p, o), (uint32_t)__shfl_up((int)x.head, o)}; }

// the signed weight of op i of the batch (nullptr: +1).  ADDONLY (psk_cbf_add_running): a negative weight can only come from a device batch
// (the host entry refuses it before anything runs); it counts as 0 and k_cbfr_perop tallies it as a contract violation.
template <bool ADDONLY>
__device__ __forceinline__ int32_t cbfr_weight(const int32_t *w, uint64_t i)
{
    if (!w) return 1;
    const int32_t x = w[i];
    return ADDONLY && x < 0 ? 0 : x;
}

// ------------------------------------------------------------------ hash
// bins[i * k + s] = h_s(key_{base + i}) % m for the n ops of the chunk (m <= 2^32)
template <class Src, bool POW2>
__global__ __launch_bounds__(kBlock) void k_cbfr_hash(Src src, Mod md, uint32_t k, uint64_t base, uint32_t n, uint32_t *bins)
{
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const typename Src::Key key = src.load(base + i);
        for_each_hash(src, key, base + i, k, [&](uint32_t s, uint64_t h) { bins[(size_t)i * k + s] = (uint32_t)reduce<POW2>(md, h); });
    }
}

// ------------------------------------------------------------------ segmented scan of maps along the sorted run
// Probes of ONE op on ONE counter lie next to each other (the sort is stable, an op's probes are consecutive in arrival order).  The first
// of such a group carries the op's map for all `cnt` of them, the others the identity: every probe of the group is then preceded by exactly
// the ops in front of its own.
struct CbfElem {
    uint32_t bin, e, cnt;  // cnt: probes of the group (its first element), 0 for the others
    int32_t w;
    bool valid, head;
};
template <bool ADDONLY>
__device__ __forceinline__ CbfElem cbfr_load(const uint2 *sorted, const int32_t *w, uint64_t base, uint32_t n, uint32_t k)
{
    const uint32_t j = blockIdx.x * kRunSegBlock + threadIdx.x;
    CbfElem x{0u, 0u, 0u, 0, j < n, true};
    if (x.valid) {
        const uint2 p = sorted[j];
        const uint32_t op = p.y / k;
        x.bin = p.x;
        x.e = p.y;
        bool first = true;
        if (j != 0) {
            const uint2 q = sorted[j - 1];
            x.head = q.x != p.x;
            first = x.head || q.y / k != op;
        }
        x.w = cbfr_weight<ADDONLY>(w, base + op);
        if (first) {
            x.cnt = 1;
            for (uint32_t t = j + 1; t < n; ++t) {  // (at most k - 1 steps)
                const uint2 q = sorted[t];
                if (q.x != p.x || q.y / k != op) break;
                ++x.cnt;
            }
        }
    }
    return x;
}
__device__ __forceinline__ CbfMap cbfr_map(const CbfElem &x)
{
    if (!x.valid) return CbfMap{0, kCbfNoAdd, 1u};  // past the end: an identity segment of its own
    return x.cnt ? CbfMap::of(x.w, x.cnt, x.head) : CbfMap::identity();
}

// agg[block] = the block as one map
template <bool ADDONLY>
__global__ __launch_bounds__(kRunSegBlock) void k_cbfr_reduce(const uint2 *sorted, const int32_t *w, uint64_t base, uint32_t n, uint32_t k, CbfMap *agg)
{
    __shared__ CbfMap wtot[kRunSegBlock / 64];
    const CbfElem x = cbfr_load<ADDONLY>(sorted, w, base, n, k);
    const CbfMap incl = block_scan<kRunSegBlock>(cbfr_map(x), wtot);
    if (threadIdx.x == kRunSegBlock - 1) agg[blockIdx.x] = incl;
}

// before[e] = the counter's value in front of the op of probe e (the first probe of a group stores it for the whole group);
// fin[j] = the counter's value behind element j, for the last element of every segment.  An op that probes a counter c > 1 times and that
// the loop would not treat as c independent steps raises *flag:
//   a remove on a counter below MAX that holds less than c * w (the loop's decrements wrap);
//   an add that crosses the rail BETWEEN its probes, before + w <= MAX < before + c * w (the loop wraps, the scan clamps).
template <bool ADDONLY>
__global__ __launch_bounds__(kRunSegBlock) void k_cbfr_apply(const uint2 *sorted, const int32_t *w, uint64_t base, uint32_t n, uint32_t k, const CbfMap *carry,
                                                             const uint32_t *table, uint32_t *before, uint32_t *fin, uint32_t *flag)
{
    __shared__ CbfMap wtot[kRunSegBlock / 64];
    __shared__ CbfMap incl_s[kRunSegBlock];
    const CbfElem x = cbfr_load<ADDONLY>(sorted, w, base, n, k);
    const CbfMap front = carry[blockIdx.x];
    incl_s[threadIdx.x] = CbfMap::combine(front, block_scan<kRunSegBlock>(cbfr_map(x), wtot));
    __syncthreads();
    if (!x.valid) return;
    const uint32_t j = blockIdx.x * kRunSegBlock + threadIdx.x;
    const uint32_t t0 = table[x.bin];
    if (x.cnt) {
        const CbfMap excl = x.head ? CbfMap::identity() : (threadIdx.x ? incl_s[threadIdx.x - 1] : front);  // the counter's ops in front of this one
        const uint32_t b = excl(t0);
        before[x.e] = b;
        for (uint32_t t = 1; t < x.cnt; ++t) before[sorted[j + t].y] = b;  // (j + t < n: cbfr_load counted them)
        if (x.cnt > 1) {
            const unsigned long long all = (unsigned long long)x.cnt * (unsigned long long)(x.w < 0 ? -(long long)x.w : (long long)x.w);
            const bool bad = x.w < 0 ? (b != kCbfMax && (unsigned long long)b < all)
                                     : ((unsigned long long)b + (unsigned long long)x.w <= kCbfMax && (unsigned long long)b + all > kCbfMax);
            if (bad) *flag = 1u;
        }
    }
    if (j + 1 == n || sorted[j + 1].x != x.bin) fin[j] = incl_s[threadIdx.x](t0);
}

// ------------------------------------------------------------------ per op
// tally: [0] added, [1] removed, [2] negative weights of a device add batch, [3] saturated probes, [4] sum |w|
constexpr int kCbfTallyWords = 8;

// out[base + i], the flag and the tallies from the k before-values of op i (the expressions of cbf_ordered_loop):
//   add      min over s of min(before_s + w, MAX); a probe with before_s + w > MAX counts as saturated
//   remove   mn = min before_s: MAX -> MAX (a no-op); else mn - w, and mn < w (absent or partial: the loop removes less) raises *flag
template <bool ADDONLY>
__global__ __launch_bounds__(kRunSegBlock) void k_cbfr_perop(const uint32_t *before, const int32_t *w, uint64_t base, uint32_t n, uint32_t k, uint32_t *out,
                                                             uint32_t *flag, unsigned long long *tally)
{
    using S = Sum<unsigned long long>;
    __shared__ S wtot[kRunSegBlock / 64];
    const uint32_t i = blockIdx.x * kRunSegBlock + threadIdx.x;
    unsigned long long added = 0, removed = 0, sat = 0, viol = 0, ab = 0;
    bool bad = false;
    if (i < n) {
        const int32_t x = cbfr_weight<ADDONLY>(w, base + i);
        if (ADDONLY && w && w[base + i] < 0) viol = 1;
        const uint32_t *b = before + (size_t)i * k;
        uint32_t r;
        if (x >= 0) {
            unsigned long long mn = ~0ULL;
            for (uint32_t s = 0; s < k; ++s) {
                unsigned long long v = (unsigned long long)b[s] + (unsigned long long)x;
                if (v > kCbfMax) { v = kCbfMax; ++sat; }
                mn = v < mn ? v : mn;
            }
            added = (unsigned long long)x;
            r = (uint32_t)mn;
        } else {
            const unsigned long long amt = (unsigned long long)(-(long long)x);
            uint32_t mn = kCbfMax;
            for (uint32_t s = 0; s < k; ++s) mn = b[s] < mn ? b[s] : mn;
            if (mn == kCbfMax) r = kCbfMax;
            else {
                bad = (unsigned long long)mn < amt;
                r = (uint32_t)((unsigned long long)mn - amt);
                removed = amt;
            }
        }
        ab = (unsigned long long)(x < 0 ? -(long long)x : (long long)x);
        out[base + i] = r;
    }
    if (__ballot(bad) && (threadIdx.x & 63u) == 0) *flag = 1u;
    // (a block's sums: < 2^8 * 2^31 * 64)
    const unsigned long long s0 = block_scan<kRunSegBlock>(S{added}, wtot).v, s1 = block_scan<kRunSegBlock>(S{removed}, wtot).v,
                             s2 = block_scan<kRunSegBlock>(S{viol}, wtot).v, s3 = block_scan<kRunSegBlock>(S{sat}, wtot).v,
                             s4 = block_scan<kRunSegBlock>(S{ab}, wtot).v;
    if (threadIdx.x == kRunSegBlock - 1) {
        if (s0) atomicAdd(tally + 0, s0);
        if (s1) atomicAdd(tally + 1, s1);
        if (s2) atomicAdd(tally + 2, s2);
        if (s3) atomicAdd(tally + 3, s3);
        if (s4) atomicAdd(tally + 4, s4);
    }
}

// the last element of every segment leaves the counter's value in the table
static __global__ __launch_bounds__(kRunSegBlock) void k_cbfr_commit(const uint2 *sorted, uint32_t n, const uint32_t *fin, uint32_t *table)
{
    const uint32_t j = blockIdx.x * kRunSegBlock + threadIdx.x;
    if (j >= n) return;
    const uint2 p = sorted[j];
    if (j + 1 == n || sorted[j + 1].x != p.x) table[p.x] = fin[j];
}

// the chunk's tallies -> the handle's counters, as cbf_ordered_book leaves them; clean = 0 (the chunk is replayed, the loop books its own):
// the negative weights alone
static __global__ void k_cbfr_book(const unsigned long long *tally, unsigned long long *ctr, uint32_t k, int clean)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    ctr[2] += tally[2];
    if (!clean) return;
    CbfOrderedTally t;
    t.added = tally[0];
    t.removed = tally[1];
    t.sat = tally[3];
    t.abs_sum = tally[4];
    cbf_ordered_book(ctr, k, t);
}

// ------------------------------------------------------------------ replay
// ops [base, base + n) of the batch, one after the other on one lane: the loop of k_cbf_ordered (k <= kMaxKOrdered)
template <class Src, bool POW2, bool ADDONLY>
__global__ __launch_bounds__(64) void k_cbfr_replay(Src src, uint32_t *tab, Mod md, uint32_t k, const int32_t *w, uint64_t base, uint32_t n, uint32_t *out,
                                                    unsigned long long *ctr)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint64_t idx[kMaxKOrdered], vals[kMaxKOrdered];
    CbfOrderedTally t;
    cbf_ordered_loop<Src, POW2>(src, tab, md, k, [&](uint64_t i) -> int64_t { return (int64_t)cbfr_weight<ADDONLY>(w, i); }, ADDONLY ? 0 : 2, base, base + n, out,
                                idx, vals, t);
    cbf_ordered_book(ctr, k, t);
}

// int32 weights of the entry -> the int64 list of k_cbf_ordered (calls that are not eligible for the passes above)
template <bool ADDONLY>
__global__ __launch_bounds__(kBlock) void k_cbfr_widen(const int32_t *w, uint64_t n, int64_t *out, unsigned long long *ctr)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    unsigned long long neg = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        neg += ADDONLY && w[i] < 0;
        out[i] = cbfr_weight<ADDONLY>(w, i);
    }
    if (neg) atomicAdd(ctr + 2, neg);
}

}  // namespace psk

// ------------------------------------------------------------------ host side (psk_cbf_running.hip; the hash and replay launches are psk_cbf.hip's)
#include "psk_cbf_running_layout.hpp"
struct psk_sketch;
struct CbfRunArena {
    CbfRunLayout l;
    uint32_t *bins;               // [cap * k]  the hash kernel's output; shares its memory with pairs[1]
    uint2 *pairs[2];              // [cap * k]  (bin, e) before / behind a sort pass; the one the last pass read holds fin afterwards
    uint32_t *before;             // [cap * k]  the counter's value in front of the op, per probe
    uint32_t *hist;               // [256][tiles]
    psk::CbfMap *agg;             // [blocks]
    unsigned long long *tally;    // [kCbfTallyWords]
};
// sizes the arena for a batch of n ops and grows the scratch (psk_sketch::s_part)
__attribute__((visibility("hidden"))) int cbf_running_arena(psk_sketch *s, uint64_t n, CbfRunArena *a);
// The optimistic passes behind the hash kernel for the chunk [base, base + n) of the batch (a.bins is filled; w / out are the BATCH's
// arrays), the verdict and, after a clean one, the commit.  *clean = false: the table and the handle's counters are as they were in front
// of the chunk (but for the negative-weight tally), the caller replays it.
__attribute__((visibility("hidden"))) int cbf_running_chunk(psk_sketch *s, const CbfRunArena &a, const int32_t *w, uint64_t base, uint32_t n, bool addonly,
                                                            uint32_t *out, hipStream_t st, bool *clean);
