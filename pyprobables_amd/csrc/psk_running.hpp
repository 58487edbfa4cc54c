// psk_running.hpp -- exact ORDERED CountMinSketch batches with every op's return value, in parallel: adds (psk_cms_add_running) and signed
// batches of adds and removes (psk_cms_update_running).  One pipeline over the skeleton of psk_segscan.hpp, two algebras (RunAddOps,
// RunSignedOps).
//
// What the reference computes (countminsketch.py:267-321), one op after the other; w >= 0 adds w, w < 0 removes -w:
//     for s < depth:  bin = T[s][h_s(key_i) % width] = clamp(bin + w_i, INT32_MIN, INT32_MAX)        value_s(i) = that bin
//     elements_added = clamp(elements_added + w_i, INT64_MIN, INT64_MAX);   return query(value_0(i) .. value_{depth-1}(i))
// (add_alt clamps above only, remove_alt below only; the value in front of the op lies inside the rails, so the full clamp describes both.)
// What an op does to its bin is a map, and maps compose associatively: value_s(i) is an inclusive SEGMENTED SCAN of maps in arrival order,
// one segment per (row, bin), applied to the table T0 the chunk starts from.  elements_added is the same thing, not segmented.
//   adds only (RunSeg)   with w >= 0 a bin never decreases, so the clamp of every step equals ONE saturating sum:
//                        value_s(i) = min(T0[s][b] + sum of w_j over j <= i with bin_s(j) = b, INT32_MAX).  The sums are kept as uint32
//                        saturating at 2^32 - 1 and T0 is added last in 64 bits: T0 >= -2^31, so a sum that hit 2^32 - 1 still clamps to
//                        INT32_MAX (a table may hold negative bins from earlier removes).  8 bytes per value.
//   signed (RunMap)      (a, lo, hi): x -> min(hi, max(lo, x + a)), lo <= hi, closed under composition: (a1, lo1, hi1) followed by
//                        (a2, lo2, hi2) is (a1 + a2, clamp(lo1 + a2, lo2, hi2), clamp(hi1 + a2, lo2, hi2)) (clamping is monotone, so it
//                        distributes over the min / max of the first map).  24 bytes per value, 0.91 - 0.93 of the add path's rate
//                        (profiles/signed_running_bench.txt): the reason the add path keeps an algebra of its own.
//
// Passes over one ordered chunk of n <= kRunChunk ops (psk_cms.hip walks a batch chunk by chunk; chunks are consecutive, each sees the
// table as the previous one left it, so exactness is unaffected and the scratch does not grow with the batch):
//   k_run_hash        bin[s][i] = h_s(key_i) % width                                        (the engine's Src / Mod functors)
//   k_run_tile / k_run_tile_scan   every 256-op tile as one value on elements_added, and elements_added in front of every tile
//   per row, ceil(lg width / 8) passes of the stable sort of (bin, i)                      (segscan_sort)
//   k_run_seg_reduce / k_seg_carry / k_run_seg_apply   the segmented scan; _apply stores value_s(i) at run[s][i] and tallies clamps
//   k_run_seg_commit  the last element of every segment stores its value into the table (a pass of its own: _apply reads T0)
//   k_run_query       per op: the depth values + elements_added after the op -> min / mean / mean-min  (countminsketch.py:429-453)
#pragma once
#include "psk_device.hpp"
#include "psk_segscan.hpp"

namespace psk {

constexpr uint32_t kRunChunk = 1u << 20;       // most ops per chunk; fewer for deep sketches: chunk * depth <= kRunCells
constexpr uint32_t kRunCells = 1u << 23;

__host__ __device__ __forceinline__ uint32_t run_sat_add(uint32_t a, uint32_t b)
{
    const uint32_t s = a + b;
    return s < a ? 0xFFFFFFFFu : s;
}
__host__ __device__ __forceinline__ long long run_sat_add64(long long a, long long b)
{
    long long s;
    if (__builtin_saddll_overflow(a, b, &s)) s = b > 0 ? INT64_MAX : INT64_MIN;
    return s;
}

// ------------------------------------------------------------------ the algebras (the contract: psk_segscan.hpp)
// Adds: v = the saturating sum of the weights of the stretch's last segment.
struct RunSeg {
    uint32_t v;
    uint32_t head;
    static __host__ __device__ __forceinline__ RunSeg identity() { return RunSeg{0u, 0u}; }
    static __host__ __device__ __forceinline__ RunSeg of(int32_t w, bool head) { return RunSeg{(uint32_t)w, head ? 1u : 0u}; }  // w >= 0
    __host__ __device__ __forceinline__ int32_t operator()(int32_t t0) const
    {
        const int64_t x = (int64_t)t0 + (int64_t)v;
        return (int32_t)(x > INT32_MAX ? INT32_MAX : x);
    }
    static __host__ __device__ __forceinline__ RunSeg combine(const RunSeg &a, const RunSeg &b)
    {
        return RunSeg{b.head ? b.v : run_sat_add(a.v, b.v), a.head | b.head};
    }
};
__device__ __forceinline__ RunSeg seg_shfl_up(const RunSeg &x, int o) { return RunSeg{(uint32_t)__shfl_up((int)x.v, o), (uint32_t)__shfl_up((int)x.head, o)}; }

// Signed: the clamp map.  `a` is a plain sum: a chunk has at most 2^20 ops of |w| <= 2^31, so |a| <= 2^51 and int64 holds it without
// saturation; lo / hi are values a bin can take, int32.
struct RunMap {
    int64_t a;
    int32_t lo, hi;
    uint32_t head;
    static __host__ __device__ __forceinline__ RunMap identity() { return RunMap{0, INT32_MIN, INT32_MAX, 0u}; }  // (the identity on the values a bin can hold)
    static __host__ __device__ __forceinline__ RunMap of(int32_t w, bool head) { return RunMap{w, INT32_MIN, INT32_MAX, head ? 1u : 0u}; }
    __host__ __device__ __forceinline__ int32_t clamp(int64_t x) const { return (int32_t)(x < lo ? lo : (x > hi ? hi : x)); }
    __host__ __device__ __forceinline__ int32_t operator()(int32_t x) const { return clamp((int64_t)x + a); }
    static __host__ __device__ __forceinline__ RunMap combine(const RunMap &a, const RunMap &b)
    {
        if (b.head) return RunMap{b.a, b.lo, b.hi, 1u};
        return RunMap{a.a + b.a, b.clamp((int64_t)a.lo + b.a), b.clamp((int64_t)a.hi + b.a), a.head};
    }
};
__device__ __forceinline__ RunMap seg_shfl_up(const RunMap &x, int o)
{
    return RunMap{(int64_t)__shfl_up((long long)x.a, o), __shfl_up(x.lo, o), __shfl_up(x.hi, o), (uint32_t)__shfl_up((int)x.head, o)};
}

// elements_added under adds: the sum of the weights (a chunk: < 2^52), saturating at INT64_MAX when it is applied (:285-287).  It is its
// own tile value: the sum of |w| is the sum.
struct RunSum {
    unsigned long long v;
    static __host__ __device__ __forceinline__ RunSum identity() { return RunSum{0}; }
    static __host__ __device__ __forceinline__ RunSum of(int32_t w) { return RunSum{(unsigned long long)w}; }  // w >= 0
    __host__ __device__ __forceinline__ long long operator()(long long x) const { return run_sat_add64(x, (long long)v); }
    static __host__ __device__ __forceinline__ RunSum combine(const RunSum &a, const RunSum &b) { return RunSum{a.v + b.v}; }
    __host__ __device__ __forceinline__ const RunSum &els() const { return *this; }
    __host__ __device__ __forceinline__ unsigned long long abs() const { return v; }
};
__device__ __forceinline__ RunSum seg_shfl_up(const RunSum &x, int o) { return RunSum{__shfl_up(x.v, o)}; }

// elements_added under signed batches: the clamp map on the int64 rails (:285-287, :317-319).  `a` as above; lo + a may leave int64 and
// saturates, which the clamp that follows cannot tell from the true sum.
struct RunMap64 {
    long long a, lo, hi;
    static __host__ __device__ __forceinline__ RunMap64 identity() { return RunMap64{0, INT64_MIN, INT64_MAX}; }
    static __host__ __device__ __forceinline__ RunMap64 of(int32_t w) { return RunMap64{w, INT64_MIN, INT64_MAX}; }
    __host__ __device__ __forceinline__ long long clamp(long long x) const { return x < lo ? lo : (x > hi ? hi : x); }
    __host__ __device__ __forceinline__ long long operator()(long long x) const { return clamp(run_sat_add64(x, a)); }
    static __host__ __device__ __forceinline__ RunMap64 combine(const RunMap64 &a, const RunMap64 &b)
    {
        return RunMap64{a.a + b.a, b.clamp(run_sat_add64(a.lo, b.a)), b.clamp(run_sat_add64(a.hi, b.a))};
    }
};
__device__ __forceinline__ RunMap64 seg_shfl_up(const RunMap64 &x, int o) { return RunMap64{__shfl_up(x.a, o), __shfl_up(x.lo, o), __shfl_up(x.hi, o)}; }

// a stretch of a signed batch as its map on elements_added and the sum of its |w| (< 2^52 per chunk)
struct RunTile {
    RunMap64 f;
    unsigned long long sum_abs;
    static __host__ __device__ __forceinline__ RunTile identity() { return RunTile{RunMap64::identity(), 0}; }
    static __host__ __device__ __forceinline__ RunTile of(int32_t w) { return RunTile{RunMap64::of(w), (unsigned long long)(w < 0 ? -(long long)w : (long long)w)}; }
    static __host__ __device__ __forceinline__ RunTile combine(const RunTile &a, const RunTile &b) { return RunTile{RunMap64::combine(a.f, b.f), a.sum_abs + b.sum_abs}; }
    __host__ __device__ __forceinline__ const RunMap64 &els() const { return f; }
    __host__ __device__ __forceinline__ unsigned long long abs() const { return sum_abs; }
};
__device__ __forceinline__ RunTile seg_shfl_up(const RunTile &x, int o) { return RunTile{seg_shfl_up(x.f, o), __shfl_up(x.sum_abs, o)}; }

// What the two entries differ in.  Bin: a stretch of a sorted row, Bin::of(w, head) one op, f(t0) the bin's value behind the stretch;
// Els: a stretch of the batch on elements_added, Els::of(w) one op; Tile: what a 256-op tile stores, with els() and abs() = its sum of |w|;
// weight(w, i): the weight of op i of the batch (nullptr: 1).
struct RunAddOps {  // psk_cms_add_running.  A negative weight can only come from a device batch (the host entry refuses it before anything
    using Bin = RunSeg;  // runs): it counts as 0 here and k_run_tile tallies it as a contract violation
    using Els = RunSum;
    using Tile = RunSum;
    static constexpr bool kNegativeIsViolation = true;
    static __device__ __forceinline__ int32_t weight(const int32_t *w, uint64_t i)
    {
        if (!w) return 1;
        const int32_t x = w[i];
        return x < 0 ? 0 : x;
    }
};
struct RunSignedOps {  // psk_cms_update_running: every int32 is valid, INT32_MIN removes 2^31
    using Bin = RunMap;
    using Els = RunMap64;
    using Tile = RunTile;
    static constexpr bool kNegativeIsViolation = false;
    static __device__ __forceinline__ int32_t weight(const int32_t *w, uint64_t i) { return w ? w[i] : 1; }
};

// ------------------------------------------------------------------ hash
// bins[s * cap + i] = h_s(key_{base + i}) % width for the n ops of the chunk (width <= 2^32)
template <class Src, bool POW2>
__global__ __launch_bounds__(kBlock) void k_run_hash(Src src, Mod md, uint32_t depth, uint64_t base, uint32_t n, uint32_t cap, uint32_t *bins)
{
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const typename Src::Key key = src.load(base + i);
        for_each_hash(src, key, base + i, depth, [&](uint32_t s, uint64_t h) { bins[(size_t)s * cap + i] = (uint32_t)reduce<POW2>(md, h); });
    }
}

// ------------------------------------------------------------------ elements_added
// tile[t] = the 256 ops of tile t as one value; negative weights of a device batch of adds -> ctr[PSK_CTR_VIOLATIONS]
template <class Ops>
__global__ __launch_bounds__(kRunSegBlock) void k_run_tile(const int32_t *w, uint64_t base, uint32_t n, typename Ops::Tile *tile, long long *ctr)
{
    using T = typename Ops::Tile;
    __shared__ T wtot[kRunSegBlock / 64];
    const uint32_t i = blockIdx.x * kRunSegBlock + threadIdx.x;
    const T incl = block_scan<kRunSegBlock>(T::of(i < n ? Ops::weight(w, base + i) : 0), wtot);
    if (threadIdx.x == kRunSegBlock - 1) tile[blockIdx.x] = incl;
    if (Ops::kNegativeIsViolation) {
        const unsigned long long bad = __ballot(i < n && w && w[base + i] < 0);
        if ((threadIdx.x & 63u) == 0 && bad) atomicAdd((unsigned long long *)(ctr + 2), (unsigned long long)__popcll(bad));
    }
}

// ONE workgroup: els[t] = elements_added in front of tile t (els may be the tile array itself where a tile has 8 bytes); st[0] =
// elements_added behind the chunk, from which the next chunk starts (both rails, per op: countminsketch.py:285-287, :317-319); the handle's
// counters follow as k_cms_ordered leaves them (ctr[5] = elements_added, ctr[4] += sum |w|)
template <class Ops>
__global__ __launch_bounds__(kRunScanThreads) void k_run_tile_scan(const typename Ops::Tile *tile, uint32_t ntiles, long long *els, long long *st, long long els_in,
                                                                   int first, long long *ctr, long long *els_out)
{
    using T = typename Ops::Tile;
    const long long start = first ? els_in : st[0];  // (every thread has read st[0] once the scan's first barrier is behind it)
    const T all = stretch_scan<kRunScanThreads, T>(ntiles, [&](uint32_t t) { return tile[t]; }, [&](uint32_t t, const T &f) { els[t] = f.els()(start); });
    if (threadIdx.x == kRunScanThreads - 1) {  // (the last thread's value is the chunk's total)
        const long long end = all.els()(start);
        st[0] = end;
        ctr[5] = end;
        if (els_out) *els_out = end;
        const unsigned long long nb = (unsigned long long)ctr[4] + all.abs();
        ctr[4] = (nb < (unsigned long long)ctr[4] || nb > (1ULL << 62)) ? (1LL << 62) : (long long)nb;
    }
}

// ------------------------------------------------------------------ segmented scan of a sorted row
// this thread's element of block blockIdx.x, row blockIdx.y: (weight, "first of its bin"); past the end: an empty segment of its own
struct RunElem {
    uint32_t bin, op;
    int32_t w;
    bool valid, head;
};
template <class Ops>
__device__ __forceinline__ RunElem run_seg_load(const uint2 *sorted, const int32_t *w, uint64_t base, uint32_t n, uint32_t cap)
{
    const uint32_t i = blockIdx.x * kRunSegBlock + threadIdx.x;
    RunElem e{0u, 0u, 0, i < n, true};
    if (e.valid) {
        const uint2 *row = sorted + (size_t)blockIdx.y * cap;
        const uint2 p = row[i];
        e.bin = p.x;
        e.op = p.y;
        e.head = i == 0 || row[i - 1].x != p.x;
        e.w = Ops::weight(w, base + p.y);
    }
    return e;
}

// agg[row * nblk + block] = the block as one value
template <class Ops>
__global__ __launch_bounds__(kRunSegBlock) void k_run_seg_reduce(const uint2 *sorted, const int32_t *w, uint64_t base, uint32_t n, uint32_t cap, uint32_t nblk,
                                                                 typename Ops::Bin *agg)
{
    using M = typename Ops::Bin;
    __shared__ M wtot[kRunSegBlock / 64];
    const RunElem e = run_seg_load<Ops>(sorted, w, base, n, cap);
    const M incl = block_scan<kRunSegBlock>(M::of(e.w, e.head), wtot);
    if (threadIdx.x == kRunSegBlock - 1) agg[(size_t)blockIdx.y * nblk + blockIdx.x] = incl;
}

// run[row * cap + op] = the bin's value after the op (countminsketch.py:276-282, :309-314).  With `before` the bin's ops in front of this
// one (the identity at a segment head), cur = before(T0) + w; the op is tallied in ctr[PSK_CTR_SATURATED] when cur lies strictly outside
// the rails, the test of k_cms_ordered (a remove that lands exactly on INT32_MIN is no clamp), and stored clamped.  One body for both
// algebras: under RunAddOps w >= 0 and before(T0) >= T0 >= INT32_MIN, so the lower rail is out of reach and the test is the add path's
// cur > INT32_MAX.
template <class Ops>
__global__ __launch_bounds__(kRunSegBlock) void k_run_seg_apply(const uint2 *sorted, const int32_t *w, uint64_t base, uint32_t n, uint32_t cap, uint32_t nblk,
                                                                const typename Ops::Bin *carry, const int32_t *table, uint64_t width, int32_t *run, long long *ctr)
{
    using M = typename Ops::Bin;
    __shared__ M wtot[kRunSegBlock / 64];
    const RunElem e = run_seg_load<Ops>(sorted, w, base, n, cap);
    const M front = carry[(size_t)blockIdx.y * nblk + blockIdx.x];
    M excl;
    block_scan<kRunSegBlock>(M::of(e.w, e.head), wtot, &excl);
    bool clamped = false;
    if (e.valid) {
        const M before = e.head ? M::identity() : M::combine(front, excl);
        const int64_t cur = (int64_t)before(table[(uint64_t)blockIdx.y * width + e.bin]) + (int64_t)e.w;
        clamped = cur > INT32_MAX || cur < INT32_MIN;
        run[(size_t)blockIdx.y * cap + e.op] = (int32_t)(cur > INT32_MAX ? INT32_MAX : (cur < INT32_MIN ? INT32_MIN : cur));
    }
    const unsigned long long c = __ballot(clamped);
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd((unsigned long long *)(ctr + 3), (unsigned long long)__popcll(c));
}

// the last op of every bin leaves the bin's value in the table
static __global__ __launch_bounds__(kRunSegBlock) void k_run_seg_commit(const uint2 *sorted, uint32_t n, uint32_t cap, const int32_t *run, int32_t *table, uint64_t width)
{
    const uint32_t i = blockIdx.x * kRunSegBlock + threadIdx.x;
    if (i >= n) return;
    const uint2 *row = sorted + (size_t)blockIdx.y * cap;
    const uint2 p = row[i];
    if (i + 1 == n || row[i + 1].x != p.x) table[(uint64_t)blockIdx.y * width + p.x] = run[(size_t)blockIdx.y * cap + p.y];
}

// ------------------------------------------------------------------ query
// the query over the depth values of op i (the expressions of k_cms_ordered); els_of(): elements_added after the op, which only a mean-min
// query with a non-zero value asks for
template <class ElsOf>
__device__ __forceinline__ int64_t run_query_value(const int32_t *run, uint32_t i, uint32_t cap, uint32_t depth, uint64_t width, int query, ElsOf els_of)
{
    int64_t r;
    if (query == 2) {  // mean-min :438-453
        int64_t vals[kMaxDepthMeanMin];
        bool all_zero = true;
        for (uint32_t s = 0; s < depth; ++s) {
            vals[s] = run[(size_t)s * cap + i];
            all_zero &= vals[s] == 0;
        }
        if (all_zero) r = 0;  // (sorted: first and last zero <=> all zero)
        else {
            const long long els = els_of();
            for (uint32_t s = 0; s < depth; ++s) vals[s] = vals[s] - floordiv((int64_t)els - vals[s], (int64_t)width - 1);
            sort_small(vals, depth);
            r = (depth % 2 == 0) ? floordiv(vals[depth / 2] + vals[depth / 2 - 1], 2) : vals[depth / 2];
        }
    } else {
        int64_t mn = INT64_MAX, sum = 0;
        for (uint32_t s = 0; s < depth; ++s) {
            const int64_t v = run[(size_t)s * cap + i];
            mn = v < mn ? v : mn;
            sum += v;
        }
        r = query == 1 ? floordiv(sum, (int64_t)depth) : mn;  // mean :434-436 / min :429-432
    }
    return r;
}

// out[base + i] = query over the depth values of op i; WIDE: int64 results (mean-min), else int32.  els[tile] = elements_added in front
// of the tile; the ops of the tile up to this one are applied to it as one value
template <class Ops, bool WIDE>
__global__ __launch_bounds__(kRunSegBlock) void k_run_query(const int32_t *run, const int32_t *w, const long long *els, uint64_t base, uint32_t n, uint32_t cap,
                                                            uint32_t depth, uint64_t width, int query, void *out)
{
    using E = typename Ops::Els;
    __shared__ E wtot[kRunSegBlock / 64];
    const uint32_t i = blockIdx.x * kRunSegBlock + threadIdx.x;
    E pre = E::identity();
    if (WIDE) pre = block_scan<kRunSegBlock>(E::of(i < n ? Ops::weight(w, base + i) : 0), wtot);  // (uniform) only the mean-min query looks at it
    if (i >= n) return;
    const int64_t r = run_query_value(run, i, cap, depth, width, query, [&]() { return pre(els[blockIdx.x]); });
    if (WIDE) ((int64_t *)out)[base + i] = r;
    else ((int32_t *)out)[base + i] = (int32_t)r;
}

// int64 results of the sequential kernel (the fall-back of both entries) -> the entry's int32 / int64 output
static __global__ __launch_bounds__(kBlock) void k_run_narrow(const int64_t *in, uint64_t n, int wide, void *out, long long *els_out)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        if (wide) ((int64_t *)out)[i] = in[i];
        else ((int32_t *)out)[i] = (int32_t)in[i];
    }
    if (els_out && blockIdx.x == 0 && threadIdx.x == 0) *els_out = in[n];
}
static __global__ void k_run_set(long long *p, long long v) { *p = v; }
static __global__ __launch_bounds__(kBlock) void k_run_widen(const int32_t *w, uint64_t n, int64_t *out)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) out[i] = w[i];
}

}  // namespace psk

// ------------------------------------------------------------------ host side (psk_running.hip; the hash launch is psk_cms.hip's)
struct psk_sketch;
// where the buffers of one chunk lie in the handle's scratch (psk_sketch::s_part), for chunks of at most `cap` ops
struct RunArena {
    uint32_t cap, passes;         // ops per chunk; radix passes per row
    uint32_t *bins;               // [depth][cap]   the hash kernel's output; shares its memory with pairs[1]
    uint2 *pairs[2];              // [depth][cap]   (bin, op) before / behind a sort pass
    int32_t *run;                 // [depth][cap]   value of row s after op i
    uint32_t *hist;               // [depth][256][tiles]
    void *agg;                    // [depth][blocks]  Ops::Bin
    long long *els;               // [blocks]         elements_added in front of every tile
    void *tile;                   // [blocks]         Ops::Tile; an 8-byte tile is scanned in place: then this is els
    long long *st;                // [0] elements_added behind the chunk in hand
};
// Ops = psk::RunAddOps / psk::RunSignedOps for both.  Sizes the arena for a batch of n ops and grows the scratch
template <class Ops>
__attribute__((visibility("hidden"))) int cms_running_arena(psk_sketch *s, uint64_t n, RunArena *a);
// everything behind the hash kernel for the chunk [base, base + n) of the batch: a.bins is filled; w / out are the BATCH's arrays
template <class Ops>
__attribute__((visibility("hidden"))) int cms_running_chunk(psk_sketch *s, const RunArena &a, const int32_t *w, uint64_t base, uint32_t n, bool first, int64_t els_in,
                                                            int query, void *out, int64_t *els_out, hipStream_t st);
