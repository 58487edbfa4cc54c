// psk_running.hpp -- exact ORDERED CountMinSketch add with every op's return value, in parallel (psk_cms_add_running); signed batches
// (adds and removes, psk_cms_update_running): the second half of this file.
//
// What the reference computes (countminsketch.py:267-288), one op after the other:
//     for s < depth:  bin = T[s][h_s(key_i) % width] = min(bin + w_i, INT32_MAX)        value_s(i) = that bin
//     elements_added = min(elements_added + w_i, INT64_MAX);   return query(value_0(i) .. value_{depth-1}(i))
// With w_i >= 0 a bin never decreases, so clamping at every step equals ONE saturating running sum:
//     value_s(i) = min(T0[s][b] + sum of w_j over j <= i with bin_s(j) = b,  INT32_MAX)          b = bin_s(i)
// and a saturating add of non-negative numbers is associative: value_s is an inclusive SEGMENTED SCAN of the weights in arrival order,
// one segment per (row, bin).  The sums are kept as uint32 saturating at 2^32 - 1 and T0 is added last in 64 bits: T0 >= -2^31, so a sum
// that hit 2^32 - 1 still clamps to INT32_MAX (a table may hold negative bins from earlier removes).
//
// Passes over one ordered chunk of n <= kRunChunk ops (psk_capi.hip walks a batch chunk by chunk; chunks are consecutive, each sees
// the table as the previous one left it, so exactness is unaffected and the scratch does not grow with the batch):
//   k_run_hash       bin[s][i] = h_s(key_i) % width                                        (the engine's Src / Mod functors)
//   k_run_wsum/_wscan  tile sums of the weights and their exclusive scan: elements_added in front of every 256-op tile
//   per row, ceil(lg width / 8) passes of a STABLE LSD radix sort of (bin, i), 8-bit digits:
//     k_run_sort_hist    digit counts per 2048-element tile (one wave per tile)
//     k_run_sort_scan    exclusive scan of the (digit, tile) counts in that order
//     k_run_sort_scatter rank inside the tile = lanes of the same digit below me (8 ballots) + what earlier 64-element steps of the
//                        tile counted (LDS, one counter per digit): equal digits keep their order, so arrival order inside a bin is free
//   segmented scan of the sorted run, reduce-then-scan with a second level (no spinning, no inter-workgroup flags):
//     k_run_seg_reduce   per 256-element block: (sum of the block's last open segment, "a segment starts in this block")
//     k_run_seg_carry    one workgroup per row scans those pairs: the open segment's sum in front of every block
//     k_run_seg_apply    recomputes the block's scan, adds the carry and T0, stores value_s(i) at run[s][i], tallies clamps
//     k_run_seg_commit   the last element of every segment stores its value into the table (a pass of its own: _apply reads T0)
//   k_run_query      per op: the depth values + elements_added after the op -> min / mean / mean-min  (countminsketch.py:429-453)
#pragma once
#include "psk_device.hpp"

namespace psk {

constexpr uint32_t kRunChunk = 1u << 20;       // most ops per chunk; fewer for deep sketches: chunk * depth <= kRunCells
constexpr uint32_t kRunCells = 1u << 23;
constexpr uint32_t kRunSortTile = 2048;        // elements per sort tile (one wave: 32 steps of 64)
constexpr uint32_t kRunSegBlock = 256;         // elements per block of the segmented scan, and ops per tile of the weight prefix
constexpr int kRunScanThreads = 1024;          // the single-workgroup second levels

__device__ __forceinline__ uint32_t run_sat_add(uint32_t a, uint32_t b)
{
    const uint32_t s = a + b;
    return s < a ? 0xFFFFFFFFu : s;
}

// (value, head) of a stretch of the sorted run: value = sum of its LAST segment as far as the stretch covers it, head = a segment
// starts inside the stretch.  Associative; b follows a.
struct RunSeg {
    uint32_t v;
    uint32_t head;
};
__device__ __forceinline__ RunSeg run_combine(const RunSeg &a, const RunSeg &b)
{
    return RunSeg{b.head ? b.v : run_sat_add(a.v, b.v), a.head | b.head};
}

// inclusive scan of one RunSeg per thread over a workgroup of NT threads (NT / 64 waves); `wtot`: NT / 64 entries of LDS
template <int NT>
__device__ __forceinline__ RunSeg run_block_segscan(RunSeg x, RunSeg *wtot)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const RunSeg y{(uint32_t)__shfl_up((int)x.v, o), (uint32_t)__shfl_up((int)x.head, o)};
        if (lane >= (uint32_t)o) x = run_combine(y, x);
    }
    if (lane == 63u) wtot[wave] = x;
    __syncthreads();
    RunSeg c{0u, 0u};
    for (uint32_t u = 0; u < wave; ++u) c = run_combine(c, wtot[u]);
    __syncthreads();  // (wtot may be reused by the caller)
    return run_combine(c, x);
}

// inclusive scan of one value per thread over a workgroup of NT threads
template <int NT, class T>
__device__ __forceinline__ T run_block_scan(T x, T *wtot)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(x, o);
        if (lane >= (uint32_t)o) x += y;
    }
    if (lane == 63u) wtot[wave] = x;
    __syncthreads();
    T c = 0;
    for (uint32_t u = 0; u < wave; ++u) c += wtot[u];
    __syncthreads();
    return c + x;
}

// the weight of op i of the batch (nullptr: 1).  A negative weight can only come from a device batch (the host entry refuses it before
// anything runs): it counts as 0 here and is tallied as a contract violation by k_run_wsum.
__device__ __forceinline__ uint32_t run_weight(const int32_t *w, uint64_t i)
{
    if (!w) return 1u;
    const int32_t x = w[i];
    return x < 0 ? 0u : (uint32_t)x;
}

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

// ------------------------------------------------------------------ weight prefix
// tsum[t] = sum of the weights of tile t (256 ops); negative weights of a device batch -> ctr[PSK_CTR_VIOLATIONS]
static __global__ __launch_bounds__(kRunSegBlock) void k_run_wsum(const int32_t *w, uint64_t base, uint32_t n, unsigned long long *tsum, long long *ctr)
{
    __shared__ unsigned long long wtot[kRunSegBlock / 64];
    const uint32_t i = blockIdx.x * kRunSegBlock + threadIdx.x;
    const bool neg = i < n && w && w[base + i] < 0;
    const unsigned long long x = i < n ? run_weight(w, base + i) : 0u;
    const unsigned long long incl = run_block_scan<kRunSegBlock>(x, wtot);
    if (threadIdx.x == kRunSegBlock - 1) tsum[blockIdx.x] = incl;
    const unsigned long long bad = __ballot(neg);
    if ((threadIdx.x & 63u) == 0 && bad) atomicAdd((unsigned long long *)(ctr + 2), (unsigned long long)__popcll(bad));
}

// ONE workgroup: tsum -> exclusive scan in place; st[1] = elements_added in front of the chunk, st[0] = behind it (clamped at INT64_MAX,
// countminsketch.py:285-287); the handle's counters follow as k_cms_ordered leaves them (ctr[5] = elements_added, ctr[4] += sum |w|)
static __global__ __launch_bounds__(kRunScanThreads) void k_run_wscan(unsigned long long *tsum, uint32_t ntiles, long long *st, long long els_in, int first,
                                                                     long long *ctr, long long *els_out)
{
    __shared__ unsigned long long wtot[kRunScanThreads / 64];
    const uint32_t per = (ntiles + kRunScanThreads - 1) / kRunScanThreads;
    const uint32_t lo = threadIdx.x * per, hi = lo + per < ntiles ? lo + per : ntiles;
    unsigned long long mine = 0;
    for (uint32_t t = lo; t < hi; ++t) mine += tsum[t];
    const unsigned long long incl = run_block_scan<kRunScanThreads>(mine, wtot);
    unsigned long long run = incl - mine;
    for (uint32_t t = lo; t < hi; ++t) {
        const unsigned long long x = tsum[t];
        tsum[t] = run;
        run += x;
    }
    if (threadIdx.x == kRunScanThreads - 1) {  // incl = the chunk's total (< 2^52)
        const long long start = first ? els_in : st[0];
        long long end;
        if (__builtin_saddll_overflow(start, (long long)incl, &end)) end = INT64_MAX;
        st[1] = start;
        st[0] = end;
        ctr[5] = end;
        if (els_out) *els_out = end;
        const unsigned long long nb = (unsigned long long)ctr[4] + incl;
        ctr[4] = (nb < (unsigned long long)ctr[4] || nb > (1ULL << 62)) ? (1LL << 62) : (long long)nb;
    }
}

// ------------------------------------------------------------------ stable radix sort of (bin, i), one row per blockIdx.y
// lanes of the wave that hold the same digit as this one (valid lanes only)
__device__ __forceinline__ unsigned long long run_match_digit(uint32_t d, bool valid)
{
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

// element e of a row: the first pass reads the hash kernel's bins (the position is the op), later passes the pairs of the pass before
template <bool FIRST>
__device__ __forceinline__ uint2 run_sort_load(const uint32_t *keys0, const uint2 *src, size_t at, uint32_t e)
{
    if (FIRST) return make_uint2(keys0[at], e);
    return src[at];
}

// hist[(row * 256 + d) * ntiles + tile] = elements of the tile with digit d
template <bool FIRST>
__global__ __launch_bounds__(64) void k_run_sort_hist(const uint32_t *keys0, const uint2 *src, uint32_t *hist, uint32_t n, uint32_t cap, uint32_t ntiles,
                                                      uint32_t shift)
{
    __shared__ uint32_t cnt[256];
    const uint32_t lane = threadIdx.x, tile = blockIdx.x, row = blockIdx.y;
#pragma unroll
    for (int q = 0; q < 4; ++q) cnt[lane + 64 * q] = 0;
    __syncthreads();
    for (uint32_t it = 0; it < kRunSortTile / 64; ++it) {
        const uint32_t e = tile * kRunSortTile + it * 64 + lane;
        const bool valid = e < n;
        const uint32_t d = valid ? (run_sort_load<FIRST>(keys0, src, (size_t)row * cap + e, e).x >> shift) & 255u : 0u;
        const unsigned long long m = run_match_digit(d, valid);
        if (valid && (m & ((1ULL << lane) - 1)) == 0) cnt[d] += (uint32_t)__popcll(m);  // the lowest lane of every digit: different counters
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) hist[((size_t)row * 256 + lane + 64 * q) * ntiles + tile] = cnt[lane + 64 * q];
}

// exclusive scan of the 256 * ntiles counts of a row, in (digit, tile) order; one workgroup per row
static __global__ __launch_bounds__(kRunScanThreads) void k_run_sort_scan(uint32_t *hist, uint32_t len)
{
    __shared__ uint32_t wtot[kRunScanThreads / 64];
    uint32_t *h = hist + (size_t)blockIdx.x * len;
    const uint32_t per = (len + kRunScanThreads - 1) / kRunScanThreads;
    const uint32_t lo = threadIdx.x * per < len ? threadIdx.x * per : len, hi = lo + per < len ? lo + per : len;
    uint32_t mine = 0;
    for (uint32_t t = lo; t < hi; ++t) mine += h[t];
    const uint32_t incl = run_block_scan<kRunScanThreads>(mine, wtot);
    uint32_t run = incl - mine;
    for (uint32_t t = lo; t < hi; ++t) {
        const uint32_t x = h[t];
        h[t] = run;
        run += x;
    }
}

// dst[row][position] = element, position = scanned count of (digit, tile) + rank among the tile's elements of that digit
template <bool FIRST>
__global__ __launch_bounds__(64) void k_run_sort_scatter(const uint32_t *keys0, const uint2 *src, uint2 *dst, const uint32_t *hist, uint32_t n, uint32_t cap,
                                                         uint32_t ntiles, uint32_t shift)
{
    __shared__ uint32_t nxt[256];  // where the next element of digit d goes
    const uint32_t lane = threadIdx.x, tile = blockIdx.x, row = blockIdx.y;
#pragma unroll
    for (int q = 0; q < 4; ++q) nxt[lane + 64 * q] = hist[((size_t)row * 256 + lane + 64 * q) * ntiles + tile];
    __syncthreads();
    for (uint32_t it = 0; it < kRunSortTile / 64; ++it) {
        const uint32_t e = tile * kRunSortTile + it * 64 + lane;
        const bool valid = e < n;
        const uint2 p = valid ? run_sort_load<FIRST>(keys0, src, (size_t)row * cap + e, e) : make_uint2(0u, 0u);
        const uint32_t d = (p.x >> shift) & 255u;
        const unsigned long long m = run_match_digit(d, valid);
        const uint32_t rank = (uint32_t)__popcll(m & ((1ULL << lane) - 1));
        const uint32_t pos = nxt[d] + rank;
        __syncthreads();  // every lane has read its counter ...
        if (valid && rank == 0) nxt[d] += (uint32_t)__popcll(m);
        __syncthreads();  // ... before the digit's lowest lane moves it on
        if (valid && pos < n) dst[(size_t)row * cap + pos] = p;
    }
}

// ------------------------------------------------------------------ segmented scan of a sorted row
// this thread's element of block blockIdx.x, row blockIdx.y: (weight, "first of its bin"); past the end: an empty segment of its own
struct RunElem {
    uint32_t bin, op, w;
    bool valid, head;
};
__device__ __forceinline__ RunElem run_seg_load(const uint2 *sorted, const int32_t *w, uint64_t base, uint32_t n, uint32_t cap)
{
    const uint32_t i = blockIdx.x * kRunSegBlock + threadIdx.x;
    RunElem e{0u, 0u, 0u, i < n, true};
    if (e.valid) {
        const uint2 *row = sorted + (size_t)blockIdx.y * cap;
        const uint2 p = row[i];
        e.bin = p.x;
        e.op = p.y;
        e.head = i == 0 || row[i - 1].x != p.x;
        e.w = run_weight(w, base + p.y);
    }
    return e;
}

// agg[row * nblk + block] = the block as one RunSeg
static __global__ __launch_bounds__(kRunSegBlock) void k_run_seg_reduce(const uint2 *sorted, const int32_t *w, uint64_t base, uint32_t n, uint32_t cap,
                                                                       uint32_t nblk, RunSeg *agg)
{
    __shared__ RunSeg wtot[kRunSegBlock / 64];
    const RunElem e = run_seg_load(sorted, w, base, n, cap);
    const RunSeg incl = run_block_segscan<kRunSegBlock>(RunSeg{e.w, e.head ? 1u : 0u}, wtot);
    if (threadIdx.x == kRunSegBlock - 1) agg[(size_t)blockIdx.y * nblk + blockIdx.x] = incl;
}

// agg[row][b] -> what lies in front of block b (exclusive scan, in place); one workgroup per row
static __global__ __launch_bounds__(kRunScanThreads) void k_run_seg_carry(RunSeg *agg, uint32_t nblk)
{
    __shared__ RunSeg wtot[kRunScanThreads / 64];
    RunSeg *a = agg + (size_t)blockIdx.x * nblk;
    const uint32_t per = (nblk + kRunScanThreads - 1) / kRunScanThreads;
    const uint32_t lo = threadIdx.x * per < nblk ? threadIdx.x * per : nblk, hi = lo + per < nblk ? lo + per : nblk;
    RunSeg mine{0u, 0u};
    for (uint32_t t = lo; t < hi; ++t) mine = run_combine(mine, a[t]);
    const RunSeg incl = run_block_segscan<kRunScanThreads>(mine, wtot);
    // what lies in front of this thread's stretch: the inclusive result of the thread before it
    __shared__ RunSeg all[kRunScanThreads];
    all[threadIdx.x] = incl;
    __syncthreads();
    RunSeg run = threadIdx.x ? all[threadIdx.x - 1] : RunSeg{0u, 0u};
    for (uint32_t t = lo; t < hi; ++t) {
        const RunSeg x = a[t];
        a[t] = run;
        run = run_combine(run, x);
    }
}

// run[row * cap + op] = the bin's value after the op (countminsketch.py:276-282); clamps -> ctr[PSK_CTR_SATURATED]
static __global__ __launch_bounds__(kRunSegBlock) void k_run_seg_apply(const uint2 *sorted, const int32_t *w, uint64_t base, uint32_t n, uint32_t cap, uint32_t nblk,
                                                                      const RunSeg *carry, const int32_t *table, uint64_t width, int32_t *run, long long *ctr)
{
    __shared__ RunSeg wtot[kRunSegBlock / 64];
    __shared__ uint32_t incl_s[kRunSegBlock];
    const RunElem e = run_seg_load(sorted, w, base, n, cap);
    const RunSeg front = carry[(size_t)blockIdx.y * nblk + blockIdx.x];
    const RunSeg incl = run_combine(front, run_block_segscan<kRunSegBlock>(RunSeg{e.w, e.head ? 1u : 0u}, wtot));
    incl_s[threadIdx.x] = incl.v;
    __syncthreads();
    bool clamped = false;
    if (e.valid) {
        const uint32_t before = e.head ? 0u : (threadIdx.x ? incl_s[threadIdx.x - 1] : front.v);  // the bin's weights in front of this op
        const int64_t t0 = table[(uint64_t)blockIdx.y * width + e.bin];
        int64_t prev = t0 + (int64_t)before;
        prev = prev > INT32_MAX ? INT32_MAX : prev;
        int64_t cur = prev + (int64_t)e.w;
        if (cur > INT32_MAX) { cur = INT32_MAX; clamped = true; }
        run[(size_t)blockIdx.y * cap + e.op] = (int32_t)cur;
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

// out[base + i] = query over the depth values of op i; WIDE: int64 results (mean-min), else int32
template <bool WIDE>
__global__ __launch_bounds__(kRunSegBlock) void k_run_query(const int32_t *run, const int32_t *w, const unsigned long long *tsum, const long long *st,
                                                            uint64_t base, uint32_t n, uint32_t cap, uint32_t depth, uint64_t width, int query, void *out)
{
    __shared__ unsigned long long wtot[kRunSegBlock / 64];
    const uint32_t i = blockIdx.x * kRunSegBlock + threadIdx.x;
    unsigned long long pre = 0;
    if (WIDE) {  // (uniform) elements_added after the op: only the mean-min query looks at it
        const unsigned long long x = i < n ? run_weight(w, base + i) : 0u;
        pre = tsum[blockIdx.x] + run_block_scan<kRunSegBlock>(x, wtot);
    }
    if (i >= n) return;
    const int64_t r = run_query_value(run, i, cap, depth, width, query, [&]() {
        long long els;
        if (__builtin_saddll_overflow(st[1], (long long)pre, &els)) els = INT64_MAX;
        return els;
    });
    if (WIDE) ((int64_t *)out)[base + i] = r;
    else ((int32_t *)out)[base + i] = (int32_t)r;
}

// int64 results of the sequential kernel (the fall-back of psk_cms_add_running) -> the entry's int32 / int64 output
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

// ================================================================== signed batches (psk_cms_update_running)
// w >= 0 adds w, w < 0 removes -w (countminsketch.py:267-321).  A bin may now fall as well as rise, so "one saturating sum" no longer
// describes it; what does is the op itself as a map.  Every op on a bin is x -> clamp(x + w, INT32_MIN, INT32_MAX) (add_alt clamps above
// only, remove_alt below only; the value in front of the op lies inside the rails, so the full clamp describes both), and maps of the form
//     (a, lo, hi):  x -> min(hi, max(lo, x + a))                                    lo <= hi
// are closed under composition: (a1, lo1, hi1) followed by (a2, lo2, hi2) is
//     (a1 + a2,  clamp(lo1 + a2, lo2, hi2),  clamp(hi1 + a2, lo2, hi2))
// (clamping is monotone, so it distributes over the min / max of the first map).  Composition of functions is associative: the value of
// a bin after op i is an inclusive segmented scan of MAPS in arrival order per (row, bin), applied to T0.  The hash, the stable sort and
// the commit pass are those of the add path; the scan passes below are the counterparts of k_run_seg_reduce / _carry / _apply.
// elements_added is the same thing on the int64 rails (:285-287, :317-319), not segmented.

// One stretch of a sorted row as a map: that of its LAST segment as far as the stretch covers it; head = a segment starts inside it.
// `a` is a plain sum: a chunk has at most 2^20 ops of |w| <= 2^31, so |a| <= 2^51 and int64 holds it without saturation; lo / hi are
// values a bin can take, int32.
struct RunMap {
    int64_t a;
    int32_t lo, hi;
    uint32_t head;
    static __device__ __forceinline__ RunMap identity() { return RunMap{0, INT32_MIN, INT32_MAX, 0u}; }  // (the identity on the values a bin can hold)
    static __device__ __forceinline__ RunMap of(int32_t w, bool head) { return RunMap{w, INT32_MIN, INT32_MAX, head ? 1u : 0u}; }
    __device__ __forceinline__ int32_t clamp(int64_t x) const { return (int32_t)(x < lo ? lo : (x > hi ? hi : x)); }
    __device__ __forceinline__ int32_t operator()(int32_t x) const { return clamp((int64_t)x + a); }
    // b follows a
    static __device__ __forceinline__ RunMap combine(const RunMap &a, const RunMap &b)
    {
        if (b.head) return RunMap{b.a, b.lo, b.hi, 1u};
        return RunMap{a.a + b.a, b.clamp((int64_t)a.lo + b.a), b.clamp((int64_t)a.hi + b.a), a.head};
    }
    static __device__ __forceinline__ RunMap shfl_up(const RunMap &x, int o)
    {
        return RunMap{(int64_t)__shfl_up((long long)x.a, o), __shfl_up(x.lo, o), __shfl_up(x.hi, o), (uint32_t)__shfl_up((int)x.head, o)};
    }
};

__device__ __forceinline__ long long run_sat_add64(long long a, long long b)
{
    long long s;
    if (__builtin_saddll_overflow(a, b, &s)) s = b > 0 ? INT64_MAX : INT64_MIN;
    return s;
}

// The same map on the int64 rails, for elements_added.  `a` as above (a tile, a chunk: |a| <= 2^51); lo + a may leave int64 and saturates,
// which the clamp that follows cannot tell from the true sum.
struct RunMap64 {
    long long a, lo, hi;
    static __device__ __forceinline__ RunMap64 identity() { return RunMap64{0, INT64_MIN, INT64_MAX}; }
    static __device__ __forceinline__ RunMap64 of(int32_t w) { return RunMap64{w, INT64_MIN, INT64_MAX}; }
    __device__ __forceinline__ long long clamp(long long x) const { return x < lo ? lo : (x > hi ? hi : x); }
    __device__ __forceinline__ long long operator()(long long x) const { return clamp(run_sat_add64(x, a)); }
    static __device__ __forceinline__ RunMap64 combine(const RunMap64 &a, const RunMap64 &b)
    {
        return RunMap64{a.a + b.a, b.clamp(run_sat_add64(a.lo, b.a)), b.clamp(run_sat_add64(a.hi, b.a))};
    }
    static __device__ __forceinline__ RunMap64 shfl_up(const RunMap64 &x, int o) { return RunMap64{__shfl_up(x.a, o), __shfl_up(x.lo, o), __shfl_up(x.hi, o)}; }
};

// inclusive scan of one map per thread over a workgroup of NT threads (run_block_segscan for M = RunMap / RunMap64); `wtot`: NT / 64 entries
template <int NT, class M>
__device__ __forceinline__ M run_block_mapscan(M x, M *wtot)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const M y = M::shfl_up(x, o);
        if (lane >= (uint32_t)o) x = M::combine(y, x);
    }
    if (lane == 63u) wtot[wave] = x;
    __syncthreads();
    M c = M::identity();
    for (uint32_t u = 0; u < wave; ++u) c = M::combine(c, wtot[u]);
    __syncthreads();  // (wtot may be reused by the caller)
    return M::combine(c, x);
}

// the signed weight of op i of the batch (nullptr: +1); every int32 is valid, INT32_MIN removes 2^31
__device__ __forceinline__ int32_t run_sweight(const int32_t *w, uint64_t i) { return w ? w[i] : 1; }

// ------------------------------------------------------------------ elements_added
// a 256-op tile of the batch as a map on elements_added, and the sum of its |w|
struct RunTile {
    RunMap64 f;
    unsigned long long abs;
};
static __global__ __launch_bounds__(kRunSegBlock) void k_run_stile(const int32_t *w, uint64_t base, uint32_t n, RunTile *tile)
{
    __shared__ RunMap64 wtot[kRunSegBlock / 64];
    __shared__ unsigned long long atot[kRunSegBlock / 64];
    const uint32_t i = blockIdx.x * kRunSegBlock + threadIdx.x;
    const int32_t x = i < n ? run_sweight(w, base + i) : 0;
    const RunMap64 incl = run_block_mapscan<kRunSegBlock>(RunMap64::of(x), wtot);
    const unsigned long long ab = run_block_scan<kRunSegBlock>((unsigned long long)(x < 0 ? -(long long)x : (long long)x), atot);
    if (threadIdx.x == kRunSegBlock - 1) tile[blockIdx.x] = RunTile{incl, ab};
}

// ONE workgroup: els[t] = elements_added in front of tile t; st[1] = in front of the chunk, st[0] = behind it (both rails, per op:
// countminsketch.py:285-287, :317-319); the handle's counters follow as k_cms_ordered leaves them (ctr[5] = elements_added, ctr[4] += sum |w|)
static __global__ __launch_bounds__(kRunScanThreads) void k_run_stile_scan(const RunTile *tile, uint32_t ntiles, long long *els, long long *st, long long els_in,
                                                                          int first, long long *ctr, long long *els_out)
{
    __shared__ RunMap64 wtot[kRunScanThreads / 64];
    __shared__ unsigned long long atot[kRunScanThreads / 64];
    __shared__ RunMap64 all[kRunScanThreads];
    const uint32_t per = (ntiles + kRunScanThreads - 1) / kRunScanThreads;
    const uint32_t lo = threadIdx.x * per < ntiles ? threadIdx.x * per : ntiles, hi = lo + per < ntiles ? lo + per : ntiles;
    RunMap64 mine = RunMap64::identity();
    unsigned long long ab = 0;
    for (uint32_t t = lo; t < hi; ++t) {
        mine = RunMap64::combine(mine, tile[t].f);
        ab += tile[t].abs;
    }
    const RunMap64 incl = run_block_mapscan<kRunScanThreads>(mine, wtot);
    const unsigned long long abs_all = run_block_scan<kRunScanThreads>(ab, atot);  // (< 2^52)
    all[threadIdx.x] = incl;
    __syncthreads();
    const long long start = first ? els_in : st[0];
    RunMap64 run = threadIdx.x ? all[threadIdx.x - 1] : RunMap64::identity();
    for (uint32_t t = lo; t < hi; ++t) {
        els[t] = run(start);
        run = RunMap64::combine(run, tile[t].f);
    }
    __syncthreads();  // every thread has read st[0]
    if (threadIdx.x == kRunScanThreads - 1) {
        const long long end = incl(start);
        st[1] = start;
        st[0] = end;
        ctr[5] = end;
        if (els_out) *els_out = end;
        const unsigned long long nb = (unsigned long long)ctr[4] + abs_all;
        ctr[4] = (nb < (unsigned long long)ctr[4] || nb > (1ULL << 62)) ? (1LL << 62) : (long long)nb;
    }
}

// ------------------------------------------------------------------ segmented scan of maps along a sorted row
struct RunSElem {
    uint32_t bin, op;
    int32_t w;
    bool valid, head;
};
// this thread's element of block blockIdx.x, row blockIdx.y; past the end: an identity segment of its own
__device__ __forceinline__ RunSElem run_sseg_load(const uint2 *sorted, const int32_t *w, uint64_t base, uint32_t n, uint32_t cap)
{
    const uint32_t i = blockIdx.x * kRunSegBlock + threadIdx.x;
    RunSElem e{0u, 0u, 0, i < n, true};
    if (e.valid) {
        const uint2 *row = sorted + (size_t)blockIdx.y * cap;
        const uint2 p = row[i];
        e.bin = p.x;
        e.op = p.y;
        e.head = i == 0 || row[i - 1].x != p.x;
        e.w = run_sweight(w, base + p.y);
    }
    return e;
}

// agg[row * nblk + block] = the block as one RunMap
static __global__ __launch_bounds__(kRunSegBlock) void k_run_sseg_reduce(const uint2 *sorted, const int32_t *w, uint64_t base, uint32_t n, uint32_t cap,
                                                                        uint32_t nblk, RunMap *agg)
{
    __shared__ RunMap wtot[kRunSegBlock / 64];
    const RunSElem e = run_sseg_load(sorted, w, base, n, cap);
    const RunMap incl = run_block_mapscan<kRunSegBlock>(RunMap::of(e.w, e.head), wtot);
    if (threadIdx.x == kRunSegBlock - 1) agg[(size_t)blockIdx.y * nblk + blockIdx.x] = incl;
}

// agg[row][b] -> what lies in front of block b (exclusive scan, in place); one workgroup per row
static __global__ __launch_bounds__(kRunScanThreads) void k_run_sseg_carry(RunMap *agg, uint32_t nblk)
{
    __shared__ RunMap wtot[kRunScanThreads / 64];
    __shared__ RunMap all[kRunScanThreads];
    RunMap *a = agg + (size_t)blockIdx.x * nblk;
    const uint32_t per = (nblk + kRunScanThreads - 1) / kRunScanThreads;
    const uint32_t lo = threadIdx.x * per < nblk ? threadIdx.x * per : nblk, hi = lo + per < nblk ? lo + per : nblk;
    RunMap mine = RunMap::identity();
    for (uint32_t t = lo; t < hi; ++t) mine = RunMap::combine(mine, a[t]);
    all[threadIdx.x] = run_block_mapscan<kRunScanThreads>(mine, wtot);
    __syncthreads();
    RunMap run = threadIdx.x ? all[threadIdx.x - 1] : RunMap::identity();
    for (uint32_t t = lo; t < hi; ++t) {
        const RunMap x = a[t];
        a[t] = run;
        run = RunMap::combine(run, x);
    }
}

// run[row * cap + op] = the bin's value after the op (countminsketch.py:276-282, :309-314); an op whose unclamped prev + w lies outside
// the rails -> ctr[PSK_CTR_SATURATED], the test of k_cms_ordered (a remove that lands exactly on INT32_MIN is no clamp)
static __global__ __launch_bounds__(kRunSegBlock) void k_run_sseg_apply(const uint2 *sorted, const int32_t *w, uint64_t base, uint32_t n, uint32_t cap, uint32_t nblk,
                                                                       const RunMap *carry, const int32_t *table, uint64_t width, int32_t *run, long long *ctr)
{
    __shared__ RunMap wtot[kRunSegBlock / 64];
    __shared__ RunMap incl_s[kRunSegBlock];
    const RunSElem e = run_sseg_load(sorted, w, base, n, cap);
    const RunMap front = carry[(size_t)blockIdx.y * nblk + blockIdx.x];
    incl_s[threadIdx.x] = RunMap::combine(front, run_block_mapscan<kRunSegBlock>(RunMap::of(e.w, e.head), wtot));
    __syncthreads();
    bool clamped = false;
    if (e.valid) {
        const RunMap before = e.head ? RunMap::identity() : (threadIdx.x ? incl_s[threadIdx.x - 1] : front);  // the bin's ops in front of this one
        const int64_t cur = (int64_t)before(table[(uint64_t)blockIdx.y * width + e.bin]) + (int64_t)e.w;
        clamped = cur > INT32_MAX || cur < INT32_MIN;
        run[(size_t)blockIdx.y * cap + e.op] = (int32_t)(cur > INT32_MAX ? INT32_MAX : (cur < INT32_MIN ? INT32_MIN : cur));
    }
    const unsigned long long c = __ballot(clamped);
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd((unsigned long long *)(ctr + 3), (unsigned long long)__popcll(c));
}

// ------------------------------------------------------------------ query
// k_run_query with the signed prefix: els[tile] = elements_added in front of the tile, the ops of the tile applied to it one map after the other
template <bool WIDE>
__global__ __launch_bounds__(kRunSegBlock) void k_run_squery(const int32_t *run, const int32_t *w, const long long *els, uint64_t base, uint32_t n, uint32_t cap,
                                                             uint32_t depth, uint64_t width, int query, void *out)
{
    __shared__ RunMap64 wtot[kRunSegBlock / 64];
    const uint32_t i = blockIdx.x * kRunSegBlock + threadIdx.x;
    RunMap64 pre = RunMap64::identity();
    if (WIDE) pre = run_block_mapscan<kRunSegBlock>(RunMap64::of(i < n ? run_sweight(w, base + i) : 0), wtot);  // (uniform)
    if (i >= n) return;
    const int64_t r = run_query_value(run, i, cap, depth, width, query, [&]() { return pre(els[blockIdx.x]); });
    if (WIDE) ((int64_t *)out)[base + i] = r;
    else ((int32_t *)out)[base + i] = (int32_t)r;
}

}  // namespace psk

// ------------------------------------------------------------------ host side (psk_running.hip; the hash launch is psk_capi.hip's)
struct psk_sketch;
// where the buffers of one chunk lie in the handle's scratch (psk_sketch::s_part), for chunks of at most `cap` ops
struct RunArena {
    uint32_t cap, passes;         // ops per chunk; radix passes per row
    uint32_t *bins;               // [depth][cap]   the hash kernel's output; shares its memory with pairs[1]
    uint2 *pairs[2];              // [depth][cap]   (bin, op) before / behind a sort pass
    int32_t *run;                 // [depth][cap]   value of row s after op i
    uint32_t *hist;               // [depth][256][tiles]
    psk::RunSeg *agg;             // [depth][blocks]
    unsigned long long *tsum;     // [blocks]       (signed batches: elements_added in front of every tile, as int64)
    long long *st;                // [0] elements_added behind the chunk in hand, [1] in front of it
    psk::RunMap *magg;            // [depth][blocks]  signed batches only: the block aggregates as maps, in place of agg
    psk::RunTile *tile;           // [blocks]         signed batches only
};
// sizes the arena for a batch of n ops and grows the scratch; sgn: a signed batch (magg and tile in place of agg)
__attribute__((visibility("hidden"))) int cms_running_arena(psk_sketch *s, uint64_t n, RunArena *a, bool sgn = false);
// everything behind the hash kernel for the chunk [base, base + n) of the batch: a.bins is filled; w / out are the BATCH's arrays
__attribute__((visibility("hidden"))) int cms_running_chunk(psk_sketch *s, const RunArena &a, const int32_t *w, uint64_t base, uint32_t n, bool first,
                                                            int64_t els_in, int query, void *out, int64_t *els_out, hipStream_t st);
// the same for a chunk of a signed batch (arena sized with sgn = true)
__attribute__((visibility("hidden"))) int cms_running_chunk_signed(psk_sketch *s, const RunArena &a, const int32_t *w, uint64_t base, uint32_t n, bool first,
                                                                   int64_t els_in, int query, void *out, int64_t *els_out, hipStream_t st);
