// psk_segscan.hpp -- the skeleton of the exact ordered batches (psk_running.hpp, psk_cbf_running.hpp), free of any sketch: a stable LSD radix
// sort of (bin, position) and a scan of an associative value along the sorted run, reduce-then-scan with a single-workgroup second level
// (no spinning, no inter-workgroup flags).  A sketch brings its algebra; the passes are
//   k_run_sort_hist    digit counts per 2048-element tile (one wave per tile)
//   k_run_sort_scan    exclusive scan of the (digit, tile) counts in that order (psk_segscan.hip)
//   k_run_sort_scatter rank inside the tile = lanes of the same digit below me (8 ballots) + what earlier 64-element steps of the tile
//                      counted (LDS, one counter per digit): equal digits keep their order, so arrival order inside a bin is free
//   <sketch>_reduce    per 256-element block: block_scan of the elements' values, the last thread stores the block as one value
//   k_seg_carry        one workgroup per row scans those: what lies in front of every block
//   <sketch>_apply     redoes the block's scan behind its carry and applies it to the table's values
//
// The contract of a scan value M (RunSeg, RunMap, RunMap64, RunTile, RunSum, CbfMap, Sum<T>):
//   M::identity()       combine(identity, x) = combine(x, identity) = x
//   M::combine(a, b)    b FOLLOWS a; associative.  A segmented value carries `head` (a segment starts inside the stretch the value stands
//                       for) and means the LAST segment of its stretch as far as the stretch covers it: a head in b cuts, combine(a, b) = b
//   seg_shfl_up(x, o)   x of the lane o below
// identity and combine are __host__ __device__ and plain C++, so a CPU program can run the algebra (tests/host/segscan_algebra_main.cpp);
// the shuffle is a device-only overload beside the struct.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace psk {

constexpr uint32_t kRunSortTile = 2048;        // elements per sort tile (one wave: 32 steps of 64)
constexpr uint32_t kRunSegBlock = 256;         // elements per block of the scan
constexpr int kRunScanThreads = 1024;          // the single-workgroup second levels

// a plain sum as a scan value
template <class T>
struct Sum {
    T v;
    static __host__ __device__ __forceinline__ Sum identity() { return Sum{0}; }
    static __host__ __device__ __forceinline__ Sum combine(const Sum &a, const Sum &b) { return Sum{a.v + b.v}; }
};
template <class T>
__device__ __forceinline__ Sum<T> seg_shfl_up(const Sum<T> &x, int o) { return Sum<T>{__shfl_up(x.v, o)}; }

// inclusive scan of one value per thread over a workgroup of NT threads (NT / 64 waves); `wtot`: NT / 64 entries of LDS.  *excl (if asked
// for) = everything in front of this thread: the inclusive value of the lane below behind the waves in front, by one more shuffle -- valid for
// any M, where a difference `inclusive - mine` would do for sums only
template <int NT, class M>
__device__ __forceinline__ M block_scan(M x, M *wtot, M *excl = nullptr)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const M y = seg_shfl_up(x, o);
        if (lane >= (uint32_t)o) x = M::combine(y, x);
    }
    if (lane == 63u) wtot[wave] = x;
    __syncthreads();
    M c = M::identity();
    for (uint32_t u = 0; u < wave; ++u) c = M::combine(c, wtot[u]);
    __syncthreads();  // (wtot may be reused by the caller)
    if (excl) {
        const M below = seg_shfl_up(x, 1);
        *excl = lane ? M::combine(c, below) : c;
    }
    return M::combine(c, x);
}

// ONE workgroup of NT threads scans n items exclusively: rd(t) reads item t, wr(t, f) rewrites it with f = everything in front of it.
// Every thread takes a stretch of ceil(n / NT) items (an empty one past the end), one block scan runs over the threads, and what lies in
// front of a stretch is that scan's exclusive value.  A thread writes only items it has read itself, so wr may overwrite what rd reads.
// Returns everything up to the end of this thread's stretch: in thread NT - 1 the total of the n items.
template <int NT, class M, class Rd, class Wr>
__device__ __forceinline__ M stretch_scan(uint32_t n, Rd rd, Wr wr)
{
    __shared__ M wtot[NT / 64];
    const uint32_t per = (n + NT - 1) / NT;
    const uint32_t lo = threadIdx.x * per < n ? threadIdx.x * per : n, hi = lo + per < n ? lo + per : n;
    M mine = M::identity();
    for (uint32_t t = lo; t < hi; ++t) mine = M::combine(mine, rd(t));
    M run;
    const M incl = block_scan<NT>(mine, wtot, &run);
    for (uint32_t t = lo; t < hi; ++t) {
        const M x = rd(t);
        wr(t, run);
        run = M::combine(run, x);
    }
    return incl;
}

// a[row][t] -> what lies in front of item t of its row of n (exclusive scan, in place); one workgroup per row
template <class M>
__global__ __launch_bounds__(kRunScanThreads) void k_seg_carry(M *a, uint32_t n)
{
    M *row = a + (size_t)blockIdx.x * n;
    stretch_scan<kRunScanThreads, M>(n, [&](uint32_t t) { return row[t]; }, [&](uint32_t t, const M &f) { row[t] = f; });
}

// ------------------------------------------------------------------ stable radix sort of (bin, position), one row per blockIdx.y
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

// element e of a row: the first pass reads the bins (the position is e itself), later passes the pairs of the pass before
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

}  // namespace psk

// The sort's passes (psk_segscan.hip) for `rows` rows of n elements, row r at [r * cap, r * cap + n) of every buffer (one row: cap 0), in
// `passes` passes of 8 bits: tiles = ceil(n / kRunSortTile), hist holds rows * 256 * tiles counts.  The bins lie in pairs[1] as uint32 (the
// first pass reads them and writes pairs[0]).  -> the buffer that holds (bin, position) in order of bin, positions ascending inside a bin.
__attribute__((visibility("hidden"))) const uint2 *segscan_sort(uint2 *const pairs[2], uint32_t *hist, uint32_t rows, uint32_t n, uint32_t cap, uint32_t tiles,
                                                                uint32_t passes, hipStream_t st);
