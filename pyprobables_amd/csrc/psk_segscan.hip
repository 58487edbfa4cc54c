// psk_segscan.hip -- host side of the ordered batches' skeleton (psk_segscan.hpp): the passes of the sort.
#include "psk_host.hpp"
#include "psk_segscan.hpp"

// Exclusive scan of the 256 * ntiles counts of a row, in (digit, tile) order; one workgroup per row.  This is stretch_scan for a plain sum,
// written out because a sum can take what lies in front of a stretch as `inclusive - mine`: the kernel is more than half of an ordered
// CountMinSketch call, and k_seg_carry<Sum<uint32_t>> in its place ran 2 us of 105 longer (profiles/ordered_scan_refactor.txt).
static __global__ __launch_bounds__(kRunScanThreads) void k_run_sort_scan(uint32_t *hist, uint32_t len)
{
    __shared__ Sum<uint32_t> wtot[kRunScanThreads / 64];
    uint32_t *h = hist + (size_t)blockIdx.x * len;
    const uint32_t per = (len + kRunScanThreads - 1) / kRunScanThreads;
    const uint32_t lo = threadIdx.x * per < len ? threadIdx.x * per : len, hi = lo + per < len ? lo + per : len;
    uint32_t mine = 0;
    for (uint32_t t = lo; t < hi; ++t) mine += h[t];
    uint32_t run = block_scan<kRunScanThreads>(Sum<uint32_t>{mine}, wtot).v - mine;
    for (uint32_t t = lo; t < hi; ++t) {
        const uint32_t x = h[t];
        h[t] = run;
        run += x;
    }
}

const uint2 *segscan_sort(uint2 *const pairs[2], uint32_t *hist, uint32_t rows, uint32_t n, uint32_t cap, uint32_t tiles, uint32_t passes, hipStream_t st)
{
    const dim3 gsort(tiles, rows);
    const uint32_t *bins = (const uint32_t *)pairs[1];
    const uint2 *sorted = nullptr;
    for (uint32_t p = 0; p < passes; ++p) {
        const uint2 *src = pairs[(p + 1) & 1];
        uint2 *dst = pairs[p & 1];
        auto pass = [&](auto first) {
            constexpr bool FIRST = decltype(first)::value;
            hipLaunchKernelGGL((k_run_sort_hist<FIRST>), gsort, dim3(64), 0, st, bins, src, hist, n, cap, tiles, 8 * p);
            hipLaunchKernelGGL(k_run_sort_scan, dim3(rows), dim3(kRunScanThreads), 0, st, hist, 256 * tiles);
            hipLaunchKernelGGL((k_run_sort_scatter<FIRST>), gsort, dim3(64), 0, st, bins, src, dst, (const uint32_t *)hist, n, cap, tiles, 8 * p);
        };
        if (p == 0) pass(std::true_type{});
        else pass(std::false_type{});
        sorted = dst;
    }
    return sorted;
}
