// psk_running.hip -- host side of the exact ordered CountMinSketch add and signed update (psk_running.hpp): scratch layout and the launches of one chunk.
#include "psk_host.hpp"
#include "psk_running.hpp"

static uint64_t up16(uint64_t b) { return (b + 15) & ~15ULL; }

int cms_running_arena(psk_sketch *s, uint64_t n, RunArena *a, bool sgn)
{
    const uint32_t depth = s->k;
    uint64_t cap = kRunCells / depth;
    if (cap > kRunChunk) cap = kRunChunk;
    if (cap > n) cap = n;
    cap = (cap + kRunSortTile - 1) / kRunSortTile * kRunSortTile;  // (>= one tile; depth <= 64: at most 2^17 + 2047 ops per chunk then)
    a->cap = (uint32_t)cap;
    uint32_t bits = 0;
    while (bits < 32 && (1ULL << bits) < s->m) ++bits;  // bins < width <= 2^32
    a->passes = bits <= 8 ? 1u : (bits + 7) / 8;
    const uint64_t cells = cap * depth, tiles = cap / kRunSortTile, blocks = cap / kRunSegBlock;
    const uint64_t b_pairs = up16(cells * 8), b_run = up16(cells * 4), b_hist = up16((uint64_t)depth * 256 * tiles * 4),
                   b_agg = up16((uint64_t)depth * blocks * (sgn ? sizeof(RunMap) : sizeof(RunSeg))), b_tsum = up16(blocks * 8),
                   b_tile = sgn ? up16(blocks * sizeof(RunTile)) : 0;
    PSK_TRY(ensure(s->s_part, 2 * b_pairs + b_run + b_hist + b_agg + b_tsum + b_tile + 16));
    char *p = (char *)s->s_part.p;
    a->pairs[0] = (uint2 *)p;
    a->pairs[1] = (uint2 *)(p + b_pairs);
    a->bins = (uint32_t *)a->pairs[1];
    p += 2 * b_pairs;
    a->run = (int32_t *)p;
    p += b_run;
    a->hist = (uint32_t *)p;
    p += b_hist;
    a->agg = sgn ? nullptr : (RunSeg *)p;
    a->magg = sgn ? (RunMap *)p : nullptr;
    p += b_agg;
    a->tsum = (unsigned long long *)p;
    p += b_tsum;
    a->tile = sgn ? (RunTile *)p : nullptr;
    p += b_tile;
    a->st = (long long *)p;
    return PSK_OK;
}

// per row: (bin, op) in order of bin, arrival order inside a bin; -> the sorted pairs
static const uint2 *run_sort_rows(const RunArena &a, uint32_t depth, uint32_t n, uint32_t tiles, hipStream_t st)
{
    const uint32_t cap = a.cap;
    const dim3 gsort(tiles, depth);
    const uint2 *sorted = nullptr;
    for (uint32_t p = 0; p < a.passes; ++p) {
        const uint2 *src = a.pairs[(p + 1) & 1];  // (pass 0 reads a.bins, which lies there)
        uint2 *dst = a.pairs[p & 1];
        if (p == 0) hipLaunchKernelGGL((k_run_sort_hist<true>), gsort, dim3(64), 0, st, (const uint32_t *)a.bins, src, a.hist, n, cap, tiles, 8 * p);
        else hipLaunchKernelGGL((k_run_sort_hist<false>), gsort, dim3(64), 0, st, (const uint32_t *)nullptr, src, a.hist, n, cap, tiles, 8 * p);
        hipLaunchKernelGGL(k_run_sort_scan, dim3(depth), dim3(kRunScanThreads), 0, st, a.hist, 256 * tiles);
        if (p == 0) hipLaunchKernelGGL((k_run_sort_scatter<true>), gsort, dim3(64), 0, st, (const uint32_t *)a.bins, src, dst, (const uint32_t *)a.hist, n, cap, tiles, 8 * p);
        else hipLaunchKernelGGL((k_run_sort_scatter<false>), gsort, dim3(64), 0, st, (const uint32_t *)nullptr, src, dst, (const uint32_t *)a.hist, n, cap, tiles, 8 * p);
        sorted = dst;
    }
    return sorted;
}

int cms_running_chunk(psk_sketch *s, const RunArena &a, const int32_t *w, uint64_t base, uint32_t n, bool first, int64_t els_in, int query, void *out,
                      int64_t *els_out, hipStream_t st)
{
    if (n == 0 || n > a.cap) return fail(PSK_EINVAL, "ordered add: chunk of %u ops, the scratch holds %u", n, a.cap);
    const uint32_t depth = s->k, cap = a.cap;
    const uint32_t tiles = (n + kRunSortTile - 1) / kRunSortTile, blocks = (n + kRunSegBlock - 1) / kRunSegBlock;
    // elements_added in front of every 256-op tile, and behind the chunk
    hipLaunchKernelGGL(k_run_wsum, dim3(blocks), dim3(kRunSegBlock), 0, st, w, base, n, a.tsum, s->ctr);
    hipLaunchKernelGGL(k_run_wscan, dim3(1), dim3(kRunScanThreads), 0, st, a.tsum, blocks, a.st, (long long)els_in, first ? 1 : 0, s->ctr, (long long *)els_out);
    const uint2 *sorted = run_sort_rows(a, depth, n, tiles, st);
    // the running value of every (row, bin) along the sorted row, the table, the per-op values
    const dim3 gseg(blocks, depth);
    hipLaunchKernelGGL(k_run_seg_reduce, gseg, dim3(kRunSegBlock), 0, st, sorted, w, base, n, cap, blocks, a.agg);
    hipLaunchKernelGGL(k_run_seg_carry, dim3(depth), dim3(kRunScanThreads), 0, st, a.agg, blocks);
    hipLaunchKernelGGL(k_run_seg_apply, gseg, dim3(kRunSegBlock), 0, st, sorted, w, base, n, cap, blocks, (const RunSeg *)a.agg, (const int32_t *)s->table, s->m, a.run,
                       s->ctr);
    hipLaunchKernelGGL(k_run_seg_commit, gseg, dim3(kRunSegBlock), 0, st, sorted, n, cap, (const int32_t *)a.run, (int32_t *)s->table, s->m);
    if (out) {
        if (query == PSK_Q_MEANMIN)
            hipLaunchKernelGGL((k_run_query<true>), dim3(blocks), dim3(kRunSegBlock), 0, st, (const int32_t *)a.run, w, (const unsigned long long *)a.tsum,
                               (const long long *)a.st, base, n, cap, depth, s->m, query, out);
        else
            hipLaunchKernelGGL((k_run_query<false>), dim3(blocks), dim3(kRunSegBlock), 0, st, (const int32_t *)a.run, w, (const unsigned long long *)a.tsum,
                               (const long long *)a.st, base, n, cap, depth, s->m, query, out);
    }
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

int cms_running_chunk_signed(psk_sketch *s, const RunArena &a, const int32_t *w, uint64_t base, uint32_t n, bool first, int64_t els_in, int query, void *out,
                             int64_t *els_out, hipStream_t st)
{
    if (n == 0 || n > a.cap || !a.magg) return fail(PSK_EINVAL, "ordered update: chunk of %u ops, the scratch holds %u", n, a.magg ? a.cap : 0u);
    const uint32_t depth = s->k, cap = a.cap;
    const uint32_t tiles = (n + kRunSortTile - 1) / kRunSortTile, blocks = (n + kRunSegBlock - 1) / kRunSegBlock;
    long long *els = (long long *)a.tsum;
    // elements_added in front of every 256-op tile, and behind the chunk
    hipLaunchKernelGGL(k_run_stile, dim3(blocks), dim3(kRunSegBlock), 0, st, w, base, n, a.tile);
    hipLaunchKernelGGL(k_run_stile_scan, dim3(1), dim3(kRunScanThreads), 0, st, (const RunTile *)a.tile, blocks, els, a.st, (long long)els_in, first ? 1 : 0, s->ctr,
                       (long long *)els_out);
    const uint2 *sorted = run_sort_rows(a, depth, n, tiles, st);
    // the map in front of every op along the sorted row, applied to the table: the per-op values; then the table
    const dim3 gseg(blocks, depth);
    hipLaunchKernelGGL(k_run_sseg_reduce, gseg, dim3(kRunSegBlock), 0, st, sorted, w, base, n, cap, blocks, a.magg);
    hipLaunchKernelGGL(k_run_sseg_carry, dim3(depth), dim3(kRunScanThreads), 0, st, a.magg, blocks);
    hipLaunchKernelGGL(k_run_sseg_apply, gseg, dim3(kRunSegBlock), 0, st, sorted, w, base, n, cap, blocks, (const RunMap *)a.magg, (const int32_t *)s->table, s->m, a.run,
                       s->ctr);
    hipLaunchKernelGGL(k_run_seg_commit, gseg, dim3(kRunSegBlock), 0, st, sorted, n, cap, (const int32_t *)a.run, (int32_t *)s->table, s->m);
    if (out) {
        if (query == PSK_Q_MEANMIN)
            hipLaunchKernelGGL((k_run_squery<true>), dim3(blocks), dim3(kRunSegBlock), 0, st, (const int32_t *)a.run, w, (const long long *)els, base, n, cap, depth, s->m,
                               query, out);
        else
            hipLaunchKernelGGL((k_run_squery<false>), dim3(blocks), dim3(kRunSegBlock), 0, st, (const int32_t *)a.run, w, (const long long *)els, base, n, cap, depth, s->m,
                               query, out);
    }
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}
