// psk_running.hip -- host side of the exact ordered CountMinSketch batches (psk_running.hpp): scratch layout and the launches of one chunk.
#include "psk_host.hpp"
#include "psk_running.hpp"

static uint64_t up16(uint64_t b) { return (b + 15) & ~15ULL; }

template <class Ops>
int cms_running_arena(psk_sketch *s, uint64_t n, RunArena *a)
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
    constexpr bool in_place = sizeof(typename Ops::Tile) == sizeof(long long);
    const uint64_t b_pairs = up16(cells * 8), b_run = up16(cells * 4), b_hist = up16((uint64_t)depth * 256 * tiles * 4),
                   b_agg = up16((uint64_t)depth * blocks * sizeof(typename Ops::Bin)), b_els = up16(blocks * 8),
                   b_tile = in_place ? 0 : up16(blocks * sizeof(typename Ops::Tile));
    PSK_TRY(ensure(s->s_part, 2 * b_pairs + b_run + b_hist + b_agg + b_els + b_tile + 16));
    char *p = (char *)s->s_part.p;
    a->pairs[0] = (uint2 *)p;
    a->pairs[1] = (uint2 *)(p + b_pairs);
    a->bins = (uint32_t *)a->pairs[1];
    p += 2 * b_pairs;
    a->run = (int32_t *)p;
    p += b_run;
    a->hist = (uint32_t *)p;
    p += b_hist;
    a->agg = p;
    p += b_agg;
    a->els = (long long *)p;
    p += b_els;
    a->tile = in_place ? (void *)a->els : (void *)p;
    p += b_tile;
    a->st = (long long *)p;
    return PSK_OK;
}

template <class Ops>
int cms_running_chunk(psk_sketch *s, const RunArena &a, const int32_t *w, uint64_t base, uint32_t n, bool first, int64_t els_in, int query, void *out,
                      int64_t *els_out, hipStream_t st)
{
    using Bin = typename Ops::Bin;
    using Tile = typename Ops::Tile;
    if (n == 0 || n > a.cap) return fail(PSK_EINVAL, "ordered batch: chunk of %u ops, the scratch holds %u", n, a.cap);
    const uint32_t depth = s->k, cap = a.cap;
    const uint32_t tiles = (n + kRunSortTile - 1) / kRunSortTile, blocks = (n + kRunSegBlock - 1) / kRunSegBlock;
    // elements_added in front of every 256-op tile, and behind the chunk
    hipLaunchKernelGGL((k_run_tile<Ops>), dim3(blocks), dim3(kRunSegBlock), 0, st, w, base, n, (Tile *)a.tile, s->ctr);
    hipLaunchKernelGGL((k_run_tile_scan<Ops>), dim3(1), dim3(kRunScanThreads), 0, st, (const Tile *)a.tile, blocks, a.els, a.st, (long long)els_in, first ? 1 : 0, s->ctr,
                       (long long *)els_out);
    // per row: (bin, op) in order of bin, arrival order inside a bin
    const uint2 *sorted = segscan_sort(a.pairs, a.hist, depth, n, cap, tiles, a.passes, st);
    // the running value of every (row, bin) along the sorted row, applied to the table: the per-op values; then the table
    const dim3 gseg(blocks, depth);
    hipLaunchKernelGGL((k_run_seg_reduce<Ops>), gseg, dim3(kRunSegBlock), 0, st, sorted, w, base, n, cap, blocks, (Bin *)a.agg);
    hipLaunchKernelGGL((k_seg_carry<Bin>), dim3(depth), dim3(kRunScanThreads), 0, st, (Bin *)a.agg, blocks);
    hipLaunchKernelGGL((k_run_seg_apply<Ops>), gseg, dim3(kRunSegBlock), 0, st, sorted, w, base, n, cap, blocks, (const Bin *)a.agg, (const int32_t *)s->table, s->m, a.run,
                       s->ctr);
    hipLaunchKernelGGL(k_run_seg_commit, gseg, dim3(kRunSegBlock), 0, st, sorted, n, cap, (const int32_t *)a.run, (int32_t *)s->table, s->m);
    if (out) {
        if (query == PSK_Q_MEANMIN)
            hipLaunchKernelGGL((k_run_query<Ops, true>), dim3(blocks), dim3(kRunSegBlock), 0, st, (const int32_t *)a.run, w, (const long long *)a.els, base, n, cap, depth,
                               s->m, query, out);
        else
            hipLaunchKernelGGL((k_run_query<Ops, false>), dim3(blocks), dim3(kRunSegBlock), 0, st, (const int32_t *)a.run, w, (const long long *)a.els, base, n, cap, depth,
                               s->m, query, out);
    }
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

template int cms_running_arena<RunAddOps>(psk_sketch *, uint64_t, RunArena *);
template int cms_running_arena<RunSignedOps>(psk_sketch *, uint64_t, RunArena *);
template int cms_running_chunk<RunAddOps>(psk_sketch *, const RunArena &, const int32_t *, uint64_t, uint32_t, bool, int64_t, int, void *, int64_t *, hipStream_t);
template int cms_running_chunk<RunSignedOps>(psk_sketch *, const RunArena &, const int32_t *, uint64_t, uint32_t, bool, int64_t, int, void *, int64_t *, hipStream_t);
