// psk_cbf_running.hip -- host side of the exact ordered CountingBloomFilter batches (psk_cbf_running.hpp): scratch layout and the launches
// of one chunk, up to its verdict.
#include "psk_host.hpp"
#include "psk_cbf_running.hpp"

static_assert(sizeof(CbfMap) == kCbfRunMapBytes, "the layout's map size");
static_assert(kCbfTallyWords * 8 == kCbfRunTallyBytes, "the layout's tally size");
static_assert(kCbfRunChunk == kRunChunk && kCbfRunCells == kRunCells && kCbfRunSortTile == kRunSortTile && kCbfRunSegBlock == kRunSegBlock &&
                  kCbfRunMaxK == (uint32_t)kMaxKOrdered,
              "the layout's constants are those of the passes");

int cbf_running_arena(psk_sketch *s, uint64_t n, CbfRunArena *a)
{
    cbf_running_layout(n, s->k, s->m, &a->l);
    PSK_TRY(ensure(s->s_part, a->l.bytes));
    char *p = (char *)s->s_part.p;
    a->pairs[0] = (uint2 *)(p + a->l.off_pairs[0]);
    a->pairs[1] = (uint2 *)(p + a->l.off_pairs[1]);
    a->bins = (uint32_t *)a->pairs[1];
    a->before = (uint32_t *)(p + a->l.off_before);
    a->hist = (uint32_t *)(p + a->l.off_hist);
    a->agg = (CbfMap *)(p + a->l.off_agg);
    a->tally = (unsigned long long *)(p + a->l.off_tally);
    return PSK_OK;
}

template <bool ADDONLY>
static int cbf_running_chunk_t(psk_sketch *s, const CbfRunArena &a, const int32_t *w, uint64_t base, uint32_t n, uint32_t *out, hipStream_t st, bool *clean)
{
    const uint32_t k = s->k;
    const uint32_t E = n * k;  // (<= cap * k < 2^24)
    const uint32_t tiles = (E + kRunSortTile - 1) / kRunSortTile, blocks = (E + kRunSegBlock - 1) / kRunSegBlock, opblocks = (n + kRunSegBlock - 1) / kRunSegBlock;
    uint32_t *flag = (uint32_t *)s->s_flag.p;
    HIP_TRY(hipMemsetAsync(flag, 0, 4, st));
    HIP_TRY(hipMemsetAsync(a.tally, 0, kCbfRunTallyBytes, st));
    // (bin, e) in order of bin, arrival order inside a bin: one row of E elements
    const uint2 *sorted = segscan_sort(a.pairs, a.hist, 1, E, 0, tiles, a.l.passes, st);
    uint32_t *fin = (uint32_t *)a.pairs[a.l.passes & 1];  // (the buffer the last pass read: free from here on)
    hipLaunchKernelGGL((k_cbfr_reduce<ADDONLY>), dim3(blocks), dim3(kRunSegBlock), 0, st, sorted, w, base, E, k, a.agg);
    hipLaunchKernelGGL((k_seg_carry<CbfMap>), dim3(1), dim3(kRunScanThreads), 0, st, a.agg, blocks);
    hipLaunchKernelGGL((k_cbfr_apply<ADDONLY>), dim3(blocks), dim3(kRunSegBlock), 0, st, sorted, w, base, E, k, (const CbfMap *)a.agg, (const uint32_t *)s->table, a.before,
                       fin, flag);
    hipLaunchKernelGGL((k_cbfr_perop<ADDONLY>), dim3(opblocks), dim3(kRunSegBlock), 0, st, (const uint32_t *)a.before, w, base, n, k, out, flag, a.tally);
    HIP_TRY(hipGetLastError());
    // the verdict: one word
    uint32_t verdict = 1;
    HIP_TRY(hipMemcpyAsync(&verdict, flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *clean = verdict == 0;
    if (*clean) hipLaunchKernelGGL(k_cbfr_commit, dim3(blocks), dim3(kRunSegBlock), 0, st, sorted, E, (const uint32_t *)fin, (uint32_t *)s->table);
    hipLaunchKernelGGL(k_cbfr_book, dim3(1), dim3(1), 0, st, (const unsigned long long *)a.tally, (unsigned long long *)s->ctr, k, *clean ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

int cbf_running_chunk(psk_sketch *s, const CbfRunArena &a, const int32_t *w, uint64_t base, uint32_t n, bool addonly, uint32_t *out, hipStream_t st, bool *clean)
{
    if (n == 0 || n > a.l.cap || s->k == 0 || s->k > (uint32_t)kMaxKOrdered || (uint64_t)n * s->k > a.l.cells)
        return fail(PSK_EINVAL, "ordered CBF batch: chunk of %u ops, the scratch holds %u", n, a.l.cap);
    PSK_TRY(ensure(s->s_flag, 8));
    return addonly ? cbf_running_chunk_t<true>(s, a, w, base, n, out, st, clean) : cbf_running_chunk_t<false>(s, a, w, base, n, out, st, clean);
}
