// psk_bloom.hip -- the BloomFilter entry points of the C ABI (include/psk.h): direct kernels of psk_device.hpp for small batches, the
// partitioned launchers (psk_part_bloom_*.hip) for large ones.
#include "psk_stage.hpp"

// ------------------------------------------------------------- BloomFilter
extern "C" int psk_bloom_add(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                             uint32_t key_len, int where, void *stream)
{
    CHECK_HANDLE(s, PSK_KIND_BLOOM);
    PSK_TRY(check_hashes_width(s, layout, key_len));
    hipStream_t st = (hipStream_t)stream;
    Batch b;
    PSK_TRY(stage_batch(s->s_keys, s->s_offs, layout, data, offsets, n, key_len, where, st, &b));
    bool done = false;
    if (!s->pend.active) PSK_TRY(bloom_add_partitioned(s, b, st, &done));  // (a pending split lookup owns the bucket buffer)
    if (done) return finish(where, nullptr, st);
    PSK_TRY(clear_materialize(s, st));  // (the partitioned insert consumes a deferred clear; the direct kernel ORs into the table)
    return direct_apply(s, b, data, where, true, nullptr, st, [&](auto P) { return BloomAdd<P.value>{(uint32_t *)s->table, s->md, s->k}; });
}

extern "C" int psk_bloom_check(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                               uint32_t key_len, int where, uint8_t *out, void *stream)
{
    CHECK_HANDLE(s, PSK_KIND_BLOOM);
    PSK_TRY(check_hashes_width(s, layout, key_len));
    if (n && !out) return fail(PSK_EINVAL, "out is NULL");
    hipStream_t st = (hipStream_t)stream;
    PSK_TRY(clear_materialize(s, st));
    Batch b;
    PSK_TRY(stage_batch(s->s_keys, s->s_offs, layout, data, offsets, n, key_len, where, st, &b));
    OutBuf o;
    PSK_TRY(stage_out(s->s_out, out, n, where, &o));
    {
        bool done = false;
        if (!s->pend.active) PSK_TRY(bloom_check_partitioned(s, b, (uint8_t *)o.dev, st, &done));
        if (done) return finish(where, &o, st);
    }
    return direct_apply(s, b, data, where, o.is_pinned, &o, st,
                        [&](auto P) { return BloomCheck<P.value>{(const uint32_t *)s->table, s->md, s->k, (uint8_t *)o.dev}; });
}

extern "C" int psk_bloom_indices(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                                uint32_t key_len, int where, uint32_t *out_idx_dev, void *stream)
{
    CHECK_HANDLE(s, PSK_KIND_BLOOM);
    PSK_TRY(check_hashes_width(s, layout, key_len));
    if (n && !out_idx_dev) return fail(PSK_EINVAL, "out_idx_dev is NULL");
    if (s->m > (1ULL << 32)) return fail(PSK_EINVAL, "bit indices are 32-bit: m must be <= 2^32");
    hipStream_t st = (hipStream_t)stream;
    Batch b;
    PSK_TRY(stage_batch(s->s_keys, s->s_offs, layout, data, offsets, n, key_len, where, st, &b));
    PSK_TRY(with_source(b, [&](auto src) {
        return with_pow2(s, [&](auto P) { return launch_apply(src, BloomIndexOut<P.value>{out_idx_dev, s->md, s->k}, n, st); });
    }));
    return finish(where, nullptr, st);
}

// Split lookup (see include/psk.h): begin = hash + partition (never reads the table), finish = probe.
extern "C" int psk_bloom_check_begin(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                                     uint32_t key_len, void *stream)
{
    CHECK_HANDLE(s, PSK_KIND_BLOOM);
    PSK_TRY(check_hashes_width(s, layout, key_len));
    if (s->pend.active) return fail(PSK_EINVAL, "a split lookup is already pending on this handle");
    if (n && !data) return fail(PSK_EINVAL, "keys are NULL");
    Batch b;
    PSK_TRY(stage_batch(s->s_keys, s->s_offs, layout, data, offsets, n, key_len, PSK_DEVICE, (hipStream_t)stream, &b));  // (device keys: checked, not copied)
    PSK_TRY(clear_materialize(s, (hipStream_t)stream));  // (begin never reads the table, the finish on the same stream does)
    return bloom_check_begin_partitioned(s, b, (hipStream_t)stream);
}

extern "C" int psk_bloom_check_finish(psk_sketch *s, uint8_t *out_dev, void *stream)
{
    CHECK_HANDLE(s, PSK_KIND_BLOOM);
    if (!s->pend.active) return fail(PSK_EINVAL, "no split lookup pending on this handle");
    s->pend.active = false;
    const Batch b = s->pend.b;
    if (b.n && !out_dev) return fail(PSK_EINVAL, "out is NULL");
    hipStream_t st = (hipStream_t)stream;
    PSK_TRY(clear_materialize(s, st));  // (a clear between begin and finish)
    bool redo = false;
    PSK_TRY(bloom_check_finish_partitioned(s, out_dev, st, &redo));
    if (!s->pend.scattered) {  // batch / table not eligible for the partitioned path: plain direct lookup now
        return with_source(b, [&](auto src) {
            return with_pow2(s, [&](auto P) { return launch_apply(src, BloomCheck<P.value>{(const uint32_t *)s->table, s->md, s->k, out_dev}, b.n, st); });
        });
    }
    if (redo) {  // exact redo of the first round, taken on the device only if a segment overflowed during begin
        const uint64_t cnt0 = b.n < s->pend.round_keys ? b.n : s->pend.round_keys;
        const uint32_t *flag = (const uint32_t *)s->s_flag.p;
        PSK_TRY(with_source(sub_batch(b, 0, cnt0), [&](auto src) {
            return with_pow2(s, [&](auto P) {
                using Op = BloomCheck<P.value>;
                hipLaunchKernelGGL((k_apply_if<decltype(src), Op>), dim3(grid_for_keys(cnt0)), dim3(kBlock), 0, st, flag, src,
                                   Op{(const uint32_t *)s->table, s->md, s->k, out_dev}, cnt0);
                HIP_TRY(hipGetLastError());
                return (int)PSK_OK;
            });
        }));
    }
    return PSK_OK;
}

// Large batches of psk_bloom_check_bits: the partitioned lookup answers a byte per key (whichever scheme the batch calls for: tile flags,
// keyed probes, return trip, lazy gathers), and this one streaming pass turns the bytes into the ballot words and counts the hits -- the
// direct kernel pays k 64-byte gathers per key (~9 G keys/s at k = 7 against the partitioned lookups' 30-50).  One atomic per workgroup.
static __global__ __launch_bounds__(kBlock) void k_pack_answer_bits(const uint8_t *ans, uint64_t n, unsigned long long *out_bits, unsigned long long *hits)
{
    __shared__ unsigned long long wsum[kBlock / 64];
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t nround = (n + 63) & ~63ULL;  // wave-uniform trip count
    unsigned long long my_hits = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nround; i += stride) {
        const unsigned long long bal = __ballot(i < n && ans[i < n ? i : 0] != 0);
        if ((threadIdx.x & 63) == 0) {
            out_bits[i >> 6] = bal;
            my_hits += (unsigned long long)__popcll(bal);
        }
    }
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = my_hits;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kBlock / 64; ++w) t += wsum[w];
        if (t) atomicAdd(hits, t);
    }
}

extern "C" int psk_bloom_check_bits(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                                    uint32_t key_len, int where, uint64_t *out_bits, uint64_t *hits, void *stream)
{
    CHECK_HANDLE(s, PSK_KIND_BLOOM);
    PSK_TRY(check_hashes_width(s, layout, key_len));
    if (n && (!out_bits || !hits)) return fail(PSK_EINVAL, "out_bits / hits is NULL");
    hipStream_t st = (hipStream_t)stream;
    PSK_TRY(clear_materialize(s, st));
    Batch b;
    PSK_TRY(stage_batch(s->s_keys, s->s_offs, layout, data, offsets, n, key_len, where, st, &b));
    const uint64_t nwords = (n + 63) / 64;
    OutBuf o;
    PSK_TRY(stage_out(s->s_out, out_bits, nwords * 8, where, &o));
    unsigned long long *hits_dev = (unsigned long long *)hits;
    const bool big = n && !s->pend.active && part_wanted(s, n, s->k, 4);
    if (where == PSK_HOST || big) PSK_TRY(ensure(s->s_aux, 16 + (big ? n : 0)));  // hits (staged for host callers) | a byte per key
    if (where == PSK_HOST) {
        hits_dev = (unsigned long long *)s->s_aux.p;
        HIP_TRY(hipMemcpyAsync(hits_dev, hits, 8, hipMemcpyHostToDevice, st));
    }
    bool packed = false;
    if (big) {
        uint8_t *ans = (uint8_t *)s->s_aux.p + 16;
        PSK_TRY(bloom_check_partitioned(s, b, ans, st, &packed));
        if (packed) {
            const uint64_t blocks = (n + kBlock - 1) / kBlock;
            hipLaunchKernelGGL(k_pack_answer_bits, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(kBlock), 0, st, (const uint8_t *)ans, n,
                               (unsigned long long *)o.dev, hits_dev);
            HIP_TRY(hipGetLastError());
        }
    }
    if (n && !packed) {
        PSK_TRY(with_source(b, [&](auto src) {
            return with_pow2(s, [&](auto P) {
                hipLaunchKernelGGL((k_bloom_check_bits<decltype(src), P.value>), dim3(grid_for_keys(n)), dim3(kBlock), 0, st, src,
                                   (const uint32_t *)s->table, s->md, s->k, n, (unsigned long long *)o.dev, hits_dev);
                HIP_TRY(hipGetLastError());
                return (int)PSK_OK;
            });
        }));
    }
    if (where == PSK_HOST) HIP_TRY(hipMemcpyAsync(hits, hits_dev, 8, hipMemcpyDeviceToHost, st));
    return finish(where, &o, st);
}
