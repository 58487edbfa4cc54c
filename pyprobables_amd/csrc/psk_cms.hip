// psk_cms.hip -- the CountMinSketch entry points of the C ABI (include/psk.h).
#include "psk_stage.hpp"
#include "psk_running.hpp"

// ---------------------------------------------------------- CountMinSketch
template <bool NEG>
static int cms_update(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len,
                      const int32_t *weights, int where, void *stream)
{
    CHECK_HANDLE(s, PSK_KIND_CMS);
    PSK_TRY(check_hashes_width(s, layout, key_len));
    hipStream_t st = (hipStream_t)stream;
    Batch b;
    PSK_TRY(stage_batch(s->s_keys, s->s_offs, layout, data, offsets, n, key_len, where, st, &b));
    const int32_t *w;
    PSK_TRY(stage_vec(s->s_w, weights, n, where, st, &w));
    PSK_TRY(post_acct(s, w, n, NEG ? PSK_CTR_REMOVED : PSK_CTR_ADDED, 1LL, st, true, true));
    unsigned long long *sat = (unsigned long long *)(s->ctr + PSK_CTR_SATURATED);
    {
        bool done = false;
        PSK_TRY(NEG ? cms_remove_partitioned(s, b, (const uint32_t *)w, st, &done) : cms_add_partitioned(s, b, (const uint32_t *)w, st, &done));
        PSK_TRY(settle_acct(s, w, n, st));
        if (done) return finish(where, nullptr, st);
    }
    return direct_apply(s, b, data, where, true, nullptr, st, [&](auto P) { return CmsAdd<P.value, NEG>{(int32_t *)s->table, s->md, s->k, w, s->ctr, sat, false}; });
}

extern "C" int psk_cms_add(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                           uint32_t key_len, const int32_t *weights, int where, void *stream)
{
    return cms_update<false>(s, layout, data, offsets, n, key_len, weights, where, stream);
}

extern "C" int psk_cms_remove(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                              uint32_t key_len, const int32_t *weights, int where, void *stream)
{
    return cms_update<true>(s, layout, data, offsets, n, key_len, weights, where, stream);
}

extern "C" int psk_cms_check(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                             uint32_t key_len, int where, int query, int32_t *out, void *stream)
{
    CHECK_HANDLE(s, PSK_KIND_CMS);
    PSK_TRY(check_hashes_width(s, layout, key_len));
    if (query != PSK_Q_MIN && query != PSK_Q_MEAN) return fail(PSK_EINVAL, "psk_cms_check handles MIN and MEAN queries");
    if (n && !out) return fail(PSK_EINVAL, "out is NULL");
    hipStream_t st = (hipStream_t)stream;
    Batch b;
    PSK_TRY(stage_batch(s->s_keys, s->s_offs, layout, data, offsets, n, key_len, where, st, &b));
    OutBuf o;
    PSK_TRY(stage_out(s->s_out, out, n * 4, where, &o));
    const bool mean = query == PSK_Q_MEAN;
    {
        bool done = false;
        PSK_TRY(cms_check_partitioned(s, b, query, 0, o.dev, st, &done));
        if (done) return finish(where, &o, st);
    }
    return direct_apply(s, b, data, where, o.is_pinned, &o, st, [&](auto P) { return CmsCheck<P.value>{(const int32_t *)s->table, s->md, s->k, (int32_t *)o.dev, mean}; });
}

extern "C" int psk_cms_check_meanmin(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                                     uint32_t key_len, int where, int64_t elements_added, int64_t *out, void *stream)
{
    CHECK_HANDLE(s, PSK_KIND_CMS);
    PSK_TRY(check_hashes_width(s, layout, key_len));
    if (s->m < 2) return fail(PSK_EINVAL, "mean-min query needs width >= 2 (divides by width-1)");
    if (n && !out) return fail(PSK_EINVAL, "out is NULL");
    hipStream_t st = (hipStream_t)stream;
    Batch b;
    PSK_TRY(stage_batch(s->s_keys, s->s_offs, layout, data, offsets, n, key_len, where, st, &b));
    OutBuf o;
    PSK_TRY(stage_out(s->s_out, out, n * 8, where, &o));
    if (s->k > (uint32_t)kMaxDepthMeanMin) {
        // deeper than the per-lane register array: the ordered kernel in query-only mode (one lane, scratch list)
        PSK_TRY(ensure(s->s_aux, 8ULL * s->k));
        if (n) {
            PSK_TRY(with_source(b, [&](auto src) {
                return with_pow2(s, [&](auto P) {
                    hipLaunchKernelGGL((k_cms_ordered<decltype(src), P.value>), dim3(1), dim3(64), 0, st, src, (int32_t *)s->table, s->md, s->k,
                                       (const int64_t *)nullptr, 3, (int)PSK_Q_MEANMIN, elements_added, n, (int64_t *)o.dev, s->ctr, (int64_t *)s->s_aux.p,
                                       (uint32_t *)nullptr, 0u);
                    HIP_TRY(hipGetLastError());
                    return (int)PSK_OK;
                });
            }));
        }
        return finish(where, &o, st);
    }
    {
        bool done = false;
        PSK_TRY(cms_check_partitioned(s, b, PSK_Q_MEANMIN, elements_added, o.dev, st, &done));
        if (done) return finish(where, &o, st);
    }
    return direct_apply(s, b, data, where, o.is_pinned, &o, st,
                        [&](auto P) { return CmsCheckMeanMin<P.value>{(const int32_t *)s->table, s->md, s->k, elements_added, (int64_t *)o.dev}; });
}

extern "C" int psk_cms_update_ordered(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                                      uint32_t key_len, const int64_t *weights, int opmode, int query,
                                      int64_t elements_added_in, int where, int64_t *out, void *stream)
{
    CHECK_HANDLE(s, PSK_KIND_CMS);
    PSK_TRY(check_hashes_width(s, layout, key_len));
    if (opmode < PSK_OP_ADD || opmode > PSK_OP_SIGNED) return fail(PSK_EINVAL, "bad opmode %d", opmode);
    if (query < PSK_Q_MIN || query > PSK_Q_MEANMIN) return fail(PSK_EINVAL, "bad query %d", query);
    if (query == PSK_Q_MEANMIN && s->m < 2) return fail(PSK_EINVAL, "mean-min query needs width >= 2");
    hipStream_t st = (hipStream_t)stream;
    Batch b;
    PSK_TRY(stage_batch(s->s_keys, s->s_offs, layout, data, offsets, n, key_len, where, st, &b));
    const int64_t *w;
    PSK_TRY(stage_vec(s->s_w, weights, n, where, st, &w));
    OutBuf o;
    PSK_TRY(stage_out(s->s_out, out, out ? (n + 1) * 8 : 0, where, &o));  // out[n] = elements_added after the batch
    int64_t *wide = nullptr;  // depth beyond the register array: the per-op value list lives in device scratch
    if (s->k > (uint32_t)kMaxDepthMeanMin) {
        PSK_TRY(ensure(s->s_aux, 8ULL * s->k));
        wide = (int64_t *)s->s_aux.p;
    }
    Mailbox mb;
    PSK_TRY(mailbox_arm(s, where, n, out && o.is_pinned, &mb));
    if (mb.word && n == 1 && weights && weights[0] == 1) w = nullptr;  // (a null weight list means 1: no read of the pinned page for `cms.add(key)`)
    KeysInline64 ik;
    PSK_TRY(with_source_one(b, inline_key(layout, data, n, key_len, mb, &ik), [&](auto src) {
        return with_pow2(s, [&](auto P) {
            hipLaunchKernelGGL((k_cms_ordered<decltype(src), P.value>), dim3(1), dim3(64), 0, st, src, (int32_t *)s->table, s->md, s->k, w,
                               opmode, query, elements_added_in, n, (int64_t *)(out ? o.dev : nullptr), s->ctr, wide, mb.dev(), mb.seq);
            HIP_TRY(hipGetLastError());
            return (int)PSK_OK;
        });
    }));
    return finish(where, &o, st, &mb);
}

// countminsketch.py:267-288 for a whole ordered batch of adds: the table, elements_added and EVERY op's return value as the reference's loop
// leaves them.  The parallel passes of psk_running.hpp wherever they apply (depth <= kMaxDepthMeanMin, width <= 2^32; weights >= 0 is the
// entry's contract), else k_cms_ordered: always exact.  Which one ran: read-only options "cms_running_fast" / "cms_running_sequential".
// SGN: psk_cms_update_running, :267-321 -- a negative weight removes; the same chunking, eligibility, passes and fall-back with the signed
// algebra (RunSignedOps in place of RunAddOps), counted by "cms_update_running_fast" / "cms_update_running_sequential".
template <bool SGN>
static int cms_running(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len, const int32_t *weights, int where,
                       int query, int64_t els_in, void *out, int64_t *els_out, void *stream)
{
    CHECK_HANDLE(s, PSK_KIND_CMS);
    PSK_TRY(check_hashes_width(s, layout, key_len));
    if (query < PSK_Q_MIN || query > PSK_Q_MEANMIN) return fail(PSK_EINVAL, "bad query %d", query);
    if (query == PSK_Q_MEANMIN && s->m < 2) return fail(PSK_EINVAL, "mean-min query needs width >= 2");
    if (n && !out) return fail(PSK_EINVAL, "out is NULL");
    if (!SGN && where == PSK_HOST && weights)
        for (uint64_t i = 0; i < n; ++i)
            if (weights[i] < 0) return fail(PSK_EINVAL, "ordered add: weight %d of op %llu is negative", weights[i], (unsigned long long)i);
    hipStream_t st = (hipStream_t)stream;
    Batch b;
    PSK_TRY(stage_batch(s->s_keys, s->s_offs, layout, data, offsets, n, key_len, where, st, &b));
    if (n == 0) {
        if (els_out && where == PSK_HOST) *els_out = els_in;
        else if (els_out) {
            hipLaunchKernelGGL(k_run_set, dim3(1), dim3(1), 0, st, (long long *)els_out, (long long)els_in);
            HIP_TRY(hipGetLastError());
        }
        return PSK_OK;
    }
    const int32_t *w;
    PSK_TRY(stage_vec(s->s_w, weights, n, where, st, &w));
    const bool wide_out = query == PSK_Q_MEANMIN;
    OutBuf o;
    PSK_TRY(stage_out(s->s_out, out, n * (wide_out ? 8 : 4), where, &o));
    // elements_added behind the batch: a device word; a host caller gets it copied back in front of the wait in finish()
    PSK_TRY(ensure(s->s_aux, 8ULL * (s->k > (uint32_t)kMaxDepthMeanMin ? s->k : 1u) + 8));
    int64_t *els_dev = where == PSK_DEVICE && els_out ? els_out : (int64_t *)s->s_aux.p;
    if (s->k <= (uint32_t)kMaxDepthMeanMin && s->m <= (1ULL << 32)) {
        __atomic_add_fetch(SGN ? &g_update_running_fast : &g_running_fast, 1, __ATOMIC_RELAXED);
        using Ops = std::conditional_t<SGN, RunSignedOps, RunAddOps>;
        RunArena a;
        PSK_TRY(cms_running_arena<Ops>(s, n, &a));
        for (uint64_t base = 0; base < n; base += a.cap) {
            const uint32_t nc = (uint32_t)(n - base < a.cap ? n - base : a.cap);
            PSK_TRY(with_source(b, [&](auto src) {
                return with_pow2(s, [&](auto P) {
                    hipLaunchKernelGGL((k_run_hash<decltype(src), P.value>), dim3(grid_for_keys(nc)), dim3(kBlock), 0, st, src, s->md, s->k, base, nc, a.cap, a.bins);
                    HIP_TRY(hipGetLastError());
                    return (int)PSK_OK;
                });
            }));
            PSK_TRY(cms_running_chunk<Ops>(s, a, w, base, nc, base == 0, els_in, query, o.dev, els_dev, st));
        }
    } else {  // one lane, one op after the other (int64 weights and results: widened / narrowed around it)
        __atomic_add_fetch(SGN ? &g_update_running_sequential : &g_running_sequential, 1, __ATOMIC_RELAXED);
        int64_t *wide = nullptr;
        if (s->k > (uint32_t)kMaxDepthMeanMin) wide = (int64_t *)s->s_aux.p + 1;
        PSK_TRY(ensure(s->s_perm, 8 * (n + 1)));
        const int64_t *w64 = nullptr;
        if (w) {
            PSK_TRY(ensure(s->s_vals, 8 * n));
            hipLaunchKernelGGL(k_run_widen, dim3(grid_for_keys(n)), dim3(kBlock), 0, st, w, n, (int64_t *)s->s_vals.p);
            w64 = (const int64_t *)s->s_vals.p;
        }
        PSK_TRY(with_source(b, [&](auto src) {
            return with_pow2(s, [&](auto P) {
                hipLaunchKernelGGL((k_cms_ordered<decltype(src), P.value>), dim3(1), dim3(64), 0, st, src, (int32_t *)s->table, s->md, s->k, w64, (int)(SGN ? PSK_OP_SIGNED : PSK_OP_ADD), query,
                                   els_in, n, (int64_t *)s->s_perm.p, s->ctr, wide, (uint32_t *)nullptr, 0u);
                HIP_TRY(hipGetLastError());
                return (int)PSK_OK;
            });
        }));
        hipLaunchKernelGGL(k_run_narrow, dim3(grid_for_keys(n)), dim3(kBlock), 0, st, (const int64_t *)s->s_perm.p, n, wide_out ? 1 : 0, o.dev, (long long *)els_dev);
        HIP_TRY(hipGetLastError());
    }
    if (where == PSK_HOST && els_out) HIP_TRY(hipMemcpyAsync(els_out, els_dev, 8, hipMemcpyDeviceToHost, st));
    return finish(where, &o, st);
}

extern "C" int psk_cms_add_running(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len,
                                   const int32_t *weights, int where, int query, int64_t els_in, void *out, int64_t *els_out, void *stream)
{
    return cms_running<false>(s, layout, data, offsets, n, key_len, weights, where, query, els_in, out, els_out, stream);
}

extern "C" int psk_cms_update_running(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len,
                                      const int32_t *weights, int where, int query, int64_t els_in, void *out, int64_t *els_out, void *stream)
{
    return cms_running<true>(s, layout, data, offsets, n, key_len, weights, where, query, els_in, out, els_out, stream);
}
