// partitioned Bloom insert launcher (own translation unit: parallel build)
#include "psk_host.hpp"

static_assert(kBloomApplyCtrWords == PSK_CTR_COUNT, "k_bloom_apply's store mode zeroes the whole counter block");
static_assert(kBloomApplyCtrSpilled == PSK_CTR_SPILLED, "... and leaves the length of pass 1's spill list in this slot");

// Bloom insert through the partitioned path; *done = false when this batch/table is not eligible
int PSK_VARIANT(bloom_add_partitioned)(psk_sketch *s, const Batch &b, hipStream_t st, bool *done)
{
    *done = false;
    if (!part_wanted(s, b.n, s->k)) return PSK_OK;
    PartGeom g;
    if (!part_slices(s->m, 20, 7, &g, 16384)) return PSK_OK;
    g.k = s->k;
    PartGeom g1;
    uint32_t sub_bits = 0;
    if (two_level_geometry(g, &g1, &sub_bits)) {
        PSK_TRY(clear_materialize(s, st));  // (the store mode serves the single-level path only)
        // more slices than one pass can bin well: coarse buckets first (inline 32-bit probes), then k_part_split
        const uint64_t round_keys = part_round_keys_two_level(s, b.n, s->k);
        for (uint64_t start = 0; start < b.n; start += round_keys) {
            const uint64_t cnt = b.n - start < round_keys ? b.n - start : round_keys;
            const Batch sub = sub_batch(b, start, cnt);
            bool handled = false;
            SpillBloomOr spill{(uint32_t *)s->table};
            PSK_TRY(with_part_source(sub, &handled, [&](auto src) {
                using Src = decltype(src);
                return with_kt<Src>(s->k, [&](auto kt) {
                    constexpr int KT = decltype(kt)::value;
                    return launch_scatter<Src, IdxBloomWide<kTuPow2>, PayZero, SpillBloomOr, KT>(s, src, IdxBloomWide<kTuPow2>{s->md}, PayZero{},
                                                                                              spill, &g1, cnt, st);
                });
            }));
            if (!handled) return PSK_OK;
            PartGeom g2 = g;
            PSK_TRY((split_level2<0, SpillBloomOr>(s, g1, &g2, sub_bits, cnt * (uint64_t)s->k, spill, st)));
            const size_t lds = (size_t)1 << (g2.shift - 3);
            PSK_TRY(set_dyn_lds(k_bloom_apply, lds));
            hipLaunchKernelGGL(k_bloom_apply, dim3(g2.nbuckets), dim3(kApplyThreads), lds, st, (uint32_t *)s->table, s->padded_bytes / 4,
                               g2, (const uint32_t *)s->s_cnt2.p, (const uint4 *)s->s_part2.p, BloomApplyStore{});
            HIP_TRY(hipGetLastError());
        }
        *done = true;
        return PSK_OK;
    }
    if (g.nbuckets > (uint32_t)kPartMaxBuckets) return PSK_OK;
    const uint64_t round_keys = part_round_keys_big_table(s, b.n, s->k, PayNone::group, s->padded_bytes);
    // a deferred clear (psk_clear) is consumed by the first round: its apply stores the slices instead of read-modify-writing them, and
    // pass 1's spills wait in a list (they would be overwritten in the table) -- one entry per probe at most, so the list is exact
    BloomApplyStore first;
    if (s->clear_pending) {
        const uint64_t probes = (b.n < round_keys ? b.n : round_keys) * (uint64_t)s->k;
        if (probes < (1ULL << 32) - 2) {
            const uint64_t oldcap = s->s_spill.cap;
            PSK_TRY(ensure(s->s_spill, (2 + probes) * 4));
            if (s->s_spill.cap != oldcap) HIP_TRY(hipMemsetAsync(s->s_spill.p, 0, 8, st));  // (new buffer: the header; k_bloom_apply resets it after use)
            first = BloomApplyStore{1u, (const uint32_t *)s->s_spill.p, (uint32_t)probes, s->ctr};
        }
    }
    if (!first.on) PSK_TRY(clear_materialize(s, st));  // (no list: the sweep goes first, pass 1 may OR spills into the table)
    for (uint64_t start = 0; start < b.n; start += round_keys) {
        const uint64_t cnt = b.n - start < round_keys ? b.n - start : round_keys;
        const Batch sub = sub_batch(b, start, cnt);
        const BloomApplyStore sm = start == 0 ? first : BloomApplyStore{};
        bool handled = false;
        PSK_TRY(with_part_source(sub, &handled, [&](auto src) {
            using Src = decltype(src);
            return with_kt<Src>(s->k, [&](auto kt) {
                constexpr int KT = decltype(kt)::value;
                SpillBloomOr spill{(uint32_t *)s->table, sm.on ? const_cast<uint32_t *>(sm.spill) : nullptr, sm.spill_cap};
                return launch_scatter<Src, IdxBloom<kTuPow2>, PayNone, SpillBloomOr, KT>(s, src, IdxBloom<kTuPow2>{s->md}, PayNone{},
                                                                                          spill, &g, cnt, st);
            });
        }));
        if (!handled) return PSK_OK;  // layout without a partitioned instantiation: nothing was launched (a deferred clear is still pending)
        if (sm.on) s->clear_pending = false;
        const size_t lds = (size_t)1 << (g.shift - 3);
        PSK_TRY(set_dyn_lds(k_bloom_apply, lds));
        hipLaunchKernelGGL(k_bloom_apply, dim3(g.nbuckets), dim3(kApplyThreads), lds, st, (uint32_t *)s->table,
                           s->padded_bytes / 4, g, (const uint32_t *)s->s_cnt.p, (const uint4 *)s->s_part.p, sm);
        HIP_TRY(hipGetLastError());
    }
    *done = true;
    return PSK_OK;
}

// Bloom lookup through the partitioned path: probes carry their key's index; out[] starts at 1 and