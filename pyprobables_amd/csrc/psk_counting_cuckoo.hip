// psk_counting_cuckoo.hip -- counting cuckoo filter (include/psk.h "CountingCuckooFilter"; reference: probables/cuckoo/countingcuckoo.py).
//
// The table is the plain filter's with two words per slot: `bins` is uint32[capacity][bucket_size][2], (fingerprint, count) pairs, a row
// filled from the left and its unused pairs 0 -- the reference's export byte for byte -- and `fill` is uint32[capacity].  A lookup of a
// present key finds fingerprint and count in the same 8 bytes.  Placement, the kick walk with its MT19937 and the row compaction are
// the plain filter's kernels instantiated for W = 2 (psk_cuckoo.hpp); psk_ck_triples and psk_ck_place_sweep serve both as they are (the
// sweep reads only `fill`).
//
// What is new here works on DISTINCT fingerprints, which own distinct bins, so no two lanes ever write the same word:
//   k_cck_add_counts   `weights[t]` repeats of a present fingerprint in one add to its first bin (idx_1's row left to right, then idx_2's):
//                      a key repeated a million times is one weighted add, not a million atomics on one word.
//   k_cck_rm_mark      `requests[t]` removes of a fingerprint: its copies are drained in that same order, granted = min(requests, sum of
//                      the counts); bins that reach 0 are marked in the per-row mask and k_ck_rm_compact<2> closes the gaps.
#include "psk_stage.hpp"
#include "psk_cuckoo.hpp"

namespace {

// the count of the first bin that holds the fingerprint: idx_1's row, else idx_2's, else 0 (countingcuckoo.py:175-191)
__device__ __forceinline__ uint32_t cck_count(const CkGeom &g, const uint32_t *bins, const uint32_t *fill, const CkTriple &t)
{
    uint32_t row = t.i1, s = ck_row_find<2>(g, bins, fill, row, t.fp);
    if (s == kNone && t.i2 != t.i1) row = t.i2, s = ck_row_find<2>(g, bins, fill, row, t.fp);
    return s == kNone ? 0u : bins[((uint64_t)row * g.B + s) * 2 + 1];
}

template <class Src>
__global__ __launch_bounds__(kBlock) void k_cck_check(Src src, CkGeom g, const uint32_t *bins, const uint32_t *fill, uint32_t *out, uint64_t n)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) out[i] = cck_count(g, bins, fill, ck_triple(src, src.load(i), i, g));
}

// missed[t]: 0 = added, 1 = no bin holds the fingerprint, 2 = count + weight would pass 2^32 - 1 (the bin is left as it is);
// flags[0] / flags[1] count the 1s / the 2s
__global__ __launch_bounds__(kBlock) void k_cck_add_counts(CkGeom g, CkTable t, const uint32_t *tr, const uint32_t *weights, uint64_t u, uint8_t *missed, uint32_t *flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < u; i += stride) {
        const uint32_t fp = tr[i], i1 = tr[u + i], i2 = tr[2 * u + i];
        uint32_t row = i1, s = kNone;
        if (i1 < g.capacity && i2 < g.capacity) {
            s = ck_row_find<2>(g, t.buckets, t.fill, row, fp);
            if (s == kNone && i2 != i1) row = i2, s = ck_row_find<2>(g, t.buckets, t.fill, row, fp);
        }
        if (s == kNone) {
            missed[i] = 1;
            atomicAdd(flags, 1u);
            continue;
        }
        uint32_t *count = t.buckets + ((uint64_t)row * g.B + s) * 2 + 1;
        const uint32_t c = *count, w = weights[i];
        if (c > 0xFFFFFFFFu - w) {
            missed[i] = 2;
            atomicAdd(flags + 1, 1u);
            continue;
        }
        *count = c + w;
        missed[i] = 0;
    }
}

// emptied[0] += bins that reached 0
__global__ __launch_bounds__(kBlock) void k_cck_rm_mark(CkGeom g, CkTable t, const uint32_t *tr, const uint32_t *requests, uint64_t u, uint32_t *marks, uint32_t *granted,
                                                        uint32_t *emptied)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < u; i += stride) {
        const uint32_t fp = tr[i], i1 = tr[u + i], i2 = tr[2 * u + i], want = requests[i];
        uint32_t left = want, gone = 0;
        if (i1 < g.capacity && i2 < g.capacity) {
            for (uint32_t which = 0; which < 2 && left; ++which) {
                if (which && i2 == i1) break;
                const uint32_t row = which ? i2 : i1;
                const uint32_t f = min(t.fill[row], g.B);
                uint32_t *p = t.buckets + (uint64_t)row * g.B * 2;
                for (uint32_t s = 0; s < f && left; ++s) {
                    if (p[2 * s] != fp) continue;
                    const uint32_t c = p[2 * s + 1], take = min(c, left);
                    p[2 * s + 1] = c - take;
                    left -= take;
                    if (c == take) {
                        atomicOr(marks + row, 1u << s);
                        ++gone;
                    }
                }
            }
        }
        granted[i] = want - left;
        if (gone) atomicAdd(emptied, gone);
    }
}

int cck_geom(uint64_t capacity, uint32_t bucket_size, uint32_t fp_bits, CkGeom *g)
{
    if (!ck_make_geom(capacity, bucket_size, fp_bits, g))
        return fail(PSK_EINVAL, "counting cuckoo filter: capacity must be in 1 .. 2^31 - 1, bucket_size >= 1, fingerprint bits in 1 .. 32 (got %llu x %u, %u bits)",
                    (unsigned long long)capacity, bucket_size, fp_bits);
    return PSK_OK;
}
// (the calls that take triples: the fingerprints are whole 32-bit words by then)
int geom_of(uint64_t capacity, uint32_t bucket_size, CkGeom *g) { return cck_geom(capacity, bucket_size, 32, g); }

}  // namespace

// out[i] = check(key_i) (countingcuckoo.py:175-191): hash, row scan and count in one kernel
extern "C" int psk_cck_check(uint64_t capacity, uint32_t bucket_size, uint32_t fp_bits, const uint32_t *bins_dev, const uint32_t *fill_dev, int layout, const void *data,
                             const uint64_t *offsets, uint64_t n, uint32_t key_len, int where, uint32_t *out, int device, void *stream)
{
    CkGeom g;
    PSK_TRY(cck_geom(capacity, bucket_size, fp_bits, &g));
    if (!bins_dev || !fill_dev) return fail(PSK_EINVAL, "NULL table pointer");
    if (layout == PSK_KEYS_HASHES && key_len < 1) return fail(PSK_EINVAL, "pre-hashed batch carries no hash per key");
    if (n && !out) return fail(PSK_EINVAL, "out is NULL");
    return keyed_call(layout, data, offsets, n, key_len, where, out, n * 4, device, stream, [&](auto src, void *out_dev, hipStream_t st) {
        hipLaunchKernelGGL((k_cck_check<decltype(src)>), dim3(grid_for_keys(n)), dim3(kBlock), 0, st, src, g, bins_dev, fill_dev, (uint32_t *)out_dev, n);
    });
}

extern "C" int psk_cck_present(uint64_t capacity, uint32_t bucket_size, const uint32_t *bins_dev, const uint32_t *fill_dev, const uint32_t *triples_dev, uint64_t n,
                               uint8_t *out_dev, int device, void *stream)
{
    CkGeom g;
    PSK_TRY(geom_of(capacity, bucket_size, &g));
    if (!bins_dev || !fill_dev) return fail(PSK_EINVAL, "NULL table pointer");
    if (n && (!triples_dev || !out_dev)) return fail(PSK_EINVAL, "NULL argument");
    PSK_USE_DEVICE(device);
    if (!n) return PSK_OK;
    hipLaunchKernelGGL(k_ck_present<2>, dim3(grid_for_keys(n)), dim3(kBlock), 0, (hipStream_t)stream, g, bins_dev, fill_dev, triples_dev, n, out_dev);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

extern "C" int psk_cck_place_apply(uint64_t capacity, uint32_t bucket_size, uint32_t *bins_dev, uint32_t *fill_dev, const uint32_t *triples_dev, const uint64_t *claims_dev,
                                   const uint32_t *pos_dev, uint64_t m, const uint8_t *d_dev, uint64_t prefix, const uint32_t *counts_dev, int device, void *stream)
{
    CkGeom g;
    PSK_TRY(geom_of(capacity, bucket_size, &g));
    if (m >= (1ull << 31) || prefix > m) return fail(PSK_EINVAL, "a placement batch holds fewer than 2^31 keys and the prefix lies inside it");
    if (!bins_dev || !fill_dev || (m && (!triples_dev || !claims_dev || !pos_dev || !d_dev))) return fail(PSK_EINVAL, "NULL argument");
    PSK_USE_DEVICE(device);
    if (!prefix) return PSK_OK;
    hipStream_t st = (hipStream_t)stream;
    const CkTable t{bins_dev, fill_dev};
    hipLaunchKernelGGL(k_ck_apply<2>, dim3(grid_for_keys(prefix)), dim3(kBlock), 0, st, g, t, triples_dev, (const unsigned long long *)claims_dev, pos_dev, (uint32_t)m, d_dev,
                       (uint32_t)prefix, counts_dev);
    hipLaunchKernelGGL(k_ck_count, dim3(grid_for_keys(prefix)), dim3(kBlock), 0, st, g, fill_dev, triples_dev, (uint32_t)m, d_dev, (uint32_t)prefix);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

extern "C" int psk_cck_insert(uint64_t capacity, uint32_t bucket_size, uint32_t max_swaps, uint32_t *bins_dev, uint32_t *fill_dev, const uint32_t *triples_dev,
                              const uint32_t *counts_dev, uint64_t n, uint64_t start, uint64_t end, uint64_t budget, uint32_t *mt_state_dev, uint32_t *result_dev, int device,
                              void *stream)
{
    CkGeom g;
    PSK_TRY(geom_of(capacity, bucket_size, &g));
    if (n >= (1ull << 32) || start > end || end > n) return fail(PSK_EINVAL, "psk_cck_insert: need start <= end <= n < 2^32");
    if (!budget) return fail(PSK_EINVAL, "psk_cck_insert: a launch needs a budget of at least one step");
    if (!bins_dev || !fill_dev || !mt_state_dev || !result_dev || (n && !triples_dev)) return fail(PSK_EINVAL, "NULL argument");
    PSK_USE_DEVICE(device);
    const CkTable t{bins_dev, fill_dev};
    hipLaunchKernelGGL(k_ck_insert<2>, dim3(1), dim3(64), 0, (hipStream_t)stream, g, t, max_swaps, triples_dev, counts_dev, n, start, end, 0, budget, mt_state_dev, result_dev);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

extern "C" int psk_cck_add_counts(uint64_t capacity, uint32_t bucket_size, uint32_t *bins_dev, uint32_t *fill_dev, const uint32_t *triples_dev, const uint32_t *weights_dev,
                                  uint64_t u, uint8_t *missed_dev, uint32_t *flags_dev, int device, void *stream)
{
    CkGeom g;
    PSK_TRY(geom_of(capacity, bucket_size, &g));
    if (!bins_dev || !fill_dev || !flags_dev) return fail(PSK_EINVAL, "NULL table or flags pointer");
    if (u && (!triples_dev || !weights_dev || !missed_dev)) return fail(PSK_EINVAL, "NULL argument");
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(flags_dev, 0, 8, st));
    if (!u) return PSK_OK;
    const CkTable t{bins_dev, fill_dev};
    hipLaunchKernelGGL(k_cck_add_counts, dim3(grid_for_keys(u)), dim3(kBlock), 0, st, g, t, triples_dev, weights_dev, u, missed_dev, flags_dev);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

extern "C" int psk_cck_remove(uint64_t capacity, uint32_t bucket_size, uint32_t *bins_dev, uint32_t *fill_dev, const uint32_t *triples_dev, const uint32_t *requests_dev,
                              uint64_t u, uint32_t *row_marks_dev, uint32_t *granted_dev, uint32_t *emptied_dev, int device, void *stream)
{
    CkGeom g;
    PSK_TRY(geom_of(capacity, bucket_size, &g));
    if (bucket_size > 32) return fail(PSK_EINVAL, "psk_cck_remove: bucket_size up to 32 (a row's removals are one 32-bit mask), got %u", bucket_size);
    if (!bins_dev || !fill_dev || !row_marks_dev || !emptied_dev) return fail(PSK_EINVAL, "NULL table pointer");
    if (u && (!triples_dev || !requests_dev || !granted_dev)) return fail(PSK_EINVAL, "NULL argument");
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(emptied_dev, 0, 4, st));
    if (!u) return PSK_OK;
    const CkTable t{bins_dev, fill_dev};
    hipLaunchKernelGGL(k_cck_rm_mark, dim3(grid_for_keys(u)), dim3(kBlock), 0, st, g, t, triples_dev, requests_dev, u, row_marks_dev, granted_dev, emptied_dev);
    hipLaunchKernelGGL(k_ck_rm_compact<2>, dim3(grid_for_keys(u)), dim3(kBlock), 0, st, g, t, triples_dev, u, row_marks_dev);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}
