// psk_cuckoo.hpp -- device side of the cuckoo filter (reference: probables/cuckoo/cuckoo.py).
//
// Table: `buckets` is uint32[capacity][bucket_size] row-major, a row filled from the left and its unused slots kept 0 (so an export is one
// copy plus the footer); `fill` is uint32[capacity], the number of fingerprints in each row (needed because fingerprint 0 is legal).
//
// A key becomes the triple (fp, idx_1, idx_2) (cuckoo.py:483-506):
//     fp    = fnv_1a(key) & (2^bits - 1)
//     idx_1 = fp % capacity
//     idx_2 = fnv_1a(str(fp)) % capacity          str(fp): the decimal ASCII digits of the fingerprint
// Both indices are functions of the fingerprint alone, so the kick walk (psk_cuckoo.hip) recomputes them for the fingerprints it evicts.
// This header holds what is templated over the key source: the triples and the fused lookup; psk_capi.hip instantiates them.
#pragma once
#include "psk_device.hpp"

namespace psk {

struct CkGeom {
    uint32_t capacity, B, fp_mask;
    uint64_t magic;  // floor(2^64 / capacity); unused for capacity 1
};

// -> false: parameters out of range (capacity and bucket_size >= 1, capacity < 2^31, 1 <= fp_bits <= 32)
inline bool ck_make_geom(uint64_t capacity, uint32_t bucket_size, uint32_t fp_bits, CkGeom *g)
{
    if (capacity < 1 || capacity >= (1ull << 31) || bucket_size < 1 || fp_bits < 1 || fp_bits > 32) return false;
    g->capacity = (uint32_t)capacity;
    g->B = bucket_size;
    g->fp_mask = fp_bits == 32 ? 0xFFFFFFFFu : (1u << fp_bits) - 1u;
    g->magic = capacity > 1 ? (uint64_t)((((unsigned __int128)1) << 64) / capacity) : 0;
    return true;
}

// h % capacity, exact: q = floor(h * magic / 2^64) is floor(h / capacity) or one less (magic > 2^64 / capacity - 1 and h < 2^64)
__device__ __forceinline__ uint32_t ck_mod(const CkGeom &g, uint64_t h)
{
    if (g.capacity == 1) return 0;
    const uint64_t q = __umul64hi(h, g.magic);
    const uint64_t r = h - q * g.capacity;
    return (uint32_t)(r >= g.capacity ? r - g.capacity : r);
}

// fnv_1a(str(fp)): at most 10 digits, most significant first, no array (the divisors are constants: multiplies)
__device__ __forceinline__ uint64_t ck_hash_decimal(uint32_t fp)
{
    uint64_t h = kFnvBasis;
    bool started = false;
    uint32_t p = 1000000000u;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        const uint32_t digit = fp / p;
        fp -= digit * p;
        started = started || digit || k == 9;
        if (started) h = (h ^ (uint64_t)(0x30u + digit)) * kFnvPrime;
        p /= 10u;
    }
    return h;
}

struct CkTriple {
    uint32_t fp, i1, i2;
};

__device__ __forceinline__ CkTriple ck_triple_of(const CkGeom &g, uint32_t fp) { return CkTriple{fp, fp % g.capacity, ck_mod(g, ck_hash_decimal(fp))}; }

// PSK_KEYS_HASHES rows carry fnv_1a(key) -- or a fingerprint itself, which the mask leaves as it is (the re-insert stream of an expansion)
template <class Src>
__device__ __forceinline__ CkTriple ck_triple(const Src &src, const typename Src::Key &key, uint64_t i, const CkGeom &g)
{
    uint64_t h[1];
    src.template hash<1>(key, i, 0, h);
    return ck_triple_of(g, (uint32_t)h[0] & g.fp_mask);
}

// `fp in buckets[row]` (cuckoo.py:440-446).  Unused slots hold 0, so only fingerprint 0 has to look at the row's count.
__device__ __forceinline__ bool ck_row_has(const CkGeom &g, const uint32_t *buckets, const uint32_t *fill, uint32_t row, uint32_t fp)
{
    const uint32_t *p = buckets + (uint64_t)row * g.B;
    const uint32_t f = fp ? g.B : min(fill[row], g.B);
    for (uint32_t s = 0; s < f; ++s)
        if (p[s] == fp) return true;
    return false;
}

__device__ __forceinline__ bool ck_contains(const CkGeom &g, const uint32_t *buckets, const uint32_t *fill, const CkTriple &t)
{
    if (ck_row_has(g, buckets, fill, t.i1, t.fp)) return true;
    return t.i2 != t.i1 && ck_row_has(g, buckets, fill, t.i2, t.fp);
}

// out[0 .. n) = fp, out[n .. 2n) = idx_1, out[2n .. 3n) = idx_2
template <class Src>
__global__ __launch_bounds__(kBlock) void k_ck_triples(Src src, CkGeom g, uint32_t *out, uint64_t n)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const CkTriple t = ck_triple(src, src.load(i), i, g);
        out[i] = t.fp;
        out[n + i] = t.i1;
        out[2 * n + i] = t.i2;
    }
}

// cuckoo.py:306-315 check: one lane per key, hash and lookup in one kernel; row idx_2 is read only when idx_1 does not hold the fingerprint
template <class Src>
__global__ __launch_bounds__(kBlock) void k_ck_check(Src src, CkGeom g, const uint32_t *buckets, const uint32_t *fill, uint8_t *out, uint64_t n)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
        out[i] = ck_contains(g, buckets, fill, ck_triple(src, src.load(i), i, g)) ? 1 : 0;
}

}  // namespace psk
