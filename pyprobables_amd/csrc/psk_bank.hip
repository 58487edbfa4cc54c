// psk_bank.hip -- BloomFilterBank (include/psk.h "BloomFilterBank"): many small Bloom filters of one geometry in one table, row f
// the reference's BloomFilter after add() of the keys sent to f (bloom.py:234-272).  The slice a probe belongs to is the caller's filter id, not
// a piece of the hash, and all k probes of a key go to the same row: what the partitioned Bloom step needs pass 1 for is given.
//   psk_bank_add / psk_bank_check   keys with an id each: two ops on k_apply (psk_device.hpp), atomics into / loads from row ids[i]
//   psk_bank_build                  keys grouped by filter: one workgroup per (filter, part) sets the bits in an LDS image of the row and ORs
//                                   the image's non-zero words into the table once (pass 2 of the Bloom step without the pass 1)
#include "psk_stage.hpp"

namespace {

constexpr uint64_t kBankMaxBits = 1ULL << 31;   // reduce_small's range, and bit indices in 32 bits; rows of up to 256 MiB
constexpr uint64_t kBankLdsRowBytes = 65536;    // the image is dynamic LDS of exactly one row: up to the default limit, two workgroups per CU at the cap
constexpr unsigned kBankGridCap = 256 * 16;     // workgroups along x (grid_for_keys' cap): more filters than that are walked with a stride
// route 0: a part whose keys * k * R is below the row's word count goes straight to the row -- clearing and sweeping the image would cost more than
// its probes.  Measured (scripts/bench_bank.py part (d), profiles/bank_bench.txt: 4096 rows of 2996 words, k = 7, one MI355X): the atomics are 5 to 14 %
// ahead up to 16 keys per filter (keys * k / words = 0.037), the image 3 % ahead at 32 (0.075), 9 % at 64, 1.33 x at 128, 6.3 x at 1024: the
// crossover lies between words / (keys * k) = 27 and 13.  One geometry only; below ~64 keys per filter the launch is most of what both routes cost.
constexpr uint32_t kBankRouteR = 16;

// bit index of hash h in a row of md.m <= 2^31 bits (bloom.py:247)
template <bool POW2>
__device__ __forceinline__ uint32_t bank_bit(const Mod &md, uint64_t h)
{
    if (POW2) return (uint32_t)(h & md.mask);
    return reduce_small(md, h);
}

template <bool POW2>
struct BankAdd {  // bloom.py:241-250 add_alt on row ids[i]; ids >= filters: no row, nothing written
    uint32_t *tab;
    uint64_t row_words, filters;
    const uint32_t *ids;
    Mod md;
    uint32_t k;
    struct State { uint32_t *row; };
    __device__ __forceinline__ void prepare() {}
    __device__ __forceinline__ State begin(uint64_t i) const
    {
        const uint64_t f = ids[i];
        return State{f < filters ? tab + f * row_words : nullptr};  // (64-bit: filters * row_bytes may exceed 2^32)
    }
    __device__ __forceinline__ void apply(State &st, uint32_t, uint64_t h) const
    {
        if (!st.row) return;
        const uint32_t b = bank_bit<POW2>(md, h);
        atomicOr(st.row + (b >> 5), 1u << (b & 31));  // result unused -> no-return global_atomic_or
    }
    __device__ __forceinline__ void end(State &, uint64_t) const {}
};

template <bool POW2>
struct BankCheck {  // bloom.py:261-272 check_alt on row ids[i]; ids >= filters answer 0
    const uint32_t *tab;
    uint64_t row_words, filters;
    const uint32_t *ids;
    Mod md;
    uint32_t k;
    uint8_t *out;
    struct State { const uint32_t *row; uint32_t ok; };
    __device__ __forceinline__ void prepare() {}
    __device__ __forceinline__ State begin(uint64_t i) const
    {
        const uint64_t f = ids[i];
        return f < filters ? State{tab + f * row_words, 1u} : State{nullptr, 0u};
    }
    __device__ __forceinline__ void apply(State &st, uint32_t, uint64_t h) const
    {
        if (!st.row) return;
        const uint32_t b = bank_bit<POW2>(md, h);
        st.ok &= (st.row[b >> 5] >> (b & 31)) & 1u;
    }
    __device__ __forceinline__ void end(State &st, uint64_t i) const { out[i] = (uint8_t)st.ok; }
};

// Workgroup (x, y) walks filters x, x + gridDim.x, ... and takes the y-th of gridDim.y contiguous parts of each filter's segment; an empty part
// costs nothing.  Everything that decides a barrier (the filter, the part's bounds, the route) is uniform over the workgroup.  Parts of one
// filter -- in this launch or in another -- meet in the row through atomicOr only, and a zero word of the image is never written.
template <class Src, bool POW2>
__global__ __launch_bounds__(kBlock) void k_bank_build(Src src, uint32_t *tab, uint64_t filters, uint32_t row_words, Mod md, uint32_t k, uint64_t n,
                                                       const uint64_t *seg, const uint32_t *perm, int route)
{
    extern __shared__ uint4 bank_img4[];  // row_words / 4 (route 2, or a row over the cap: none)
    uint32_t *img = reinterpret_cast<uint32_t *>(bank_img4);
    const uint32_t split = gridDim.y, part = blockIdx.y, quads = row_words >> 2;
    const bool fits = (uint64_t)row_words * 4 <= kBankLdsRowBytes;
    for (uint64_t f = blockIdx.x; f < filters; f += gridDim.x) {
        uint64_t s0 = seg[f], s1 = seg[f + 1];
        if (s1 > n) s1 = n;  // (the contract says seg[filters] <= n: no key is read beyond the batch whatever seg holds)
        if (s1 <= s0) continue;
        const uint64_t per = (s1 - s0 + split - 1) / split;
        const uint64_t a = s0 + per * part;
        if (a >= s1) continue;
        const uint64_t b = a + per < s1 ? a + per : s1;
        uint32_t *row = tab + f * (uint64_t)row_words;
        const bool image = route == 1 || (route == 0 && fits && (b - a) * k * kBankRouteR >= row_words);
        if (image) {
            for (uint32_t w = threadIdx.x; w < quads; w += kBlock) bank_img4[w] = make_uint4(0u, 0u, 0u, 0u);
            __syncthreads();
            for (uint64_t j = a + threadIdx.x; j < b; j += kBlock) {
                const uint64_t i = perm ? perm[j] : j;
                if (i >= n) continue;
                const typename Src::Key key = src.load(i);
                for_each_hash(src, key, i, k, [&](uint32_t, uint64_t h) {
                    const uint32_t bit = bank_bit<POW2>(md, h);
                    atomicOr(img + (bit >> 5), 1u << (bit & 31));  // ds_or_b32, no return value
                });
            }
            __syncthreads();
            for (uint32_t w = threadIdx.x; w < quads; w += kBlock) {
                const uint4 v = bank_img4[w];
                uint32_t *p = row + 4u * w;
                if (v.x) atomicOr(p, v.x);
                if (v.y) atomicOr(p + 1, v.y);
                if (v.z) atomicOr(p + 2, v.z);
                if (v.w) atomicOr(p + 3, v.w);
            }
            __syncthreads();  // the next filter's clear must not overtake this sweep
        } else {
            for (uint64_t j = a + threadIdx.x; j < b; j += kBlock) {
                const uint64_t i = perm ? perm[j] : j;
                if (i >= n) continue;
                const typename Src::Key key = src.load(i);
                for_each_hash(src, key, i, k, [&](uint32_t, uint64_t h) {
                    const uint32_t bit = bank_bit<POW2>(md, h);
                    atomicOr(row + (bit >> 5), 1u << (bit & 31));
                });
            }
        }
    }
}

Mod bank_mod(uint64_t m, bool *pow2)
{
    Mod md;
    md.m = m;
    *pow2 = (m & (m - 1)) == 0;
    md.mask = m - 1;
    md.magic = *pow2 ? 0 : (uint64_t)((((unsigned __int128)1) << 64) / m);
    return md;
}

template <class F>
int bank_with_pow2(bool pow2, F &&f)
{
    if (pow2) return f(std::true_type{});
    return f(std::false_type{});
}

int bank_check_args(const void *table_dev, uint64_t filters, uint64_t m_bits, uint32_t k, int layout, uint64_t n, uint32_t key_len)
{
    if (!table_dev) return fail(PSK_EINVAL, "NULL table pointer");
    if (filters == 0 || filters > (1ULL << 32)) return fail(PSK_EINVAL, "a bank holds 1 .. 2^32 filters; %llu were asked for", (unsigned long long)filters);
    if (m_bits == 0 || m_bits > kBankMaxBits) return fail(PSK_EINVAL, "a bank's filters hold 1 .. 2^31 bits; %llu were asked for", (unsigned long long)m_bits);
    if (k == 0) return fail(PSK_EINVAL, "number of hashes must be > 0");
    if (n >> 32) return fail(PSK_EINVAL, "a bank call takes fewer than 2^32 keys; %llu were passed", (unsigned long long)n);
    if (layout == PSK_KEYS_HASHES && key_len < k) return fail(PSK_EINVAL, "pre-hashed batch carries %u hashes per key, the bank needs %u", key_len, k);
    return PSK_OK;
}

// the staged filter ids of a PSK_HOST call: the one buffer a bank call needs beside ThreadStage's three
DevBuf &bank_ids_stage()
{
    static thread_local DevBuf ids;
    return ids;
}

// One keyed bank call: on `device`, stage the batch, its ids and out[out_bytes] (none: an update), run launch(src, ids_dev, out_dev, stream), end the call.
template <class Launch>
int bank_keyed_call(int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len, int where, const uint32_t *ids, void *out,
                    uint64_t out_bytes, int device, void *stream, Launch &&launch)
{
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    ThreadStage &ts = thread_stage();
    Batch b;
    PSK_TRY(stage_batch(ts.keys, ts.offs, layout, data, offsets, n, key_len, where, st, &b));
    const uint32_t *ids_dev = nullptr;
    PSK_TRY(stage_vec(bank_ids_stage(), ids, n, where, st, &ids_dev));
    OutBuf o;
    PSK_TRY(stage_out(ts.out, out, out_bytes, where, &o));
    if (n) PSK_TRY(with_source(b, [&](auto src) { return launch(src, ids_dev, o.dev, st); }));
    return finish(where, out_bytes ? &o : nullptr, st);
}

}  // namespace

extern "C" uint64_t psk_bank_row_bytes(uint64_t m_bits) { return psk_bloom_table_bytes(m_bits); }

extern "C" int psk_bank_add(void *table_dev, uint64_t filters, uint64_t m_bits, uint32_t k, int layout, const void *data, const uint64_t *offsets,
                            uint64_t n, uint32_t key_len, int where, const uint32_t *ids, int device, void *stream)
{
    PSK_TRY(bank_check_args(table_dev, filters, m_bits, k, layout, n, key_len));
    if (n && !ids) return fail(PSK_EINVAL, "ids is NULL");
    bool pow2;
    const Mod md = bank_mod(m_bits, &pow2);
    const uint64_t row_words = psk_bank_row_bytes(m_bits) / 4;
    return bank_keyed_call(layout, data, offsets, n, key_len, where, ids, nullptr, 0, device, stream, [&](auto src, const uint32_t *ids_dev, void *, hipStream_t st) {
        return bank_with_pow2(pow2, [&](auto P) { return launch_apply(src, BankAdd<P.value>{(uint32_t *)table_dev, row_words, filters, ids_dev, md, k}, n, st); });
    });
}

extern "C" int psk_bank_check(const void *table_dev, uint64_t filters, uint64_t m_bits, uint32_t k, int layout, const void *data, const uint64_t *offsets,
                              uint64_t n, uint32_t key_len, int where, const uint32_t *ids, uint8_t *out, int device, void *stream)
{
    PSK_TRY(bank_check_args(table_dev, filters, m_bits, k, layout, n, key_len));
    if (n && (!ids || !out)) return fail(PSK_EINVAL, "ids or out is NULL");
    bool pow2;
    const Mod md = bank_mod(m_bits, &pow2);
    const uint64_t row_words = psk_bank_row_bytes(m_bits) / 4;
    return bank_keyed_call(layout, data, offsets, n, key_len, where, ids, out, n, device, stream, [&](auto src, const uint32_t *ids_dev, void *out_dev, hipStream_t st) {
        return bank_with_pow2(pow2, [&](auto P) {
            return launch_apply(src, BankCheck<P.value>{(const uint32_t *)table_dev, row_words, filters, ids_dev, md, k, (uint8_t *)out_dev}, n, st);
        });
    });
}

extern "C" int psk_bank_build(void *table_dev, uint64_t filters, uint64_t m_bits, uint32_t k, int layout, const void *data, const uint64_t *offsets,
                              uint64_t n, uint32_t key_len, const uint64_t *seg_dev, const uint32_t *perm_dev, uint32_t split, int route, int device,
                              void *stream)
{
    PSK_TRY(bank_check_args(table_dev, filters, m_bits, k, layout, n, key_len));
    if (!seg_dev) return fail(PSK_EINVAL, "seg_dev is NULL");
    if (split < 1 || split > 65535) return fail(PSK_EINVAL, "split must be 1 .. 65535 workgroups per filter; %u was passed", split);
    if (route < 0 || route > 2) return fail(PSK_EINVAL, "route must be 0 (auto), 1 (LDS image) or 2 (global atomics)");
    const uint64_t row_bytes = psk_bank_row_bytes(m_bits);
    if (route == 1 && row_bytes > kBankLdsRowBytes)
        return fail(PSK_EINVAL, "rows of %llu bytes do not fit the LDS image (at most %llu)", (unsigned long long)row_bytes, (unsigned long long)kBankLdsRowBytes);
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    Batch b;
    ThreadStage &ts = thread_stage();
    PSK_TRY(stage_batch(ts.keys, ts.offs, layout, data, offsets, n, key_len, PSK_DEVICE, st, &b));
    if (n == 0) return PSK_OK;
    bool pow2;
    const Mod md = bank_mod(m_bits, &pow2);
    const size_t lds = route != 2 && row_bytes <= kBankLdsRowBytes ? (size_t)row_bytes : 0;
    const dim3 grid((unsigned)(filters < kBankGridCap ? filters : kBankGridCap), split);
    return with_source(b, [&](auto src) {
        return bank_with_pow2(pow2, [&](auto P) {
            hipLaunchKernelGGL((k_bank_build<decltype(src), P.value>), grid, dim3(kBlock), lds, st, src, (uint32_t *)table_dev, filters, (uint32_t)(row_bytes / 4), md, k, n,
                               seg_dev, perm_dev, route);
            HIP_TRY(hipGetLastError());
            return (int)PSK_OK;
        });
    });
}
