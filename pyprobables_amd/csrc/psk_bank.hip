// psk_bank.hip -- BloomFilterBank (include/psk.h "BloomFilterBank"): many small Bloom filters of one geometry in one table, row f
// the reference's BloomFilter after add() of the keys sent to f (bloom.py:234-272).  The slice a probe belongs to is the caller's filter id, not
// a piece of the hash, and all k probes of a key go to the same row: what the partitioned Bloom step needs pass 1 for is given.
//   psk_bank_add / psk_bank_check   keys with an id each: two ops on k_apply (psk_device.hpp), atomics into / loads from row ids[i]
//   psk_bank_build                  keys grouped by filter: one workgroup per (filter, part) sets the bits in an LDS image of the row and ORs
//                                   the image's non-zero words into the table once (pass 2 of the Bloom step without the pass 1)
//   psk_bank_slices / psk_bank_match  the bank transposed (slice row p = bit p of every filter) and "which filters may hold this key": the AND of
//                                   the key's k slice rows, as a mask, a count or a list of filter ids
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

int slice_check_geometry(uint64_t filters, uint64_t m_bits)
{
    if (filters == 0 || filters > (1ULL << 32)) return fail(PSK_EINVAL, "a bank holds 1 .. 2^32 filters; %llu were asked for", (unsigned long long)filters);
    if (m_bits == 0 || m_bits > kBankMaxBits) return fail(PSK_EINVAL, "a bank's filters hold 1 .. 2^31 bits; %llu were asked for", (unsigned long long)m_bits);
    return PSK_OK;
}

int bank_check_args(const void *table_dev, uint64_t filters, uint64_t m_bits, uint32_t k, int layout, uint64_t n, uint32_t key_len)
{
    if (!table_dev) return fail(PSK_EINVAL, "NULL table pointer");
    PSK_TRY(slice_check_geometry(filters, m_bits));
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

// ---------------------------------------------------------------- the slice image (include/psk.h "slice image")
// slices[p][f >> 5] bit (f & 31) == bit p of bank row f: the bank transposed, so that "which filters may hold this key" is the AND of k rows.
//
// k_bank_slices: a workgroup transposes a tile of 128 filters x 32 row words (16 KiB).  Load: 8 lanes read 128 contiguous bytes of one filter's row,
// 16 bytes each, 32 filters a pass, 4 passes.  The tile lies in LDS with a row stride of 33 words: the four ds_write_b32 of a lane fall on banks
// (filter + 4 * quad + j) mod 32, all different inside a 32-lane half (4 consecutive filters x 8 quads), and the transposed read -- lane = filter, one
// word -- on banks (33 * lane + w) mod 32 = (lane + w) mod 32, all different too.  Transpose: a wave takes 8 of the 32 words; per word it reads that
// word of filters 0..63 and of filters 64..127 and issues 32 ballots on each; lane b keeps the two ballots of bit b, and lanes 0..31 store them as ONE
// 16-byte piece of slice row 32 * word + b: 128 columns.  A ranged call stores only the words of its columns (whole words: the range is 32-aligned).
constexpr uint32_t kSliceTileFilters = 128, kSliceTileWords = 32, kSliceLdsStride = kSliceTileWords + 1;
constexpr uint64_t kSliceGridCap = 1ULL << 20;
constexpr uint32_t kBankMatchMaxK = 64;  // k_bank_match keeps k * kBlock positions in dynamic LDS: 64 KiB, the default limit, at the cap

// tiles: x = 32-word pieces of the rows (fastest), y = 128-filter groups from col0 (a multiple of 128) on.  Columns are stored as words
// [word_lo, word_hi) of a slice row; filters beyond `load_hi` read as zero.
__global__ __launch_bounds__(kBlock) void k_bank_slices(const uint32_t *tab, uint32_t row_words, uint64_t m_bits, uint32_t *slices, uint64_t srw, uint64_t col0,
                                                        uint64_t load_lo, uint64_t load_hi, uint64_t word_lo, uint64_t word_hi, uint32_t wtiles, uint64_t tiles)
{
    __shared__ uint32_t img[kSliceTileFilters * kSliceLdsStride];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t quad = threadIdx.x & 7, frow = threadIdx.x >> 3;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t f0 = col0 + (t / wtiles) * kSliceTileFilters;
        const uint32_t w0 = (uint32_t)(t % wtiles) * kSliceTileWords;
#pragma unroll
        for (uint32_t pass = 0; pass < kSliceTileFilters / 32; ++pass) {
            const uint32_t fl = pass * 32 + frow;
            const uint64_t f = f0 + fl;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (f >= load_lo && f < load_hi && w0 + 4 * quad < row_words)  // (row_words is a multiple of 4: the 16 bytes lie inside the row)
                v = *reinterpret_cast<const uint4 *>(tab + f * (uint64_t)row_words + w0 + 4 * quad);
            uint32_t *d = img + fl * kSliceLdsStride + 4 * quad;
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        }
        __syncthreads();
        const uint64_t cw = f0 >> 5;  // first of this tile's four words in a slice row
        const bool whole = cw >= word_lo && cw + 4 <= word_hi;
        for (uint32_t j = 0; j < kSliceTileWords / 4; ++j) {
            const uint32_t w = wave * (kSliceTileWords / 4) + j;
            const uint32_t v0 = img[lane * kSliceLdsStride + w], v1 = img[(64 + lane) * kSliceLdsStride + w];
            uint64_t r0 = 0, r1 = 0;
#pragma unroll 8
            for (uint32_t b = 0; b < 32; ++b) {
                const uint64_t b0 = __ballot((v0 >> b) & 1u), b1 = __ballot((v1 >> b) & 1u);
                if (lane == b) r0 = b0, r1 = b1;
            }
            const uint64_t p = (uint64_t)(w0 + w) * 32 + lane;  // slice row = bit index
            if (lane < 32 && p < m_bits) {
                uint32_t *o = slices + p * srw + cw;
                const uint32_t r[4] = {(uint32_t)r0, (uint32_t)(r0 >> 32), (uint32_t)r1, (uint32_t)(r1 >> 32)};
                if (whole) {
                    *reinterpret_cast<uint4 *>(o) = make_uint4(r[0], r[1], r[2], r[3]);
                } else {
#pragma unroll
                    for (uint32_t c = 0; c < 4; ++c)
                        if (cw + c >= word_lo && cw + c < word_hi) o[c] = r[c];
                }
            }
        }
        __syncthreads();  // the next tile's load must not overtake these reads
    }
}

// k_bank_match: a workgroup takes 256 keys a round.  Phase A, lane = key: the k bit positions go to LDS as pos[j][thread].  Phase B, per wave over
// its 64 keys: G lanes per key (G = 2^lgG covers the row's 16-byte pieces, at most 64; wider rows are walked in 1 KiB chunks), each lane ANDs the k
// 16-byte pieces of its column block -- k independent loads, four in flight -- and stores the mask piece; popcounts are reduced (count) or scanned
// (the ids' write positions) across the group.  Everything that decides a shuffle or a barrier is wave- / workgroup-uniform.
template <class Src, bool POW2>
__global__ __launch_bounds__(kBlock) void k_bank_match(Src src, const uint4 *slices, uint32_t quads, Mod md, uint32_t k, uint64_t n, uint32_t lgG, uint4 *mask,
                                                       uint32_t *count, const uint64_t *out_offs, uint32_t *ids)
{
    extern __shared__ uint32_t match_pos[];  // [k][kBlock]
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t G = 1u << lgG, gl = lane & (G - 1), sub = lane >> lgG, per = 64u >> lgG;
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < n; base += (uint64_t)gridDim.x * kBlock) {
        const uint64_t i = base + threadIdx.x;
        if (i < n) {
            const typename Src::Key key = src.load(i);
            for_each_hash(src, key, i, k, [&](uint32_t j, uint64_t h) { match_pos[j * kBlock + threadIdx.x] = bank_bit<POW2>(md, h); });
        }
        __syncthreads();
        const uint64_t wbase = base + wave * 64;
        for (uint32_t t0 = 0; t0 < 64 && wbase + t0 < n; t0 += per) {
            const uint32_t t = t0 + sub;
            const uint64_t ki = wbase + t;
            const bool live = ki < n;
            const uint32_t *pp = match_pos + wave * 64 + t;
            uint32_t cnt = 0;
            uint64_t wr = (ids && live) ? out_offs[ki] : 0;
            for (uint32_t c0 = 0; c0 < quads; c0 += 64) {
                const uint32_t qd = c0 + gl;
                const bool on = live && qd < quads;
                uint4 acc = make_uint4(0u, 0u, 0u, 0u);
                if (on) {
                    acc = make_uint4(~0u, ~0u, ~0u, ~0u);
                    const uint4 *col = slices + qd;
                    uint32_t j = 0;
                    for (; j + 4 <= k; j += 4) {
                        const uint32_t p0 = pp[j * kBlock], p1 = pp[(j + 1) * kBlock], p2 = pp[(j + 2) * kBlock], p3 = pp[(j + 3) * kBlock];
                        const uint4 a0 = col[(uint64_t)p0 * quads], a1 = col[(uint64_t)p1 * quads], a2 = col[(uint64_t)p2 * quads], a3 = col[(uint64_t)p3 * quads];
                        acc.x &= a0.x & a1.x & a2.x & a3.x;
                        acc.y &= a0.y & a1.y & a2.y & a3.y;
                        acc.z &= a0.z & a1.z & a2.z & a3.z;
                        acc.w &= a0.w & a1.w & a2.w & a3.w;
                    }
                    for (; j < k; ++j) {
                        const uint4 a = col[(uint64_t)pp[j * kBlock] * quads];
                        acc.x &= a.x, acc.y &= a.y, acc.z &= a.z, acc.w &= a.w;
                    }
                    if (mask) mask[ki * quads + qd] = acc;
                }
                const uint32_t pc = __popc(acc.x) + __popc(acc.y) + __popc(acc.z) + __popc(acc.w);
                cnt += pc;
                if (ids) {  // (uniform)
                    uint32_t x = pc;  // inclusive scan over the group's lanes = ascending columns
                    for (uint32_t d = 1; d < G; d <<= 1) {
                        const uint32_t y = (uint32_t)__shfl_up((int)x, d);
                        if (gl >= d) x += y;
                    }
                    const uint32_t total = (uint32_t)__shfl((int)x, (int)(lane | (G - 1)));
                    if (pc) {
                        uint32_t *o = ids + wr + (x - pc);
                        const uint32_t wv[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
                        for (uint32_t c = 0; c < 4; ++c)
                            for (uint32_t v = wv[c]; v; v &= v - 1) *o++ = qd * 128u + c * 32u + (uint32_t)__builtin_ctz(v);
                    }
                    wr += total;
                }
            }
            if (count) {  // (uniform)
                for (uint32_t o = 1; o < G; o <<= 1) cnt += (uint32_t)__shfl_xor((int)cnt, (int)o);
                if (live && gl == 0) count[ki] = cnt;
            }
        }
        __syncthreads();  // the next round's positions must not overtake these reads
    }
}

}  // namespace

extern "C" uint64_t psk_bank_row_bytes(uint64_t m_bits) { return psk_bloom_table_bytes(m_bits); }

extern "C" int psk_bank_add(void *table_dev, uint64_t filters, uint64_t m_bits, uint32_t k, int layout, const void *data, const uint64_t *offsets,
                            uint64_t n, uint32_t key_len, int where, const uint32_t *ids, int device, void *stream)
{
    PSK_TRY(bank_check_args(table_dev, filters, m_bits, k, layout, n, key_len));
    if (n && !ids) return fail(PSK_EINVAL, "ids is NULL");
    bool pow2;
    const Mod md = make_mod(m_bits, &pow2);
    const uint64_t row_words = psk_bank_row_bytes(m_bits) / 4;
    return bank_keyed_call(layout, data, offsets, n, key_len, where, ids, nullptr, 0, device, stream, [&](auto src, const uint32_t *ids_dev, void *, hipStream_t st) {
        return with_pow2(pow2, [&](auto P) { return launch_apply(src, BankAdd<P.value>{(uint32_t *)table_dev, row_words, filters, ids_dev, md, k}, n, st); });
    });
}

extern "C" int psk_bank_check(const void *table_dev, uint64_t filters, uint64_t m_bits, uint32_t k, int layout, const void *data, const uint64_t *offsets,
                              uint64_t n, uint32_t key_len, int where, const uint32_t *ids, uint8_t *out, int device, void *stream)
{
    PSK_TRY(bank_check_args(table_dev, filters, m_bits, k, layout, n, key_len));
    if (n && (!ids || !out)) return fail(PSK_EINVAL, "ids or out is NULL");
    bool pow2;
    const Mod md = make_mod(m_bits, &pow2);
    const uint64_t row_words = psk_bank_row_bytes(m_bits) / 4;
    return bank_keyed_call(layout, data, offsets, n, key_len, where, ids, out, n, device, stream, [&](auto src, const uint32_t *ids_dev, void *out_dev, hipStream_t st) {
        return with_pow2(pow2, [&](auto P) {
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
    const Mod md = make_mod(m_bits, &pow2);
    const size_t lds = route != 2 && row_bytes <= kBankLdsRowBytes ? (size_t)row_bytes : 0;
    const dim3 grid((unsigned)(filters < kBankGridCap ? filters : kBankGridCap), split);
    return with_source(b, [&](auto src) {
        return with_pow2(pow2, [&](auto P) {
            hipLaunchKernelGGL((k_bank_build<decltype(src), P.value>), grid, dim3(kBlock), lds, st, src, (uint32_t *)table_dev, filters, (uint32_t)(row_bytes / 4), md, k, n,
                               seg_dev, perm_dev, route);
            HIP_TRY(hipGetLastError());
            return (int)PSK_OK;
        });
    });
}

extern "C" uint64_t psk_bank_slice_row_bytes(uint64_t filters) { return ((filters + 7) / 8 + 15) & ~15ULL; }

extern "C" int psk_bank_slices(const void *table_dev, uint64_t filters, uint64_t m_bits, void *slices_dev, uint64_t first_filter, uint64_t last_filter, int device,
                               void *stream)
{
    if (!table_dev || !slices_dev) return fail(PSK_EINVAL, "NULL table or slice image pointer");
    if (((uintptr_t)table_dev | (uintptr_t)slices_dev) & 15) return fail(PSK_EINVAL, "the table and the slice image must be 16-byte aligned");
    PSK_TRY(slice_check_geometry(filters, m_bits));
    if (first_filter > last_filter || last_filter > filters)
        return fail(PSK_EINVAL, "filter range [%llu, %llu) does not lie in the bank's [0, %llu)", (unsigned long long)first_filter, (unsigned long long)last_filter,
                    (unsigned long long)filters);
    if ((first_filter & 31) || ((last_filter & 31) && last_filter != filters))
        return fail(PSK_EINVAL, "a slice range starts at a multiple of 32 filters and ends at one or at the bank's end; [%llu, %llu) was passed",
                    (unsigned long long)first_filter, (unsigned long long)last_filter);
    if (first_filter == last_filter) return PSK_OK;
    const uint64_t srw = psk_bank_slice_row_bytes(filters) / 4;
    const uint64_t word_lo = first_filter >> 5, word_hi = last_filter == filters ? srw : last_filter >> 5;  // (the bank's end takes the row's pad words along)
    const uint64_t col0 = first_filter & ~(uint64_t)(kSliceTileFilters - 1);
    const uint64_t ftiles = (word_hi * 32 - col0 + kSliceTileFilters - 1) / kSliceTileFilters;
    const uint32_t wtiles = (uint32_t)(((m_bits + 31) / 32 + kSliceTileWords - 1) / kSliceTileWords);
    const uint64_t tiles = ftiles * wtiles;
    PSK_USE_DEVICE(device);
    hipLaunchKernelGGL(k_bank_slices, dim3((unsigned)(tiles < kSliceGridCap ? tiles : kSliceGridCap)), dim3(kBlock), 0, (hipStream_t)stream, (const uint32_t *)table_dev,
                       (uint32_t)(psk_bank_row_bytes(m_bits) / 4), m_bits, (uint32_t *)slices_dev, srw, col0, first_filter, last_filter, word_lo, word_hi, wtiles, tiles);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

extern "C" int psk_bank_match(const void *slices_dev, uint64_t filters, uint64_t m_bits, uint32_t k, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                              uint32_t key_len, int where, uint32_t *mask_dev, uint32_t *count_dev, const uint64_t *out_offsets_dev, uint32_t *ids_dev, int device,
                              void *stream)
{
    if (!slices_dev) return fail(PSK_EINVAL, "NULL slice image pointer");
    PSK_TRY(bank_check_args(slices_dev, filters, m_bits, k, layout, n, key_len));
    if (k > kBankMatchMaxK)
        return fail(PSK_EINVAL, "psk_bank_match takes at most %u hashes (k * 1024 bytes of LDS per workgroup); %u were asked for", kBankMatchMaxK, k);
    if (!mask_dev && !count_dev && !ids_dev && !out_offsets_dev) return fail(PSK_EINVAL, "no output: pass mask_dev, count_dev or ids_dev with out_offsets_dev");
    if (!ids_dev != !out_offsets_dev) return fail(PSK_EINVAL, "ids_dev and out_offsets_dev go together");
    if (((uintptr_t)slices_dev | (uintptr_t)mask_dev) & 15) return fail(PSK_EINVAL, "the slice image and mask_dev must be 16-byte aligned");
    const uint64_t quads = psk_bank_slice_row_bytes(filters) / 16;
    uint32_t lgG = 0;
    while (lgG < 6 && (1ULL << lgG) < quads) ++lgG;
    bool pow2;
    const Mod md = make_mod(m_bits, &pow2);
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    ThreadStage &ts = thread_stage();
    Batch b;
    PSK_TRY(stage_batch(ts.keys, ts.offs, layout, data, offsets, n, key_len, where, st, &b));
    if (n)
        PSK_TRY(with_source(b, [&](auto src) {
            return with_pow2(pow2, [&](auto P) {
                hipLaunchKernelGGL((k_bank_match<decltype(src), P.value>), dim3(grid_for_keys(n)), dim3(kBlock), (size_t)k * kBlock * 4, st, src, (const uint4 *)slices_dev,
                                   (uint32_t)quads, md, k, n, lgG, (uint4 *)mask_dev, count_dev, out_offsets_dev, ids_dev);
                HIP_TRY(hipGetLastError());
                return (int)PSK_OK;
            });
        }));
    return finish(where, nullptr, st);
}
