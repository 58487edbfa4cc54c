// psk_bank.hip -- BloomFilterBank (include/psk.h "BloomFilterBank"): many small Bloom filters of one geometry in one table, row f
// the reference's BloomFilter after add() of the keys sent to f (bloom.py:234-272).  The slice a probe belongs to is the caller's filter id, not
// a piece of the hash, and all k probes of a key go to the same row: what the partitioned Bloom step needs pass 1 for is given.
//   psk_bank_add / psk_bank_check   keys with an id each: two ops on k_apply (psk_device.hpp), atomics into / loads from row ids[i]
//   psk_bank_build                  keys grouped by filter: one workgroup per (filter, part) sets the bits in an LDS image of the row and ORs
//                                   the image's non-zero words into the table once (pass 2 of the Bloom step without the pass 1)
//   psk_bank_slices / psk_bank_match  the bank transposed (slice row p = bit p of every filter) and "which filters may hold this key": the AND of
//                                   the key's k slice rows, as a mask, a count or a list of filter ids
//   psk_bank_score / psk_bank_score_select  a query = a set of keys: per filter, how many of the query's keys it may hold (the same row-AND, added
//                                   into bit-plane counters in registers), and the filters of each query that reach a threshold
//   psk_bank_popcount / psk_bank_overlap / psk_bank_reduce  the filters as sets: bits per row, popcount(a AND b) for all pairs (a tiled GEMM over
//                                   (AND, popcount-add)), and the OR / AND of groups of rows stored as a new table
#include "psk_bank_stage.hpp"

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

// The AND of a key's k slice rows at one 16-byte column piece: `col` = the piece in slice row 0, pp[j * stride] = bit position j of the key (LDS),
// rows `quads` pieces apart (64-bit: position * row bytes may pass 2^32).  k independent loads, four in flight.  Shared by k_bank_match and k_bank_score.
__device__ __forceinline__ uint4 bank_row_and(const uint4 *col, const uint32_t *pp, uint32_t stride, uint32_t k, uint32_t quads)
{
    uint4 acc = make_uint4(~0u, ~0u, ~0u, ~0u);
    uint32_t j = 0;
    for (; j + 4 <= k; j += 4) {
        const uint32_t p0 = pp[j * stride], p1 = pp[(j + 1) * stride], p2 = pp[(j + 2) * stride], p3 = pp[(j + 3) * stride];
        const uint4 a0 = col[(uint64_t)p0 * quads], a1 = col[(uint64_t)p1 * quads], a2 = col[(uint64_t)p2 * quads], a3 = col[(uint64_t)p3 * quads];
        acc.x &= a0.x & a1.x & a2.x & a3.x;
        acc.y &= a0.y & a1.y & a2.y & a3.y;
        acc.z &= a0.z & a1.z & a2.z & a3.z;
        acc.w &= a0.w & a1.w & a2.w & a3.w;
    }
    for (; j < k; ++j) {
        const uint4 a = col[(uint64_t)pp[j * stride] * quads];
        acc.x &= a.x, acc.y &= a.y, acc.z &= a.z, acc.w &= a.w;
    }
    return acc;
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
                    acc = bank_row_and(slices + qd, pp, kBlock, k, quads);
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

// ---------------------------------------------------------------- scoring a query (include/psk.h "score"; DESIGN.md 3.13 "Scoring a query")
// k_bank_score: score[q][f] = the number of keys of query q whose k bits are all set in filter f.  The work item is (query, column chunk, part):
// workgroup (x, y) walks the items (q, chunk) = x, x + gridDim.x, ... and takes the y-th of gridDim.y contiguous parts of the query's keys; a chunk
// is up to kScoreChunkQuads 16-byte pieces of the slice rows (8192 filters), so the workgroup's uint32 counters are at most 32 KiB of LDS.  Per round
// of KR keys (256; 128 where k > 32, so that positions + counters never pass 64 KiB): phase A as in k_bank_match, positions to LDS as pos[j][key];
// phase B, G lanes per key, lane = one column piece, bank_row_and, and the 128 result bits go into the lane's vertical counters: kScorePlanes
// bit-planes of a uint4, plane b = bit b of 128 running counts (a ripple add: carry = plane & x, plane ^= x, x = carry).  After 2^P - 1 keys, and at
// the part's end, the planes are flushed into the LDS counters (ds_add of the non-zero values; lane l starts at bit l & 31, so that the 32 lanes of a
// half-wave -- whose columns lie 128 words apart -- hit 32 different banks).  Then the counters go to scores: plain stores where the query is one
// part (zeros included), atomicAdd of the non-zero ones onto the zeroed output otherwise.  Everything that decides a barrier (the item, the part's
// bounds, the round) is uniform over the workgroup; phase B has no shuffle.
constexpr uint32_t kScoreChunkQuads = 64, kScorePlanes = 6, kScoreFlushKeys = (1u << kScorePlanes) - 1;

__device__ __forceinline__ void score_flush(uint32_t (&pl)[kScorePlanes][4], uint32_t *cnt, uint32_t rot)
{
    for (uint32_t s = 0; s < 32; ++s) {
        const uint32_t bit = (s + rot) & 31;
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
            uint32_t v = 0;
#pragma unroll
            for (uint32_t b = 0; b < kScorePlanes; ++b) v |= ((pl[b][c] >> bit) & 1u) << b;
            if (v) atomicAdd(cnt + c * 32 + bit, v);  // ds_add_u32, no return value
        }
    }
#pragma unroll
    for (uint32_t b = 0; b < kScorePlanes; ++b) pl[b][0] = pl[b][1] = pl[b][2] = pl[b][3] = 0;
}

template <class Src, bool POW2>
__global__ __launch_bounds__(kBlock) void k_bank_score(Src src, const uint4 *slices, uint32_t quads, Mod md, uint32_t k, uint64_t n, const uint64_t *qoff,
                                                       uint64_t queries, uint64_t filters, uint32_t chunks, uint32_t KR, uint32_t *scores)
{
    extern __shared__ uint32_t score_lds[];  // counters [min(quads, 64) * 128], then pos [k][KR]
    const uint32_t cwords = (quads < kScoreChunkQuads ? quads : kScoreChunkQuads) * 128u;
    uint32_t *cnt = score_lds, *pos = score_lds + cwords;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kpw = KR >> 2;  // keys per wave and round
    const uint32_t split = gridDim.y, part = blockIdx.y;
    const uint64_t items = queries * chunks;
    for (uint64_t w = blockIdx.x; w < items; w += gridDim.x) {
        const uint64_t q = w / chunks;
        const uint32_t q0 = (uint32_t)(w % chunks) * kScoreChunkQuads;                  // the chunk's first piece
        const uint32_t cq = quads - q0 < kScoreChunkQuads ? quads - q0 : kScoreChunkQuads;  // ... and its pieces
        uint64_t s0 = qoff[q], s1 = qoff[q + 1];
        if (s1 > n) s1 = n;  // (no key is read at or beyond n whatever the offsets hold)
        if (s0 > s1) s0 = s1;
        const uint64_t per = (s1 - s0 + split - 1) / split;
        const uint64_t a = s0 + per * part;
        if (split > 1 && a >= s1) continue;  // an empty part of a query in parts: the entry point zeroed the output
        const uint64_t b = a + per < s1 ? a + per : s1;
        uint32_t lgG = 0;
        while ((1u << lgG) < cq) ++lgG;
        const uint32_t G = 1u << lgG, gl = lane & (G - 1), sub = lane >> lgG, slots = 64u >> lgG;
        for (uint32_t i = threadIdx.x; i < cq * 128u; i += kBlock) cnt[i] = 0;
        __syncthreads();
        uint32_t pl[kScorePlanes][4] = {};
        uint32_t pending = 0;
        for (uint64_t base = a; base < b; base += KR) {
            const uint64_t i = base + threadIdx.x;
            if (threadIdx.x < KR && i < b) {
                const typename Src::Key key = src.load(i);
                for_each_hash(src, key, i, k, [&](uint32_t j, uint64_t h) { pos[j * KR + threadIdx.x] = bank_bit<POW2>(md, h); });
            }
            __syncthreads();
            const uint64_t wbase = base + wave * kpw;
            for (uint32_t t0 = 0; t0 < kpw && wbase + t0 < b; t0 += slots) {
                const uint32_t t = t0 + sub;
                if (t < kpw && wbase + t < b && gl < cq) {
                    uint4 x = bank_row_and(slices + q0 + gl, pos + wave * kpw + t, KR, k, quads);
#pragma unroll
                    for (uint32_t p = 0; p < kScorePlanes; ++p) {
                        const uint4 c = make_uint4(pl[p][0] & x.x, pl[p][1] & x.y, pl[p][2] & x.z, pl[p][3] & x.w);
                        pl[p][0] ^= x.x, pl[p][1] ^= x.y, pl[p][2] ^= x.z, pl[p][3] ^= x.w;
                        x = c;
                    }
                }
                if (++pending == kScoreFlushKeys) {  // (uniform over the wave: a count of rounds, not of live keys)
                    if (gl < cq) score_flush(pl, cnt + gl * 128u, lane & 31);
                    pending = 0;
                }
            }
            __syncthreads();  // the next round's positions must not overtake these reads
        }
        if (gl < cq) score_flush(pl, cnt + gl * 128u, lane & 31);
        __syncthreads();
        uint32_t *row = scores + q * filters;  // (64-bit: queries * filters may pass 2^32)
        for (uint32_t i = threadIdx.x; i < cq * 128u; i += kBlock) {
            const uint64_t f = (uint64_t)q0 * 128u + i;
            if (f >= filters) break;
            const uint32_t v = cnt[i];
            if (split == 1) row[f] = v;
            else if (v) atomicAdd(row + f, v);
        }
        __syncthreads();  // the next item's clear must not overtake this sweep
    }
}

// k_bank_score_select: the filters of a row of finished scores that reach the row's threshold.  WAVE: a wave per row, four rows per workgroup
// (rows of up to kScoreSelWaveCols columns); else a workgroup per row.  Rows beyond the grid are walked with a stride.  A pass over 64 (256)
// columns: the ballot of score >= threshold gives a lane its rank among the pass's hits, the hits before the pass are a running sum (the workgroup
// form adds the waves in front through LDS).  count: hits per row; ids / hit_scores: written at out_offs[row], ascending by column.
constexpr uint32_t kScoreSelWaveCols = 2048;
template <bool WAVE>
__global__ __launch_bounds__(kBlock) void k_bank_score_select(const uint32_t *scores, uint64_t queries, uint64_t filters, const uint32_t *thr, uint32_t *count,
                                                              const uint64_t *out_offs, uint32_t *ids, uint32_t *hit_scores)
{
    __shared__ uint32_t wsum[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t below = (1ULL << lane) - 1;
    const uint64_t step = WAVE ? (uint64_t)gridDim.x * 4 : gridDim.x;
    for (uint64_t q = WAVE ? (uint64_t)blockIdx.x * 4 + wave : blockIdx.x; q < queries; q += step) {  // (WAVE: uniform over the wave, no barrier below)
        const uint32_t *row = scores + q * filters;
        const uint32_t t = thr[q];
        const uint64_t wr = ids ? out_offs[q] : 0;
        uint64_t hits = 0;
        for (uint64_t c0 = 0; c0 < filters; c0 += WAVE ? 64 : kBlock) {
            const uint64_t f = c0 + (WAVE ? lane : threadIdx.x);
            const uint32_t v = f < filters ? row[f] : 0;
            const bool hit = f < filters && v >= t;
            const uint64_t bal = __ballot(hit);
            uint32_t before = 0, total = (uint32_t)__popcll(bal);
            if (!WAVE) {
                if (lane == 0) wsum[wave] = total;
                __syncthreads();
                for (uint32_t x = 0; x < wave; ++x) before += wsum[x];
                total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
                __syncthreads();
            }
            if (hit && ids) {
                const uint64_t o = wr + hits + before + (uint32_t)__popcll(bal & below);
                ids[o] = (uint32_t)f;
                if (hit_scores) hit_scores[o] = v;
            }
            hits += total;
        }
        if (count && (WAVE ? lane == 0 : threadIdx.x == 0)) count[q] = (uint32_t)hits;
    }
}

// ---------------------------------------------------------------- the filters as sets (include/psk.h "bank statistics")
// Rows are read whole, 16 bytes a lane: the pad bits of a row are never set, so a popcount over the padded row is the filter's bit count.
__device__ __forceinline__ uint32_t popc4(uint4 v) { return __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w); }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (uint32_t o = 1; o < 64; o <<= 1) v += (uint32_t)__shfl_xor((int)v, (int)o);
    return v;
}

// sum over the workgroup, in every thread; `red` = 4 words of LDS.  Two barriers: the caller may call it again at once.
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *red)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return v;
}

// k_bank_popcount: WAVE: a wave per row, four rows per workgroup (rows of up to kBankPopWaveQuads 16-byte pieces); else a workgroup per row.
// Row groups beyond the grid are walked with a stride.  Everything that decides a shuffle or a barrier is wave- / workgroup-uniform.
constexpr uint32_t kBankPopWaveQuads = 256;  // 4 KiB: up to four loads per lane; wider rows take the whole workgroup
template <bool WAVE>
__global__ __launch_bounds__(kBlock) void k_bank_popcount(const uint4 *tab, uint64_t filters, uint32_t quads, const uint32_t *ids, uint64_t n, uint64_t *out)
{
    __shared__ uint32_t red[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t per = WAVE ? 4 : 1, me = WAVE ? lane : threadIdx.x, step = WAVE ? 64 : kBlock;
    for (uint64_t base = (uint64_t)blockIdx.x * per; base < n; base += (uint64_t)gridDim.x * per) {
        const uint64_t i = base + (WAVE ? wave : 0);
        const uint64_t f = i < n ? (ids ? ids[i] : i) : filters;
        uint32_t c = 0;
        if (f < filters) {
            const uint4 *row = tab + f * quads;  // (64-bit: filters * row_bytes may exceed 2^32)
            for (uint32_t q = me; q < quads; q += step) c += popc4(row[q]);
        }
        if (WAVE) {
            c = wave_sum(c);
            if (lane == 0 && i < n) out[i] = c;
        } else {
            c = block_sum(c, red);
            if (threadIdx.x == 0) out[i] = c;
        }
    }
}

// k_bank_overlap: out[i][j] = popcount(row a_i AND row b_j): a GEMM over the (AND, popcount-add) semiring.  A workgroup owns a T x T tile of
// outputs, thread (ty, tx) = (tid >> 4, tid & 15) the 4 x 4 block at (4 ty, 4 tx).  The rows are walked in chunks of C words.  A chunk of the T
// a-rows and of the T b-rows is loaded 16 bytes a lane -- four lanes read 64 contiguous bytes of one row, row pointers resolved through the id
// lists -- and parked in LDS TRANSPOSED: word w of row r at [w][r], so that a thread's four rows at one word are ONE ds_read_b128.  The stride
// of [w] is T + 4 words (a multiple of 4: the 16-byte reads stay aligned): the four ds_write_b32 of a lane fall on banks
// (16 (quad & 1) + 4 j + row) mod 32 -- inside a 32-lane half (8 rows x 4 quads) 16 different banks, two lanes each, which a ds_write_b32 takes
// at no extra cost; without the pad all four quads of a row would meet on ONE bank.  The reads: the a-side has 4 addresses per wave (broadcast),
// the b-side 16 consecutive 16-byte pieces.  Per word and thread: 2 ds_read_b128 (8 dwords) feed 16 v_and_b32 + 16 v_bcnt_u32_b32.
// A chunk's global loads are issued before the chunk in LDS is computed and land in registers under it.
// Edges: a row beyond na / nb (a tile that hangs over) or an id beyond its table loads zeros; a chunk beyond the row's end loads zeros and the
// inner loop stops at the row's last word; only outputs inside [na, nb) are stored.  Tiles are linearised on x and walked with a stride.
// Few tiles of long rows (two filters of 2^31 bits are ONE tile) are cut along the rows: `splits` workgroups per tile take split_words words
// each and add their counts into the zeroed output with atomics.
// SYM (same table, same ids, na == nb): only tiles with tj >= ti exist (t = tj (tj + 1) / 2 + ti); each is stored at (ti, tj) and, off the
// diagonal, transposed at (tj, ti).
constexpr uint32_t kBankOvlT = 64, kBankOvlC = 32, kBankOvlStride = kBankOvlT + 4;
constexpr uint32_t kBankOvlSplitChunks = 16;  // a part of a row, where rows are cut, is at least this many chunks
constexpr uint32_t kBankOvlLoads = kBankOvlT * (kBankOvlC / 4) / kBlock;  // 16-byte loads per thread, chunk and side: 2
static_assert(kBankOvlT == 64 && kBlock == 256 && kBankOvlC % 16 == 0, "the thread layout of k_bank_overlap");

template <bool SYM>
__global__ __launch_bounds__(kBlock) void k_bank_overlap(const uint4 *ta, uint64_t filters_a, const uint32_t *a_ids, uint64_t na, const uint4 *tb, uint64_t filters_b,
                                                         const uint32_t *b_ids, uint64_t nb, uint32_t quads, uint32_t *out, uint64_t tiles_j, uint64_t work, int vec,
                                                         uint32_t splits, uint32_t split_words)
{
    __shared__ __attribute__((aligned(16))) uint32_t la[kBankOvlC * kBankOvlStride], lb[kBankOvlC * kBankOvlStride];
    const uint32_t tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const uint32_t lrow = threadIdx.x >> 2, lq = threadIdx.x & 3;  // the load: row lrow of the tile, 16-byte piece lq + 4 p of the chunk
    for (uint64_t item = blockIdx.x; item < work; item += gridDim.x) {
        const uint64_t t = item / splits;
        const uint32_t w_lo = (uint32_t)(item % splits) * split_words;  // this workgroup's words of the rows: [w_lo, w_hi), whole chunks but for the row's end
        const uint32_t w_hi = quads * 4 - w_lo < split_words ? quads * 4 : w_lo + split_words;
        uint64_t ti, tj;
        if (SYM) {
            tj = (uint64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
            while (tj * (tj + 1) / 2 > t) --tj;
            while ((tj + 1) * (tj + 2) / 2 <= t) ++tj;
            ti = t - tj * (tj + 1) / 2;
        } else {
            ti = t / tiles_j, tj = t % tiles_j;
        }
        const uint64_t i0 = ti * kBankOvlT, j0 = tj * kBankOvlT;
        const uint64_t ia = i0 + lrow, jb = j0 + lrow;
        const uint64_t fa = ia < na ? (a_ids ? a_ids[ia] : ia) : filters_a;
        const uint64_t fb = jb < nb ? (b_ids ? b_ids[jb] : jb) : filters_b;
        const uint4 *ra = fa < filters_a ? ta + fa * quads : nullptr;  // (64-bit: filters * row_bytes may exceed 2^32)
        const uint4 *rb = fb < filters_b ? tb + fb * quads : nullptr;
        uint32_t acc[4][4] = {};
        uint4 va[kBankOvlLoads], vb[kBankOvlLoads];
        // step s: issue the loads of chunk s, compute chunk s - 1 from LDS under them, then park chunk s
        for (uint32_t w0 = w_lo;; w0 += kBankOvlC) {
            const bool more = w0 < w_hi;
            if (more) {
#pragma unroll
                for (uint32_t p = 0; p < kBankOvlLoads; ++p) {
                    const uint32_t q = (w0 >> 2) + lq + 4 * p;
                    va[p] = vb[p] = make_uint4(0u, 0u, 0u, 0u);
                    if (ra && q < quads) va[p] = ra[q];
                    if (rb && q < quads) vb[p] = rb[q];
                }
            }
            if (w0 != w_lo) {
                const uint32_t left = w_hi - (w0 - kBankOvlC), cw = left < kBankOvlC ? left : kBankOvlC;  // (a multiple of 4)
#pragma clang loop vectorize(disable) unroll(disable)
                for (uint32_t w4 = 0; w4 < cw; w4 += 4)
#pragma unroll
                for (uint32_t w = w4; w < w4 + 4; ++w) {
                    const uint4 a = *reinterpret_cast<const uint4 *>(la + w * kBankOvlStride + 4 * ty);
                    const uint4 b = *reinterpret_cast<const uint4 *>(lb + w * kBankOvlStride + 4 * tx);
                    acc[0][0] += __popc(a.x & b.x), acc[0][1] += __popc(a.x & b.y), acc[0][2] += __popc(a.x & b.z), acc[0][3] += __popc(a.x & b.w);
                    acc[1][0] += __popc(a.y & b.x), acc[1][1] += __popc(a.y & b.y), acc[1][2] += __popc(a.y & b.z), acc[1][3] += __popc(a.y & b.w);
                    acc[2][0] += __popc(a.z & b.x), acc[2][1] += __popc(a.z & b.y), acc[2][2] += __popc(a.z & b.z), acc[2][3] += __popc(a.z & b.w);
                    acc[3][0] += __popc(a.w & b.x), acc[3][1] += __popc(a.w & b.y), acc[3][2] += __popc(a.w & b.z), acc[3][3] += __popc(a.w & b.w);
                }
            }
            if (!more) break;
            __syncthreads();  // every thread is done reading the chunk before (the tile before)
#pragma unroll
            for (uint32_t p = 0; p < kBankOvlLoads; ++p) {
                uint32_t *da = la + (4 * (lq + 4 * p)) * kBankOvlStride + lrow, *db = lb + (4 * (lq + 4 * p)) * kBankOvlStride + lrow;
                da[0] = va[p].x, da[kBankOvlStride] = va[p].y, da[2 * kBankOvlStride] = va[p].z, da[3 * kBankOvlStride] = va[p].w;
                db[0] = vb[p].x, db[kBankOvlStride] = vb[p].y, db[2 * kBankOvlStride] = vb[p].z, db[3 * kBankOvlStride] = vb[p].w;
            }
            __syncthreads();
        }
        const uint64_t oi = i0 + 4 * ty, oj = j0 + 4 * tx;
        if (splits > 1) {  // (uniform) the parts of a pair's rows meet in the zeroed output through atomics
#pragma unroll
            for (uint32_t r = 0; r < 4; ++r)
#pragma unroll
                for (uint32_t c = 0; c < 4; ++c) {
                    if (oi + r >= na || oj + c >= nb || !acc[r][c]) continue;
                    atomicAdd(out + (oi + r) * nb + oj + c, acc[r][c]);
                    if (SYM && ti != tj) atomicAdd(out + (oj + c) * nb + oi + r, acc[r][c]);
                }
            continue;
        }
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
            if (oi + r >= na) continue;
            uint32_t *o = out + (oi + r) * nb + oj;
            if (vec && oj + 4 <= nb) {
                *reinterpret_cast<uint4 *>(o) = make_uint4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
            } else {
#pragma unroll
                for (uint32_t c = 0; c < 4; ++c)
                    if (oj + c < nb) o[c] = acc[r][c];
            }
        }
        if (SYM && ti != tj) {  // (na == nb: the transposed block lies at rows oj .., columns oi ..)
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c) {
                if (oj + c >= nb) continue;
                uint32_t *o = out + (oj + c) * nb + oi;
                if (vec && oi + 4 <= na) {
                    *reinterpret_cast<uint4 *>(o) = make_uint4(acc[0][c], acc[1][c], acc[2][c], acc[3][c]);
                } else {
#pragma unroll
                    for (uint32_t r = 0; r < 4; ++r)
                        if (oi + r < na) o[r] = acc[r][c];
                }
            }
        }
    }
}

// k_bank_reduce: a workgroup per (group, piece of kBlock 16-byte pieces of the row), linearised on x and walked with a stride.  A thread folds its
// 16 bytes of the group's member rows in registers (four members' loads in flight), STORES the result and adds the piece's popcount to
// bits[g]: a plain store where the row is one piece, an atomic on the zeroed counter else.  An empty group stores zeros under either op; a
// member >= filters counts as an empty row.
__global__ __launch_bounds__(kBlock) void k_bank_reduce(const uint4 *src, uint64_t filters, uint32_t quads, const uint64_t *seg, const uint32_t *members, uint64_t groups,
                                                        int op_and, uint4 *dst, uint64_t *bits, uint32_t pieces, uint64_t work)
{
    __shared__ uint32_t red[4];
    for (uint64_t t = blockIdx.x; t < work; t += gridDim.x) {
        const uint64_t g = t / pieces;
        const uint32_t q = (uint32_t)(t % pieces) * kBlock + threadIdx.x;
        const uint64_t s0 = seg[g], s1 = seg[g + 1];
        const bool on = q < quads;
        const uint32_t init = op_and && s1 > s0 ? ~0u : 0u;
        uint4 acc = make_uint4(init, init, init, init);
        if (on) {
            auto row = [&](uint64_t j) {
                const uint64_t f = members[j];
                return f < filters ? src[f * quads + q] : make_uint4(0u, 0u, 0u, 0u);
            };
            auto fold = [&](const uint4 &v) {
                if (op_and) acc.x &= v.x, acc.y &= v.y, acc.z &= v.z, acc.w &= v.w;
                else acc.x |= v.x, acc.y |= v.y, acc.z |= v.z, acc.w |= v.w;
            };
            uint64_t j = s0;
            for (; j + 4 <= s1; j += 4) {
                const uint4 v0 = row(j), v1 = row(j + 1), v2 = row(j + 2), v3 = row(j + 3);
                fold(v0), fold(v1), fold(v2), fold(v3);
            }
            for (; j < s1; ++j) fold(row(j));
            dst[g * quads + q] = acc;
        }
        if (bits) {  // (uniform)
            const uint32_t c = block_sum(on ? popc4(acc) : 0u, red);
            if (threadIdx.x == 0) {
                if (pieces == 1) bits[g] = c;
                else if (c) atomicAdd(reinterpret_cast<unsigned long long *>(bits + g), (unsigned long long)c);
            }
        }
    }
}

int stats_check_table(const void *table_dev, uint64_t filters, uint64_t m_bits)
{
    if (!table_dev) return fail(PSK_EINVAL, "NULL table pointer");
    if ((uintptr_t)table_dev & 15) return fail(PSK_EINVAL, "a bank table must be 16-byte aligned");
    return slice_check_geometry(filters, m_bits);
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

extern "C" int psk_bank_score(const void *slices_dev, uint64_t filters, uint64_t m_bits, uint32_t k, int layout, const void *data, const uint64_t *offsets, uint64_t n,
                              uint32_t key_len, int where, const uint64_t *query_offsets_dev, uint64_t queries, uint32_t split, uint32_t *scores_dev, int device,
                              void *stream)
{
    if (!slices_dev) return fail(PSK_EINVAL, "NULL slice image pointer");
    PSK_TRY(bank_check_args(slices_dev, filters, m_bits, k, layout, n, key_len));
    if (k > kBankMatchMaxK)
        return fail(PSK_EINVAL, "psk_bank_score takes at most %u hashes (the positions of a round of keys live in LDS); %u were asked for", kBankMatchMaxK, k);
    if (!query_offsets_dev || !scores_dev) return fail(PSK_EINVAL, "query_offsets_dev or scores_dev is NULL");
    if (split < 1 || split > 65535) return fail(PSK_EINVAL, "split must be 1 .. 65535 workgroups per query; %u was passed", split);
    if ((uintptr_t)slices_dev & 15) return fail(PSK_EINVAL, "the slice image must be 16-byte aligned");
    if (queries == 0) return PSK_OK;
    const uint64_t quads = psk_bank_slice_row_bytes(filters) / 16;
    const uint64_t chunks = (quads + kScoreChunkQuads - 1) / kScoreChunkQuads;
    const uint32_t KR = k <= 32 ? kBlock : kBlock / 2;  // positions + counters stay within 64 KiB of LDS
    const size_t lds = ((size_t)(quads < kScoreChunkQuads ? quads : kScoreChunkQuads) * 128 + (size_t)k * KR) * 4;
    bool pow2;
    const Mod md = make_mod(m_bits, &pow2);
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    if (split > 1 || n == 0) HIP_TRY(hipMemsetAsync(scores_dev, 0, (size_t)queries * filters * 4, st));
    if (n == 0) return PSK_OK;  // (no keys: every row is zeros, no kernel)
    ThreadStage &ts = thread_stage();
    Batch b;
    PSK_TRY(stage_batch(ts.keys, ts.offs, layout, data, offsets, n, key_len, where, st, &b));
    const uint64_t items = queries * chunks;
    const dim3 grid((unsigned)(items < kBankGridCap ? items : kBankGridCap), split);
    PSK_TRY(with_source(b, [&](auto src) {
        return with_pow2(pow2, [&](auto P) {
            hipLaunchKernelGGL((k_bank_score<decltype(src), P.value>), grid, dim3(kBlock), lds, st, src, (const uint4 *)slices_dev, (uint32_t)quads, md, k, n,
                               query_offsets_dev, queries, filters, (uint32_t)chunks, KR, scores_dev);
            HIP_TRY(hipGetLastError());
            return (int)PSK_OK;
        });
    }));
    return finish(where, nullptr, st);
}

extern "C" int psk_bank_score_select(const uint32_t *scores_dev, uint64_t queries, uint64_t filters, const uint32_t *thresholds_dev, uint32_t *count_dev,
                                     const uint64_t *out_offsets_dev, uint32_t *ids_dev, uint32_t *hit_scores_dev, int device, void *stream)
{
    if (!scores_dev || !thresholds_dev) return fail(PSK_EINVAL, "scores_dev or thresholds_dev is NULL");
    if (filters == 0 || filters > (1ULL << 32)) return fail(PSK_EINVAL, "a bank holds 1 .. 2^32 filters; %llu were asked for", (unsigned long long)filters);
    if (!count_dev && !ids_dev && !out_offsets_dev && !hit_scores_dev) return fail(PSK_EINVAL, "no output: pass count_dev, or ids_dev with out_offsets_dev");
    if (!ids_dev != !out_offsets_dev) return fail(PSK_EINVAL, "ids_dev and out_offsets_dev go together");
    if (hit_scores_dev && !ids_dev) return fail(PSK_EINVAL, "hit_scores_dev goes with ids_dev");
    if (queries == 0) return PSK_OK;
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    if (filters <= kScoreSelWaveCols) {
        const uint64_t groups = (queries + 3) / 4;
        hipLaunchKernelGGL(k_bank_score_select<true>, dim3((unsigned)(groups < kBankGridCap ? groups : kBankGridCap)), dim3(kBlock), 0, st, scores_dev, queries, filters,
                           thresholds_dev, count_dev, out_offsets_dev, ids_dev, hit_scores_dev);
    } else {
        hipLaunchKernelGGL(k_bank_score_select<false>, dim3((unsigned)(queries < kBankGridCap ? queries : kBankGridCap)), dim3(kBlock), 0, st, scores_dev, queries, filters,
                           thresholds_dev, count_dev, out_offsets_dev, ids_dev, hit_scores_dev);
    }
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

// ---------------------------------------------------------------- bank statistics: bit counts, all-pairs overlap, row folds
extern "C" int psk_bank_popcount(const void *table_dev, uint64_t filters, uint64_t m_bits, const uint32_t *ids_dev, uint64_t n, uint64_t *out_dev, int device,
                                 void *stream)
{
    PSK_TRY(stats_check_table(table_dev, filters, m_bits));
    if (!ids_dev && n != filters)
        return fail(PSK_EINVAL, "without ids every row is counted: n must be the number of filters (%llu), not %llu", (unsigned long long)filters, (unsigned long long)n);
    if (n == 0) return PSK_OK;
    if (!out_dev) return fail(PSK_EINVAL, "out_dev is NULL");
    const uint64_t quads = psk_bank_row_bytes(m_bits) / 16;
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    if (quads <= kBankPopWaveQuads) {
        const uint64_t wgs = (n + 3) / 4;
        hipLaunchKernelGGL(k_bank_popcount<true>, dim3((unsigned)(wgs < kBankGridCap ? wgs : kBankGridCap)), dim3(kBlock), 0, st, (const uint4 *)table_dev, filters,
                           (uint32_t)quads, ids_dev, n, out_dev);
    } else {
        hipLaunchKernelGGL(k_bank_popcount<false>, dim3((unsigned)(n < kBankGridCap ? n : kBankGridCap)), dim3(kBlock), 0, st, (const uint4 *)table_dev, filters,
                           (uint32_t)quads, ids_dev, n, out_dev);
    }
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

extern "C" int psk_bank_overlap(const void *table_a_dev, uint64_t filters_a, const uint32_t *a_ids_dev, uint64_t na, const void *table_b_dev, uint64_t filters_b,
                                const uint32_t *b_ids_dev, uint64_t nb, uint64_t m_bits, uint32_t *out_dev, int device, void *stream)
{
    PSK_TRY(stats_check_table(table_a_dev, filters_a, m_bits));
    PSK_TRY(stats_check_table(table_b_dev, filters_b, m_bits));
    if (!a_ids_dev && na > filters_a)
        return fail(PSK_EINVAL, "without a_ids rows 0 .. na - 1 are taken: na = %llu exceeds the table's %llu filters", (unsigned long long)na, (unsigned long long)filters_a);
    if (!b_ids_dev && nb > filters_b)
        return fail(PSK_EINVAL, "without b_ids rows 0 .. nb - 1 are taken: nb = %llu exceeds the table's %llu filters", (unsigned long long)nb, (unsigned long long)filters_b);
    if ((na >> 32) || (nb >> 32)) return fail(PSK_EINVAL, "an overlap call takes fewer than 2^32 rows a side; %llu x %llu were passed", (unsigned long long)na, (unsigned long long)nb);
    if (na == 0 || nb == 0) return PSK_OK;
    if (!out_dev) return fail(PSK_EINVAL, "out_dev is NULL");
    const uint64_t quads = psk_bank_row_bytes(m_bits) / 16;
    const uint64_t tiles_i = (na + kBankOvlT - 1) / kBankOvlT, tiles_j = (nb + kBankOvlT - 1) / kBankOvlT;
    const bool sym = table_a_dev == table_b_dev && a_ids_dev == b_ids_dev && na == nb && filters_a == filters_b;
    const uint64_t tiles = sym ? tiles_i * (tiles_i + 1) / 2 : tiles_i * tiles_j;
    const int vec = (nb & 3) == 0 && ((uintptr_t)out_dev & 15) == 0;  // 16-byte stores of a thread's four columns
    // fewer tiles than the grid holds: cut the rows into parts of at least kBankOvlSplitChunks chunks until the grid is full
    const uint64_t chunks = (quads * 4 + kBankOvlC - 1) / kBankOvlC;
    uint64_t splits = chunks / kBankOvlSplitChunks < kBankGridCap / tiles ? chunks / kBankOvlSplitChunks : kBankGridCap / tiles;
    if (splits < 1) splits = 1;
    const uint64_t per = (chunks + splits - 1) / splits;
    splits = (chunks + per - 1) / per;  // (no empty part)
    const uint64_t work = tiles * splits;
    const dim3 grid((unsigned)(work < kBankGridCap ? work : kBankGridCap));
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    if (splits > 1) HIP_TRY(hipMemsetAsync(out_dev, 0, na * nb * sizeof(uint32_t), st));
    if (sym)
        hipLaunchKernelGGL(k_bank_overlap<true>, grid, dim3(kBlock), 0, st, (const uint4 *)table_a_dev, filters_a, a_ids_dev, na, (const uint4 *)table_b_dev, filters_b,
                           b_ids_dev, nb, (uint32_t)quads, out_dev, tiles_j, work, vec, (uint32_t)splits, (uint32_t)(per * kBankOvlC));
    else
        hipLaunchKernelGGL(k_bank_overlap<false>, grid, dim3(kBlock), 0, st, (const uint4 *)table_a_dev, filters_a, a_ids_dev, na, (const uint4 *)table_b_dev, filters_b,
                           b_ids_dev, nb, (uint32_t)quads, out_dev, tiles_j, work, vec, (uint32_t)splits, (uint32_t)(per * kBankOvlC));
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

extern "C" int psk_bank_reduce(const void *src_dev, uint64_t filters, uint64_t m_bits, const uint64_t *seg_dev, const uint32_t *members_dev, uint64_t groups, int op,
                               void *dst_dev, uint64_t *bits_dev, int device, void *stream)
{
    PSK_TRY(stats_check_table(src_dev, filters, m_bits));
    if (op != 0 && op != 1) return fail(PSK_EINVAL, "op must be 0 (OR) or 1 (AND); %d was passed", op);
    if (groups >> 32) return fail(PSK_EINVAL, "a reduce call takes fewer than 2^32 groups; %llu were passed", (unsigned long long)groups);
    if (groups == 0) return PSK_OK;
    if (!dst_dev || ((uintptr_t)dst_dev & 15)) return fail(PSK_EINVAL, "dst_dev must be a 16-byte aligned device pointer");
    if (!seg_dev) return fail(PSK_EINVAL, "seg_dev is NULL");
    const uint64_t row_bytes = psk_bank_row_bytes(m_bits), quads = row_bytes / 16;
    const uintptr_t s0 = (uintptr_t)src_dev, s1 = s0 + filters * row_bytes, d0 = (uintptr_t)dst_dev, d1 = d0 + groups * row_bytes;
    if (d0 < s1 && s0 < d1) return fail(PSK_EINVAL, "dst overlaps src: a fold is stored, never done in place");
    const uint64_t pieces = (quads + kBlock - 1) / kBlock, work = groups * pieces;
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    if (bits_dev && pieces > 1) HIP_TRY(hipMemsetAsync(bits_dev, 0, groups * sizeof(uint64_t), st));
    hipLaunchKernelGGL(k_bank_reduce, dim3((unsigned)(work < kBankGridCap ? work : kBankGridCap)), dim3(kBlock), 0, st, (const uint4 *)src_dev, filters, (uint32_t)quads,
                       seg_dev, members_dev, groups, op, (uint4 *)dst_dev, bits_dev, (uint32_t)pieces, work);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}
