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
// This header holds what is templated over the key source (the triples and the fused lookup) and what the counting filter shares with the
// plain one (psk_counting_cuckoo.hip): a table of W words per slot -- W = 1: the fingerprint, W = 2: (fingerprint, count), a row still
// filled from the left -- goes through the same row scan, placement, kick walk (with its MT19937) and row compaction.
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

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint8_t kKick = 3;

struct CkTable {
    uint32_t *buckets, *fill;
};

// `fp in buckets[row]` (cuckoo.py:440-446) -> the first slot that holds it, kNone: none.  Unused slots hold 0, so only fingerprint 0 has
// to look at the row's count.
template <uint32_t W>
__device__ __forceinline__ uint32_t ck_row_find(const CkGeom &g, const uint32_t *buckets, const uint32_t *fill, uint32_t row, uint32_t fp)
{
    const uint32_t *p = buckets + (uint64_t)row * g.B * W;
    const uint32_t f = fp ? g.B : min(fill[row], g.B);
    for (uint32_t s = 0; s < f; ++s)
        if (p[(uint64_t)s * W] == fp) return s;
    return kNone;
}

__device__ __forceinline__ bool ck_row_has(const CkGeom &g, const uint32_t *buckets, const uint32_t *fill, uint32_t row, uint32_t fp)
{
    return ck_row_find<1>(g, buckets, fill, row, fp) != kNone;
}

template <uint32_t W = 1>
__device__ __forceinline__ bool ck_contains(const CkGeom &g, const uint32_t *buckets, const uint32_t *fill, const CkTriple &t)
{
    if (ck_row_find<W>(g, buckets, fill, t.i1, t.fp) != kNone) return true;
    return t.i2 != t.i1 && ck_row_find<W>(g, buckets, fill, t.i2, t.fp) != kNone;
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

// ---- shared by the plain filter (W = 1) and the counting one (W = 2)
template <uint32_t W>
__global__ __launch_bounds__(kBlock) void k_ck_present(CkGeom g, const uint32_t *buckets, const uint32_t *fill, const uint32_t *tr, uint64_t n, uint8_t *out)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
    {
        const CkTriple t{tr[i], tr[n + i], tr[2 * n + i]};
        out[i] = t.i1 < g.capacity && t.i2 < g.capacity && ck_contains<W>(g, buckets, fill, t) ? 1 : 0;
    }
}

// ---- parallel placement
// claims[p] = bucket << 32 | j << 1 | which, ascending; pos[which * m + j] = where key j's claim `which` stands in it.
// -> the number of active claims of bucket b in front of position p that belong to keys t < j, counted up to `room`; kNone after kMaxWalk
//    claims without an answer.  The caller then decides K, which only ends the accepted prefix early (the sequential kernel does that key
//    exactly, kick or not): the map stays triangular, so the stable-prefix argument holds for it, and in front of the first such K it is the
//    reference's.  A window holds at most capacity * B keys, 2 B claims per bucket on average; only crafted fingerprints get near kMaxWalk.
constexpr uint32_t kMaxWalk = 1024;
__device__ __forceinline__ uint32_t ck_active_before(const unsigned long long *claims, const uint8_t *d, uint32_t m, uint32_t p, uint32_t b, uint32_t j, uint32_t room)
{
    uint32_t c = 0;
    if (p >= 2u * m) return room;  // (not a position of this claim list: a caller's garbage decides "no room")
    for (uint32_t walked = 0; p > 0 && c < room; ++walked) {
        if (walked == kMaxWalk) return kNone;
        const unsigned long long cl = claims[--p];
        if ((uint32_t)(cl >> 32) != b) break;
        const uint32_t t = (uint32_t)cl >> 1, which = (uint32_t)cl & 1u;
        if (t != j && t < m && d[t] == which + 1u) ++c;  // (t == j: the key's own other claim, when idx_1 == idx_2)
    }
    return c;
}

// keys [0, p) with final decisions: write the fingerprints -- W = 2: with counts[j], 1 where `counts` is NULL -- (fill is read, not
// written: k_ck_count follows)
template <uint32_t W>
__global__ __launch_bounds__(kBlock) void k_ck_apply(CkGeom g, CkTable t, const uint32_t *tr, const unsigned long long *claims, const uint32_t *pos, uint32_t m,
                                                     const uint8_t *d, uint32_t p, const uint32_t *counts)
{
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < p; j += stride) {
        const uint32_t which = d[j] - 1u;
        if (which > 1u) continue;
        const uint32_t b = tr[(uint64_t)(1 + which) * m + j];
        if (b >= g.capacity) continue;
        // (a key that decided 1 or 2 saw its whole segment within kMaxWalk, and this is the same walk)
        const uint32_t c = ck_active_before(claims, d, m, pos[(uint64_t)which * m + j], b, j, g.B);
        const uint32_t slot = c == kNone ? kNone : t.fill[b] + c;
        if (slot < g.B) {
            uint32_t *q = t.buckets + ((uint64_t)b * g.B + slot) * W;
            q[0] = tr[j];
            if constexpr (W == 2) q[1] = counts ? counts[j] : 1u;
        }
    }
}

static __global__ __launch_bounds__(kBlock) void k_ck_count(CkGeom g, uint32_t *fill, const uint32_t *tr, uint32_t m, const uint8_t *d, uint32_t p)
{
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < p; j += stride) {
        const uint32_t which = d[j] - 1u;
        if (which > 1u) continue;
        const uint32_t b = tr[(uint64_t)(1 + which) * m + j];
        if (b < g.capacity) atomicAdd(fill + b, 1u);
    }
}

// ---- sequential insert
struct Mt {
    uint32_t *w;  // 624 words in LDS
    uint32_t idx;
    bool bad;
    __device__ uint32_t next()
    {
        if (idx >= 624u) {  // genrand_uint32 of _randommodule.c: regenerate the block
            for (uint32_t k = 0; k < 624u; ++k) {
                const uint32_t y = (w[k] & 0x80000000u) | (w[k == 623u ? 0u : k + 1u] & 0x7FFFFFFFu);
                w[k] = w[k < 227u ? k + 397u : k - 227u] ^ (y >> 1) ^ ((y & 1u) ? 0x9908B0DFu : 0u);
            }
            idx = 0;
        }
        uint32_t y = w[idx++];
        y ^= y >> 11;
        y ^= (y << 7) & 0x9D2C5680u;
        y ^= (y << 15) & 0xEFC60000u;
        return y ^ (y >> 18);
    }
    // random._randbelow_with_getrandbits(n), 1 <= n < 2^31
    __device__ uint32_t below(uint32_t n)
    {
        const uint32_t shift = (uint32_t)__clz(n);  // 32 - n.bit_length()
        for (int tries = 0; tries < 256; ++tries) {
            const uint32_t r = next() >> shift;
            if (r < n) return r;
        }
        bad = true;
        return 0;
    }
};

// res: [0] status (0: stopped at `end` or out of budget in front of key res[1], 1: a walk failed at key res[1], 2: bad data, 3: out of budget
//      inside the walk of key res[1]), [1] the first key not done, [2] the fingerprint left over by the failed walk, [3] fingerprints added
//      to the count, [4] keys that began to walk, [5] steps used, [6] fingerprint in hand, [7] row and [8] swaps done of a suspended walk.
//      A launch that finds res[0] == 3 takes that walk up at key `start`; every other launch starts with res[0] == 0.
// W = 2 (countingcuckoo.py:230-265): a key placed directly takes counts[i] (1 where `counts` is NULL) with it, a key that has to walk goes
//      in hand with count 1 whatever counts[i] says, a swap exchanges (fingerprint, count) pairs; [9] the count of the leftover and
//      [10] the count in hand of a suspended walk.
template <uint32_t W>
__global__ __launch_bounds__(64) void k_ck_insert(CkGeom g, CkTable t, uint32_t max_swaps, const uint32_t *tr, const uint32_t *counts, uint64_t n, uint64_t start,
                                                  uint64_t end, int dedup, uint64_t budget, uint32_t *state, uint32_t *res)
{
    __shared__ uint32_t words[624];
    const uint32_t lane = threadIdx.x;
    for (uint32_t k = lane; k < 624u; k += 64u) words[k] = state[k];
    __syncthreads();
    Mt mt{words, state[624], false};
    if (mt.idx > 624u) mt.idx = 624u;
    uint32_t status = 0, leftover = 0, added = 0, walked = 0, hand = 0, hand_row = 0, hand_swaps = 0, left_count = 0, hand_count = 0;
    bool resume = res[0] == 3u;
    uint64_t steps = 0, i = start;
    bool stop = false;
    for (uint64_t base = start; base < end && !stop; base += 64) {
        {  // all lanes: pull the two rows of the next 64 keys towards the cache; nothing is decided here
            const uint64_t k = base + lane;
            if (k < end) {
                const uint32_t r1 = tr[n + k], r2 = tr[2 * n + k];
                if (r1 < g.capacity && r2 < g.capacity) {
                    uint32_t a = t.buckets[(uint64_t)r1 * g.B * W], b = t.buckets[(uint64_t)r2 * g.B * W];
                    asm volatile("" ::"v"(a), "v"(b));
                }
            }
        }
        if (lane != 0) continue;
        const uint64_t top = base + 64 < end ? base + 64 : end;
        for (i = base; i < top; ++i) {
            if (steps >= budget) { stop = true; break; }
            uint32_t fp, idx, s = 0, cnt = 1;
            if (resume) {  // (budget >= 1: this launch does at least one swap of it)
                resume = false;
                fp = res[6], idx = res[7], s = res[8];
                if constexpr (W == 2) cnt = res[10];
                if (idx >= g.capacity) { status = 2; stop = true; break; }
            } else {
                ++steps;
                fp = tr[i];
                const uint32_t i1 = tr[n + i], i2 = tr[2 * n + i];
                if (i1 >= g.capacity || i2 >= g.capacity) { status = 2; stop = true; break; }
                if (dedup && ck_contains<W>(g, t.buckets, t.fill, CkTriple{fp, i1, i2})) continue;
                uint32_t f = t.fill[i1], row = i1;
                if (f >= g.B) f = t.fill[i2], row = i2;
                if (f < g.B) {
                    uint32_t *q = t.buckets + ((uint64_t)row * g.B + f) * W;
                    q[0] = fp;
                    if constexpr (W == 2) q[1] = counts ? counts[i] : 1u;
                    t.fill[row] = f + 1u;
                    ++added;
                    continue;
                }
                ++walked;
                idx = mt.below(2u) ? i2 : i1;  // random.choice([idx_1, idx_2])
            }
            bool placed = false, suspended = false;
            for (; s < max_swaps && !mt.bad; ++s) {
                if (steps >= budget) { suspended = true; break; }
                ++steps;
                uint32_t *slot = t.buckets + ((uint64_t)idx * g.B + mt.below(g.B)) * W;  // random.randint(0, bucket_size - 1)
                const uint32_t out = slot[0];
                slot[0] = fp;
                fp = out;
                if constexpr (W == 2) {
                    const uint32_t out_count = slot[1];
                    slot[1] = cnt;
                    cnt = out_count;
                }
                const CkTriple e = ck_triple_of(g, fp);
                idx = idx == e.i1 ? e.i2 : e.i1;
                const uint32_t fe = t.fill[idx];
                if (fe < g.B) {
                    uint32_t *q = t.buckets + ((uint64_t)idx * g.B + fe) * W;
                    q[0] = fp;
                    if constexpr (W == 2) q[1] = cnt;
                    t.fill[idx] = fe + 1u;
                    ++added;
                    placed = true;
                    break;
                }
            }
            if (mt.bad) { status = 2; stop = true; break; }
            if (suspended) { status = 3, hand = fp, hand_row = idx, hand_swaps = s, hand_count = cnt; stop = true; break; }
            if (!placed) { status = 1, leftover = fp, left_count = cnt; stop = true; break; }
        }
    }
    __syncthreads();
    if (lane == 0) {
        res[0] = status, res[1] = (uint32_t)i, res[2] = leftover, res[3] = added, res[4] = walked, res[5] = (uint32_t)(steps > 0xFFFFFFFFull ? 0xFFFFFFFFull : steps);
        res[6] = hand, res[7] = hand_row, res[8] = hand_swaps;
        if constexpr (W == 2) res[9] = left_count, res[10] = hand_count;
        state[624] = mt.idx;
    }
    for (uint32_t k = lane; k < 624u; k += 64u) state[k] = words[k];
}

// ---- the second half of a removal: the lane that swaps a row's non-zero mask out compacts that row to the left, zeroes what it vacates
// and lowers `fill`
template <uint32_t W>
__global__ __launch_bounds__(kBlock) void k_ck_rm_compact(CkGeom g, CkTable t, const uint32_t *tr, uint64_t n, uint32_t *marks)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        for (int which = 0; which < 2; ++which) {
            const uint32_t row = tr[(uint64_t)(1 + which) * n + i];
            if (row >= g.capacity || !marks[row]) continue;
            const uint32_t gone = atomicExch(marks + row, 0u);  // one lane gets the mask, and with it the row
            if (!gone) continue;
            uint32_t *p = t.buckets + (uint64_t)row * g.B * W;
            const uint32_t f = min(t.fill[row], g.B);
            uint32_t w = 0;
            for (uint32_t s = 0; s < f; ++s) {
                if ((gone >> s) & 1u) continue;
                for (uint32_t k = 0; k < W; ++k) p[w * W + k] = p[s * W + k];
                ++w;
            }
            for (uint32_t s = w * W; s < f * W; ++s) p[s] = 0;
            t.fill[row] = w;
        }
    }
}

}  // namespace psk
