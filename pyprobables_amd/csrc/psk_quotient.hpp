// psk_quotient.hpp -- device side of the quotient filter (reference: probables/quotientfilter/quotientfilter.py).
//
// Table: 2^q slots.  `filter` holds the remainders (r = 32 - q bits) as uint8 / uint16 / uint32 by r <= 8 / <= 16 / else (the reference's
// three array type codes), `occupied` / `continuation` / `shifted` are bit arrays packed LSB-first into 32-bit words (max(2^q / 32, 1)
// words each; a table of 8 or 16 slots lives in the low bits of one word).
//
// The reference drops duplicates, keeps a run sorted by remainder and the runs of a cluster in quotient order, so the four arrays are a
// function of the SET of hashes (DESIGN.md "Quotient filter"): the build places sorted distinct hashes with one prefix-max scan
// (psk_quotient.hip), and this header holds what a key needs on the way in -- the reference's 32-bit FNV-1a and the lookup walk.
#pragma once
#include "psk_device.hpp"

namespace psk {

// ------------------------------------------------------------------ fnv_1a_32(key, 0)  (hashes.py:106-122)
constexpr uint32_t kFnv32Basis = 0x811C9DC5u, kFnv32Prime = 0x01000193u;
__device__ __forceinline__ uint32_t qf_step(uint32_t h, uint32_t e) { return (h ^ e) * kFnv32Prime; }
__device__ __forceinline__ uint32_t qf_word(uint32_t h, uint32_t w)
{
#pragma unroll
    for (int b = 0; b < 4; ++b) h = qf_step(h, (w >> (8 * b)) & 0xFFu);
    return h;
}

// one overload per key source of with_source (psk_capi.hip): the sources load the key, the chain is this file's
__device__ __forceinline__ uint32_t qf_hash(const KeysFixed16 &, const KeysFixed16::Key &k, uint64_t)
{
    return qf_word(qf_word(qf_word(qf_word(kFnv32Basis, k.w.x), k.w.y), k.w.z), k.w.w);
}
__device__ __forceinline__ uint32_t qf_hash(const KeysFixed8 &, const KeysFixed8::Key &k, uint64_t) { return qf_word(qf_word(kFnv32Basis, k.w.x), k.w.y); }
__device__ __forceinline__ uint32_t qf_hash(const KeysFixed32 &, const KeysFixed32::Key &k, uint64_t)
{
    uint32_t h = qf_word(qf_word(qf_word(qf_word(kFnv32Basis, k.a.x), k.a.y), k.a.z), k.a.w);
    return qf_word(qf_word(qf_word(qf_word(h, k.b.x), k.b.y), k.b.z), k.b.w);
}
template <bool DWORDS>
__device__ __forceinline__ uint32_t qf_hash(const KeysFixed<DWORDS> &s, const typename KeysFixed<DWORDS>::Key &k, uint64_t)
{
    uint32_t h = kFnv32Basis;
    if (DWORDS) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(k.q);
        for (uint32_t j = 0; j < s.L / 4; ++j) h = qf_word(h, q[j]);
    } else {
        walk_key_bytes(k.q, s.L, [&](uint32_t w) { h = qf_word(h, w); }, [&](uint32_t e) { h = qf_step(h, e); });
    }
    return h;
}
template <class T>
__device__ __forceinline__ uint32_t qf_hash(const KeysVarlen<T> &s, const typename KeysVarlen<T>::Key &k, uint64_t i)
{
    uint32_t h = kFnv32Basis;
    auto step = [&](uint32_t e) { h = qf_step(h, e); };  // a code point > 255 XORs whole into the state (hashes.py:118)
    if (k.len == kKeyLenBig) {
        const uint64_t len = s.off[i + 1] - s.off[i];
        for (uint64_t j = 0; j < len; ++j) step((uint32_t)s.ptr(k)[j]);
        return h;
    }
    if constexpr (sizeof(T) == 1) walk_key_bytes(reinterpret_cast<const uint8_t *>(s.ptr(k)), s.first(k), k.len, [&](uint32_t w) { h = qf_word(h, w); }, step);
    else walk_key_elems(reinterpret_cast<const uint32_t *>(s.ptr(k)), s.first(k), k.len, step);
    return h;
}
// pre-computed hashes (add_alt / check_alt, a custom hash_function): the low 32 bits of the first hash of the row
__device__ __forceinline__ uint32_t qf_hash(const KeysHashes &, const KeysHashes::Key &k, uint64_t) { return (uint32_t)k.q[0]; }

template <class Src>
__global__ __launch_bounds__(kBlock) void k_qf_hash(Src src, uint32_t *out, uint64_t n)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) out[i] = qf_hash(src, src.load(i), i);
}

// ------------------------------------------------------------------ lookup  (quotientfilter.py:328-353 _get_start_index, :471-491 _contained_at_loc)
struct QfTable {
    const void *filter;
    const uint32_t *occ, *cont, *sh;
    uint32_t q;
};

__device__ __forceinline__ uint32_t qf_rem(const void *f, uint32_t rbits, uint32_t p)
{
    if (rbits <= 8) return reinterpret_cast<const uint8_t *>(f)[p];
    if (rbits <= 16) return reinterpret_cast<const uint16_t *>(f)[p];
    return reinterpret_cast<const uint32_t *>(f)[p];
}

// Is hash h in the table?  Both walks go a 32-bit metadata word at a time:
//   back    from slot q over `shifted` to the cluster start b (the highest clear bit at or below q), counting the occupied bits of [b, q):
//           that many runs lie between b and q's own run;
//   forward from b to the (count + 1)-th clear bit of `continuation`: the start of q's run;
//   then the run itself, remainder by remainder, until one is >= r or the run ends.
// A table of 8 or 16 slots is one word whose pattern is replicated to 32 bits: the ring of 32 virtual slots is the table unrolled, every
// walk (shorter than the table) stays exact, and a slot's remainder is at (virtual position mod size).  Every loop is bounded by the
// table's size, so a table that is not a quotient filter's (a caller's garbage) ends in `false`, never in a spin.
//
// qf_find is that walk with two by-products for removal (psk_quotient.hip k_qf_locate): the slot the hash sits in and the start of its cluster, the slot
// where the walk back stopped.  qf_contains drops both, and the compiler with them.
__device__ inline bool qf_find(const QfTable &t, uint32_t h, uint32_t &slot, uint32_t &start)
{
    const uint32_t rbits = 32u - t.q, smask = (1u << t.q) - 1u;
    const uint32_t quot = h >> rbits, rem = h & ((1u << rbits) - 1u);
    const uint32_t rep = t.q >= 5 ? 1u : (t.q == 4 ? 0x00010001u : 0x01010101u);
    const uint32_t wmask = t.q >= 5 ? (smask >> 5) : 0u;
    uint32_t w = (quot >> 5) & wmask, b = quot & 31u;
    if (!((t.occ[w] * rep >> b) & 1u)) return false;

    uint32_t upto = 0xFFFFFFFFu >> (31u - b);  // bits 0 .. b of q's word: where the cluster start may be
    uint32_t before = upto >> 1;               // bits 0 .. b - 1: the slots in front of q
    uint32_t skip = 0, j = 0;
    bool found = false;
    for (uint32_t guard = 0; guard <= wmask + 1u; ++guard) {
        const uint32_t nsh = ~(t.sh[w] * rep) & upto, oc = t.occ[w] * rep;
        if (nsh) {
            j = 31u - (uint32_t)__clz(nsh);
            skip += __popc(oc & before & (0xFFFFFFFFu << j));
            found = true;
            break;
        }
        skip += __popc(oc & before);
        w = (w - 1u) & wmask;
        upto = before = 0xFFFFFFFFu;
    }
    if (!found) return false;
    start = ((w << 5) | j) & smask;

    uint32_t from = 0xFFFFFFFFu << j, c = 0;
    found = false;
    for (uint32_t guard = 0; guard <= wmask + 1u; ++guard) {
        c = t.cont[w] * rep;
        uint32_t z = ~c & from;
        const uint32_t pc = __popc(z);
        if (pc > skip) {
            for (; skip; --skip) z &= z - 1u;
            j = (uint32_t)__ffs(z) - 1u;
            found = true;
            break;
        }
        skip -= pc;
        w = (w + 1u) & wmask;
        from = 0xFFFFFFFFu;
    }
    if (!found) return false;

    for (uint32_t steps = 0; steps <= smask; ++steps) {
        slot = ((w << 5) | j) & smask;
        const uint32_t v = qf_rem(t.filter, rbits, slot);
        if (v >= rem) return v == rem;  // the run is sorted: the reference stops at the first remainder > r too
        if (++j == 32u) {
            j = 0;
            w = (w + 1u) & wmask;
            c = t.cont[w] * rep;
        }
        if (!((c >> j) & 1u)) return false;  // the run ended
    }
    return false;
}

__device__ __forceinline__ bool qf_contains(const QfTable &t, uint32_t h)
{
    uint32_t slot = 0, start = 0;
    return qf_find(t, h, slot, start);
}

template <class Src>
__global__ __launch_bounds__(kBlock) void k_qf_check(Src src, QfTable t, uint8_t *out, uint64_t n)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) out[i] = qf_contains(t, qf_hash(src, src.load(i), i)) ? 1 : 0;
}

}  // namespace psk
