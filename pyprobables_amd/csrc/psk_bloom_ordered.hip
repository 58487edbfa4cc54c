// psk_bloom_ordered.hip -- psk_bloom_add_running: the loop
//     for key in batch:  seen = key in table;  table.add(key)
// for a whole ordered batch at once, fused: hash, resolve and insert without writing the bit indices to memory.
//
// The rule (proved for the conditional insert in the header of psk_index_ops.hip; here every key is added).  Let S be the table in front
// of an ordered piece of the stream and first[b] the smallest position i of the piece whose key touches bit b, for every bit b clear in S.
// Bit b is set in front of key i exactly when b is in S or first[b] < i, so
//     seen[i] = 0  <=>  first[b] == i for one of key i's bits that are clear in S,
// and the table afterwards is S plus every bit touched.  The rule holds for any ordered piece as long as the next piece sees the table
// as the previous one left it: the batch is cut into chunks, and each chunk is two launches of k_apply (launch_apply) on one stream.
//   first   per key: hash, reduce to the k positions, test S; every clear position goes into a bounded open-addressing map
//           (compare-and-swap on the 64-bit position, atomicMin on the chunk-relative key index).
//   settle  per key: the positions again, each looked up in the map.  A position that is not in the map was set in S.  The key whose
//           index an entry holds is that position's first[]: the key is new (seen = 0) and ORs that bit into the table.  Every entry has
//           such a key, so the table ends as S plus every position of the map -- every bit touched.
//           The kernel NEVER READS THE TABLE: other lanes of the same launch are writing it, and "is b clear in S" asked again here would
//           find a bit that first[b]'s lane has just set and turn a first occurrence into "seen".  S is frozen in the map instead.
//
// The map: 16-byte slots (position, key index, pad), position all-ones = empty (legal: m < 2^63), one layout for every m.  It has the
// power of two >= 2 * chunk * k slots, at least twice what a chunk can insert, so it cannot fill; a walk that nevertheless goes once round
// sets the handle's error word and ends, and the call returns an error.  Every loop is bounded by the slot count.
// RESET: a fill of the part used, in front of the next chunk (k_ord_fill: one streaming fill, at most 32 MiB per default chunk; resetting
// only the touched slots would hash every key a third time) -- and only if the chunk before inserted anything.  A word in front of the
// slots, `touched`, holds the sequence number of the last chunk whose first-kernel inserted a position (the numbers count the handle's
// chunks and are never 0).  In front of chunk c everything outside the previous chunk's part is all-ones, and that part is too unless
// touched names the previous chunk: the fill is skipped then, and a settle kernel whose own chunk is not named has an empty map -- every
// position of every key was set in S, every key is seen -- and neither hashes nor probes (its op's k becomes 0).  A stream of keys that
// are all present costs the first kernel alone.
//
// CHUNK: default min(2^18, 2^20 / k) keys -- the stacked filters' 2^18, cut down so that 2 * chunk * k <= 2^21 slots = 32 MiB: the map of
// a chunk then stays inside the 256 MB Infinity Cache next to the keys, and the handle's scratch within a few tens of MiB whatever k is
// (k = 7: 149 796 keys).  A caller's chunk_keys overrides it (the tests reach the seams that way); it is capped where the map would
// exceed 2^26 slots (1 GiB).  The answers do not depend on the chunk.
#include "psk_stage.hpp"

namespace {

constexpr unsigned long long kPosNone = ~0ULL;
constexpr uint32_t kMapLgDefault = 21, kMapLgMax = 26;

struct OrdSlot {
    unsigned long long pos;  // bit position, kPosNone = empty
    uint32_t idx;            // smallest chunk-relative index of a key that touches it (all-ones after the fill)
    uint32_t pad;
};

constexpr uint64_t kMapHeader = 256;  // bytes in front of the slots: word 0 = touched

__global__ __launch_bounds__(kBlock) void k_ord_fill(uint4 *slots, uint64_t nvec, const uint32_t *touched, uint32_t seq_prev)
{
    if (*touched != seq_prev) return;  // (read by every workgroup, written by none of this launch)
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nvec; i += stride) slots[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
}

__device__ __forceinline__ uint32_t ord_slot_of(uint64_t b, uint32_t lg) { return (uint32_t)((b * 0x9E3779B97F4A7C15ULL) >> (64 - lg)); }  // lg >= 1

template <bool POW2>
struct BloomOrdFirst {
    const uint32_t *tab;
    Mod md;
    uint32_t k;
    OrdSlot *slots;
    uint32_t lg;
    uint32_t *touched;  // = seq by every wave that inserted
    uint32_t seq;
    uint32_t *err;
    struct State { uint32_t i, ins; };
    __device__ __forceinline__ void prepare() {}
    __device__ __forceinline__ State begin(uint64_t i) const { return State{(uint32_t)i, 0u}; }
    __device__ __forceinline__ void apply(State &st, uint32_t, uint64_t h) const
    {
        const uint64_t b = reduce<POW2>(md, h);
        if ((tab[b >> 5] >> (uint32_t)(b & 31)) & 1u) return;  // set in S: never in the map
        const uint32_t mask = (1u << lg) - 1u;
        uint32_t s = ord_slot_of(b, lg);
        for (uint32_t tries = 0; tries <= mask; ++tries, s = (s + 1u) & mask) {
            const unsigned long long old = atomicCAS(&slots[s].pos, kPosNone, (unsigned long long)b);
            if (old == kPosNone || old == b) {
                atomicMin(&slots[s].idx, st.i);
                st.ins = 1u;
                return;
            }
        }
        *err = 1u;  // once round a full map (cannot happen with the host's sizing; never spin for ever, never answer silently)
    }
    __device__ __forceinline__ void end(State &st, uint64_t) const
    {
        const unsigned long long active = __ballot(1);
        if (__ballot(st.ins != 0) && (int)(threadIdx.x & 63u) == __ffsll((long long)active) - 1) *touched = seq;  // one store per wave
    }
};

template <bool POW2>
struct BloomOrdSettle {  // (no pointer to read the table through: see the header)
    uint32_t *tab;
    Mod md;
    uint32_t k;
    const OrdSlot *slots;
    uint32_t lg;
    uint8_t *seen;               // [chunk]
    unsigned long long *fresh;   // += keys of the chunk with seen == 0
    const uint32_t *touched;
    uint32_t seq;
    uint32_t *err;
    struct State { uint32_t i, fresh; };
    __device__ __forceinline__ void prepare()
    {
        if (*touched != seq) k = 0;  // the chunk inserted nothing: the map is empty, every key is seen -- no hashing, no probes
    }
    __device__ __forceinline__ State begin(uint64_t i) const { return State{(uint32_t)i, 0u}; }
    __device__ __forceinline__ void apply(State &st, uint32_t, uint64_t h) const
    {
        const uint64_t b = reduce<POW2>(md, h);
        const uint32_t mask = (1u << lg) - 1u;
        uint32_t s = ord_slot_of(b, lg);
        for (uint32_t tries = 0; tries <= mask; ++tries, s = (s + 1u) & mask) {
            const unsigned long long pos = slots[s].pos;
            if (pos == b) {
                if (slots[s].idx == st.i) {  // this key is first[b]
                    st.fresh = 1u;
                    atomicOr(tab + (b >> 5), 1u << (uint32_t)(b & 31));
                }
                return;
            }
            if (pos == kPosNone) return;  // not in the map: set in S
        }
        *err = 1u;
    }
    __device__ __forceinline__ void end(State &st, uint64_t i) const
    {
        seen[i] = st.fresh ? 0 : 1;
        // one atomic per wave at most: the lowest active lane adds the wave's count
        const unsigned long long active = __ballot(1), fr = __ballot(st.fresh != 0);
        if (fr && (int)(threadIdx.x & 63u) == __ffsll((long long)active) - 1) atomicAdd(fresh, (unsigned long long)__popcll(fr));
    }
};

uint32_t map_lg(uint64_t chunk, uint32_t k)  // smallest lg >= 1 with 2^lg >= 2 * chunk * k
{
    uint32_t lg = 1;
    while ((1ULL << lg) < 2 * chunk * (uint64_t)k) ++lg;
    return lg;
}

}  // namespace

extern "C" int psk_bloom_add_running(psk_sketch *s, int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len,
                                     int where, uint64_t chunk_keys, uint8_t *seen_out, uint64_t *new_out, void *stream)
{
    CHECK_HANDLE(s, PSK_KIND_BLOOM);
    PSK_TRY(check_hashes_width(s, layout, key_len));
    if (n && !seen_out) return fail(PSK_EINVAL, "seen_out is NULL");
    hipStream_t st = (hipStream_t)stream;
    // the error word: pinned, so that the host reads it without a copy; it outlives the call, so a PSK_DEVICE call (enqueue only) that
    // overflowed its map is reported by the next call on the handle
    const bool fresh_page = !s->s_omap.pin;
    uint32_t *err;
    PSK_TRY(pinned(s->s_omap, (void **)&err));
    if (fresh_page) *err = 0u;
    if (__atomic_load_n(err, __ATOMIC_ACQUIRE) != 0u) {
        *err = 0u;
        return fail(PSK_EHIP, "an earlier psk_bloom_add_running on this handle overflowed its map: its answers and the table are not to be trusted");
    }
    PSK_TRY(clear_materialize(s, st));
    Batch b;
    PSK_TRY(stage_batch(s->s_keys, s->s_offs, layout, data, offsets, n, key_len, where, st, &b));
    if (n == 0) {
        if (new_out && where == PSK_HOST) *new_out = 0;
        if (new_out && where == PSK_DEVICE) HIP_TRY(hipMemsetAsync(new_out, 0, 8, st));
        return PSK_OK;
    }
    OutBuf o;
    PSK_TRY(stage_out(s->s_out, seen_out, n, where, &o));
    unsigned long long *fresh_dev = (unsigned long long *)new_out;
    if (where == PSK_HOST || !new_out) {
        PSK_TRY(ensure(s->s_aux, 16));
        fresh_dev = (unsigned long long *)s->s_aux.p;
    }
    HIP_TRY(hipMemsetAsync(fresh_dev, 0, 8, st));

    const uint64_t k = s->k;
    uint64_t chunk = (1ULL << (kMapLgDefault - 1)) / k;
    if (chunk > (1ULL << 18)) chunk = 1ULL << 18;
    if (chunk_keys) chunk = chunk_keys;
    const uint64_t cap = (1ULL << (kMapLgMax - 1)) / k;  // 2 * chunk * k <= 2^kMapLgMax slots (k <= 2^25 here or nothing fits)
    if (cap == 0) return fail(PSK_EINVAL, "k = %llu hashes do not fit the ordered map", (unsigned long long)k);
    if (chunk > cap) chunk = cap;
    if (chunk > n) chunk = n;
    if (chunk == 0) chunk = 1;
    const uint64_t need = kMapHeader + (sizeof(OrdSlot) << map_lg(chunk, s->k));  // (grown in front of the first launch: the first chunk is the largest)
    if (need > s->s_omap.cap) {  // a new buffer: every slot it holds empty, `touched` names nobody (0 is no chunk's number)
        PSK_TRY(ensure(s->s_omap, need));
        HIP_TRY(hipMemsetAsync(s->s_omap.p, 0, kMapHeader, st));
        HIP_TRY(hipMemsetAsync((uint8_t *)s->s_omap.p + kMapHeader, 0xFF, s->s_omap.cap - kMapHeader, st));
        s->omap_prev_lg = 0;
    }
    uint32_t *touched = (uint32_t *)s->s_omap.p;
    OrdSlot *slots = (OrdSlot *)((uint8_t *)s->s_omap.p + kMapHeader);
    uint8_t *seen_dev = (uint8_t *)o.dev;
    for (uint64_t off = 0; off < n; off += chunk) {
        const uint64_t cnt = n - off < chunk ? n - off : chunk;
        const uint32_t lg = map_lg(cnt, s->k);
        const uint32_t seq_prev = s->omap_seq;
        if (++s->omap_seq == 0) ++s->omap_seq;  // (a number that comes round again can only cost a fill that was not needed)
        const uint32_t seq = s->omap_seq;
        if (s->omap_prev_lg) {  // the part the chunk before used, if that chunk inserted anything (see RESET in the header)
            const uint64_t nvec = 1ULL << s->omap_prev_lg, blocks = (nvec + kBlock - 1) / kBlock;
            hipLaunchKernelGGL(k_ord_fill, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(kBlock), 0, st, (uint4 *)slots, nvec, (const uint32_t *)touched, seq_prev);
            HIP_TRY(hipGetLastError());
        }
        s->omap_prev_lg = lg;
        PSK_TRY(with_source(sub_batch(b, off, cnt), [&](auto src) {
            return with_pow2(s, [&](auto P) {
                PSK_TRY(launch_apply(src, BloomOrdFirst<P.value>{(const uint32_t *)s->table, s->md, s->k, slots, lg, touched, seq, err}, cnt, st));
                return launch_apply(src, BloomOrdSettle<P.value>{(uint32_t *)s->table, s->md, s->k, slots, lg, seen_dev + off, fresh_dev, touched, seq, err}, cnt,
                                    st);
            });
        }));
    }
    if (where == PSK_DEVICE) return PSK_OK;
    unsigned long long fresh = 0;
    HIP_TRY(hipMemcpyAsync(&fresh, fresh_dev, 8, hipMemcpyDeviceToHost, st));
    PSK_TRY(finish(where, &o, st));
    if (__atomic_load_n(err, __ATOMIC_ACQUIRE) != 0u) {
        *err = 0u;
        return fail(PSK_EHIP, "psk_bloom_add_running: the ordered map overflowed: the answers and the table are not to be trusted");
    }
    if (new_out) *new_out = fresh;
    return PSK_OK;
}
