// psk_quotient.hip -- quotient filter: bulk build, lookup of pre-computed hashes, batch removal in place, decode (include/psk.h "QuotientFilter").
//
// Build (k_qf_tile_max / k_qf_tile_scan / k_qf_place).  For the sorted distinct hashes h_0 < h_1 < ..., quotients q_i = h_i >> r, the
// reference's table stores element i at
//     pos_i = max(q_i, pos_{i-1} + 1) = i + max_{j <= i} (q_j - j)                 (quotientfilter.py:291-394 _shift_insert / _add)
// -- a prefix max over d_j = q_j - j, done as reduce (one max per tile of 1024), scan (the tile maxima, one workgroup), apply (each tile
// rescans itself behind its carry).  When pos_{n-1} = n - 1 + max_j d_j reaches past the last slot the tail wraps and pushes the head: the
// same recurrence with pos_{-1} = c = pos_{n-1} - size, i.e. pos_i = i + max(c + 1, max_{j <= i} d_j).  c + 1 is ONE constant known after
// the scan, so the "second sweep" is a max inside the apply; it cannot move pos_{n-1} again while n <= size (c + 1 + n - 1 <= pos_{n-1}).
// Metadata bits go into the zeroed table with word-level atomicOr: a lane's 4 elements land in ascending slots, so it gathers the bits of
// one word in a register and issues an atomic only when the word changes (one per word it touches, not one per bit); lanes of neighbouring
// elements share words, which is what the atomic resolves.  (One word per lane group without atomics would need the elements regrouped by
// destination word -- a second scan over pos -- for the same 3 x size / 8 bytes written.)
//
// Decode (k_qf_decode_count / k_qf_decode_emit): run starts are slots with !continuation & (occupied | shifted); the k-th run start in
// slot order belongs to the occupied quotient number (k - w) mod runs, where w = (run starts before x) - (occupied bits before x) for ANY
// slot x with continuation = shifted = 0: an empty slot (the next run behind it belongs to the next occupied quotient) or a cluster start
// (its run is its own quotient's).  Such a slot exists in every table, the full one included (the element with the largest q_j - j sits
// in its own slot), so a full table decodes like any other.
#include "psk_stage.hpp"
#include "psk_quotient.hpp"

namespace {

constexpr int kItems = 4;                      // consecutive elements per lane (one 16-byte load)
constexpr uint32_t kTile = kBlock * kItems;    // elements per workgroup
constexpr int32_t kNegInf = INT32_MIN;

__device__ __forceinline__ int32_t wave_max(int32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// d_j = q_j - j fits int32: 0 <= q_j < 2^31, 0 <= j < 2^31
__device__ __forceinline__ int32_t qf_d(uint32_t h, uint32_t rbits, uint64_t j) { return (int32_t)((int64_t)(h >> rbits) - (int64_t)j); }

__global__ __launch_bounds__(kBlock) void k_qf_tile_max(const uint32_t *hs, uint64_t n, uint32_t rbits, int32_t *tile_max)
{
    __shared__ int32_t part[kBlock / 64];
    const uint64_t base = (uint64_t)blockIdx.x * kTile;
    int32_t m = kNegInf;
    for (uint32_t e = threadIdx.x; e < kTile; e += kBlock) {
        const uint64_t i = base + e;
        if (i < n) m = max(m, qf_d(hs[i], rbits, i));
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) m = max(m, part[w]);
        tile_max[blockIdx.x] = m;
    }
}

// tile_max[t] <- max of the tiles in front of t (exclusive), tile_max[ntiles] <- max of all; one workgroup
__global__ __launch_bounds__(kBlock) void k_qf_tile_scan(int32_t *tile_max, uint32_t ntiles)
{
    __shared__ int32_t buf[kBlock];
    int32_t carry = kNegInf;
    for (uint32_t base = 0; base < ntiles; base += kBlock) {
        const uint32_t t = base + threadIdx.x;
        const int32_t mine = t < ntiles ? tile_max[t] : kNegInf;
        int32_t v = mine;
        buf[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < kBlock; o <<= 1) {
            const int32_t other = (int)threadIdx.x >= o ? buf[threadIdx.x - o] : kNegInf;
            __syncthreads();
            v = max(v, other);
            buf[threadIdx.x] = v;
            __syncthreads();
        }
        const int32_t excl = max(carry, threadIdx.x ? buf[threadIdx.x - 1] : kNegInf);
        if (t < ntiles) tile_max[t] = excl;
        carry = max(carry, buf[kBlock - 1]);
        __syncthreads();
    }
    if (threadIdx.x == 0) tile_max[ntiles] = carry;
}

template <class T>
__global__ __launch_bounds__(kBlock) void k_qf_place(const uint32_t *hs, uint64_t n, uint32_t q, const int32_t *tile_carry, uint32_t ntiles, T *filter,
                                                     uint32_t *occ, uint32_t *cont, uint32_t *sh)
{
    __shared__ int32_t wave_tot[kBlock / 64];
    const uint32_t rbits = 32u - q, smask = (1u << q) - 1u, rmask = (1u << rbits) - 1u;
    const uint64_t first = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kItems;
    uint32_t h[kItems];
    int32_t run = kNegInf;  // max of d over this lane's elements
#pragma unroll
    for (int e = 0; e < kItems; ++e) {
        h[e] = first + e < n ? hs[first + e] : 0u;
        if (first + e < n) run = max(run, qf_d(h[e], rbits, first + e));
    }
    // exclusive prefix max over the lanes of the tile: inside the wave by shuffles, across the four waves through LDS
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    int32_t incl = run;
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t other = __shfl_up(incl, o);
        if ((int)lane >= o) incl = max(incl, other);
    }
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    int32_t m = tile_carry[blockIdx.x];
    for (uint32_t x = 0; x < wv; ++x) m = max(m, wave_tot[x]);
    const int32_t up = __shfl_up(incl, 1);
    if (lane) m = max(m, up);

    const int64_t size = (int64_t)smask + 1, last = (int64_t)n - 1 + tile_carry[ntiles];
    const int64_t wrap = last >= size ? last - size + 1 : INT64_MIN;  // c + 1 of the wrapped tail, see above
    uint32_t prev_q = first && first < n ? hs[first - 1] >> rbits : 0xFFFFFFFFu;
    uint32_t mw = 0xFFFFFFFFu, cbits = 0, sbits = 0;  // metadata word being gathered
    uint32_t ow = 0xFFFFFFFFu, obits = 0;
#pragma unroll
    for (int e = 0; e < kItems; ++e) {
        const uint64_t i = first + e;
        if (i >= n) break;
        const uint32_t qi = h[e] >> rbits;
        m = max(m, qf_d(h[e], rbits, i));
        const int64_t mm = (int64_t)m > wrap ? (int64_t)m : wrap;
        const uint32_t p = (uint32_t)((int64_t)i + mm) & smask;
        filter[p] = (T)(h[e] & rmask);
        if ((p >> 5) != mw) {
            if (cbits) atomicOr(cont + mw, cbits);
            if (sbits) atomicOr(sh + mw, sbits);
            mw = p >> 5, cbits = sbits = 0;
        }
        if (qi == prev_q) cbits |= 1u << (p & 31u);
        if (p != qi) sbits |= 1u << (p & 31u);
        if ((qi >> 5) != ow) {
            if (obits) atomicOr(occ + ow, obits);
            ow = qi >> 5, obits = 0;
        }
        obits |= 1u << (qi & 31u);
        prev_q = qi;
    }
    if (cbits) atomicOr(cont + mw, cbits);
    if (sbits) atomicOr(sh + mw, sbits);
    if (obits) atomicOr(occ + ow, obits);
}

__global__ __launch_bounds__(kBlock) void k_qf_check_alt(psk::QfTable t, const uint32_t *hashes, uint64_t n, uint8_t *out)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) out[i] = psk::qf_contains(t, hashes[i]) ? 1 : 0;
}

// ---- removal (psk_qf_remove_alt; q >= 5: a metadata word is 32 real slots; DESIGN.md "Quotient filter: removal", tests/qf_remove_model.py is this code step by step)
// A cluster is a slot with shifted = 0 in use and the shifted slots behind it.  Taking elements out moves the rest of THEIR cluster left and
// nothing else: the next cluster's head sits in its own quotient's slot and stays there.  So launch 1 marks, launch 2 repairs each marked cluster
// by itself, in place.
//
// k_qf_locate: one lane per hash, the lookup walk.  A hit sets its slot's bit in `dead`; the lane that sets the bit for the first time counts it
// and sets the cluster start's bit in `dirty`, and the lane that sets THAT bit for the first time owns the cluster: it appends the start to `list`.
__global__ __launch_bounds__(kBlock) void k_qf_locate(psk::QfTable t, const uint32_t *hashes, uint64_t n, uint32_t *dead, uint32_t *dirty, uint32_t *cursor,
                                                      uint32_t *list, uint32_t *removed)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    uint32_t hits = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        uint32_t slot = 0, start = 0;
        if (!psk::qf_find(t, hashes[i], slot, start)) continue;
        const uint32_t bit = 1u << (slot & 31u);
        if (atomicOr(dead + (slot >> 5), bit) & bit) continue;  // the same hash twice in the batch
        ++hits;
        const uint32_t sbit = 1u << (start & 31u);
        if (atomicOr(dirty + (start >> 5), sbit) & sbit) continue;
        const uint32_t at = atomicAdd(cursor, 1u);
        if (at < n) list[at] = start;
    }
    for (int o = 32; o > 0; o >>= 1) hits += __shfl_xor(hits, o);
    if ((threadIdx.x & 63) == 0 && hits) atomicAdd(removed, hits);
}

// k_qf_repack: one lane per listed cluster, start b.  The lane reads the cluster slot by slot (offset `steps` from b, modulo the table) up to the
// first slot with shifted = 0 -- an empty slot or the next cluster's head -- and writes the survivors behind its read position:
//     offset of a survivor = max(offset of its quotient, offset of the survivor before it + 1)        (the build's rule, restarted at b)
// with continuation = "same run as the survivor before" and shifted = "not in its quotient's slot".  The k-th run of the cluster belongs to the
// k-th set `occupied` bit from b (`oc` walks them); a run without survivors clears its bit.  Offsets no survivor took are zeroed in filter,
// continuation and shifted: the tail the cluster gave up, and gaps -- a survivor that falls back to its own quotient's slot behind a gap heads a
// cluster of its own, so a cluster may leave as several.  Nothing is written before the first dead slot (the slots in front of it keep their
// place).  Writes never pass the read position (a survivor's old offset is >= its quotient's and >= the count of slots before it), and every bit
// the lane reads ahead is one only this lane may change: quotients, slots, dead bits of [b, end) are the cluster's own.
// Two clusters can share a metadata word, so bits are changed with atomicAnd / atomicOr on the word, gathered per word (`mw`); remainders are
// plain stores.  The lane clears the dead bits it read and its dirty bit: the scratch goes back zeroed.
// Bounds: every loop ends after at most `size` steps and every slot index is masked, so arrays that are no quotient filter's give some table, not
// a spin or an access outside the arrays.
template <class T>
__global__ __launch_bounds__(kBlock) void k_qf_repack(T *filter, uint32_t *occ, uint32_t *cont, uint32_t *sh, uint32_t q, uint32_t *dead, uint32_t *dirty,
                                                      const uint32_t *cursor, const uint32_t *list, uint64_t cap)
{
    const uint32_t smask = (1u << q) - 1u, wmask = smask >> 5;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t count = *cursor < cap ? *cursor : cap;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) {
        const uint32_t b = list[i] & smask;
        uint32_t mw = b >> 5, mmask = 0, mc = 0, ms = 0;  // the metadata word being written: bits decided, continuation and shifted values
        auto flush = [&]() {
            const uint32_t c0 = mmask & ~mc, s0 = mmask & ~ms;
            if (c0) atomicAnd(cont + mw, ~c0);
            if (mc) atomicOr(cont + mw, mc);
            if (s0) atomicAnd(sh + mw, ~s0);
            if (ms) atomicOr(sh + mw, ms);
            mmask = mc = ms = 0;
        };
        auto emit = [&](uint32_t off, bool c, bool s, T rem) {  // offsets arrive ascending, each once
            const uint32_t p = (b + off) & smask, bit = 1u << (p & 31u);
            if ((p >> 5) != mw) {
                flush();
                mw = p >> 5;
            }
            mmask |= bit;
            if (c) mc |= bit;
            if (s) ms |= bit;
            filter[p] = rem;
        };
        uint32_t rw = 0xFFFFFFFFu, wsh = 0, wcont = 0, wdead = 0, dbits = 0;  // the word being read, and the dead bits consumed in it
        uint32_t oc = b, alive = 0;  // the quotient of the run being read, its survivors so far
        uint32_t next = 0, eo = 0;   // the earliest offset the next survivor may take; the next offset to write
        bool moved = false;          // a dead slot was met: from `eo` on the cluster is rewritten
        bool sound = true;
        uint32_t steps = 0;
        for (; steps <= smask; ++steps) {
            const uint32_t p = (b + steps) & smask, bit = 1u << (p & 31u);
            if ((p >> 5) != rw) {
                if (dbits) atomicAnd(dead + rw, ~dbits);
                rw = p >> 5, dbits = 0;
                wsh = sh[rw], wcont = cont[rw], wdead = dead[rw];
            }
            if (steps && !(wsh & bit)) break;
            if (steps && !(wcont & bit)) {  // the next run starts here
                if (!alive) atomicAnd(occ + (oc >> 5), ~(1u << (oc & 31u)));
                alive = 0;
                const uint32_t x = (oc + 1u) & smask;
                uint32_t w = x >> 5, m = occ[w] & (0xFFFFFFFFu << (x & 31u));
                for (uint32_t guard = 0; guard <= wmask && !m; ++guard) {
                    w = (w + 1u) & wmask;
                    m = occ[w];
                }
                if (!m) {  // more runs than occupied bits: not a quotient filter's table
                    sound = false;
                    break;
                }
                oc = (w << 5) + (uint32_t)__ffs(m) - 1u;
            }
            if (wdead & bit) {
                dbits |= bit;
                if (!moved) moved = true, eo = steps;
                continue;
            }
            const uint32_t qo = (oc - b) & smask, wo = qo > next ? qo : next;
            next = wo + 1u;
            if (moved) {
                const T rem = filter[p];
                for (; eo < wo; ++eo) emit(eo, false, false, (T)0);
                emit(wo, alive != 0, wo != qo, rem);
                eo = wo + 1u;
            }
            ++alive;
        }
        if (sound && !alive) atomicAnd(occ + (oc >> 5), ~(1u << (oc & 31u)));
        if (moved)
            for (; eo < steps; ++eo) emit(eo, false, false, (T)0);
        flush();
        if (dbits) atomicAnd(dead + rw, ~dbits);
        atomicAnd(dirty + (b >> 5), ~(1u << (b & 31u)));
    }
}

// ---- insertion in place (psk_qf_add_alt; q >= 5; DESIGN.md "Quotient filter: insertion in place", tests/qf_insert_model.py is this code step by step)
// Adding elements only raises positions in pos_i = max(q_i, pos_{i-1} + 1), so a new hash disturbs the table from the start b of the cluster that
// holds its quotient's slot (the slot itself when it is empty) up to the first item that still finds its own quotient's slot free.
//
// k_qf_add_starts: one lane per batch hash, b into bs[].  Hashes with equal b are a group, contiguous in ring order; its leader comes first from b.
// k_qf_add_spans:  one lane per leader, qf_walk from b as if no carry arrived there (read only).  The walk merges the old elements in slot order with the
//                  batch hashes from the leader on by (quotient, remainder), gives each item the next free offset `nxt`, lets empty slots under the
//                  frontier go, and stops in front of the first item whose quotient's offset is >= nxt: that item and all behind keep their place.
//                  A hash of another group that the walk takes in sets that group's bit in `covered`: the real carry at a slot is at least this walk's.
//                  A frontier that comes round to b is a union that does not fit: status word.
// k_qf_add_write:  a leader nobody covered heads a region and its walk is exact.  It walks again, then writes from the end backward: from the first
//                  new hash's offset p0 on the region is contiguous, so the items in descending order take the offsets end - 1 .. p0; the write
//                  offset is never below the old slot being read.  An old element's quotient comes from a cursor over `occupied` that steps back at
//                  every run start; the new hashes' occupied bits are set last, behind every read of the cursor.  Covered leaders clear their bit.
// Lanes of the write launch share words, not bits: a lane reads its own region and the stop slot (which reads "empty or head" whatever its owner
// does), changes metadata with atomicAnd / atomicOr gathered per word, and stores remainders to its own slots.  Every loop is bounded, every index masked.
struct QfWalk {
    uint32_t b, end, rend, p0, added, oc_last, pq;
    uint64_t used;
    bool has_pq, over;
};

__device__ __forceinline__ uint32_t qf_next_occ(const uint32_t *occ, uint32_t oc, uint32_t smask)  // the next set bit behind oc, round the ring
{
    const uint32_t wmask = smask >> 5, x = (oc + 1u) & smask;
    uint32_t w = x >> 5, m = occ[w] & (0xFFFFFFFFu << (x & 31u));
    for (uint32_t g = 0; g <= wmask && !m; ++g) {
        w = (w + 1u) & wmask;
        m = occ[w];
    }
    return m ? (w << 5) + (uint32_t)__ffs(m) - 1u : oc;
}

__device__ __forceinline__ uint32_t qf_prev_occ(const uint32_t *occ, uint32_t oc, uint32_t smask)  // the set bit before oc
{
    const uint32_t wmask = smask >> 5, x = (oc - 1u) & smask;
    uint32_t w = x >> 5, m = occ[w] & (0xFFFFFFFFu >> (31u - (x & 31u)));
    for (uint32_t g = 0; g <= wmask && !m; ++g) {
        w = (w - 1u) & wmask;
        m = occ[w];
    }
    return m ? (w << 5) + 31u - (uint32_t)__clz(m) : oc;
}

__device__ __forceinline__ bool qf_add_leader(const uint32_t *hs, const uint32_t *bs, uint64_t n, uint64_t i, uint32_t rbits)
{
    if (n == 1) return true;
    const uint64_t p = i ? i - 1 : n - 1;
    if (bs[p] != bs[i]) return true;
    return hs[p] - (bs[p] << rbits) > hs[i] - (bs[i] << rbits);  // ring order from b: the one descent of a group that is the whole batch
}

template <class T>
__device__ QfWalk qf_walk(const T *filter, const uint32_t *occ, const uint32_t *cont, const uint32_t *sh, uint32_t q, const uint32_t *hs, uint64_t n,
                          const uint32_t *bs, uint64_t i0, uint32_t *covered)
{
    const uint32_t rbits = 32u - q, smask = (1u << q) - 1u, rmask = (1u << rbits) - 1u;
    QfWalk w{};
    const uint32_t b = w.b = bs[i0] & smask;
    uint32_t ro = 0, nxt = 0, added = 0;  // offsets from b: the old slot being read, the write frontier; new hashes so far
    uint64_t used = 0, j = i0;            // batch hashes taken in, the next one's index
    uint32_t oc = b, oc_at = 0xFFFFFFFFu;  // the quotient of the old element at offset oc_at
    uint32_t rw = 0xFFFFFFFFu, wo = 0, wc = 0, ws = 0, marked = 0xFFFFFFFFu;
    w.oc_last = b;
    bool stopped = false;
    const uint64_t limit = 2ull * ((uint64_t)smask + 1ull) + n + 4ull;
    for (uint64_t g = 0; g < limit; ++g) {
        if (nxt > smask) break;  // round the ring
        const uint32_t s = (b + ro) & smask, bit = 1u << (s & 31u);
        if ((s >> 5) != rw) rw = s >> 5, wo = occ[rw], wc = cont[rw], ws = sh[rw];
        const bool have_old = ((wo | ws) & bit) != 0;
        if (!have_old && ro < nxt) {  // empty slots under the frontier each take one unit of carry: to the next slot in use of this word
            const uint32_t above = (wo | ws) & (0xFFFFFFFFu << (s & 31u));
            const uint32_t run = (above ? (uint32_t)__ffs(above) - 1u : 32u) - (s & 31u);
            ro += run < nxt - ro ? run : nxt - ro;
            continue;
        }
        if (have_old && oc_at != ro) {
            if (!(wc & bit)) oc = (ws & bit) ? qf_next_occ(occ, oc, smask) : s;
            oc_at = ro;
        }
        const bool have_new = used < n;
        uint32_t nq = 0, nr = 0, bj = 0;
        bool own = false;
        if (have_new) {
            const uint32_t h = hs[j];
            nq = ((h >> rbits) - b) & smask, nr = h & rmask, bj = bs[j] & smask;
            own = bj == b;
        }
        if (!have_old && !have_new) {
            stopped = true;
            break;
        }
        const uint32_t qo = (oc - b) & smask;
        bool take_old = have_old, same = false;
        if (have_old && have_new) {
            if (qo != nq) take_old = qo < nq;
            else {
                const uint32_t orem = (uint32_t)filter[s];
                take_old = orem < nr, same = orem == nr;
            }
        }
        const uint32_t cq = (take_old || same) ? qo : nq;
        if (cq >= nxt && !own) {
            stopped = true;
            break;
        }
        if (have_new && !take_old && covered && !own && bj != marked) {
            atomicOr(covered + (bj >> 5), 1u << (bj & 31u));
            marked = bj;
        }
        if (same) {  // the hash is in the table already
            ++used;
            if (++j == n) j = 0;
            continue;
        }
        if (take_old) {
            if (!added) w.pq = qo, w.has_pq = true;
            w.oc_last = oc;
            ++ro, ++nxt;
            w.rend = ro;
        } else {
            if (!added) w.p0 = nxt;
            ++added, ++used, ++nxt;
            if (++j == n) j = 0;
        }
    }
    w.over = !stopped;
    w.end = nxt, w.used = used, w.added = added;
    return w;
}

template <class T>
__device__ void qf_write_region(T *filter, uint32_t *occ, uint32_t *cont, uint32_t *sh, uint32_t q, const uint32_t *hs, uint64_t n, uint64_t i0, const QfWalk &w)
{
    const uint32_t rbits = 32u - q, smask = (1u << q) - 1u, rmask = (1u << rbits) - 1u, b = w.b;
    uint64_t k = w.used, jk = k ? (i0 + k - 1) % n : 0;  // batch hashes not yet placed, the last one's index
    uint32_t ro = w.rend, oc = w.oc_last;
    bool step = false;
    uint32_t mw = 0xFFFFFFFFu, mmask = 0, mc = 0, ms = 0;  // the metadata word being written: bits decided, continuation and shifted values
    auto flush = [&]() {
        const uint32_t c0 = mmask & ~mc, s0 = mmask & ~ms;
        if (c0) atomicAnd(cont + mw, ~c0);
        if (mc) atomicOr(cont + mw, mc);
        if (s0) atomicAnd(sh + mw, ~s0);
        if (ms) atomicOr(sh + mw, ms);
        mmask = mc = ms = 0;
    };
    auto emit = [&](uint32_t p, uint32_t qoff, uint32_t rem, bool c) {  // offsets arrive descending, each once
        const uint32_t slot = (b + p) & smask, bit = 1u << (slot & 31u);
        if ((slot >> 5) != mw) {
            if (mmask) flush();
            mw = slot >> 5;
        }
        mmask |= bit;
        if (c) mc |= bit;
        if (p != qoff) ms |= bit;
        filter[slot] = (T)rem;
    };
    uint32_t rw = 0xFFFFFFFFu, wo = 0, wc = 0, ws = 0;
    bool have_prev = false;
    uint32_t pp = 0, pqo = 0, prem = 0;  // the item of the offset above, written once the one below it is known
    for (uint32_t wp = w.end; wp-- > w.p0;) {
        bool have_old = false, have_new = false, ocont = false;
        uint32_t oq = 0, orem = 0, nq = 0, nr = 0;
        for (uint64_t g = 0; g <= n; ++g) {
            uint32_t s = 0, bit = 0;
            while (ro > 0) {  // empty slots between two old clusters
                s = (b + ro - 1u) & smask, bit = 1u << (s & 31u);
                if ((s >> 5) != rw) rw = s >> 5, wo = occ[rw], wc = cont[rw], ws = sh[rw];
                if ((wo | ws) & bit) break;
                --ro;
            }
            have_old = ro > 0, have_new = k > 0;
            if (have_old) {
                if (step) oc = qf_prev_occ(occ, oc, smask), step = false;
                oq = (oc - b) & smask, orem = (uint32_t)filter[s], ocont = (wc & bit) != 0;
            }
            if (have_new) {
                const uint32_t h = hs[jk];
                nq = ((h >> rbits) - b) & smask, nr = h & rmask;
            }
            if (!(have_old && have_new && oq == nq && orem == nr)) break;
            --k;  // in the table already
            jk = jk ? jk - 1 : n - 1;
        }
        if (!have_old && !have_new) break;  // (fewer items than the walk counted: not a quotient filter's table)
        const bool take_old = have_old && (!have_new || oq > nq || (oq == nq && orem > nr));
        const uint32_t iq = take_old ? oq : nq, irem = take_old ? orem : nr;
        if (take_old) {
            step = !ocont;  // a run start: the element below belongs to the occupied quotient before this one
            --ro;
        } else {
            --k;
            jk = jk ? jk - 1 : n - 1;
        }
        if (have_prev) emit(pp, pqo, prem, pqo == iq);
        pp = wp, pqo = iq, prem = irem, have_prev = true;
    }
    if (have_prev) emit(pp, pqo, prem, w.has_pq && w.pq == pqo);
    if (mmask) flush();
    uint32_t ow = 0xFFFFFFFFu, ob = 0;
    uint64_t j = i0;
    for (uint64_t x = 0; x < w.used; ++x) {
        const uint32_t qq = hs[j] >> rbits;
        if ((qq >> 5) != ow) {
            if (ob) atomicOr(occ + ow, ob);
            ow = qq >> 5, ob = 0;
        }
        ob |= 1u << (qq & 31u);
        if (++j == n) j = 0;
    }
    if (ob) atomicOr(occ + ow, ob);
}

__global__ __launch_bounds__(kBlock) void k_qf_add_starts(const uint32_t *occ, const uint32_t *sh, uint32_t q, const uint32_t *hs, uint64_t n, uint32_t *bs)
{
    const uint32_t rbits = 32u - q, smask = (1u << q) - 1u, wmask = smask >> 5;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const uint32_t quot = hs[i] >> rbits;
        uint32_t w = quot >> 5, start = quot;
        if (((occ[w] | sh[w]) >> (quot & 31u)) & 1u) {  // the slot is in use: back over `shifted` to the start of its cluster
            uint32_t upto = 0xFFFFFFFFu >> (31u - (quot & 31u));
            for (uint32_t g = 0; g <= wmask + 1u; ++g) {
                const uint32_t nsh = ~sh[w] & upto;
                if (nsh) {
                    start = (w << 5) | (31u - (uint32_t)__clz(nsh));
                    break;
                }
                w = (w - 1u) & wmask;
                upto = 0xFFFFFFFFu;
            }
        }
        bs[i] = start & smask;
    }
}

template <class T>
__global__ __launch_bounds__(kBlock) void k_qf_add_spans(const T *filter, const uint32_t *occ, const uint32_t *cont, const uint32_t *sh, uint32_t q,
                                                         const uint32_t *hs, uint64_t n, const uint32_t *bs, uint32_t *covered, uint32_t *result)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        if (!qf_add_leader(hs, bs, n, i, 32u - q)) continue;
        if (qf_walk(filter, occ, cont, sh, q, hs, n, bs, i, covered).over) atomicOr(result + 1, 1u);
    }
}

template <class T>
__global__ __launch_bounds__(kBlock) void k_qf_add_write(T *filter, uint32_t *occ, uint32_t *cont, uint32_t *sh, uint32_t q, const uint32_t *hs, uint64_t n,
                                                         const uint32_t *bs, uint32_t *covered, uint32_t *result)
{
    const uint32_t smask = (1u << q) - 1u;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const bool refused = result[1] != 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        if (!qf_add_leader(hs, bs, n, i, 32u - q)) continue;
        const uint32_t b = bs[i] & smask, bit = 1u << (b & 31u);
        if (covered[b >> 5] & bit) {  // inside another group's region; the scratch goes back zeroed
            atomicAnd(covered + (b >> 5), ~bit);
            continue;
        }
        if (refused) continue;
        const QfWalk w = qf_walk(filter, occ, cont, sh, q, hs, n, bs, i, (uint32_t *)nullptr);
        if (w.over || !w.added) continue;
        qf_write_region(filter, occ, cont, sh, q, hs, n, i, w);
        atomicAdd(result, w.added);
    }
}

// ---- decode
// per metadata word: run starts, occupied bits, slots in use (counts[0 / 1 / 2][w]); marks[0] = the first slot with continuation = shifted = 0
// (the anchor x above), marks[1] = the first empty slot (0xFFFFFFFF: none, the table is full)
__global__ __launch_bounds__(kBlock) void k_qf_decode_count(const uint32_t *occ, const uint32_t *cont, const uint32_t *sh, uint32_t nwords, uint32_t valid,
                                                            long long *counts, uint32_t *marks)
{
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t w = blockIdx.x * kBlock + threadIdx.x; w < nwords; w += stride) {
        const uint32_t o = occ[w] & valid, c = cont[w] & valid, s = sh[w] & valid;
        counts[w] = __popc(~c & (o | s));
        counts[(uint64_t)nwords + w] = __popc(o);
        counts[2ull * nwords + w] = __popc(o | c | s);
        const uint32_t anchor = ~(c | s) & valid, empty = ~(o | c | s) & valid;
        if (anchor) atomicMin(marks, (w << 5) + (uint32_t)__ffs(anchor) - 1u);
        if (empty) atomicMin(marks + 1, (w << 5) + (uint32_t)__ffs(empty) - 1u);
    }
}

__device__ __forceinline__ long long excl(const long long *inc, uint32_t w) { return w ? inc[w - 1] : 0; }
__device__ __forceinline__ uint32_t below(uint32_t bit) { return (1u << bit) - 1u; }  // bits 0 .. bit - 1

// counts: the three rows above as INCLUSIVE prefix sums.  One lane per slot; a slot in use writes its hash at its rank among the slots in use.
template <class T>
__global__ __launch_bounds__(kBlock) void k_qf_decode_emit(const T *filter, const uint32_t *occ, const uint32_t *cont, const uint32_t *sh, uint32_t q, uint32_t nwords,
                                                           uint32_t valid, const long long *counts, const uint32_t *marks, uint32_t *out, uint64_t out_cap)
{
    const long long *runs = counts, *occs = counts + nwords, *used = counts + 2ull * nwords;
    const uint64_t size = 1ull << q, stride = (uint64_t)gridDim.x * kBlock;
    const long long nruns = runs[nwords - 1];
    if (!nruns || marks[0] >= size) return;  // (an anchor exists in every quotient filter's table: see the file comment; none = not one, nothing to list)
    const uint32_t x = marks[0], xw = x >> 5, xb = x & 31u;
    const long long wrapped = excl(runs, xw) + __popc(~cont[xw] & (occ[xw] | sh[xw]) & below(xb)) - excl(occs, xw) - __popc(occ[xw] & below(xb));
    for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < size; p += stride) {
        const uint32_t w = (uint32_t)(p >> 5), b = (uint32_t)p & 31u;
        const uint32_t o = occ[w] & valid, c = cont[w] & valid, s = sh[w] & valid, inuse = o | c | s;
        if (!((inuse >> b) & 1u)) continue;
        const long long k = excl(runs, w) + __popc(~c & (o | s) & (0xFFFFFFFFu >> (31u - b))) - 1;  // this slot's run, in slot order (-1: the run wrapped in from the end)
        long long idx = (k - wrapped) % nruns;
        if (idx < 0) idx += nruns;
        // the idx-th occupied quotient: the first word whose inclusive count passes idx, then the bit inside it
        uint32_t lo = 0, hi = nwords - 1;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (occs[mid] > idx) hi = mid;
            else lo = mid + 1;
        }
        uint32_t bits = occ[lo] & valid;
        for (long long t = idx - excl(occs, lo); t > 0 && bits; --t) bits &= bits - 1u;
        const uint32_t quot = (lo << 5) + (bits ? (uint32_t)__ffs(bits) - 1u : 0u);
        const uint64_t at = (uint64_t)excl(used, w) + __popc(inuse & below(b));
        if (at < out_cap) out[at] = (quot << (32u - q)) | (uint32_t)filter[p];
    }
}

unsigned grid_of(uint64_t n)
{
    const uint64_t g = (n + kBlock - 1) / kBlock;
    return (unsigned)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

int check_q(uint32_t q)
{
    if (q < 3 || q > 31) return fail(PSK_EINVAL, "quotient must be between 3 and 31; %u was provided", q);
    return PSK_OK;
}

uint32_t words_of(uint32_t q) { return q >= 5 ? 1u << (q - 5) : 1u; }
uint32_t valid_of(uint32_t q) { return q >= 5 ? 0xFFFFFFFFu : (1u << (1u << q)) - 1u; }
size_t rem_bytes(uint32_t q) { return 32 - q <= 8 ? 1 : (32 - q <= 16 ? 2 : 4); }

}  // namespace

extern "C" int psk_qf_build(uint32_t q, const uint32_t *sorted_hashes_dev, uint64_t n, void *filter_dev, uint32_t *occupied_dev, uint32_t *continuation_dev,
                            uint32_t *shifted_dev, int32_t *scratch_dev, int device, void *stream)
{
    PSK_TRY(check_q(q));
    if (!filter_dev || !occupied_dev || !continuation_dev || !shifted_dev) return fail(PSK_EINVAL, "NULL table pointer");
    if (n > (1ull << q)) return fail(PSK_EINVAL, "%llu distinct hashes do not fit a table of 2^%u slots", (unsigned long long)n, q);
    if (n && (!sorted_hashes_dev || !scratch_dev)) return fail(PSK_EINVAL, "NULL argument");
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const size_t wbytes = (size_t)words_of(q) * 4;
    HIP_TRY(hipMemsetAsync(filter_dev, 0, rem_bytes(q) << q, st));
    HIP_TRY(hipMemsetAsync(occupied_dev, 0, wbytes, st));
    HIP_TRY(hipMemsetAsync(continuation_dev, 0, wbytes, st));
    HIP_TRY(hipMemsetAsync(shifted_dev, 0, wbytes, st));
    if (!n) return PSK_OK;
    const uint32_t ntiles = (uint32_t)((n + kTile - 1) / kTile), rbits = 32 - q;
    hipLaunchKernelGGL(k_qf_tile_max, dim3(ntiles), dim3(kBlock), 0, st, sorted_hashes_dev, n, rbits, scratch_dev);
    hipLaunchKernelGGL(k_qf_tile_scan, dim3(1), dim3(kBlock), 0, st, scratch_dev, ntiles);
    const int32_t *carry = scratch_dev;
    if (rbits <= 8)
        hipLaunchKernelGGL((k_qf_place<uint8_t>), dim3(ntiles), dim3(kBlock), 0, st, sorted_hashes_dev, n, q, carry, ntiles, (uint8_t *)filter_dev, occupied_dev, continuation_dev, shifted_dev);
    else if (rbits <= 16)
        hipLaunchKernelGGL((k_qf_place<uint16_t>), dim3(ntiles), dim3(kBlock), 0, st, sorted_hashes_dev, n, q, carry, ntiles, (uint16_t *)filter_dev, occupied_dev, continuation_dev, shifted_dev);
    else
        hipLaunchKernelGGL((k_qf_place<uint32_t>), dim3(ntiles), dim3(kBlock), 0, st, sorted_hashes_dev, n, q, carry, ntiles, (uint32_t *)filter_dev, occupied_dev, continuation_dev, shifted_dev);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

extern "C" int psk_qf_check_alt(uint32_t q, const void *filter_dev, const uint32_t *occupied_dev, const uint32_t *continuation_dev, const uint32_t *shifted_dev,
                                const uint32_t *hashes_dev, uint64_t n, uint8_t *out_dev, int device, void *stream)
{
    PSK_TRY(check_q(q));
    if (!filter_dev || !occupied_dev || !continuation_dev || !shifted_dev) return fail(PSK_EINVAL, "NULL table pointer");
    if (n && (!hashes_dev || !out_dev)) return fail(PSK_EINVAL, "NULL argument");
    PSK_USE_DEVICE(device);
    if (!n) return PSK_OK;
    const psk::QfTable t{filter_dev, occupied_dev, continuation_dev, shifted_dev, q};
    hipLaunchKernelGGL(k_qf_check_alt, dim3(grid_for_keys(n)), dim3(kBlock), 0, (hipStream_t)stream, t, hashes_dev, n, out_dev);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

// the table without the hashes of the batch: `for h in hashes: remove_alt(h)` (quotientfilter.py:177-185, :396-469) on a table with an empty slot.
// scratch_dev (uint32): dead[words], dirty[words], the list cursor and a pad word -- zero on entry, zero again when the call has run -- then n list entries.
extern "C" int psk_qf_remove_alt(uint32_t q, void *filter_dev, uint32_t *occupied_dev, uint32_t *continuation_dev, uint32_t *shifted_dev,
                                 const uint32_t *sorted_hashes_dev, uint64_t n, uint32_t *scratch_dev, uint32_t *removed_dev, int device, void *stream)
{
    PSK_TRY(check_q(q));
    if (q < 5) return fail(PSK_EINVAL, "a table of 2^%u slots shares one metadata word between all its slots: rebuild it (psk_qf_build)", q);
    if (!filter_dev || !occupied_dev || !continuation_dev || !shifted_dev || !removed_dev) return fail(PSK_EINVAL, "NULL table pointer");
    if (n > (1ull << 32)) return fail(PSK_EINVAL, "%llu hashes cannot be distinct", (unsigned long long)n);
    if (n && (!sorted_hashes_dev || !scratch_dev)) return fail(PSK_EINVAL, "NULL argument");
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(removed_dev, 0, 4, st));
    if (!n) return PSK_OK;
    const uint32_t nwords = words_of(q);
    uint32_t *dead = scratch_dev, *dirty = scratch_dev + nwords, *cursor = scratch_dev + 2ull * nwords, *list = cursor + 2;
    const psk::QfTable t{filter_dev, occupied_dev, continuation_dev, shifted_dev, q};
    hipLaunchKernelGGL(k_qf_locate, dim3(grid_for_keys(n)), dim3(kBlock), 0, st, t, sorted_hashes_dev, n, dead, dirty, cursor, list, removed_dev);
    const unsigned grid = grid_of(n);
    const uint32_t rbits = 32 - q;
    if (rbits <= 8)
        hipLaunchKernelGGL((k_qf_repack<uint8_t>), dim3(grid), dim3(kBlock), 0, st, (uint8_t *)filter_dev, occupied_dev, continuation_dev, shifted_dev, q, dead, dirty, cursor, list, n);
    else if (rbits <= 16)
        hipLaunchKernelGGL((k_qf_repack<uint16_t>), dim3(grid), dim3(kBlock), 0, st, (uint16_t *)filter_dev, occupied_dev, continuation_dev, shifted_dev, q, dead, dirty, cursor, list, n);
    else
        hipLaunchKernelGGL((k_qf_repack<uint32_t>), dim3(grid), dim3(kBlock), 0, st, (uint32_t *)filter_dev, occupied_dev, continuation_dev, shifted_dev, q, dead, dirty, cursor, list, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(cursor, 0, 4, st));
    return PSK_OK;
}

// the table with the hashes of the batch: `for h in hashes: add_alt(h)` (quotientfilter.py:154-166, :355-394), auto-expansion left to the caller.
// scratch_dev (uint32): the removal's layout, so that one allocation serves both -- 2 * words + 2 words that are zero on entry and zero again when the call
// has run (the first `words` are the covered bitmap, the rest is not touched), then n cluster starts.  result_dev: added, status.
extern "C" int psk_qf_add_alt(uint32_t q, void *filter_dev, uint32_t *occupied_dev, uint32_t *continuation_dev, uint32_t *shifted_dev,
                              const uint32_t *sorted_hashes_dev, uint64_t n, uint32_t *scratch_dev, uint32_t *result_dev, int device, void *stream)
{
    PSK_TRY(check_q(q));
    if (q < 5) return fail(PSK_EINVAL, "a table of 2^%u slots shares one metadata word between all its slots: rebuild it (psk_qf_build)", q);
    if (!filter_dev || !occupied_dev || !continuation_dev || !shifted_dev || !result_dev) return fail(PSK_EINVAL, "NULL table pointer");
    if (n > (1ull << 32)) return fail(PSK_EINVAL, "%llu hashes cannot be distinct", (unsigned long long)n);
    if (n && (!sorted_hashes_dev || !scratch_dev)) return fail(PSK_EINVAL, "NULL argument");
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(result_dev, 0, 8, st));
    if (!n) return PSK_OK;
    uint32_t *covered = scratch_dev, *bs = scratch_dev + 2ull * words_of(q) + 2;
    const unsigned grid = grid_of(n);
    const uint32_t rbits = 32 - q;
    hipLaunchKernelGGL(k_qf_add_starts, dim3(grid), dim3(kBlock), 0, st, occupied_dev, shifted_dev, q, sorted_hashes_dev, n, bs);
    auto run = [&](auto *filter) {
        using T = std::remove_pointer_t<decltype(filter)>;
        hipLaunchKernelGGL((k_qf_add_spans<T>), dim3(grid), dim3(kBlock), 0, st, filter, occupied_dev, continuation_dev, shifted_dev, q, sorted_hashes_dev, n, bs, covered, result_dev);
        hipLaunchKernelGGL((k_qf_add_write<T>), dim3(grid), dim3(kBlock), 0, st, filter, occupied_dev, continuation_dev, shifted_dev, q, sorted_hashes_dev, n, bs, covered, result_dev);
    };
    if (rbits <= 8) run((uint8_t *)filter_dev);
    else if (rbits <= 16) run((uint16_t *)filter_dev);
    else run((uint32_t *)filter_dev);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

extern "C" int psk_qf_decode(uint32_t q, const void *filter_dev, const uint32_t *occupied_dev, const uint32_t *continuation_dev, const uint32_t *shifted_dev,
                             int64_t *word_counts_dev, uint32_t *marks_dev, uint32_t *out_dev, uint64_t out_cap, int device, void *stream)
{
    PSK_TRY(check_q(q));
    if (!filter_dev || !occupied_dev || !continuation_dev || !shifted_dev || !word_counts_dev || !marks_dev) return fail(PSK_EINVAL, "NULL argument");
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nwords = words_of(q), valid = valid_of(q);
    if (!out_dev) {  // pass 1: the per-word counts and the two marks
        HIP_TRY(hipMemsetAsync(marks_dev, 0xFF, 8, st));
        hipLaunchKernelGGL(k_qf_decode_count, dim3(grid_of(nwords)), dim3(kBlock), 0, st, occupied_dev, continuation_dev, shifted_dev, nwords, valid,
                           (long long *)word_counts_dev, marks_dev);
        HIP_TRY(hipGetLastError());
        return PSK_OK;
    }
    const long long *counts = (const long long *)word_counts_dev;
    const unsigned grid = grid_of(1ull << q);
    const uint32_t rbits = 32 - q;
    if (rbits <= 8)
        hipLaunchKernelGGL((k_qf_decode_emit<uint8_t>), dim3(grid), dim3(kBlock), 0, st, (const uint8_t *)filter_dev, occupied_dev, continuation_dev, shifted_dev, q, nwords, valid, counts, marks_dev, out_dev, out_cap);
    else if (rbits <= 16)
        hipLaunchKernelGGL((k_qf_decode_emit<uint16_t>), dim3(grid), dim3(kBlock), 0, st, (const uint16_t *)filter_dev, occupied_dev, continuation_dev, shifted_dev, q, nwords, valid, counts, marks_dev, out_dev, out_cap);
    else
        hipLaunchKernelGGL((k_qf_decode_emit<uint32_t>), dim3(grid), dim3(kBlock), 0, st, (const uint32_t *)filter_dev, occupied_dev, continuation_dev, shifted_dev, q, nwords, valid, counts, marks_dev, out_dev, out_cap);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

// out[i] = fnv_1a_32(key_i, 0)  (hashes.py:106-122; quotientfilter.py:151 add, :194 check); PSK_KEYS_HASHES: the low half of each row's first hash
extern "C" int psk_qf_hash(int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len, int where, uint32_t *out, int device,
                           void *stream)
{
    if (layout == PSK_KEYS_HASHES && key_len < 1) return fail(PSK_EINVAL, "pre-hashed batch carries no hash per key");
    if (n && !out) return fail(PSK_EINVAL, "out is NULL");
    return keyed_call(layout, data, offsets, n, key_len, where, out, n * 4, device, stream, [&](auto src, void *out_dev, hipStream_t st) {
        hipLaunchKernelGGL((k_qf_hash<decltype(src)>), dim3(grid_for_keys(n)), dim3(kBlock), 0, st, src, (uint32_t *)out_dev, n);
    });
}

// out[i] = key_i's hash is in the table (quotientfilter.py:187-206 check / check_alt): hash and walk in one kernel
extern "C" int psk_qf_check(uint32_t q, const void *filter_dev, const uint32_t *occupied_dev, const uint32_t *continuation_dev, const uint32_t *shifted_dev,
                            int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len, int where, uint8_t *out, int device,
                            void *stream)
{
    PSK_TRY(check_q(q));
    if (!filter_dev || !occupied_dev || !continuation_dev || !shifted_dev) return fail(PSK_EINVAL, "NULL table pointer");
    if (layout == PSK_KEYS_HASHES && key_len < 1) return fail(PSK_EINVAL, "pre-hashed batch carries no hash per key");
    if (n && !out) return fail(PSK_EINVAL, "out is NULL");
    const psk::QfTable t{filter_dev, occupied_dev, continuation_dev, shifted_dev, q};
    return keyed_call(layout, data, offsets, n, key_len, where, out, n, device, stream, [&](auto src, void *out_dev, hipStream_t st) {
        hipLaunchKernelGGL((k_qf_check<decltype(src)>), dim3(grid_for_keys(n)), dim3(kBlock), 0, st, src, t, (uint8_t *)out_dev, n);
    });
}
