// psk_cuckoo.hip -- cuckoo filter: parallel placement, the sequential kick walk, ordered removal (include/psk.h "CuckooFilter").
//
// Parallel placement (k_ck_sweep / k_ck_apply / k_ck_count).  The stream is a list of triples that are known not to be in the table and not
// to repeat (the host removed those).  Key j goes to bucket idx_1 if that row still has room after the earlier keys of the stream that went
// there, else to idx_2 by the same test, else it needs a kick (K) -- cuckoo.py:361-368.  Its decision d_j in {1, 2, K} depends only on d_t
// for t < j, so the decisions are the unique fixed point of a triangular system, and Jacobi sweeps from "all 1" have a STABLE PREFIX: if
// no d_t with t < e changed in a sweep, [0, e) is a fixed point of its own sub-system, which is unique by induction on t, hence final.
// Every sweep extends that prefix by at least one key.  Each key owns two claims (bucket, j, which); the host sorts the 2m claims once
// (torch: rocPRIM's radix sort), a lane walks back over the claims of its bucket in front of its own and counts the active ones
// (d_t == which + 1).  The accepted prefix ends at min(e, first K): everything in front of it is placed exactly as the reference would,
// slot = fill + (active claims in front), and nothing random has happened yet.
//
// Sequential insert (k_ck_insert).  One lane walks the triples in order and applies cuckoo.py:291-304 / :361-392 as written; the kicks
// draw from an MT19937 whose 625 words (random.getstate()) it reads from and writes back to a device buffer, so the table AND the
// generator end as the reference's would.  The other 63 lanes of the wave only touch the rows of the next keys so that they are in cache.
// Every loop has a bound valid data cannot reach (the rejection loop of _randbelow: 256 draws, each accepted with probability >= 1/2),
// and the step budget of a launch is also tested inside a walk: a walk that runs out of it is suspended (fingerprint in hand, row, swaps done go to
// `res`) and the next launch takes it up there, so max_swaps does not bound how long a launch runs.
//
// Ordered removal (k_ck_rm_mark / k_ck_rm_compact).  `for k in keys: remove(k)` removes, for every fingerprint, its copies in the order
// idx_1's row left to right, then idx_2's row (cuckoo.py:317-330, list.remove takes the first occurrence), one per request: the t-th
// request for a fingerprint (t from 0, the host ranks them) succeeds iff t < copies and takes copy number t.  Lanes mark slots in a
// per-row bit mask; the lane that swaps a non-zero mask out compacts that row to the left, zeroes what it vacates and lowers `fill`.
#include "psk_stage.hpp"
#include "psk_cuckoo.hpp"

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint8_t kKick = 3;

struct CkTable {
    uint32_t *buckets, *fill;
};

__global__ __launch_bounds__(kBlock) void k_ck_present(CkGeom g, const uint32_t *buckets, const uint32_t *fill, const uint32_t *tr, uint64_t n, uint8_t *out)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
    {
        const CkTriple t{tr[i], tr[n + i], tr[2 * n + i]};
        out[i] = t.i1 < g.capacity && t.i2 < g.capacity && ck_contains(g, buckets, fill, t) ? 1 : 0;
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

// marks[0] = min j whose decision changed in this sweep, marks[1] = min j that decided K in this sweep
__global__ __launch_bounds__(kBlock) void k_ck_sweep(CkGeom g, const uint32_t *fill, const uint32_t *tr, const unsigned long long *claims, const uint32_t *pos,
                                                     uint32_t m, const uint8_t *d_in, uint8_t *d_out, uint32_t *marks)
{
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < m; j += stride) {
        uint8_t d = kKick;
        for (uint32_t which = 0; which < 2; ++which) {
            const uint32_t b = tr[(uint64_t)(1 + which) * m + j];
            if (b >= g.capacity) continue;
            const uint32_t f = fill[b];
            if (f >= g.B) continue;
            const uint32_t room = g.B - f;
            const uint32_t c = ck_active_before(claims, d_in, m, pos[(uint64_t)which * m + j], b, j, room);
            if (c == kNone) break;  // K
            if (c < room) {
                d = (uint8_t)(which + 1);
                break;
            }
        }
        d_out[j] = d;
        if (d != d_in[j]) atomicMin(marks, j);
        if (d == kKick) atomicMin(marks + 1, j);
    }
}

// keys [0, p) with final decisions: write the fingerprints (fill is read, not written: k_ck_count follows)
__global__ __launch_bounds__(kBlock) void k_ck_apply(CkGeom g, CkTable t, const uint32_t *tr, const unsigned long long *claims, const uint32_t *pos, uint32_t m,
                                                     const uint8_t *d, uint32_t p)
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
        if (slot < g.B) t.buckets[(uint64_t)b * g.B + slot] = tr[j];
    }
}

__global__ __launch_bounds__(kBlock) void k_ck_count(CkGeom g, uint32_t *fill, const uint32_t *tr, uint32_t m, const uint8_t *d, uint32_t p)
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
__global__ __launch_bounds__(64) void k_ck_insert(CkGeom g, CkTable t, uint32_t max_swaps, const uint32_t *tr, uint64_t n, uint64_t start, uint64_t end,
                                                  int dedup, uint64_t budget, uint32_t *state, uint32_t *res)
{
    __shared__ uint32_t words[624];
    const uint32_t lane = threadIdx.x;
    for (uint32_t k = lane; k < 624u; k += 64u) words[k] = state[k];
    __syncthreads();
    Mt mt{words, state[624], false};
    if (mt.idx > 624u) mt.idx = 624u;
    uint32_t status = 0, leftover = 0, added = 0, walked = 0, hand = 0, hand_row = 0, hand_swaps = 0;
    bool resume = res[0] == 3u;
    uint64_t steps = 0, i = start;
    bool stop = false;
    for (uint64_t base = start; base < end && !stop; base += 64) {
        {  // all lanes: pull the two rows of the next 64 keys towards the cache; nothing is decided here
            const uint64_t k = base + lane;
            if (k < end) {
                const uint32_t r1 = tr[n + k], r2 = tr[2 * n + k];
                if (r1 < g.capacity && r2 < g.capacity) {
                    uint32_t a = t.buckets[(uint64_t)r1 * g.B], b = t.buckets[(uint64_t)r2 * g.B];
                    asm volatile("" ::"v"(a), "v"(b));
                }
            }
        }
        if (lane != 0) continue;
        const uint64_t top = base + 64 < end ? base + 64 : end;
        for (i = base; i < top; ++i) {
            if (steps >= budget) { stop = true; break; }
            uint32_t fp, idx, s = 0;
            if (resume) {  // (budget >= 1: this launch does at least one swap of it)
                resume = false;
                fp = res[6], idx = res[7], s = res[8];
                if (idx >= g.capacity) { status = 2; stop = true; break; }
            } else {
                ++steps;
                fp = tr[i];
                const uint32_t i1 = tr[n + i], i2 = tr[2 * n + i];
                if (i1 >= g.capacity || i2 >= g.capacity) { status = 2; stop = true; break; }
                if (dedup && ck_contains(g, t.buckets, t.fill, CkTriple{fp, i1, i2})) continue;
                uint32_t f = t.fill[i1], row = i1;
                if (f >= g.B) f = t.fill[i2], row = i2;
                if (f < g.B) {
                    t.buckets[(uint64_t)row * g.B + f] = fp;
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
                uint32_t *slot = t.buckets + (uint64_t)idx * g.B + mt.below(g.B);  // random.randint(0, bucket_size - 1)
                const uint32_t out = *slot;
                *slot = fp;
                fp = out;
                const CkTriple e = ck_triple_of(g, fp);
                idx = idx == e.i1 ? e.i2 : e.i1;
                const uint32_t fe = t.fill[idx];
                if (fe < g.B) {
                    t.buckets[(uint64_t)idx * g.B + fe] = fp;
                    t.fill[idx] = fe + 1u;
                    ++added;
                    placed = true;
                    break;
                }
            }
            if (mt.bad) { status = 2; stop = true; break; }
            if (suspended) { status = 3, hand = fp, hand_row = idx, hand_swaps = s; stop = true; break; }
            if (!placed) { status = 1, leftover = fp; stop = true; break; }
        }
    }
    __syncthreads();
    if (lane == 0) {
        res[0] = status, res[1] = (uint32_t)i, res[2] = leftover, res[3] = added, res[4] = walked, res[5] = (uint32_t)(steps > 0xFFFFFFFFull ? 0xFFFFFFFFull : steps);
        res[6] = hand, res[7] = hand_row, res[8] = hand_swaps;
        state[624] = mt.idx;
    }
    for (uint32_t k = lane; k < 624u; k += 64u) state[k] = words[k];
}

// ---- ordered removal
// -> copies of fp in the row; *slot = where copy number `want` stands (kNone: there are fewer)
__device__ __forceinline__ uint32_t ck_copies(const CkGeom &g, const CkTable &t, uint32_t row, uint32_t fp, uint32_t want, uint32_t *slot)
{
    const uint32_t f = min(t.fill[row], g.B);
    const uint32_t *p = t.buckets + (uint64_t)row * g.B;
    uint32_t c = 0;
    *slot = kNone;
    for (uint32_t s = 0; s < f; ++s)
        if (p[s] == fp) {
            if (c == want) *slot = s;
            ++c;
        }
    return c;
}

__global__ __launch_bounds__(kBlock) void k_ck_rm_mark(CkGeom g, CkTable t, const uint32_t *tr, const uint32_t *rank, uint64_t n, uint32_t *marks, uint8_t *out)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const uint32_t fp = tr[i], i1 = tr[n + i], i2 = tr[2 * n + i], want = rank[i];
        if (i1 >= g.capacity || i2 >= g.capacity) {
            out[i] = 0;
            continue;
        }
        uint32_t slot, row = i1;
        const uint32_t c1 = ck_copies(g, t, i1, fp, want, &slot);
        if (slot == kNone && i2 != i1 && want >= c1) {
            row = i2;
            ck_copies(g, t, i2, fp, want - c1, &slot);
        }
        if (slot != kNone) atomicOr(marks + row, 1u << slot);
        out[i] = slot != kNone ? 1 : 0;
    }
}

__global__ __launch_bounds__(kBlock) void k_ck_rm_compact(CkGeom g, CkTable t, const uint32_t *tr, uint64_t n, uint32_t *marks)
{
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        for (int which = 0; which < 2; ++which) {
            const uint32_t row = tr[(uint64_t)(1 + which) * n + i];
            if (row >= g.capacity || !marks[row]) continue;
            const uint32_t gone = atomicExch(marks + row, 0u);  // one lane gets the mask, and with it the row
            if (!gone) continue;
            uint32_t *p = t.buckets + (uint64_t)row * g.B;
            const uint32_t f = min(t.fill[row], g.B);
            uint32_t w = 0;
            for (uint32_t s = 0; s < f; ++s) {
                const uint32_t v = p[s];
                if (!((gone >> s) & 1u)) p[w++] = v;
            }
            for (uint32_t s = w; s < f; ++s) p[s] = 0;
            t.fill[row] = w;
        }
    }
}

int ck_geom(uint64_t capacity, uint32_t bucket_size, uint32_t fp_bits, CkGeom *g)
{
    if (!ck_make_geom(capacity, bucket_size, fp_bits, g))
        return fail(PSK_EINVAL, "cuckoo filter: capacity must be in 1 .. 2^31 - 1, bucket_size >= 1, fingerprint bits in 1 .. 32 (got %llu x %u, %u bits)",
                    (unsigned long long)capacity, bucket_size, fp_bits);
    return PSK_OK;
}
// (the calls that take triples: the fingerprints are whole 32-bit words by then)
int geom_of(uint64_t capacity, uint32_t bucket_size, CkGeom *g) { return ck_geom(capacity, bucket_size, 32, g); }

}  // namespace

extern "C" int psk_ck_present(uint64_t capacity, uint32_t bucket_size, const uint32_t *buckets_dev, const uint32_t *fill_dev, const uint32_t *triples_dev, uint64_t n,
                              uint8_t *out_dev, int device, void *stream)
{
    CkGeom g;
    PSK_TRY(geom_of(capacity, bucket_size, &g));
    if (!buckets_dev || !fill_dev) return fail(PSK_EINVAL, "NULL table pointer");
    if (n && (!triples_dev || !out_dev)) return fail(PSK_EINVAL, "NULL argument");
    PSK_USE_DEVICE(device);
    if (!n) return PSK_OK;
    hipLaunchKernelGGL(k_ck_present, dim3(grid_for_keys(n)), dim3(kBlock), 0, (hipStream_t)stream, g, buckets_dev, fill_dev, triples_dev, n, out_dev);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

extern "C" int psk_ck_place_sweep(uint64_t capacity, uint32_t bucket_size, const uint32_t *fill_dev, const uint32_t *triples_dev, const uint64_t *claims_dev,
                                  const uint32_t *pos_dev, uint64_t m, const uint8_t *d_in_dev, uint8_t *d_out_dev, uint32_t *marks_dev, int device, void *stream)
{
    CkGeom g;
    PSK_TRY(geom_of(capacity, bucket_size, &g));
    if (m >= (1ull << 31)) return fail(PSK_EINVAL, "a placement batch holds fewer than 2^31 keys");
    if (!fill_dev || !marks_dev || (m && (!triples_dev || !claims_dev || !pos_dev || !d_in_dev || !d_out_dev))) return fail(PSK_EINVAL, "NULL argument");
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(marks_dev, 0xFF, 8, st));
    if (!m) return PSK_OK;
    hipLaunchKernelGGL(k_ck_sweep, dim3(grid_for_keys(m)), dim3(kBlock), 0, st, g, fill_dev, triples_dev, (const unsigned long long *)claims_dev, pos_dev, (uint32_t)m,
                       d_in_dev, d_out_dev, marks_dev);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

extern "C" int psk_ck_place_apply(uint64_t capacity, uint32_t bucket_size, uint32_t *buckets_dev, uint32_t *fill_dev, const uint32_t *triples_dev,
                                  const uint64_t *claims_dev, const uint32_t *pos_dev, uint64_t m, const uint8_t *d_dev, uint64_t prefix, int device, void *stream)
{
    CkGeom g;
    PSK_TRY(geom_of(capacity, bucket_size, &g));
    if (m >= (1ull << 31) || prefix > m) return fail(PSK_EINVAL, "a placement batch holds fewer than 2^31 keys and the prefix lies inside it");
    if (!buckets_dev || !fill_dev || (m && (!triples_dev || !claims_dev || !pos_dev || !d_dev))) return fail(PSK_EINVAL, "NULL argument");
    PSK_USE_DEVICE(device);
    if (!prefix) return PSK_OK;
    hipStream_t st = (hipStream_t)stream;
    const CkTable t{buckets_dev, fill_dev};
    hipLaunchKernelGGL(k_ck_apply, dim3(grid_for_keys(prefix)), dim3(kBlock), 0, st, g, t, triples_dev, (const unsigned long long *)claims_dev, pos_dev, (uint32_t)m, d_dev,
                       (uint32_t)prefix);
    hipLaunchKernelGGL(k_ck_count, dim3(grid_for_keys(prefix)), dim3(kBlock), 0, st, g, fill_dev, triples_dev, (uint32_t)m, d_dev, (uint32_t)prefix);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

extern "C" int psk_ck_insert(uint64_t capacity, uint32_t bucket_size, uint32_t max_swaps, uint32_t *buckets_dev, uint32_t *fill_dev, const uint32_t *triples_dev,
                             uint64_t n, uint64_t start, uint64_t end, int dedup, uint64_t budget, uint32_t *mt_state_dev, uint32_t *result_dev, int device, void *stream)
{
    CkGeom g;
    PSK_TRY(geom_of(capacity, bucket_size, &g));
    if (n >= (1ull << 32) || start > end || end > n) return fail(PSK_EINVAL, "psk_ck_insert: need start <= end <= n < 2^32");
    if (!budget) return fail(PSK_EINVAL, "psk_ck_insert: a launch needs a budget of at least one step");
    if (!buckets_dev || !fill_dev || !mt_state_dev || !result_dev || (n && !triples_dev)) return fail(PSK_EINVAL, "NULL argument");
    PSK_USE_DEVICE(device);
    const CkTable t{buckets_dev, fill_dev};
    hipLaunchKernelGGL(k_ck_insert, dim3(1), dim3(64), 0, (hipStream_t)stream, g, t, max_swaps, triples_dev, n, start, end, dedup, budget, mt_state_dev, result_dev);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

extern "C" int psk_ck_remove(uint64_t capacity, uint32_t bucket_size, uint32_t *buckets_dev, uint32_t *fill_dev, const uint32_t *triples_dev, const uint32_t *rank_dev,
                             uint64_t n, uint32_t *row_marks_dev, uint8_t *out_dev, int device, void *stream)
{
    CkGeom g;
    PSK_TRY(geom_of(capacity, bucket_size, &g));
    if (bucket_size > 32) return fail(PSK_EINVAL, "psk_ck_remove: bucket_size up to 32 (a row's removals are one 32-bit mask), got %u", bucket_size);
    if (!buckets_dev || !fill_dev || !row_marks_dev) return fail(PSK_EINVAL, "NULL table pointer");
    if (n && (!triples_dev || !rank_dev || !out_dev)) return fail(PSK_EINVAL, "NULL argument");
    PSK_USE_DEVICE(device);
    if (!n) return PSK_OK;
    hipStream_t st = (hipStream_t)stream;
    const CkTable t{buckets_dev, fill_dev};
    hipLaunchKernelGGL(k_ck_rm_mark, dim3(grid_for_keys(n)), dim3(kBlock), 0, st, g, t, triples_dev, rank_dev, n, row_marks_dev, out_dev);
    hipLaunchKernelGGL(k_ck_rm_compact, dim3(grid_for_keys(n)), dim3(kBlock), 0, st, g, t, triples_dev, n, row_marks_dev);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

// out[3][n] = (fp, idx_1, idx_2) of every key (cuckoo.py:483-506 _indicies_from_fingerprint / _generate_fingerprint_info)
extern "C" int psk_ck_triples(uint64_t capacity, uint32_t fp_bits, int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len, int where,
                              uint32_t *out, int device, void *stream)
{
    CkGeom g;
    PSK_TRY(ck_geom(capacity, 1, fp_bits, &g));
    if (layout == PSK_KEYS_HASHES && key_len < 1) return fail(PSK_EINVAL, "pre-hashed batch carries no hash per key");
    if (n && !out) return fail(PSK_EINVAL, "out is NULL");
    return keyed_call(layout, data, offsets, n, key_len, where, out, n * 12, device, stream, [&](auto src, void *out_dev, hipStream_t st) {
        hipLaunchKernelGGL((k_ck_triples<decltype(src)>), dim3(grid_for_keys(n)), dim3(kBlock), 0, st, src, g, (uint32_t *)out_dev, n);
    });
}

// out[i] = check(key_i) (cuckoo.py:306-315): hash, idx_1's row, idx_2's row only if needed, in one kernel
extern "C" int psk_ck_check(uint64_t capacity, uint32_t bucket_size, uint32_t fp_bits, const uint32_t *buckets_dev, const uint32_t *fill_dev, int layout,
                            const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len, int where, uint8_t *out, int device, void *stream)
{
    CkGeom g;
    PSK_TRY(ck_geom(capacity, bucket_size, fp_bits, &g));
    if (!buckets_dev || !fill_dev) return fail(PSK_EINVAL, "NULL table pointer");
    if (layout == PSK_KEYS_HASHES && key_len < 1) return fail(PSK_EINVAL, "pre-hashed batch carries no hash per key");
    if (n && !out) return fail(PSK_EINVAL, "out is NULL");
    return keyed_call(layout, data, offsets, n, key_len, where, out, n, device, stream, [&](auto src, void *out_dev, hipStream_t st) {
        hipLaunchKernelGGL((k_ck_check<decltype(src)>), dim3(grid_for_keys(n)), dim3(kBlock), 0, st, src, g, buckets_dev, fill_dev, (uint8_t *)out_dev, n);
    });
}
