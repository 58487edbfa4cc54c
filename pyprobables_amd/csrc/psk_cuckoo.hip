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
// Sequential insert (k_ck_insert, psk_cuckoo.hpp: the counting filter runs the same walk over (fingerprint, count) pairs).  One lane walks the triples in order and applies cuckoo.py:291-304 / :361-392 as written; the kicks
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

// ---- parallel placement (ck_active_before, k_ck_apply, k_ck_count: psk_cuckoo.hpp)
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

// ---- ordered removal (k_ck_rm_compact: psk_cuckoo.hpp)
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
    hipLaunchKernelGGL(k_ck_present<1>, dim3(grid_for_keys(n)), dim3(kBlock), 0, (hipStream_t)stream, g, buckets_dev, fill_dev, triples_dev, n, out_dev);
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
    hipLaunchKernelGGL(k_ck_apply<1>, dim3(grid_for_keys(prefix)), dim3(kBlock), 0, st, g, t, triples_dev, (const unsigned long long *)claims_dev, pos_dev, (uint32_t)m, d_dev,
                       (uint32_t)prefix, (const uint32_t *)nullptr);
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
    hipLaunchKernelGGL(k_ck_insert<1>, dim3(1), dim3(64), 0, (hipStream_t)stream, g, t, max_swaps, triples_dev, (const uint32_t *)nullptr, n, start, end, dedup, budget, mt_state_dev, result_dev);
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
    hipLaunchKernelGGL(k_ck_rm_compact<1>, dim3(grid_for_keys(n)), dim3(kBlock), 0, st, g, t, triples_dev, n, row_marks_dev);
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
