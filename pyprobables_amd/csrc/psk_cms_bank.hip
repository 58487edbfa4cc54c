// psk_cms_bank.hip -- CountMinSketchBank (include/psk.h "CountMinSketchBank"): many small count-min sketches of one geometry
// (width, depth) in one table, row s the reference's CountMinSketch after add(key, num_els) of the ops sent to s (countminsketch.py:257-288).
// Only adds enter a bank, with weights >= 0: every bin ends at min(old + the weights that reached it, INT32_MAX) in any order of execution.
//   psk_cms_bank_add / _check / _check_meanmin   keys with a sketch id each: ops on k_apply (psk_device.hpp), atomics into / loads from row ids[i]
//   psk_cms_bank_build    keys grouped by sketch: one workgroup per (sketch, part) counts in an LDS image of the row and adds the image's non-zero
//                         counters to the row once (`depth` read-modify-writes a key stay on the CU)
//   psk_cms_bank_reduce   groups of rows folded by the reference's join (countminsketch.py:380-399) into a new table
// The bound: bound_dev[s] is the caller's upper bound on every bin of sketch s AFTER the call.  At or below INT32_MAX nothing of s can reach the rail
// and an add is a plain no-return atomic; above it (or without a bound) it is cms_sat_add, the clamping CAS loop of the single sketch.
#include "psk_bank_stage.hpp"

namespace {

constexpr uint64_t kCmsBankMaxWidth = 1ULL << 31;  // reduce_small's range
constexpr uint32_t kCmsBankLdsInts = 16384;        // the image is dynamic LDS of exactly one row: 64 KiB, the default limit, at the cap
constexpr unsigned kCmsBankGridCap = 256 * 16;     // workgroups along x: more sketches (reduce: groups x row pieces) than that are walked with a stride
// route 0: a part whose keys * depth * R is below the row's ints goes straight to the row -- clearing and sweeping the image would cost more than
// its probes.  Measured (scripts/bench_cms_bank.py part (c), profiles/cms_bank_bench.txt: 4096 rows of 10240 ints, depth 5, one MI355X, run with the
// Bloom bank's R = 16): the atomics are 7 to 20 % ahead up to 128 keys per sketch (keys * depth / ints = 0.0625), level at 256 (0.125: 1.01 x), the
// image 1.20 x ahead at 512 and 1.66 x at 1024: the crossover lies at ints / (keys * depth) = 8.  One geometry only.
constexpr uint32_t kCmsBankRouteR = 8;

// column of hash h in a row of md.m <= 2^31 columns (countminsketch.py:275)
template <bool POW2>
__device__ __forceinline__ uint32_t cms_bank_col(const Mod &md, uint64_t h)
{
    if (POW2) return (uint32_t)(h & md.mask);
    return reduce_small(md, h);
}

// v >= 0 onto a bin of the table: plain where the bound says no bin of the sketch reaches the rail, else clamped (countminsketch.py:280-282)
__device__ __forceinline__ void cms_bank_bin_add(int32_t *p, uint32_t v, bool plain, unsigned long long *sat)
{
    if (plain) atomicAdd(p, (int32_t)v);  // result unused -> no-return global_atomic_add
    else cms_sat_add(p, (int64_t)v, sat);
}

__device__ __forceinline__ bool cms_bank_plain(const int64_t *bound, uint64_t s) { return bound && bound[s] <= (int64_t)INT32_MAX; }

template <bool POW2>
struct CmsBankAdd {  // countminsketch.py:267-288 add_alt on row ids[i]; ids >= sketches: no row, nothing written; a negative weight counts as 0
    int32_t *tab;
    uint64_t row_ints, sketches;
    const uint32_t *ids;
    Mod md;
    uint32_t k;
    const int32_t *weights;
    const int64_t *bound;
    unsigned long long *sat;
    struct State { int32_t *row; uint32_t w; bool plain; };
    __device__ __forceinline__ void prepare() {}
    __device__ __forceinline__ State begin(uint64_t i) const
    {
        const uint64_t s = ids[i];
        const int32_t w = weights ? weights[i] : 1;
        if (s >= sketches || w <= 0) return State{nullptr, 0u, false};
        return State{tab + s * row_ints, (uint32_t)w, cms_bank_plain(bound, s)};  // (64-bit: sketches * row_bytes may exceed 2^32)
    }
    __device__ __forceinline__ void apply(State &st, uint32_t j, uint64_t h) const
    {
        if (!st.row) return;
        cms_bank_bin_add(st.row + (cms_bank_col<POW2>(md, h) + (uint64_t)j * md.m), st.w, st.plain, sat);
    }
    __device__ __forceinline__ void end(State &, uint64_t) const {}
};

// the two lookups: CmsCheck / CmsCheckMeanMin (psk_device.hpp) pointed at row ids[i]; ids >= sketches answer 0
template <bool POW2>
struct CmsBankCheck {
    const int32_t *tab;
    uint64_t row_ints, sketches;
    const uint32_t *ids;
    Mod md;
    uint32_t k;
    int32_t *out;
    bool mean;
    using Row = CmsCheck<POW2>;
    struct State { const int32_t *row; typename Row::State st; };
    __device__ __forceinline__ Row on(const int32_t *row) const { return Row{row, md, k, out, mean}; }
    __device__ __forceinline__ void prepare() {}
    __device__ __forceinline__ State begin(uint64_t i) const
    {
        const uint64_t s = ids[i];
        return State{s < sketches ? tab + s * row_ints : nullptr, on(nullptr).begin(i)};
    }
    __device__ __forceinline__ void apply(State &st, uint32_t j, uint64_t h) const
    {
        if (st.row) on(st.row).apply(st.st, j, h);
    }
    __device__ __forceinline__ void end(State &st, uint64_t i) const
    {
        if (st.row) on(st.row).end(st.st, i);
        else out[i] = 0;
    }
};

template <bool POW2>
struct CmsBankCheckMeanMin {
    const int32_t *tab;
    uint64_t row_ints, sketches;
    const uint32_t *ids;
    Mod md;
    uint32_t k;
    const int64_t *els;  // elements_added per sketch, device
    int64_t *out;
    using Row = CmsCheckMeanMin<POW2>;
    struct State { const int32_t *row; int64_t els; typename Row::State st; };
    __device__ __forceinline__ Row on(const State &st) const { return Row{st.row, md, k, st.els, out}; }
    __device__ __forceinline__ void prepare() {}
    __device__ __forceinline__ State begin(uint64_t i) const
    {
        const uint64_t s = ids[i];
        State st;
        st.row = s < sketches ? tab + s * row_ints : nullptr;
        st.els = st.row ? els[s] : 0;
        return st;
    }
    __device__ __forceinline__ void apply(State &st, uint32_t j, uint64_t h) const
    {
        if (st.row) on(st).apply(st.st, j, h);
    }
    __device__ __forceinline__ void end(State &st, uint64_t i) const
    {
        if (st.row) on(st).end(st.st, i);
        else out[i] = 0;
    }
};

// Workgroup (x, y) walks sketches x, x + gridDim.x, ... and takes the y-th of gridDim.y contiguous parts of each sketch's segment; an empty part
// costs nothing.  Everything that decides a barrier (the sketch, the part's bounds, the route) is uniform over the workgroup.  A part takes the image
// when the row fits it, the route asks for it, and no 32-bit LDS counter can wrap inside the part: unit weights (a part holds fewer than 2^32 keys,
// and the `depth` probes of a key fall into `depth` different counters), or a sketch whose bound is at or below INT32_MAX.  Any other part adds
// straight to the row, clamped.  Parts of one sketch -- in this launch or in another -- meet in the row through atomics only, and a zero counter of
// the image (the row's pad ints among them) is never written.
template <class Src, bool POW2>
__global__ __launch_bounds__(kBlock) void k_cms_bank_build(Src src, int32_t *tab, uint64_t sketches, uint32_t row_ints, Mod md, uint32_t k, uint64_t n,
                                                           const uint64_t *seg, const uint32_t *perm, const int32_t *weights, const int64_t *bound,
                                                           unsigned long long *sat, int route)
{
    extern __shared__ uint4 cms_img4[];  // row_ints / 4 (route 2, or a row over the cap: none)
    uint32_t *img = reinterpret_cast<uint32_t *>(cms_img4);
    const uint32_t split = gridDim.y, part = blockIdx.y, quads = row_ints >> 2;
    const bool fits = row_ints <= kCmsBankLdsInts;
    for (uint64_t s = blockIdx.x; s < sketches; s += gridDim.x) {
        uint64_t s0 = seg[s], s1 = seg[s + 1];
        if (s1 > n) s1 = n;  // (the contract says seg[sketches] <= n: no key is read beyond the batch whatever seg holds)
        if (s1 <= s0) continue;
        const uint64_t per = (s1 - s0 + split - 1) / split;
        const uint64_t a = s0 + per * part;
        if (a >= s1) continue;
        const uint64_t b = a + per < s1 ? a + per : s1;
        int32_t *row = tab + s * (uint64_t)row_ints;
        const bool plain = cms_bank_plain(bound, s);
        const bool image = fits && (!weights || plain) && (route == 1 || (route == 0 && (b - a) * k * kCmsBankRouteR >= row_ints));
        if (image) {
            for (uint32_t q = threadIdx.x; q < quads; q += kBlock) cms_img4[q] = make_uint4(0u, 0u, 0u, 0u);
            __syncthreads();
            for (uint64_t j = a + threadIdx.x; j < b; j += kBlock) {
                const uint64_t i = perm ? perm[j] : j;
                if (i >= n) continue;
                const int32_t w = weights ? weights[i] : 1;
                if (w <= 0) continue;
                const typename Src::Key key = src.load(i);
                for_each_hash(src, key, i, k, [&](uint32_t d, uint64_t h) {
                    atomicAdd(img + (cms_bank_col<POW2>(md, h) + d * (uint32_t)md.m), (uint32_t)w);  // ds_add_u32, no return value
                });
            }
            __syncthreads();
            for (uint32_t q = threadIdx.x; q < quads; q += kBlock) {
                const uint4 v = cms_img4[q];
                int32_t *p = row + 4u * q;
                if (v.x) cms_bank_bin_add(p, v.x, plain, sat);
                if (v.y) cms_bank_bin_add(p + 1, v.y, plain, sat);
                if (v.z) cms_bank_bin_add(p + 2, v.z, plain, sat);
                if (v.w) cms_bank_bin_add(p + 3, v.w, plain, sat);
            }
            __syncthreads();  // the next sketch's clear must not overtake this sweep
        } else {
            for (uint64_t j = a + threadIdx.x; j < b; j += kBlock) {
                const uint64_t i = perm ? perm[j] : j;
                if (i >= n) continue;
                const int32_t w = weights ? weights[i] : 1;
                if (w <= 0) continue;
                const typename Src::Key key = src.load(i);
                for_each_hash(src, key, i, k, [&](uint32_t d, uint64_t h) {
                    cms_bank_bin_add(row + (cms_bank_col<POW2>(md, h) + (uint64_t)d * md.m), (uint32_t)w, plain, sat);
                });
            }
        }
    }
}

// countminsketch.py:382-391 for one bin: an accumulator on either rail stays frozen, else clamp(acc + b), computed in int64
__device__ __forceinline__ int32_t cms_join_bin(int32_t acc, int32_t b)
{
    if (acc == INT32_MIN || acc == INT32_MAX) return acc;
    const int64_t v = (int64_t)acc + b;
    return v > INT32_MAX ? INT32_MAX : (v < INT32_MIN ? INT32_MIN : (int32_t)v);
}

// countminsketch.py:394-399
__device__ __forceinline__ int64_t cms_join_els(int64_t acc, int64_t b)
{
    if (b > 0 && acc > INT64_MAX - b) return INT64_MAX;
    if (b < 0 && acc < INT64_MIN - b) return INT64_MIN;
    return acc + b;
}

// k_cms_bank_reduce: a workgroup per (group, piece of kBlock 16-byte pieces of the row), linearised on x and walked with a stride.  A thread folds
// its four bins of the group's member rows in member order (the fold is not associative at the rails) and STORES the result; the thread of a
// group's first piece folds elements_added.  An empty group stores zeros; a member >= sketches counts as an empty sketch.
__global__ __launch_bounds__(kBlock) void k_cms_bank_reduce(const int4 *src, const int64_t *els, uint64_t sketches, uint32_t quads, const uint64_t *seg,
                                                            const uint32_t *members, uint64_t groups, int4 *dst, int64_t *els_out, uint32_t pieces, uint64_t work)
{
    for (uint64_t t = blockIdx.x; t < work; t += gridDim.x) {
        const uint64_t g = t / pieces;
        const uint32_t piece = (uint32_t)(t % pieces), q = piece * kBlock + threadIdx.x;
        const uint64_t s0 = seg[g], s1 = seg[g + 1];
        if (q < quads) {
            int4 acc = make_int4(0, 0, 0, 0);
            for (uint64_t j = s0; j < s1; ++j) {
                const uint64_t f = members[j];
                if (f >= sketches) continue;  // (an empty sketch: acc + 0)
                const int4 v = src[f * quads + q];  // (64-bit: sketches * row_bytes may exceed 2^32)
                acc.x = cms_join_bin(acc.x, v.x), acc.y = cms_join_bin(acc.y, v.y), acc.z = cms_join_bin(acc.z, v.z), acc.w = cms_join_bin(acc.w, v.w);
            }
            dst[g * quads + q] = acc;
        }
        if (els_out && piece == 0 && threadIdx.x == 0) {
            int64_t e = 0;
            for (uint64_t j = s0; j < s1; ++j) {
                const uint64_t f = members[j];
                if (f < sketches) e = cms_join_els(e, els ? els[f] : 0);
            }
            els_out[g] = e;
        }
    }
}

// where cms_sat_add counts a clamped add when the caller keeps no counter of its own
int cms_bank_sat_sink(unsigned long long **out)
{
    static thread_local DevBuf sink;
    PSK_TRY(ensure(sink, sizeof(unsigned long long)));
    *out = (unsigned long long *)sink.p;
    return PSK_OK;
}

int cms_bank_check_args(const void *table_dev, uint64_t sketches, uint64_t width, uint32_t depth, int layout, uint64_t n, uint32_t key_len)
{
    if (!table_dev) return fail(PSK_EINVAL, "NULL table pointer");
    if ((uintptr_t)table_dev & 15) return fail(PSK_EINVAL, "a bank table must be 16-byte aligned");
    if (sketches == 0 || sketches > (1ULL << 32)) return fail(PSK_EINVAL, "a bank holds 1 .. 2^32 sketches; %llu were asked for", (unsigned long long)sketches);
    if (width == 0 || width > kCmsBankMaxWidth) return fail(PSK_EINVAL, "a bank's sketches are 1 .. 2^31 wide; %llu was asked for", (unsigned long long)width);
    if (depth == 0 || depth > (uint32_t)kMaxDepthMeanMin)
        return fail(PSK_EINVAL, "a bank's sketches are 1 .. %d deep; %u was asked for", kMaxDepthMeanMin, depth);
    if (n >> 32) return fail(PSK_EINVAL, "a bank call takes fewer than 2^32 keys; %llu were passed", (unsigned long long)n);
    if (layout == PSK_KEYS_HASHES && key_len < depth) return fail(PSK_EINVAL, "pre-hashed batch carries %u hashes per key, the bank needs %u", key_len, depth);
    return PSK_OK;
}

}  // namespace

extern "C" int psk_cms_bank_add(void *table_dev, uint64_t sketches, uint64_t width, uint32_t depth, int layout, const void *data, const uint64_t *offsets,
                                uint64_t n, uint32_t key_len, int where, const uint32_t *ids, const int32_t *weights, const int64_t *bound_dev,
                                uint64_t *saturated_dev, int device, void *stream)
{
    PSK_TRY(cms_bank_check_args(table_dev, sketches, width, depth, layout, n, key_len));
    if (n && !ids) return fail(PSK_EINVAL, "ids is NULL");
    if (where == PSK_HOST && weights)
        for (uint64_t i = 0; i < n; ++i)
            if (weights[i] < 0) return fail(PSK_EINVAL, "bank add: weight %d of key %llu is negative", weights[i], (unsigned long long)i);
    bool pow2;
    const Mod md = make_mod(width, &pow2);
    const uint64_t row_ints = psk_cms_table_bytes(width, depth) / 4;
    return bank_keyed_call(layout, data, offsets, n, key_len, where, ids, weights, nullptr, 0, device, stream,
                           [&](auto src, const uint32_t *ids_dev, const int32_t *w_dev, void *, hipStream_t st) {
                               unsigned long long *sat = (unsigned long long *)saturated_dev;
                               if (!sat) PSK_TRY(cms_bank_sat_sink(&sat));
                               return with_pow2(pow2, [&](auto P) {
                                   return launch_apply(src, CmsBankAdd<P.value>{(int32_t *)table_dev, row_ints, sketches, ids_dev, md, depth, w_dev, bound_dev, sat}, n, st);
                               });
                           });
}

extern "C" int psk_cms_bank_check(const void *table_dev, uint64_t sketches, uint64_t width, uint32_t depth, int layout, const void *data,
                                  const uint64_t *offsets, uint64_t n, uint32_t key_len, int where, const uint32_t *ids, int query, int32_t *out, int device,
                                  void *stream)
{
    PSK_TRY(cms_bank_check_args(table_dev, sketches, width, depth, layout, n, key_len));
    if (query != PSK_Q_MIN && query != PSK_Q_MEAN) return fail(PSK_EINVAL, "psk_cms_bank_check handles MIN and MEAN queries");
    if (n && (!ids || !out)) return fail(PSK_EINVAL, "ids or out is NULL");
    bool pow2;
    const Mod md = make_mod(width, &pow2);
    const uint64_t row_ints = psk_cms_table_bytes(width, depth) / 4;
    return bank_keyed_call(layout, data, offsets, n, key_len, where, ids, out, n * 4, device, stream, [&](auto src, const uint32_t *ids_dev, void *out_dev, hipStream_t st) {
        return with_pow2(pow2, [&](auto P) {
            return launch_apply(src, CmsBankCheck<P.value>{(const int32_t *)table_dev, row_ints, sketches, ids_dev, md, depth, (int32_t *)out_dev, query == PSK_Q_MEAN}, n, st);
        });
    });
}

extern "C" int psk_cms_bank_check_meanmin(const void *table_dev, uint64_t sketches, uint64_t width, uint32_t depth, int layout, const void *data,
                                          const uint64_t *offsets, uint64_t n, uint32_t key_len, int where, const uint32_t *ids, const int64_t *els_dev,
                                          int64_t *out, int device, void *stream)
{
    PSK_TRY(cms_bank_check_args(table_dev, sketches, width, depth, layout, n, key_len));
    if (width < 2) return fail(PSK_EINVAL, "mean-min query needs width >= 2 (divides by width-1)");
    if (!els_dev) return fail(PSK_EINVAL, "els_dev is NULL");
    if (n && (!ids || !out)) return fail(PSK_EINVAL, "ids or out is NULL");
    bool pow2;
    const Mod md = make_mod(width, &pow2);
    const uint64_t row_ints = psk_cms_table_bytes(width, depth) / 4;
    return bank_keyed_call(layout, data, offsets, n, key_len, where, ids, out, n * 8, device, stream, [&](auto src, const uint32_t *ids_dev, void *out_dev, hipStream_t st) {
        return with_pow2(pow2, [&](auto P) {
            return launch_apply(src, CmsBankCheckMeanMin<P.value>{(const int32_t *)table_dev, row_ints, sketches, ids_dev, md, depth, els_dev, (int64_t *)out_dev}, n, st);
        });
    });
}

extern "C" int psk_cms_bank_build(void *table_dev, uint64_t sketches, uint64_t width, uint32_t depth, int layout, const void *data, const uint64_t *offsets,
                                  uint64_t n, uint32_t key_len, const uint64_t *seg_dev, const uint32_t *perm_dev, const int32_t *weights_dev,
                                  const int64_t *bound_dev, uint64_t *saturated_dev, uint32_t split, int route, int device, void *stream)
{
    PSK_TRY(cms_bank_check_args(table_dev, sketches, width, depth, layout, n, key_len));
    if (!seg_dev) return fail(PSK_EINVAL, "seg_dev is NULL");
    if (split < 1 || split > 65535) return fail(PSK_EINVAL, "split must be 1 .. 65535 workgroups per sketch; %u was passed", split);
    if (route < 0 || route > 2) return fail(PSK_EINVAL, "route must be 0 (auto), 1 (LDS image) or 2 (global atomics)");
    const uint64_t row_ints = psk_cms_table_bytes(width, depth) / 4;
    if (row_ints >> 32)  // (the build kernel indexes a row with 32 bits; psk_cms_bank_add carries 64)
        return fail(PSK_EINVAL, "psk_cms_bank_build takes rows of fewer than 2^32 ints; %llu x %u was asked for: use psk_cms_bank_add", (unsigned long long)width, depth);
    if (route == 1 && row_ints > kCmsBankLdsInts)
        return fail(PSK_EINVAL, "rows of %llu ints do not fit the LDS image (at most %u)", (unsigned long long)row_ints, kCmsBankLdsInts);
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    Batch b;
    ThreadStage &ts = thread_stage();
    PSK_TRY(stage_batch(ts.keys, ts.offs, layout, data, offsets, n, key_len, PSK_DEVICE, st, &b));
    if (n == 0) return PSK_OK;
    unsigned long long *sat = (unsigned long long *)saturated_dev;
    if (!sat) PSK_TRY(cms_bank_sat_sink(&sat));
    bool pow2;
    const Mod md = make_mod(width, &pow2);
    const size_t lds = route != 2 && row_ints <= kCmsBankLdsInts ? (size_t)row_ints * 4 : 0;
    const dim3 grid((unsigned)(sketches < kCmsBankGridCap ? sketches : kCmsBankGridCap), split);
    return with_source(b, [&](auto src) {
        return with_pow2(pow2, [&](auto P) {
            hipLaunchKernelGGL((k_cms_bank_build<decltype(src), P.value>), grid, dim3(kBlock), lds, st, src, (int32_t *)table_dev, sketches, (uint32_t)row_ints, md, depth, n,
                               seg_dev, perm_dev, weights_dev, bound_dev, sat, route);
            HIP_TRY(hipGetLastError());
            return (int)PSK_OK;
        });
    });
}

extern "C" int psk_cms_bank_reduce(const void *src_dev, const int64_t *els_dev, uint64_t sketches, uint64_t width, uint32_t depth, const uint64_t *seg_dev,
                                   const uint32_t *members_dev, uint64_t groups, void *dst_dev, int64_t *els_out_dev, int device, void *stream)
{
    PSK_TRY(cms_bank_check_args(src_dev, sketches, width, depth, PSK_KEYS_FIXED, 0, 0));
    if (groups >> 32) return fail(PSK_EINVAL, "a reduce call takes fewer than 2^32 groups; %llu were passed", (unsigned long long)groups);
    if (groups == 0) return PSK_OK;
    if (!dst_dev || ((uintptr_t)dst_dev & 15)) return fail(PSK_EINVAL, "dst_dev must be a 16-byte aligned device pointer");
    if (!seg_dev) return fail(PSK_EINVAL, "seg_dev is NULL");
    const uint64_t row_bytes = psk_cms_table_bytes(width, depth), quads = row_bytes / 16;
    if (quads >> 30)  // (the reduce kernel indexes a row's 16-byte pieces with 32 bits)
        return fail(PSK_EINVAL, "psk_cms_bank_reduce takes rows of fewer than 2^32 ints; %llu x %u was asked for", (unsigned long long)width, depth);
    const uintptr_t s0 = (uintptr_t)src_dev, s1 = s0 + sketches * row_bytes, d0 = (uintptr_t)dst_dev, d1 = d0 + groups * row_bytes;
    if (d0 < s1 && s0 < d1) return fail(PSK_EINVAL, "dst overlaps src: a fold is stored, never done in place");
    const uint64_t pieces = (quads + kBlock - 1) / kBlock, work = groups * pieces;
    PSK_USE_DEVICE(device);
    hipLaunchKernelGGL(k_cms_bank_reduce, dim3((unsigned)(work < kCmsBankGridCap ? work : kCmsBankGridCap)), dim3(kBlock), 0, (hipStream_t)stream, (const int4 *)src_dev,
                       els_dev, sketches, (uint32_t)quads, seg_dev, members_dev, groups, (int4 *)dst_dev, els_out_dev, (uint32_t)pieces, work);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}
