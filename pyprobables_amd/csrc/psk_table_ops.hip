// psk_table_ops.hip -- calls of the C ABI on bare device tables (include/psk.h): table algebra, slice reduction, the synthetic streams of
// the benchmarks.
#include "psk_host.hpp"

// ------------------------------------------------------------ table algebra
static int check_vec(const void *a, const void *b, uint64_t nwords32)
{
    if (!a || !b) return fail(PSK_EINVAL, "table pointer is NULL");
    if (nwords32 % 4 || ((uintptr_t)a & 15) || ((uintptr_t)b & 15))
        return fail(PSK_EINVAL, "tables must be 16-byte aligned and a multiple of 16 bytes long");
    return PSK_OK;
}

extern "C" int psk_table_or(void *dst, const void *src, uint64_t nwords32, int device, void *stream)
{
    PSK_TRY(check_vec(dst, src, nwords32));
    PSK_USE_DEVICE(device);
    if (!nwords32) return PSK_OK;
    hipLaunchKernelGGL((k_table_binop<OpOr>), dim3(grid_for_keys(nwords32 / 4)), dim3(kBlock), 0, (hipStream_t)stream, (uint4 *)dst,
                       (const uint4 *)src, nwords32 / 4, OpOr{});
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

extern "C" int psk_table_and(void *dst, const void *src, uint64_t nwords32, int device, void *stream)
{
    PSK_TRY(check_vec(dst, src, nwords32));
    PSK_USE_DEVICE(device);
    if (!nwords32) return PSK_OK;
    hipLaunchKernelGGL((k_table_binop<OpAnd>), dim3(grid_for_keys(nwords32 / 4)), dim3(kBlock), 0, (hipStream_t)stream, (uint4 *)dst,
                       (const uint4 *)src, nwords32 / 4, OpAnd{});
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

// One launch that tallies into `words` 64-bit device words: allocated and zeroed, launch(tally_dev) if there is work (`n`), copied to
// out_host[words], the stream waited for, freed.  `what` names the caller in the error text.
template <class Launch>
static int with_tally(int words, uint64_t n, uint64_t *out_host, hipStream_t st, const char *what, Launch &&launch)
{
    unsigned long long *d = nullptr;
    HIP_TRY(hipMalloc((void **)&d, 8 * words));
    hipError_t e = hipMemsetAsync(d, 0, 8 * words, st);
    if (e == hipSuccess && n) {
        launch(d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out_host, d, 8 * words, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    hipFree(d);
    if (e != hipSuccess) return fail(PSK_EHIP, "%s failed: %s", what, hipGetErrorString(e));
    return PSK_OK;
}

static int table_count(const void *tab, uint64_t nwords32, int mode, uint64_t *out_host, int device, void *stream)
{
    PSK_TRY(check_vec(tab, tab, nwords32));
    if (!out_host) return fail(PSK_EINVAL, "out is NULL");
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    return with_tally(1, nwords32, out_host, st, "table count", [&](unsigned long long *d) {
        const int g = grid_for_keys(nwords32 / 4) > 1024 ? 1024 : grid_for_keys(nwords32 / 4);
        hipLaunchKernelGGL(k_table_count, dim3(g), dim3(kBlock), 0, st, (const uint4 *)tab, nwords32 / 4, mode, d);
    });
}

extern "C" int psk_table_popcount(const void *tab, uint64_t nwords32, uint64_t *out_host, int device, void *stream)
{
    return table_count(tab, nwords32, 0, out_host, device, stream);
}

extern "C" int psk_table_nonzero_u32(const void *tab, uint64_t nwords32, uint64_t *out_host, int device, void *stream)
{
    return table_count(tab, nwords32, 1, out_host, device, stream);
}

extern "C" int psk_table_add_sat_i32(void *dst, const void *src, uint64_t n, int device, void *stream)
{
    if (!dst || !src) return fail(PSK_EINVAL, "table pointer is NULL");
    PSK_USE_DEVICE(device);
    if (!n) return PSK_OK;
    hipLaunchKernelGGL(k_add_sat_i32, dim3(grid_for_keys(n)), dim3(kBlock), 0, (hipStream_t)stream, (int32_t *)dst, (const int32_t *)src, n);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

extern "C" int psk_table_add_u32(void *dst, const void *src, uint64_t n, uint64_t *overflowed_host, int device, void *stream)
{
    if (!dst || !src) return fail(PSK_EINVAL, "table pointer is NULL");
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    uint64_t ov = 0;
    PSK_TRY(with_tally(1, n, &ov, st, "table add", [&](unsigned long long *d) {
        hipLaunchKernelGGL(k_add_u32, dim3(grid_for_keys(n)), dim3(kBlock), 0, st, (uint32_t *)dst, (const uint32_t *)src, n, d);
    }));
    if (overflowed_host) *overflowed_host = ov;
    return PSK_OK;
}

extern "C" int psk_cbf_intersect(void *dst, const void *a, const void *b, uint64_t n, uint64_t *overflowed_host, int device, void *stream)
{
    if (!dst || !a || !b) return fail(PSK_EINVAL, "table pointer is NULL");
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    uint64_t ov = 0;
    PSK_TRY(with_tally(1, n, &ov, st, "cbf intersect", [&](unsigned long long *d) {
        const int g = grid_for_keys(n) > 2048 ? 2048 : grid_for_keys(n);
        hipLaunchKernelGGL(k_cbf_intersect, dim3(g), dim3(kBlock), 0, st, (uint32_t *)dst, (const uint32_t *)a, (const uint32_t *)b, n, d);
    }));
    if (overflowed_host) *overflowed_host = ov;
    return PSK_OK;
}

extern "C" int psk_cbf_jaccard_counts(const void *a, const void *b, uint64_t n, uint64_t out_host[2], int device, void *stream)
{
    if (!a || !b || !out_host) return fail(PSK_EINVAL, "NULL argument");
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    return with_tally(2, n, out_host, st, "cbf jaccard", [&](unsigned long long *d) {
        const int g = grid_for_keys(n) > 1024 ? 1024 : grid_for_keys(n);
        hipLaunchKernelGGL(k_cbf_jaccard, dim3(g), dim3(kBlock), 0, st, (const uint32_t *)a, (const uint32_t *)b, n, d);
    });
}

extern "C" int psk_or_reduce_slices(void *dst, const void *src, uint32_t nslices, uint64_t slice_words32, int device, void *stream)
{
    PSK_TRY(check_vec(dst, src, slice_words32));
    if (nslices == 0) return fail(PSK_EINVAL, "nslices must be > 0");
    PSK_USE_DEVICE(device);
    if (!slice_words32) return PSK_OK;
    hipLaunchKernelGGL(k_or_reduce, dim3(grid_for_keys(slice_words32 / 4)), dim3(kBlock), 0, (hipStream_t)stream, (uint4 *)dst,
                       (const uint4 *)src, nslices, slice_words32 / 4);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

// ------------------------------------------------------- synthetic streams
extern "C" int psk_gen_keys16(void *dst_dev, uint64_t start, uint64_t n, uint64_t seed, int device, void *stream)
{
    if (n && (!dst_dev || ((uintptr_t)dst_dev & 15))) return fail(PSK_EINVAL, "dst must be a 16-byte aligned device pointer");
    PSK_USE_DEVICE(device);
    if (!n) return PSK_OK;
    hipLaunchKernelGGL(k_gen_keys16, dim3(grid_for_keys(n)), dim3(kBlock), 0, (hipStream_t)stream, (ulonglong2 *)dst_dev, start, n, seed);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

extern "C" int psk_gen_weights(void *dst_dev, uint64_t start, uint64_t n, uint64_t seed, int device, void *stream)
{
    if (n && !dst_dev) return fail(PSK_EINVAL, "dst is NULL");
    PSK_USE_DEVICE(device);
    if (!n) return PSK_OK;
    hipLaunchKernelGGL(k_gen_weights, dim3(grid_for_keys(n)), dim3(kBlock), 0, (hipStream_t)stream, (int32_t *)dst_dev, start, n, seed);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

extern "C" int psk_gups(void *table_dev, uint64_t nwords32, uint64_t n, int op, uint64_t seed, uint64_t *sink_dev, int device,
                        void *stream)
{
    if (!table_dev || !nwords32) return fail(PSK_EINVAL, "bad table");
    if (op == 2 && !sink_dev) return fail(PSK_EINVAL, "load mode needs a sink");
    PSK_USE_DEVICE(device);
    if (!n) return PSK_OK;
    hipStream_t st = (hipStream_t)stream;
    dim3 g(grid_for_keys(n)), blk(kBlock);
    if (op == 0) hipLaunchKernelGGL((k_gups<0>), g, blk, 0, st, (uint32_t *)table_dev, nwords32, n, seed, (unsigned long long *)sink_dev);
    else if (op == 1) hipLaunchKernelGGL((k_gups<1>), g, blk, 0, st, (uint32_t *)table_dev, nwords32, n, seed, (unsigned long long *)sink_dev);
    else if (op == 2) hipLaunchKernelGGL((k_gups<2>), g, blk, 0, st, (uint32_t *)table_dev, nwords32, n, seed, (unsigned long long *)sink_dev);
    else return fail(PSK_EINVAL, "bad gups op %d", op);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}
