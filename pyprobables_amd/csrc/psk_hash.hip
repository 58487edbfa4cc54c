// psk_hash.hip -- the hashing calls of the C ABI that need no sketch (include/psk.h): the FNV-1a chain and the digest chains.
#include "psk_stage.hpp"
#include "psk_digest.hpp"

extern "C" int psk_fnv1a_hash(int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len,
                              uint32_t depth, int where, uint64_t *out, int device, void *stream)
{
    if (layout == PSK_KEYS_HASHES) return fail(PSK_EINVAL, "psk_fnv1a_hash needs a key layout");
    if (n && depth && !out) return fail(PSK_EINVAL, "out is NULL");
    return keyed_call(layout, data, offsets, n, key_len, where, out, n * depth * 8, device, stream, [&](auto src, void *out_dev, hipStream_t st) {
        hipLaunchKernelGGL((k_hash<decltype(src)>), dim3(grid_for_keys(n)), dim3(kBlock), 0, st, src, (uint64_t *)out_dev, depth, n);
    });
}

// hashes.py:125-150 default_md5 / default_sha256 as digest chains (psk_digest.hpp); byte keys only
extern "C" int psk_digest_chain(int algo, int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len,
                                uint32_t depth, int where, uint64_t *out, int device, void *stream)
{
    if (algo != PSK_DIGEST_MD5 && algo != PSK_DIGEST_SHA256) return fail(PSK_EINVAL, "unknown digest %d", algo);
    if (layout != PSK_KEYS_FIXED && layout != PSK_KEYS_VARLEN8)
        return fail(PSK_EINVAL, "digest chains hash bytes: use PSK_KEYS_FIXED or PSK_KEYS_VARLEN8 (a str is UTF-8 encoded by the caller)");
    if (n && depth && !out) return fail(PSK_EINVAL, "out is NULL");
    // (the chain reads raw bytes and offsets: no dispatch over the key source)
    return keyed_call_batch(layout, data, offsets, n, key_len, where, out, n * depth * 8, device, stream, [&](const Batch &b, void *out_dev, hipStream_t st) {
        const uint64_t *offs = layout == PSK_KEYS_VARLEN8 ? b.offs : nullptr;
        const dim3 grid((unsigned)((n + 255) / 256 > 65535 ? 65535 : (n + 255) / 256));
        if (algo == PSK_DIGEST_MD5)
            hipLaunchKernelGGL((k_digest_chain<Md5>), grid, dim3(256), 0, st, (const uint8_t *)b.data, offs, key_len, n, depth, (uint64_t *)out_dev);
        else
            hipLaunchKernelGGL((k_digest_chain<Sha256>), grid, dim3(256), 0, st, (const uint8_t *)b.data, offs, key_len, n, depth, (uint64_t *)out_dev);
        HIP_TRY(hipGetLastError());
        return (int)PSK_OK;
    });
}
