// psk_bank_stage.hpp -- the staging of a keyed bank call (BloomFilterBank: psk_bank.hip; CountMinSketchBank: psk_cms_bank.hip): keys with a
// row id each, and for the counting bank a weight each, on top of the handle-less staging of psk_stage.hpp.
#pragma once
#include "psk_stage.hpp"

// the staged per-key vectors of a PSK_HOST call: the buffers a bank call needs beside ThreadStage's three
struct BankStage {
    DevBuf ids, weights;
};
inline BankStage &bank_stage()
{
    static thread_local BankStage bs;
    return bs;
}

// One keyed bank call: on `device`, stage the batch, its ids, its weights (NULL: none) and out[out_bytes] (none: an update), run
// launch(src, ids_dev, weights_dev, out_dev, stream), end the call.
template <class Launch>
static int bank_keyed_call(int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len, int where, const uint32_t *ids,
                           const int32_t *weights, void *out, uint64_t out_bytes, int device, void *stream, Launch &&launch)
{
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    ThreadStage &ts = thread_stage();
    Batch b;
    PSK_TRY(stage_batch(ts.keys, ts.offs, layout, data, offsets, n, key_len, where, st, &b));
    const uint32_t *ids_dev = nullptr;
    PSK_TRY(stage_vec(bank_stage().ids, ids, n, where, st, &ids_dev));
    const int32_t *w_dev = nullptr;
    PSK_TRY(stage_vec(bank_stage().weights, weights, n, where, st, &w_dev));
    OutBuf o;
    PSK_TRY(stage_out(ts.out, out, out_bytes, where, &o));
    if (n) PSK_TRY(with_source(b, [&](auto src) { return launch(src, ids_dev, w_dev, o.dev, st); }));
    return finish(where, out_bytes ? &o : nullptr, st);
}

// ... without weights: launch(src, ids_dev, out_dev, stream)
template <class Launch>
static int bank_keyed_call(int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len, int where, const uint32_t *ids, void *out,
                           uint64_t out_bytes, int device, void *stream, Launch &&launch)
{
    return bank_keyed_call(layout, data, offsets, n, key_len, where, ids, (const int32_t *)nullptr, out, out_bytes, device, stream,
                           [&](auto src, const uint32_t *ids_dev, const int32_t *, void *out_dev, hipStream_t st) { return launch(src, ids_dev, out_dev, st); });
}
