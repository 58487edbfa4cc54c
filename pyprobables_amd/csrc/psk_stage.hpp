// psk_stage.hpp -- the staging layer of the C ABI: what every entry point that takes KEYS needs around its launch.  A call validates and
// stages its batch (stage_batch), its optional per-key vector (stage_vec) and its results (stage_out), dispatches over the batch's concrete
// key source (with_source) and the table's modulus (with_pow2), launches, and ends in finish().  The templates live here; the rest is
// defined once, in psk_stage.hip.
#pragma once
#include "psk_host.hpp"

#include <utility>

// ---- completion mailbox of tiny PSK_HOST batches (mailbox_post, psk_device.hpp): the kernel stores the call's sequence number into a
// pinned word behind its results (which it wrote into a pinned page) and the host polls that word -- a value-returning single-key call
// ends when its answer is in host memory; the stream wait (a barrier packet, its signal, the runtime's bookkeeping: ~5 us of a ~15 us
// call) is what the reference's per-key callers would otherwise pay on every `key in blm`.  The poll gives up after host_poll_us
// microseconds (option; 0 = never poll) and falls back to the stream wait, which also reports a kernel that died.
struct Mailbox {
    volatile uint32_t *word = nullptr;  // nullptr: not armed -- finish() waits for the stream
    uint32_t seq = 0;
    uint32_t *timeouts = nullptr;       // the handle's count of polls in a row that gave up (mailbox_arm)
    uint32_t *dev() const { return const_cast<uint32_t *>(word); }
};
static inline void mailbox_disarm(Mailbox *mb) { mb->word = nullptr; }
PSK_HIDDEN int mailbox_arm(psk_sketch *s, int where, uint64_t n, bool out_pinned, Mailbox *mb);

// ---------------------------------------------------------- key batches
// Validate, and for PSK_HOST stage the batch into the handle's device scratch.
PSK_HIDDEN int stage_batch(DevBuf &kbuf, DevBuf &obuf, int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len, int where,
                           hipStream_t st, Batch *b);

// Dispatch a functor over the concrete key-source type of a batch.
template <class F>
static int with_source(const Batch &b, F &&f)
{
    switch (b.layout) {
        case PSK_KEYS_FIXED:
            if (b.key_len == 16 && ((uintptr_t)b.data & 15) == 0) return f(KeysFixed16{(const uint4 *)b.data});
            if (b.key_len == 8 && ((uintptr_t)b.data & 7) == 0) return f(KeysFixed8{(const uint2 *)b.data});
            if (b.key_len == 32 && ((uintptr_t)b.data & 15) == 0) return f(KeysFixed32{(const uint4 *)b.data});
            if (b.key_len % 4 == 0 && ((uintptr_t)b.data & 3) == 0) return f(KeysFixed<true>{(const uint8_t *)b.data, b.key_len, b.n});
            return f(KeysFixed<false>{(const uint8_t *)b.data, b.key_len, b.n});
        case PSK_KEYS_VARLEN8: return f(KeysVarlen<uint8_t>{(const uint8_t *)b.data, b.offs, b.n});
        case PSK_KEYS_VARLEN32: return f(KeysVarlen<uint32_t>{(const uint32_t *)b.data, b.offs, b.n});
        case PSK_KEYS_HASHES: return f(KeysHashes{(const uint64_t *)b.data, b.key_len});
    }
    return fail(PSK_EINVAL, "unknown key layout");
}

// ONE fixed-layout key of a PSK_HOST call that ends on the mailbox travels in the kernel arguments (KeysInline64, psk_device.hpp), not
// through the pinned page stage_batch filled; `data` is the caller's pointer.  -> the source to launch with, or nullptr (the batch's own)
PSK_HIDDEN const KeysInline64 *inline_key(int layout, const void *data, uint64_t n, uint32_t key_len, const Mailbox &mb, KeysInline64 *k);
template <class F>
static int with_source_one(const Batch &b, const KeysInline64 *one, F &&f)
{
    if (one) return f(*one);
    return with_source(b, f);
}

template <class Src, class Op>
static int launch_apply(const Src &src, const Op &op, uint64_t n, hipStream_t st, Mailbox *mb = nullptr)
{
    if (n == 0) return PSK_OK;
    const uint32_t grid = grid_for_keys(n);
    if (mb && grid != 1) mailbox_disarm(mb);  // (the kernel's one workgroup posts it: see mailbox_post, psk_device.hpp)
    // (thread t of workgroup 0 takes keys t, t + kBlock ...: a batch of up to 64 keys needs one wave)
    hipLaunchKernelGGL((k_apply<Src, Op>), dim3(grid), dim3(n <= 64 ? 64 : kBlock), 0, st, src, op, n, mb ? mb->dev() : nullptr, mb ? mb->seq : 0u);
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

// The modulus of a table of m cells: mask for a power of two (*pow2), else the Barrett magic floor(2^64 / m).
static inline Mod make_mod(uint64_t m, bool *pow2)
{
    Mod md;
    md.m = m;
    *pow2 = (m & (m - 1)) == 0;
    md.mask = m - 1;
    md.magic = *pow2 ? 0 : (uint64_t)((((unsigned __int128)1) << 64) / m);
    return md;
}

// Dispatch a functor over the table's modulus as a compile-time constant: f(std::true_type{}) for a power-of-two table (mask), else
// f(std::false_type{}) (Barrett).  Inside `[&](auto P) { ... }` the constant is P.value.
template <class F>
static inline int with_pow2(bool pow2, F &&f)
{
    if (pow2) return f(std::true_type{});
    return f(std::false_type{});
}
template <class F>
static inline int with_pow2(const psk_sketch *s, F &&f)
{
    return with_pow2(s->pow2, std::forward<F>(f));
}

PSK_HIDDEN int check_hashes_width(const psk_sketch *s, int layout, uint32_t key_len);

// small-transfer fast path: lazily allocated pinned (host-coherent, device-visible) page per scratch buffer
PSK_HIDDEN int pinned(DevBuf &b, void **out);

// stage an optional per-key vector (weights); returns device pointer or nullptr
template <class T>
static int stage_vec(DevBuf &buf, const T *v, uint64_t n, int where, hipStream_t st, const T **dev)
{
    *dev = v;
    if (!v || where == PSK_DEVICE || n == 0) return PSK_OK;
    if (n * sizeof(T) <= kPinBytes) {
        void *pp;
        PSK_TRY(pinned(buf, &pp));
        memcpy(pp, v, n * sizeof(T));
        *dev = (const T *)pp;
        return PSK_OK;
    }
    PSK_TRY(ensure(buf, n * sizeof(T)));
    HIP_TRY(hipMemcpyAsync(buf.p, v, n * sizeof(T), hipMemcpyHostToDevice, st));
    *dev = (const T *)buf.p;
    return PSK_OK;
}

// output buffer: device pointer to write into (+ copy-back for PSK_HOST)
struct OutBuf {
    void *dev = nullptr;
    void *host = nullptr;
    uint64_t bytes = 0;
    bool is_pinned = false;  // dev is pinned host memory: no device-to-host copy, just a sync and a memcpy
};
PSK_HIDDEN int stage_out(DevBuf &buf, void *out, uint64_t bytes, int where, OutBuf *o);
// end of a call: for PSK_HOST the results go to the caller and the call waits (mailbox, else stream); o = nullptr: no results
PSK_HIDDEN int finish(int where, const OutBuf *o, hipStream_t st, const Mailbox *mb = nullptr);

// The tail of a direct (small-batch) call, when the partitioned path did not take the staged batch `b`: arm the mailbox (out_pinned: what the
// kernel writes for the host lies in pinned memory -- true for updates, which return nothing, OutBuf::is_pinned for lookups), send ONE fixed-layout
// key inside the kernel arguments (`data` is the caller's pointer, not the staged copy), launch k_apply with the op make_op(P) builds for the
// table's modulus, and end the call (finish: mailbox or stream wait, results to the host; o = nullptr: no results).
template <class MakeOp>
static int direct_apply(psk_sketch *s, const Batch &b, const void *data, int where, bool out_pinned, const OutBuf *o, hipStream_t st, MakeOp &&make_op)
{
    Mailbox mb;  // (an update returns nothing, but a PSK_HOST call ends when the kernel has read the caller's keys: the same mailbox says so)
    PSK_TRY(mailbox_arm(s, where, b.n, out_pinned, &mb));
    KeysInline64 ik;
    PSK_TRY(with_source_one(b, inline_key(b.layout, data, b.n, b.key_len, mb, &ik), [&](auto src) {
        return with_pow2(s, [&](auto P) { return launch_apply(src, make_op(P), b.n, st, &mb); });
    }));
    return finish(where, o, st, &mb);
}

// ---- the keyed calls WITHOUT a handle (hashing, quotient / cuckoo lookups): the calling thread's own staging buffers
struct ThreadStage {
    DevBuf keys, offs, out;
};
PSK_HIDDEN ThreadStage &thread_stage();

// One such call, its own arguments checked: on `device`, stage the batch and out[out_bytes], run launch(batch, out_dev, stream) -> PSK_* if
// there is anything to compute (out_bytes != 0), and end the call.
template <class Launch>
static int keyed_call_batch(int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len, int where, void *out, uint64_t out_bytes, int device,
                           void *stream, Launch &&launch)
{
    PSK_USE_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    ThreadStage &ts = thread_stage();
    Batch b;
    PSK_TRY(stage_batch(ts.keys, ts.offs, layout, data, offsets, n, key_len, where, st, &b));
    OutBuf o;
    PSK_TRY(stage_out(ts.out, out, out_bytes, where, &o));
    if (out_bytes) PSK_TRY(launch(b, o.dev, st));
    return finish(where, &o, st);
}

// ... whose kernel is templated over the key source: launch(src, out_dev, stream) only launches
template <class Launch>
static int keyed_call(int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len, int where, void *out, uint64_t out_bytes, int device,
                     void *stream, Launch &&launch)
{
    return keyed_call_batch(layout, data, offsets, n, key_len, where, out, out_bytes, device, stream, [&](const Batch &b, void *out_dev, hipStream_t st) {
        return with_source(b, [&](auto src) {
            launch(src, out_dev, st);
            HIP_TRY(hipGetLastError());
            return (int)PSK_OK;
        });
    });
}

// ------------------------------------------------------ counters / weights (CountingBloomFilter and CountMinSketch)
// grow_bound = false: the batch only lowers counters (CBF removes) -- the wrap-free bound on |counter| stays as it is
template <class W>
static int account_weights(psk_sketch *s, const W *w_dev, uint64_t n, int which, long long bound_mult, hipStream_t st, bool grow_bound = true)
{
    if (n == 0) return PSK_OK;
    if (w_dev) {
        HIP_TRY(hipMemsetAsync(s->ctr + 6, 0, sizeof(long long), st));  // per-batch sum|w| (partitioned path wrap check)
        hipLaunchKernelGGL((k_weight_sum<W>), dim3(grid_for_keys(n) > 256 ? 256 : grid_for_keys(n)), dim3(kBlock), 0, st, w_dev, n,
                           s->ctr, which, bound_mult, (int)grow_bound);
    } else {
        hipLaunchKernelGGL(k_ctr_add, dim3(1), dim3(1), 0, st, s->ctr, which, (long long)n, grow_bound ? (long long)n * bound_mult : 0LL);
    }
    HIP_TRY(hipGetLastError());
    return PSK_OK;
}

// Accounting of a weighted batch, fused into pass 1 when the partitioned path takes it (PayWeight::tally): post the request,
// try the partitioned launcher, settle what it did not take over with the stand-alone pass over the weights.
template <class W>
static int post_acct(psk_sketch *s, const W *w_dev, uint64_t n, int which, long long bound_mult, hipStream_t st, bool grow_bound, bool weights_signed)
{
    s->acct.pending = false;
    if (!w_dev || n == 0) return account_weights(s, w_dev, n, which, bound_mult, st, grow_bound);  // unit weights: a one-thread kernel
    s->acct.pending = true;
    s->acct.which = which;
    s->acct.bound_mult = bound_mult;
    s->acct.grow_bound = grow_bound;
    s->acct.weights_signed = weights_signed;
    s->acct.weights01 = false;
    return PSK_OK;
}

template <class W>
static int settle_acct(psk_sketch *s, const W *w_dev, uint64_t n, hipStream_t st)
{
    if (!s->acct.pending) return PSK_OK;
    s->acct.pending = false;
    return account_weights(s, w_dev, n, s->acct.which, s->acct.bound_mult, st, s->acct.grow_bound);
}
