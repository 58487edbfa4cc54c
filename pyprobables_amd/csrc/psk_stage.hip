// psk_stage.hip -- the staging layer's functions that are no templates (psk_stage.hpp): host code only, no kernel.
#include "psk_stage.hpp"

#include <chrono>

int mailbox_arm(psk_sketch *s, int where, uint64_t n, bool out_pinned, Mailbox *mb)
{
    mb->word = nullptr;
    if (where != PSK_HOST || n == 0 || n > kBlock || !out_pinned || g_host_poll_us <= 0) return PSK_OK;
    // Eight polls in a row that gave up -- a stream that always has long work queued in front of the call, or pinned memory the host does not
    // see device stores to while the kernel runs -- and the handle stops paying host_poll_us per call for nothing: stream waits, one more try
    // every 1024 calls
    if (s->mbox_timeouts >= 8 && (++s->mbox_skipped & 1023u) != 0) return PSK_OK;
    if (!s->mbox) {
        void *pp = nullptr;
        HIP_TRY(hipHostMalloc(&pp, 64, hipHostMallocDefault));
        *(volatile uint32_t *)pp = 0;
        s->mbox = (volatile uint32_t *)pp;
    }
    if (++s->mbox_seq == 0) ++s->mbox_seq;  // (never the word's initial 0)
    mb->word = s->mbox;
    mb->seq = s->mbox_seq;
    mb->timeouts = &s->mbox_timeouts;
    return PSK_OK;
}
static bool mailbox_wait(const Mailbox *mb)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 1;; ++spins) {
        if (__atomic_load_n(mb->word, __ATOMIC_ACQUIRE) == mb->seq) return true;
        __builtin_ia32_pause();
        if ((spins & 1023) == 0 &&
            std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > g_host_poll_us)
            return false;
    }
}

int pinned(DevBuf &b, void **out)
{
    if (!b.pin) HIP_TRY(hipHostMalloc(&b.pin, kPinBytes, hipHostMallocDefault));
    *out = b.pin;
    return PSK_OK;
}

static int elem_bytes(int layout) { return layout == PSK_KEYS_VARLEN32 ? 4 : (layout == PSK_KEYS_HASHES ? 8 : 1); }

int stage_batch(DevBuf &kbuf, DevBuf &obuf, int layout, const void *data, const uint64_t *offsets, uint64_t n, uint32_t key_len, int where,
                hipStream_t st, Batch *b)
{
    if (layout < PSK_KEYS_FIXED || layout > PSK_KEYS_HASHES) return fail(PSK_EINVAL, "unknown key layout %d", layout);
    if (where != PSK_HOST && where != PSK_DEVICE) return fail(PSK_EINVAL, "`where` must be PSK_HOST or PSK_DEVICE");
    const bool varlen = layout == PSK_KEYS_VARLEN8 || layout == PSK_KEYS_VARLEN32;
    if (n && !data && !(layout == PSK_KEYS_FIXED && key_len == 0)) return fail(PSK_EINVAL, "key data pointer is NULL");
    if (n && varlen && !offsets) return fail(PSK_EINVAL, "variable-length layout needs offsets[n+1]");
    b->layout = layout;
    b->n = n;
    b->key_len = key_len;
    b->data = data;
    b->offs = offsets;
    if (where == PSK_DEVICE || n == 0) return PSK_OK;
    uint64_t nbytes;
    if (varlen) {
        const uint64_t total = offsets[n] - offsets[0];
        if (offsets[0] != 0) return fail(PSK_EINVAL, "host offsets must start at 0");
        nbytes = total * (uint64_t)elem_bytes(layout);
        if ((n + 1) * 8 <= kPinBytes) {
            void *pp;
            PSK_TRY(pinned(obuf, &pp));
            memcpy(pp, offsets, (n + 1) * 8);
            b->offs = (const uint64_t *)pp;
        } else {
            PSK_TRY(ensure(obuf, (n + 1) * 8));
            HIP_TRY(hipMemcpyAsync(obuf.p, offsets, (n + 1) * 8, hipMemcpyHostToDevice, st));
            b->offs = (const uint64_t *)obuf.p;
        }
    } else {
        nbytes = n * (uint64_t)key_len * (uint64_t)elem_bytes(layout);
    }
    if (nbytes <= kPinBytes) {  // tiny batch (single-key API): the kernel reads the keys straight from pinned host memory
        void *pp;
        PSK_TRY(pinned(kbuf, &pp));
        if (nbytes) memcpy(pp, data, nbytes);
        b->data = pp;
        return PSK_OK;
    }
    PSK_TRY(ensure(kbuf, nbytes));
    HIP_TRY(hipMemcpyAsync(kbuf.p, data, nbytes, hipMemcpyHostToDevice, st));
    b->data = kbuf.p;
    return PSK_OK;
}

const KeysInline64 *inline_key(int layout, const void *data, uint64_t n, uint32_t key_len, const Mailbox &mb, KeysInline64 *k)
{
    if (!mb.word || n != 1 || layout != PSK_KEYS_FIXED || key_len > sizeof k->w) return nullptr;
    memset(k->w, 0, sizeof k->w);
    if (key_len) memcpy(k->w, data, key_len);
    k->L = key_len;
    return k;
}

int check_hashes_width(const psk_sketch *s, int layout, uint32_t key_len)
{
    if (layout == PSK_KEYS_HASHES && key_len < s->k)
        return fail(PSK_EINVAL, "pre-hashed batch carries %u hashes per key, the sketch needs %u", key_len, s->k);
    return PSK_OK;
}

int stage_out(DevBuf &buf, void *out, uint64_t bytes, int where, OutBuf *o)
{
    o->bytes = bytes;
    if (where == PSK_DEVICE || bytes == 0) {
        o->dev = out;
        return PSK_OK;
    }
    o->host = out;
    if (bytes <= kPinBytes) {
        PSK_TRY(pinned(buf, &o->dev));
        o->is_pinned = true;
        return PSK_OK;
    }
    PSK_TRY(ensure(buf, bytes));
    o->dev = buf.p;
    return PSK_OK;
}

int finish(int where, const OutBuf *o, hipStream_t st, const Mailbox *mb)
{
    if (where == PSK_HOST) {
        const bool copy = o && o->host && o->bytes;
        if (copy && !o->is_pinned) HIP_TRY(hipMemcpyAsync(o->host, o->dev, o->bytes, hipMemcpyDeviceToHost, st));
        bool posted = false;
        if (mb && mb->word) {
            posted = mailbox_wait(mb);
            if (mb->timeouts) *mb->timeouts = posted ? 0u : *mb->timeouts + 1u;
        }
        if (!posted) HIP_TRY(hipStreamSynchronize(st));
        if (copy && o->is_pinned) memcpy(o->host, o->dev, o->bytes);
    }
    return PSK_OK;
}

ThreadStage &thread_stage()
{
    static thread_local ThreadStage ts;
    return ts;
}
