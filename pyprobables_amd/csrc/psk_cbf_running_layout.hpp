// psk_cbf_running_layout.hpp -- chunk size and scratch layout of the ordered CountingBloomFilter batches (psk_cbf_running.hpp): plain
// integer arithmetic without a HIP call, so that a host program can check it on its own (tests/host/cbf_running_layout_main.cpp).
#pragma once
#include <cstdint>

constexpr uint32_t kCbfRunChunk = 1u << 20;    // most ops per chunk (psk::kRunChunk); fewer for many hashes: chunk * k <= kCbfRunCells
constexpr uint32_t kCbfRunCells = 1u << 23;    // (psk::kRunCells)
constexpr uint32_t kCbfRunSortTile = 2048;     // (psk::kRunSortTile)
constexpr uint32_t kCbfRunSegBlock = 256;      // (psk::kRunSegBlock)
constexpr uint32_t kCbfRunMapBytes = 24;       // sizeof(psk::CbfMap)
constexpr uint32_t kCbfRunTallyBytes = 64;     // kCbfTallyWords * 8
constexpr uint32_t kCbfRunMaxK = 64;           // eligibility: k <= 64, m <= 2^32

// where the buffers of one chunk lie, for chunks of at most `cap` ops of k probes
struct CbfRunLayout {
    uint32_t cap, passes;                                                    // ops per chunk; radix passes
    uint64_t cells, tiles, blocks;                                           // probes, sort tiles and scan blocks of a full chunk
    uint64_t off_pairs[2], off_before, off_hist, off_agg, off_tally, bytes;  // byte offsets into the scratch, and its size
};

// the layout for a batch of n >= 1 ops into m <= 2^32 counters with 1 <= k <= 64 hashes
static inline void cbf_running_layout(uint64_t n, uint32_t k, uint64_t m, CbfRunLayout *l)
{
    auto up16 = [](uint64_t b) { return (b + 15) & ~15ULL; };
    uint64_t cap = kCbfRunCells / k;
    if (cap > kCbfRunChunk) cap = kCbfRunChunk;
    if (cap > n) cap = n;
    if (cap == 0) cap = 1;
    cap = (cap + kCbfRunSortTile - 1) / kCbfRunSortTile * kCbfRunSortTile;  // (>= one tile; at most kCbfRunCells + 2047 * 64 probes per chunk)
    l->cap = (uint32_t)cap;
    uint32_t bits = 0;
    while (bits < 32 && (1ULL << bits) < m) ++bits;  // bins < m <= 2^32
    l->passes = bits <= 8 ? 1u : (bits + 7) / 8;
    l->cells = cap * k;
    l->tiles = l->cells / kCbfRunSortTile;
    l->blocks = l->cells / kCbfRunSegBlock;
    uint64_t at = 0;
    l->off_pairs[0] = at;
    at += up16(l->cells * 8);
    l->off_pairs[1] = at;
    at += up16(l->cells * 8);
    l->off_before = at;
    at += up16(l->cells * 4);
    l->off_hist = at;
    at += up16(256 * l->tiles * 4);
    l->off_agg = at;
    at += up16(l->blocks * kCbfRunMapBytes);
    l->off_tally = at;
    at += kCbfRunTallyBytes;
    l->bytes = at + 16;
}

// the chunks of a batch of n ops: chunk c covers ops [c * cap, min(n, (c + 1) * cap))
static inline uint64_t cbf_running_chunks(uint64_t n, const CbfRunLayout &l) { return (n + l.cap - 1) / l.cap; }
static inline uint32_t cbf_running_chunk_ops(uint64_t n, const CbfRunLayout &l, uint64_t c)
{
    const uint64_t base = c * l.cap;
    return (uint32_t)(n - base < l.cap ? n - base : l.cap);
}
