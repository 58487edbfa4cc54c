// Stand-alone check of the scan values of the ordered batches (csrc/psk_running.hpp: RunSeg, RunMap, RunSum, RunMap64, RunTile; csrc/psk_cbf_running.hpp:
// CbfMap) on the CPU, for a build with -fsanitize=address,undefined on the host.  The algebra members are __host__ __device__, so this is the
// code the kernels run, not a restatement.
//   1. the laws of the contract (csrc/psk_segscan.hpp): the identity on both sides, associativity over every triple of a fixed set with the
//      rails in it.  Two values are equal when they agree as maps on every probe value and in their head flag.
//   2. the three levels of the scan in plain C++ (blocks of 4 elements reduced to one value, an exclusive carry over the block values in
//      stretches of 2, the block's scan redone behind its carry) over short streams: every op's value and every bin's final value must
//      equal the reference's loop, one op after the other, which is written out below.
#include "../../pyprobables_amd/csrc/psk_cbf_running.hpp"

#include <algorithm>
#include <cstdio>
#include <vector>

using namespace psk;

static int g_fail = 0;
static void fail(const char *type, const char *what, long at)
{
    if (++g_fail <= 20) std::fprintf(stderr, "FAIL %s: %s (%ld)\n", type, what, at);
}

static uint64_t g_seed = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd()  // splitmix64
{
    uint64_t z = (g_seed += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

template <class M> uint32_t head_of(const M &m) { return m.head; }
static uint32_t head_of(const RunSum &) { return 0; }
static uint32_t head_of(const RunMap64 &) { return 0; }

template <class M, class V>
static bool same(const M &a, const M &b, const std::vector<V> &probes)
{
    if (head_of(a) != head_of(b)) return false;
    for (V x : probes)
        if (a(x) != b(x)) return false;
    return true;
}

static bool same(const RunTile &a, const RunTile &b, const std::vector<long long> &probes)  // its map on elements_added and its sum of |w|
{
    return a.abs() == b.abs() && same(a.els(), b.els(), probes);
}

// ------------------------------------------------------------------ 1. the laws
template <class M, class V>
static void laws(const char *type, const std::vector<M> &set, const std::vector<V> &probes)
{
    for (size_t i = 0; i < set.size(); ++i) {
        if (!same(M::combine(M::identity(), set[i]), set[i], probes)) fail(type, "identity on the left", (long)i);
        if (!same(M::combine(set[i], M::identity()), set[i], probes)) fail(type, "identity on the right", (long)i);
        for (size_t j = 0; j < set.size(); ++j)
            for (size_t k = 0; k < set.size(); ++k)
                if (!same(M::combine(M::combine(set[i], set[j]), set[k]), M::combine(set[i], M::combine(set[j], set[k])), probes))
                    fail(type, "associativity", (long)((i * set.size() + j) * set.size() + k));
    }
}

// ------------------------------------------------------------------ 2. the three levels
struct Op {
    uint32_t bin;
    int32_t w;
};
constexpr size_t kBlockElems = 4, kStretch = 2;

// make(w, head): one op as a value; step(x, w): what the reference's op does to a bin that holds x; start[b]: the table in front
template <class M, class V, class Make, class Step>
static void levels(const char *type, const std::vector<Op> &ops, const std::vector<V> &start, Make make, Step step)
{
    const size_t n = ops.size();
    // the reference: one op after the other
    std::vector<V> table = start, want(n);
    for (size_t i = 0; i < n; ++i) want[i] = table[ops[i].bin] = step(table[ops[i].bin], ops[i].w);
    // stable sort of (bin, position); past the end of the last block: empty segments of their own
    std::vector<size_t> pos(n);
    for (size_t i = 0; i < n; ++i) pos[i] = i;
    std::stable_sort(pos.begin(), pos.end(), [&](size_t a, size_t b) { return ops[a].bin < ops[b].bin; });
    const size_t nblk = (n + kBlockElems - 1) / kBlockElems;
    std::vector<M> elem(nblk * kBlockElems, make(0, true));
    std::vector<bool> head(n);
    for (size_t j = 0; j < n; ++j) {
        head[j] = j == 0 || ops[pos[j - 1]].bin != ops[pos[j]].bin;
        elem[j] = make(ops[pos[j]].w, head[j]);
    }
    // level 1: every block as one value
    std::vector<M> agg(nblk, M::identity());
    for (size_t b = 0; b < nblk; ++b)
        for (size_t t = 0; t < kBlockElems; ++t) agg[b] = M::combine(agg[b], elem[b * kBlockElems + t]);
    // level 2: "threads" with a stretch of 2 block values each, an inclusive scan over the threads, the stretch rewritten exclusively
    const size_t nthr = (nblk + kStretch - 1) / kStretch;
    std::vector<M> incl(nthr, M::identity());
    for (size_t t = 0; t < nthr; ++t) {
        M mine = M::identity();
        for (size_t b = t * kStretch; b < std::min(nblk, (t + 1) * kStretch); ++b) mine = M::combine(mine, agg[b]);
        incl[t] = t ? M::combine(incl[t - 1], mine) : mine;
    }
    for (size_t t = 0; t < nthr; ++t) {
        M run = t ? incl[t - 1] : M::identity();
        for (size_t b = t * kStretch; b < std::min(nblk, (t + 1) * kStretch); ++b) {
            const M x = agg[b];
            agg[b] = run;
            run = M::combine(run, x);
        }
    }
    // level 3: the block's scan behind its carry; `before` = the bin's ops in front of this one
    std::vector<V> got = start;
    for (size_t b = 0; b < nblk; ++b) {
        M run = agg[b];
        for (size_t t = 0; t < kBlockElems && b * kBlockElems + t < n; ++t) {
            const size_t j = b * kBlockElems + t, i = pos[j];
            const V t0 = start[ops[i].bin];
            const M before = head[j] ? M::identity() : run;
            run = M::combine(run, elem[j]);
            if (step(before(t0), ops[i].w) != want[i]) fail(type, "the value in front of an op, then the op", (long)i);
            if (run(t0) != want[i]) fail(type, "the value behind an op", (long)i);
            if (j + 1 == n || ops[pos[j + 1]].bin != ops[i].bin) got[ops[i].bin] = run(t0);
        }
    }
    if (got != table) fail(type, "the final table", (long)n);
}

// streams of `type`: every length and bin count below, start values on and next to the rails; gen(x, r) makes a weight that is
// valid for a bin that holds x (CbfMap: a remove must be full); a value without segments gets one bin
template <class M, class V, class Make, class Step, class Gen>
static void streams(const char *type, bool segmented, const std::vector<V> &rails, Make make, Step step, Gen gen)
{
    const size_t lens[] = {1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 37, 64, 129, 300};
    const uint32_t bins[] = {1, 2, 5};
    for (size_t n : lens)
        for (uint32_t nb : bins)
            for (int rep = 0; rep < 4 && (segmented || nb == 1); ++rep) {
                std::vector<V> start(nb), now;
                for (uint32_t b = 0; b < nb; ++b) start[b] = rails[(b + rep * 3 + n) % rails.size()];
                now = start;
                std::vector<Op> ops(n);
                for (size_t i = 0; i < n; ++i) {
                    const uint32_t b = rep == 3 ? 0 : (uint32_t)(rnd() % nb);  // (rep 3: one bin, one segment over every block)
                    ops[i] = Op{b, gen(now[b], rnd())};
                    now[b] = step(now[b], ops[i].w);
                }
                levels<M, V>(type, ops, start, make, step);
            }
}

static int64_t clamp64(__int128 x, int64_t lo, int64_t hi) { return x < lo ? lo : (x > hi ? hi : (int64_t)x); }

int main()
{
    const std::vector<int32_t> p32 = {INT32_MIN, INT32_MIN + 1, INT32_MIN + 3, -2, -1, 0, 1, 2, INT32_MAX - 3, INT32_MAX - 1, INT32_MAX};
    const std::vector<long long> p64 = {INT64_MIN, INT64_MIN + 1, INT64_MIN + 3, INT32_MIN, -1, 0, 1, INT32_MAX, INT64_MAX - 3, INT64_MAX - 1, INT64_MAX};
    const std::vector<uint32_t> pu = {0u, 1u, 2u, 5u, 0x7FFFFFFFu, 0x80000000u, kCbfMax - 5, kCbfMax - 2, kCbfMax - 1, kCbfMax};
    const int32_t signed_w[] = {INT32_MIN, -INT32_MAX, -2, -1, 0, 1, 2, INT32_MAX - 1, INT32_MAX};
    const int32_t add_w[] = {0, 1, 2, INT32_MAX - 1, INT32_MAX};

    // ---- the laws
    std::vector<RunSeg> segs = {RunSeg::identity(), RunSeg{0xFFFFFFFFu, 0u}, RunSeg{0xFFFFFFFEu, 1u}};
    std::vector<RunSum> sums = {RunSum::identity(), RunSum{1ULL << 51}};
    for (int32_t w : add_w) {
        sums.push_back(RunSum::of(w));
        for (bool h : {false, true}) segs.push_back(RunSeg::of(w, h));
    }
    std::vector<RunMap> maps = {RunMap::identity(), RunMap{5, INT32_MIN + 5, INT32_MAX, 0u}, RunMap{-7, -3, 9, 1u}};
    std::vector<RunMap64> maps64 = {RunMap64::identity(), RunMap64{5, INT64_MIN + 5, INT64_MAX}, RunMap64{-(1LL << 51), INT64_MIN, INT64_MAX - (1LL << 51)}, RunMap64{-7, -3, 9}};
    std::vector<CbfMap> cbfs = {CbfMap::identity()};
    std::vector<RunTile> tiles = {RunTile::identity(), RunTile{RunMap64{-7, -3, 9}, 7}, RunTile{RunMap64{1LL << 51, INT64_MIN + (1LL << 51), INT64_MAX}, 1ULL << 51}};
    for (int32_t w : signed_w) {
        maps64.push_back(RunMap64::of(w));
        tiles.push_back(RunTile::of(w));
        for (bool h : {false, true}) {
            maps.push_back(RunMap::of(w, h));
            cbfs.push_back(CbfMap::of(w, 1, h));
        }
        cbfs.push_back(CbfMap::of(w, 2, false));
    }
    laws("RunSeg", segs, p32);
    laws("RunSum", sums, p64);
    laws("RunMap", maps, p32);
    laws("RunMap64", maps64, p64);
    laws("RunTile", tiles, p64);
    laws("CbfMap", cbfs, pu);

    // ---- the three levels against the reference's loops
    // countminsketch.py:276-284: bin = min(bin + w, INT32_MAX), w >= 0
    auto add_step = [](int32_t x, int32_t w) { return (int32_t)std::min<int64_t>((int64_t)x + w, INT32_MAX); };
    auto add_gen = [&](int32_t, uint64_t r) { return r % 3 == 0 ? add_w[(r >> 8) % 5] : (int32_t)((r >> 8) % (r % 3 == 1 ? 7 : 0x7FFFFFFFu)); };
    streams<RunSeg, int32_t>("RunSeg", true, p32, [](int32_t w, bool h) { return RunSeg::of(w, h); }, add_step, add_gen);
    // :276-284 / :309-316: an add clamps at INT32_MAX, a remove (w < 0 removes -w) at INT32_MIN
    auto signed_step = [](int32_t x, int32_t w) { return (int32_t)clamp64((__int128)x + w, INT32_MIN, INT32_MAX); };
    auto signed_gen = [&](int32_t, uint64_t r) { return r % 3 == 0 ? signed_w[(r >> 8) % 9] : (int32_t)(r % 3 == 1 ? (int64_t)((r >> 8) % 11) - 5 : (int64_t)((r >> 8) & 0xFFFFFFFFu) - (1LL << 31)); };
    streams<RunMap, int32_t>("RunMap", true, p32, [](int32_t w, bool h) { return RunMap::of(w, h); }, signed_step, signed_gen);
    // elements_added, :285-287 / :317-319: the same on the int64 rails, one "bin" (no segments: the head is ignored)
    auto els_add_step = [](long long x, int32_t w) { return (long long)clamp64((__int128)x + w, INT64_MIN, INT64_MAX); };
    streams<RunSum, long long>("RunSum", false, p64, [](int32_t w, bool) { return RunSum::of(w); }, els_add_step, add_gen);
    streams<RunMap64, long long>("RunMap64", false, p64, [](int32_t w, bool) { return RunMap64::of(w); }, els_add_step, signed_gen);
    // countingbloom.py:135-155 / :186-208 on one counter (k = 1): an add clamps at 2^32 - 1, which is sticky; a remove of w from a counter
    // below it that holds at least w takes w (the map is optimistic: only such FULL removes are generated), a counter on the rail stays
    auto cbf_step = [](uint32_t x, int32_t w) {
        if (w >= 0) return (uint32_t)std::min<uint64_t>((uint64_t)x + (uint64_t)w, kCbfMax);
        return x == kCbfMax ? kCbfMax : (uint32_t)((int64_t)x + w);
    };
    auto cbf_gen = [&](uint32_t x, uint64_t r) {
        const int32_t w = signed_gen(0, r);
        if (w >= 0 || x == kCbfMax) return w;
        return (int32_t)-std::min<int64_t>(-(int64_t)w, x);  // (at most what the counter holds; 0 from an empty one)
    };
    streams<CbfMap, uint32_t>("CbfMap", true, pu, [](int32_t w, bool h) { return CbfMap::of(w, 1, h); }, cbf_step, cbf_gen);

    std::printf("%d failures\n", g_fail);
    return g_fail ? 1 : 0;
}
