"""Pass 1's bins carry a bin's remainder (fewer than six probes) into the next tile instead of closing every (tile, slice) bin with a padded
group (psk_part_bins.hpp): the probes that reach pass 2 are the same multiset, only their grouping changes, so every table and every answer
must still equal the plain-C oracle's, bit for bit.  The shapes are the smallest at which the carry can go wrong: pass 1 starts at most 512
workgroups, so a batch needs more than 2 x 512 x 1536 keys to give every workgroup three tiles.  bloom.py:241-272, countminsketch.py:267-288,
hashes.py:71-103."""

import numpy as np
import pytest

from bins_carry_model import bin_capacity, cms_indices, fnv_indices, plan, segment_capacity, spills

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILE = 1536                      # keys per full pass-1 tile (kBinThreads x kBinKpt)
N3 = 3 * 512 * TILE              # three full tiles for each of the 512 workgroups
HEADLINE = dict(est_elements=28005615, false_positive_rate=0.01)   # m = 2^28, k = 7: 256 slices of 2^20 bits


@pytest.fixture(scope="module")
def pa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pyprobables_amd

    return pyprobables_amd


@pytest.fixture()
def N():
    from pyprobables_amd import _native as N

    names = ("partition", "partition_min_keys", "pass1_bins", "bloom_lookup", "even_tiles", "cms_small_weights")
    old = [N.get_option(k) for k in names]
    N.set_option("partition", 1)
    N.set_option("pass1_bins", 1)
    yield N
    for k, v in zip(names, old):
        N.set_option(k, v)


@pytest.fixture(scope="module")
def keys(oracle):
    return oracle.gen_keys16(1000, 2_400_000)


@pytest.fixture(scope="module")
def absent(oracle):
    return oracle.gen_keys16(3_000_000_000, 4096)


@pytest.fixture(scope="module")
def headline_table(oracle, keys):
    """the oracle's m = 2^28, k = 7 filter of keys[:N3] (read-only: shared)"""
    ob = oracle.OracleBloom(2**28, 7)
    ob.add_keys(keys[:N3])
    return ob


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _table(f):
    return np.frombuffer(bytes(f.bloom), dtype=np.uint8)


def _check(blm, probe):
    return blm.check_many(_dev(probe)).cpu().numpy().astype(np.uint8)


@pytest.mark.parametrize("even_tiles", [1, 0])
def test_one_key_last_tile_and_the_flush(pa, oracle, N, keys, headline_table, even_tiles):
    """3 x 512 x 1536 + 1 keys.  even_tiles = 0: 1537 tiles, the last one of ONE key -- workgroup 0 runs a fourth tile that brings seven probes,
    every other workgroup flushes after its third.  even_tiles = 1 (the default): four tiles of 1216 keys per workgroup, the last one short."""
    n = N3 + 1
    assert plan(n, 7, 256, even_tiles)[0] == (1216 if even_tiles else TILE)
    N.set_option("even_tiles", even_tiles)
    blm = pa.BloomFilter(**HEADLINE)
    blm.add_many(_dev(keys[:n]))
    ob = oracle.OracleBloom(blm.number_bits, blm.number_hashes)
    ob.bloom[:] = headline_table.bloom
    ob.add_keys(keys[N3:n])
    assert np.array_equal(_table(blm), ob.bloom)
    for scheme in (3, 0):       # tile flags (pass 1 = the insert's bins), keyed probes
        blm.set_engine_option("bloom_lookup", scheme)
        assert bool(blm.check_many(_dev(keys[:n])).all())


@pytest.mark.parametrize("est,fpr,k,m,shift", [
    (100_000_000, 0.5, 1, 144269505, 19),    # 276 slices: 4.4 probes per bin and 1216-key tile
    (60_000_000, 0.25, 2, 173123405, 19),    # 331 slices: 7.3
])
def test_thin_bins_send_a_carry_out_with_the_next_tile(pa, oracle, N, keys, absent, est, fpr, k, m, shift):
    """most bins hold fewer than six probes after a tile: inserts keep carrying them, tile-flag lookups must send a carried probe out with the
    next tile, as a short group where the bin is still short of six (a group of ordinal o holds nothing older than tile o - 1)"""
    n = N3 + 1
    blm = pa.BloomFilter(est_elements=est, false_positive_rate=fpr)
    assert (blm.number_hashes, blm.number_bits) == (k, m)
    nslices = -(-m // (1 << shift))
    assert 128 <= nslices <= 511 and (m >> shift) >= 256     # part_slices: 2^8 .. 2^9 - 1 slices of 2^(floor(lg m) - 8) bits
    shape = spills(fnv_indices(keys[:n], k, m), nslices, shift, bin_capacity(k, nslices, True), True)
    assert shape["thin"] > (0.6 if k == 1 else 0.2), shape    # share of (tile, slice) bins with fewer than six probes of their own
    blm.add_many(_dev(keys[:n]))
    ob = oracle.OracleBloom(m, k)
    ob.add_keys(keys[:n])
    assert np.array_equal(_table(blm), ob.bloom)
    probe = keys[:n].copy()
    probe[5::1000] = absent[: probe[5::1000].shape[0]]       # a miss in nearly every tile
    want = ob.check_keys(probe).astype(np.uint8)
    assert 0 < int((want == 0).sum())
    blm.set_engine_option("bloom_lookup", 3)
    assert np.array_equal(_check(blm, probe), want)
    assert bool(blm.check_many(_dev(keys[:n])).all())


def test_skew_fills_bins_and_segments(pa, oracle, N, keys, absent):
    """every second key is the same one: its k bins overflow in every tile, and what does not fit takes the exact fallback; nothing is lost
    and the lookups still answer every key.  (At this size the hot slices' SEGMENTS do not fill: four tiles per workgroup hand a segment at
    most 4 x 12 groups and it has room for 55; a hot bin is always exactly full, so it never holds a remainder either.  The segment-full
    branches are what the three test_full_segment_* cases below run.)"""
    n = 2_400_000
    skew = keys[:n].copy()
    skew[::2] = keys[7]
    per_tile = plan(n, 7, 256)[0] // 2                         # copies of the hot key per tile: each of its bins gets that many probes
    assert per_tile > 5 * bin_capacity(7, 256, True)
    blm = pa.BloomFilter(**HEADLINE)
    blm.add_many(_dev(skew))
    ob = oracle.OracleBloom(blm.number_bits, blm.number_hashes)
    ob.add_keys(skew)
    assert np.array_equal(_table(blm), ob.bloom)
    probe = skew.copy()
    probe[1::2000] = absent[: probe[1::2000].shape[0]]
    probe[0:4000:2] = absent[4000]                             # an absent key as the hot one of the first tiles
    want = ob.check_keys(probe).astype(np.uint8)
    assert 0 < int((want == 0).sum())
    blm.set_engine_option("bloom_lookup", 3)
    assert np.array_equal(_check(blm, probe), want)
    assert np.array_equal(_check(blm, skew), np.ones(n, dtype=np.uint8))


def test_tile_flag_lookups_answer_misses_at_tile_seams(pa, oracle, N, keys, absent, headline_table):
    """the last keys of a tile take the last slots of their bins, the ones a bin carries into the next tile's first group: a miss among them
    leaves pass 1 under the NEXT tile's ordinal and must still clear its own key's answer.  3 x 512 full tiles; workgroup w runs the tiles
    w, w + 512, w + 1024.  (At k = 7 an absent key has about four clear probes, and one of them in a slot that was NOT carried flags the
    right tile already, so this case would rarely notice a missing o - 1 flag in k_bloom_test_flag; which probes a bin carries also depends
    on the order of the LDS atomics.  What pins that flag, and the rule that a carry leaves with the next tile, is the k = 1 case of
    test_thin_bins_send_a_carry_out_with_the_next_tile: one probe per key, most of them carried.)"""
    n = N3
    assert plan(n, 7, 256) == (TILE, 512, 3)
    blm = pa.BloomFilter(**HEADLINE)
    blm.add_many(_dev(keys[:n]))
    assert np.array_equal(_table(blm), headline_table.bloom)
    probe = keys[:n].copy()
    tiles = [0, 1, 5, 511, 512, 517, 1023, 1024, 1029, 1535]      # first / middle / last tile of workgroups 0, 5 and 511, and a lone one
    a = 0
    for t in tiles:
        probe[(t + 1) * TILE - 3:(t + 1) * TILE] = absent[a:a + 3]
        a += 3
    probe[1200 * TILE] = absent[a]                             # ... and a tile's first key
    want = headline_table.check_keys(probe).astype(np.uint8)
    assert int((want == 0).sum()) >= 3 * len(tiles) - 2        # (k = 7 at this load: a false positive among 28 absent keys is unlikely, two are not expected)
    blm.set_engine_option("bloom_lookup", 3)
    assert np.array_equal(_check(blm, probe), want)
    N.set_option("even_tiles", 0)
    assert np.array_equal(_check(blm, np.concatenate([probe, absent[100:101]])), np.append(want, headline_table.check_keys(absent[100:101]).astype(np.uint8)))


def test_weighted_cms_adds_carry_their_weights(pa, oracle, N, keys):
    """CountMinSketch 2^20 x 5 (160 slices), 2.4 M adds with weights 1 .. 7 in the compact probe format: a carried field keeps its weight, the
    flush pads with the all-zero field"""
    n = 2_400_000
    w = oracle.gen_weights(1000, n)
    assert int(w.min()) == 1 and int(w.max()) == 7
    N.set_option("cms_small_weights", 2)                       # the compact format whatever the hint says
    cms = pa.CountMinSketch(width=2**20, depth=5)
    cms.add_many(_dev(keys[:n]), _dev(w))
    oc = oracle.OracleCMS(2**20, 5)
    oc.add_keys(keys[:n], w)
    assert np.array_equal(np.frombuffer(bytes(cms._bins), dtype=np.int32), oc.bins)
    assert cms.elements_added == oc.els_added


def test_spilled_probes_stay_a_small_share(pa, oracle, N, keys, headline_table):
    """How many probes find their bin full and take the exact fallback, on the headline geometry with 3 x 512 full tiles of random keys.
    The count follows from the keys alone (tests/bins_carry_model.py).  The figures for the library before the carry come from that HOST
    MODEL, not from a run of that library, which had no counter: with a padded group per (tile, slice) and bins of 66 probes the model has
    these keys spill 219 of their 16 515 072 probes (1.3e-5), and eight other key ranges of this size 207 .. 262, a spread of 55.  The model
    is checked against the engine for this build only.  A bin now starts a tile with up to five carried probes: at 66 the same keys would
    spill 756, which is why bins_plan adds one group (72): 26.  The engine's own count (PSK_CTR_SPILLED, an insert behind a clear) must be
    that and must not be zero; the bound against the modelled old count plus its spread follows from the equality and is kept because it
    is the condition the capacity was chosen by."""
    n = N3
    idx = fnv_indices(keys[:n], 7, 2**28)
    before = spills(idx, 256, 20, bin_capacity(7, 256, False), False)
    after = spills(idx, 256, 20, bin_capacity(7, 256, True), True)
    assert before["tile"] == TILE and before["bin_spills"] == 219 and after["bin_spills"] == 26
    blm = pa.BloomFilter(**HEADLINE)
    blm.clear()                                                # (the insert behind a clear keeps pass 1's spills in a list and counts them)
    blm.add_many(_dev(keys[:n]))
    spilled = blm._tab.counters()[N.CTR_SPILLED]
    print(f"spilled probes: {spilled} of {n * 7} ({spilled / (n * 7):.2e}); model {after['bin_spills']}; padded bins of 66: {before['bin_spills']}")
    assert np.array_equal(_table(blm), headline_table.bloom)
    assert spilled == after["bin_spills"]
    assert 0 < spilled <= before["bin_spills"] + 55


# ---- full segments.  A segment has room for the round's mean load plus a margin (launch_scatter_bins); a bin hands it at most cap / 6 groups
# per tile, so with bins a segment can fill up only where a workgroup runs about ten tiles (Bloom, k = 7) or eight (the 2^20 x 5
# CountMinSketch).  The batches below are drawn from a small pool of keys, so the host model follows every bin and every segment cursor
# exactly and cheaply: three hot keys whose slices no other key of the pool touches, and 4096 cold ones.
#   hot key 0: cap - 6 .. cap - 1 copies per tile, drawn per tile -- its bins keep remainders, and its segments fill up while they hold one;
#   hot key 1: 6 x segcap + 3 copies in all, never more than a bin holds -- its cursors reach the segment's end EXACTLY, on the fast path,
#              and the flush behind the last tile finds no room for the three probes left;
#   hot key 2: a full bin in every tile -- its segments fill up first, and the write-outs after that find the cursor past the end.
def _full_segment_batch(slices, per_wg, nwg, tk, cap, segcap):
    """slices[p, j] = slice of probe j of pool key p -> (ids of the batch's keys in the pool, the three hot pool keys, the cold ones)"""
    k = slices.shape[1]
    hot, used = [], set()
    for p in range(slices.shape[0]):
        mine = set(slices[p].tolist())
        if len(mine) == k and not (mine & used):
            hot.append(p)
            used |= mine
            if len(hot) == 3:
                break
    cold = np.flatnonzero(~np.isin(slices, sorted(used)).any(axis=1))[:4096]
    assert len(hot) == 3 and cold.shape[0] == 4096
    total = 6 * segcap + 3
    copies = [np.random.default_rng(7).integers(cap - 6, cap, (per_wg, nwg)),       # copies[h][o, w]: of hot key h in the o-th tile of workgroup w
              np.repeat(np.full(per_wg, total // per_wg) + (np.arange(per_wg) < total % per_wg), nwg).reshape(per_wg, nwg),
              np.full((per_wg, nwg), cap)]
    assert int(copies[1].max()) + 5 < cap
    n = per_wg * nwg * tk
    ids = cold[np.arange(n) % 4096].reshape(per_wg, nwg, tk)      # tile o * nwg + w = the o-th tile of workgroup w
    step = tk // cap
    for h in range(3):                                            # every step-th key of a tile, from its h-th on
        ids[:, :, h:h + step * cap:step][np.arange(cap) < copies[h][:, :, None]] = hot[h]
    return ids.reshape(-1), hot, cold


@pytest.fixture(scope="module")
def full_segments(oracle, keys):
    """the Bloom batch (m = 2^28, k = 7: 11 tiles of 1408 keys for each of 512 workgroups), what the model says about it as an insert and as a
    tile-flag lookup, and the oracle's filter of it"""
    per_wg, nwg, tk = 11, 512, 1408
    n = per_wg * nwg * tk
    assert plan(n, 7, 256) == (tk, nwg, per_wg)
    cap, segcap = bin_capacity(7, 256, True), segment_capacity(n, 7, 256)
    pool = keys[:8192]
    idx = fnv_indices(pool, 7, 2**28)
    ids, hot, cold = _full_segment_batch((idx >> np.uint64(20)).astype(np.int64), per_wg, nwg, tk, cap, segcap)
    shapes = [spills(idx, 256, 20, cap, True, ids=ids, segcap=segcap, tile_tag=tag) for tag in (False, True)]
    ob = oracle.OracleBloom(2**28, 7)
    ob.add_keys(pool[np.concatenate([hot, cold])])             # (a Bloom filter of a batch = that of its distinct keys)
    return pool, ids, hot, cold, shapes, ob


def _assert_segments_fill(shape, after=True):
    print(shape)
    assert shape["seg_full_rem"] > 0 and shape["flush_spills"] > 0 and shape["seg_spills"] > 0, shape
    if after:
        assert shape["seg_full_after"] > 0, shape


def test_full_segment_insert_spills_the_remainder(pa, oracle, N, full_segments):
    """k_part_bins<PayNone>: a write-out that does not fit its segment writes what fits and hands the rest, the bin's remainder included, to the
    exact fallback; the flush does the same with a remainder it finds no room for.  Nothing is lost: the table is the oracle's."""
    pool, ids, hot, cold, shapes, ob = full_segments
    _assert_segments_fill(shapes[0])
    batch = _dev(pool[ids])
    blm = pa.BloomFilter(**HEADLINE)
    blm.add_many(batch)                                        # the fallback ORs into the table
    assert np.array_equal(_table(blm), ob.bloom)
    blm.clear()
    blm.add_many(batch)                                        # behind a clear: the fallback's probes wait in a list, and the engine counts them
    spilled = blm._tab.counters()[N.CTR_SPILLED]
    assert np.array_equal(_table(blm), ob.bloom)
    assert spilled == shapes[0]["bin_spills"] + shapes[0]["seg_spills"] + shapes[0]["flush_spills"]


def test_full_segment_tile_flag_lookup_answers_spilled_misses(pa, oracle, N, full_segments):
    """k_part_bins<PayTileTag>: the filter holds every key of the batch but hot key 0, so each of its copies is a miss -- in the workgroups' last
    tiles all of its probes, what the bins carried from the tile before among them, reach pass 2 through the exact fallback alone (flagging
    the tile and the one before).  Every key's answer is the oracle's."""
    pool, ids, hot, cold, shapes, _ = full_segments
    _assert_segments_fill(shapes[1])
    held = pool[np.concatenate([hot[1:], cold])]
    ob = oracle.OracleBloom(2**28, 7)
    ob.add_keys(held)
    blm = pa.BloomFilter(**HEADLINE)
    blm.add_many(_dev(held))
    assert np.array_equal(_table(blm), ob.bloom)
    probe = pool[ids]
    want = ob.check_keys(probe).astype(np.uint8)
    assert int(want[ids == hot[0]].max()) == 0                               # (hot key 0 is no false positive of this filter)
    blm.set_engine_option("bloom_lookup", 3)
    assert np.array_equal(_check(blm, probe), want)


def test_full_segment_weighted_cms_add_spills_fields_with_their_weights(pa, oracle, N, keys):
    """k_part_bins<PayWeightSmall>, CountMinSketch 2^20 x 5 (160 slices of 2^15 cells), eight tiles of 1408 keys per workgroup, weights 1 .. 7:
    a field that leaves through the exact fallback -- from a full segment or from the flush -- adds its own weight to its own cell"""
    per_wg, nwg, tk = 8, 512, 1408
    n = per_wg * nwg * tk
    assert plan(n, 5, 160) == (tk, nwg, per_wg)
    cap, segcap = bin_capacity(5, 160, True), segment_capacity(n, 5, 160)
    pool = keys[:8192]
    idx = cms_indices(pool, 5, 2**20)
    ids, hot, cold = _full_segment_batch((idx >> np.uint64(15)).astype(np.int64), per_wg, nwg, tk, cap, segcap)
    _assert_segments_fill(spills(idx, 160, 15, cap, True, ids=ids, segcap=segcap), after=False)   # (a full bin of 14 groups a tile fills 103 in the eighth)
    batch, w = pool[ids], oracle.gen_weights(1000, n)
    N.set_option("cms_small_weights", 2)                       # the compact format whatever the hint says
    cms = pa.CountMinSketch(width=2**20, depth=5)
    cms.add_many(_dev(batch), _dev(w))
    oc = oracle.OracleCMS(2**20, 5)
    oc.add_keys(batch, w)
    assert np.array_equal(np.frombuffer(bytes(cms._bins), dtype=np.int32), oc.bins)
    assert cms.elements_added == oc.els_added
