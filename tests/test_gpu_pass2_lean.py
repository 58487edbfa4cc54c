"""Pass 2 of the Bloom step without the per-probe predication (k_bloom_apply, k_bloom_test_flag in psk_partition.hpp): where pass 1 goes
through the bins of a Bloom insert or of a tile-flag lookup, the slots of a short group past its counts hold a COPY of the group's first
probe (PartGeom::dup_pads) instead of the all-ones pad, so pass 2 may OR / test all six fields of every group it loaded; the counts are
written as before and the rare path of the lookup still goes by them.  An OR or a test of the same bit twice changes nothing: every table,
every answer, every flag-driven re-check and the miss tally must equal the plain-C oracle's.  Streams whose consumers add (CountingBloomFilter
unit updates) or that k_part_scatter writes (ragged keys, tables of more than 1536 slices) keep their pads.  bloom.py:241-272,
countingbloom.py:135-155, hashes.py:71-103."""

import numpy as np
import pytest

from bins_carry_model import bin_capacity, fnv_indices, plan, spills

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

    names = ("partition", "partition_min_keys", "pass1_bins", "bloom_lookup", "even_tiles")
    old = [N.get_option(k) for k in names]
    N.set_option("partition", 1)
    N.set_option("pass1_bins", 1)
    yield N
    for k, v in zip(names, old):
        N.set_option(k, v)


@pytest.fixture(scope="module")
def keys(oracle):
    return oracle.gen_keys16(1000, N3 + 1)


@pytest.fixture(scope="module")
def absent(oracle):
    return oracle.gen_keys16(3_000_000_000, 4096)


@pytest.fixture(scope="module")
def headline_table(oracle, keys):
    """the oracle's m = 2^28, k = 7 filter of all N3 + 1 keys (read-only: shared)"""
    ob = oracle.OracleBloom(2**28, 7)
    ob.add_keys(keys)
    return ob


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _table(f, dtype=np.uint8):
    return np.frombuffer(bytes(f.bloom), dtype=dtype)


def _check(blm, probe):
    return blm.check_many(_dev(probe)).cpu().numpy().astype(np.uint8)


def test_insert_whole_table_with_one_padded_group_per_segment(pa, N, keys, headline_table):
    """3 x 512 x 1536 + 1 keys into the headline geometry: every workgroup flushes one padded group per segment behind its last tile.  The
    WHOLE table equals the oracle's: a copied probe sets nothing new, and neither bit 0 nor bit 2^20 - 1 of a slice (what a zero or an
    all-ones pad field would address) is set unless a key sets it."""
    n = N3 + 1
    assert plan(n, 7, 256)[1:] == (512, 4)
    blm = pa.BloomFilter(**HEADLINE)
    blm.add_many(_dev(keys[:n]))
    got = _table(blm)
    assert np.array_equal(got, headline_table.bloom)
    per = (1 << 20) // 8                                         # bytes per slice: its bit 0 and its bit 2^20 - 1
    first, last = got[::per] & 1, got[per - 1::per] >> 7
    assert first.shape == (256,) and last.shape == (256,)
    assert np.array_equal(first, headline_table.bloom[::per] & 1) and np.array_equal(last, headline_table.bloom[per - 1::per] >> 7)
    assert int(first.sum()) < 64 and int(last.sum()) < 64       # (at 6 % fill most slices leave both clear: a pad that leaked would show)


@pytest.mark.parametrize("est,fpr,k,m,shift", [
    (100_000_000, 0.5, 1, 144269505, 19),    # 276 slices: 4.4 probes per bin and 1216-key tile -- most groups are short
    (60_000_000, 0.25, 2, 173123405, 19),    # 331 slices: 7.3
])
def test_thin_bins_short_groups_everywhere(pa, oracle, N, keys, absent, est, fpr, k, m, shift):
    """the two thin-bin geometries: most groups that reach pass 2 are short, so most of what the fast paths OR and test are copies.  Table,
    answers (absent keys in nearly every tile: the rare path, the flags, the re-check) equal the oracle's."""
    n = N3 + 1
    blm = pa.BloomFilter(est_elements=est, false_positive_rate=fpr)
    assert (blm.number_hashes, blm.number_bits) == (k, m)
    nslices = -(-m // (1 << shift))
    shape = spills(fnv_indices(keys[:n], k, m), nslices, shift, bin_capacity(k, nslices, True), True)
    assert shape["thin"] > (0.6 if k == 1 else 0.2), shape
    blm.add_many(_dev(keys[:n]))
    ob = oracle.OracleBloom(m, k)
    ob.add_keys(keys[:n])
    assert np.array_equal(_table(blm), ob.bloom)
    probe = keys[:n].copy()
    probe[5::1000] = absent[: probe[5::1000].shape[0]]
    want = ob.check_keys(probe).astype(np.uint8)
    assert 0 < int((want == 0).sum())
    blm.set_engine_option("bloom_lookup", 3)
    assert np.array_equal(_check(blm, probe), want)
    assert bool(blm.check_many(_dev(keys[:n])).all())


def test_empty_filter_every_probe_misses_and_copies_are_not_counted(pa, N, keys):
    """a tile-flag lookup into an empty filter: every answer is False, and the tally of probes that found their bit clear is exactly n x k --
    a copy in a short group's spare slots misses too and is not counted (the rare path masks with the counts).  (A probe that met a full
    bin is tested by pass 1's fallback, which does not tally: the host model says these keys fill no bin.)"""
    n = N3 + 1
    shape = spills(fnv_indices(keys[:n], 7, 2**28), 256, 20, bin_capacity(7, 256, True), True, tile_tag=True)
    assert shape["bin_spills"] == 0 and shape["pads"] > 0, shape
    blm = pa.BloomFilter(**HEADLINE)
    blm.set_engine_option("bloom_lookup", 3)
    got = _check(blm, keys[:n])
    assert got.shape == (n,) and not got.any()
    assert blm.get_engine_option("bloom_lookup_misses") == n * 7


def test_all_present_lookup_tallies_nothing_and_flags_no_tile(pa, oracle, N, keys):
    """every key present: the fast path sends no group to the rare path -- the tally is 0 and no tile is flagged (a flagged tile is the only
    way a tally could stay 0 with a wrong answer, and every answer is True).  A filter that holds all keys but the first answers that one
    False and tallies exactly its clear probes: one group per clear probe took the rare path."""
    n = N3 + 1
    blm = pa.BloomFilter(**HEADLINE)
    blm.add_many(_dev(keys[:n]))
    blm.set_engine_option("bloom_lookup", 3)
    assert _check(blm, keys[:n]).all()
    assert blm.get_engine_option("bloom_lookup_misses") == 0
    part = pa.BloomFilter(**HEADLINE)
    part.add_many(_dev(keys[1:n]))
    ob = oracle.OracleBloom(2**28, 7)
    ob.add_keys(keys[1:n])
    assert np.array_equal(_table(part), ob.bloom)
    idx = fnv_indices(keys[:1], 7, 2**28)[0].astype(np.int64)
    clear = 7 - int(((ob.bloom[idx >> 3] >> (idx & 7)) & 1).sum())
    assert clear > 0                                              # (key 0 is no false positive of the filter without it)
    part.set_engine_option("bloom_lookup", 3)
    assert np.array_equal(_check(part, keys[:n]), ob.check_keys(keys[:n]).astype(np.uint8))
    assert part.get_engine_option("bloom_lookup_misses") == clear


def test_dense_walk_with_copies(pa, oracle, N, keys, absent):
    """700 001 keys into the headline geometry: one tile per workgroup, segments of ~7 groups -- the end-to-end (dense) walk of pass 2 with the
    bins' copies in every segment's last group"""
    n = 700_001
    blm = pa.BloomFilter(**HEADLINE)
    blm.add_many(_dev(keys[:n]))
    ob = oracle.OracleBloom(2**28, 7)
    ob.add_keys(keys[:n])
    assert np.array_equal(_table(blm), ob.bloom)
    probe = keys[:n].copy()
    probe[3::777] = absent[: probe[3::777].shape[0]]
    blm.set_engine_option("bloom_lookup", 3)
    assert np.array_equal(_check(blm, probe), ob.check_keys(probe).astype(np.uint8))


def test_dense_walk_two_thousand_slices(pa, oracle, N, keys, absent):
    """m = 2^31 (2048 slices: more than the bins serve, pass 1 is k_part_scatter and its pads stay all ones), a round of 2^21 keys: segments of
    a few groups, the dense walk.  The oracle's table and answers."""
    n = 1 << 21
    blm = pa.BloomFilter(est_elements=224044920, false_positive_rate=0.01)
    assert (blm.number_bits, blm.number_hashes) == (2**31, 7)
    blm.add_many(_dev(keys[:n]))
    ob = oracle.OracleBloom(2**31, 7)
    ob.add_keys(keys[:n])
    assert np.array_equal(_table(blm), ob.bloom)
    probe = keys[:n].copy()
    probe[9::1500] = absent[: probe[9::1500].shape[0]]
    want = ob.check_keys(probe).astype(np.uint8)
    for scheme in (3, 0):
        blm.set_engine_option("bloom_lookup", scheme)
        assert np.array_equal(_check(blm, probe), want)


def test_ragged_keys_keep_their_pads(pa, oracle, N):
    """keys of different lengths go through k_part_scatter (the bins take the 16- and 8-byte layouts only): all-ones pads, counted halves,
    today's pass 2.  Table and tile-flag answers against the oracle."""
    assert N.get_option("pass1_bins") == 1 and N.get_option("partition") == 1
    N.set_option("partition_min_keys", 1)
    rng = np.random.default_rng(8)
    ragged = [bytes(rng.integers(0, 256, size=int(l), dtype=np.uint8)) for l in rng.integers(1, 40, size=120_000)]
    blm = pa.BloomFilter(**HEADLINE)
    blm.add_many(ragged)
    ob = oracle.OracleBloom(2**28, 7)
    ob.add_varlen(ragged)
    assert np.array_equal(_table(blm), ob.bloom)
    probe = ragged[:60_000] + [b"absent-%d" % i for i in range(60_000)]
    blm.set_engine_option("bloom_lookup", 3)
    assert np.array_equal(np.asarray(blm.check_many(probe)).astype(np.uint8), ob.check_varlen(probe).astype(np.uint8))


def test_cbf_unit_adds_through_the_bins_get_no_copies(pa, oracle, N, keys):
    """a CountingBloomFilter unit add goes through the bins with the SAME probe groups (countingbloom.py:135-155): a copied probe there would
    count twice, so these streams keep their pads -- the counters equal the oracle's"""
    assert N.get_option("pass1_bins") == 1 and N.get_option("partition") == 1
    N.set_option("partition_min_keys", 1)
    n = 600_001
    cbf = pa.CountingBloomFilter(est_elements=2_000_000, false_positive_rate=0.01)   # 1.9e7 counters, k = 7: 32-bit slices
    cbf.add_many(_dev(keys[:n]))
    cbf.add_many(_dev(keys[: n // 3]))
    ocb = oracle.OracleCBF(cbf.number_bits, cbf.number_hashes)
    ocb.update_keys(keys[:n])
    ocb.update_keys(keys[: n // 3])
    assert np.array_equal(_table(cbf, np.uint32), ocb.bloom)
    assert cbf.elements_added == ocb.els_added
