"""k_part_bins (psk_part_bins.hpp) loads a tile's keys one tile ahead into registers of their own (knext[] / wnext[]) and hands them over in
front of barrier 1.  That changes no result, so every table, answer and tally must equal the plain-C oracle's.  (The last test pins how the
automatic lookup scheme follows the tallies a handle's calls publish: the sequence a by-value publish number -- measured, no gain, not
kept: NOTES 18 -- would have had to preserve.)  The batches are sized from the geometry the engine reports (per-sketch options pass1_bins_tile_keys /
pass1_bins_workgroups / pass1_bins_launches) to pin what a wrong hand-over would break: with even_tiles = 0 a tile is 1536 keys and the
grid at most 512 workgroups, so
  N1 = 512 x 1536 + 1      workgroup 0 runs two tiles, every other workgroup one,
  N2 = 2 x 512 x 1536 + 1  workgroup 0 runs three tiles, every other workgroup two (both parities of a loop unrolled by two),
both one more than a whole number of rounds of the grid, the last tile holding ONE key (a workgroup's last prefetch is clamped to that key);
  NS = 3 x 1536 + 1        four tiles: fewer tiles than the 512 workgroups.  The launcher never starts a workgroup without a tile (its grid is
                           min(512, tiles), launch_scatter_bins), so "a workgroup that runs no tile" cannot occur: the test pins the grid.
Table: m = 2^24 bits, k = 7 (256 slices of 2^16 bits: the headline's bins at 1/16 of its table).  bloom.py:241-272, countminsketch.py:267-288,
hashes.py:71-103."""

import numpy as np
import pytest

from bins_carry_model import bin_capacity, fnv_indices, plan, spills

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILE, WGS = 1536, 512            # kBinThreads x kBinKpt keys per full tile; two workgroups on each of 256 CUs
N1 = WGS * TILE + 1
N2 = 2 * WGS * TILE + 1
NS = 3 * TILE + 1
M, K = 1 << 24, 7
EST, FPR = 1_754_141, 0.0101     # est_elements / false_positive_rate whose filter has exactly 2^24 bits and 7 hashes (the est fixture checks)


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
    N.set_option("partition_min_keys", 1)
    N.set_option("pass1_bins", 1)
    N.set_option("even_tiles", 0)
    yield N
    for k, v in zip(names, old):
        N.set_option(k, v)


@pytest.fixture(scope="module")
def est(oracle):
    assert oracle.bloom_params(EST, FPR)[1:] == (K, M)
    return EST


@pytest.fixture(scope="module")
def keys(oracle):
    return oracle.gen_keys16(8000, N2)   # (none of the four keys the lookup test leaves out is a false positive of the filter without it)


@pytest.fixture(scope="module")
def keys8():
    return np.random.default_rng(11).integers(0, 256, size=(N2, 8), dtype=np.uint8)


@pytest.fixture(scope="module")
def absent(oracle):
    return oracle.gen_keys16(3_500_000_000, 100_000)


def _oracle_tables(oracle, kk):
    """the oracle's filters of kk[:NS], kk[:N1] and kk[:N2], each built on the one before (read-only: shared)"""
    out, ob, done = {}, oracle.OracleBloom(M, K), 0
    for n in (NS, N1, N2):
        ob.add_keys(kk[done:n])
        out[n], done = ob.bloom.copy(), n
    return out


@pytest.fixture(scope="module")
def tables16(oracle, keys):
    return _oracle_tables(oracle, keys)


@pytest.fixture(scope="module")
def tables8(oracle, keys8):
    return _oracle_tables(oracle, keys8)


@pytest.fixture(scope="module")
def all_but_first(oracle, keys):
    """the oracle's filter of keys[1:N2] and how many of key 0's probes find their bit clear in it"""
    ob = oracle.OracleBloom(M, K)
    ob.add_keys(keys[1:N2])
    return ob, _clear_probes(ob, keys[:1])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _table(f):
    return np.frombuffer(bytes(f.bloom), dtype=np.uint8)


def _check(blm, probe):
    return blm.check_many(_dev(probe)).cpu().numpy().astype(np.uint8)


def _clear_probes(ob, kk):
    """probes of the 16-byte keys kk that find their bit clear in the oracle's table (every probe of a key counts, as the tile flags tally)"""
    idx = fnv_indices(kk, ob.k, ob.m).astype(np.int64)
    return int(idx.size - ((ob.bloom[idx >> 3] >> (idx & 7)) & 1).sum())


def _geometry(f):
    return f.get_engine_option("pass1_bins_tile_keys"), f.get_engine_option("pass1_bins_workgroups")


def _expect_grid(n):
    """(tile, workgroups) of a bins launch over n keys with even_tiles = 0, and the tiles workgroup 0 / the last workgroup run"""
    tk, nwg, _ = plan(n, K, 256, 0)
    ntiles = -(-n // tk)
    return (tk, nwg), (-(-ntiles // nwg), -(-(ntiles - (nwg - 1)) // nwg))


def test_the_batches_are_what_the_docstring_says():
    assert _expect_grid(N1) == ((TILE, WGS), (2, 1)) and _expect_grid(N2) == ((TILE, WGS), (3, 2)) and _expect_grid(NS) == ((TILE, 4), (1, 1))
    assert N1 % TILE == 1 and N2 % TILE == 1 and NS % TILE == 1 and (N1 - 1) % (WGS * TILE) == 0 and (N2 - 1) % (WGS * TILE) == 0


@pytest.mark.parametrize("n", [NS, N1, N2])
@pytest.mark.parametrize("key_bytes", [16, 8])
def test_bloom_insert_builds_the_oracles_table(pa, N, est, keys, keys8, tables16, tables8, key_bytes, n):
    kk, tabs = (keys, tables16) if key_bytes == 16 else (keys8, tables8)
    blm = pa.BloomFilter(est_elements=est, false_positive_rate=FPR)
    assert (blm.number_bits, blm.number_hashes) == (M, K)
    blm.add_many(_dev(kk[:n]))
    assert blm.get_engine_option("pass1_bins_launches") == 1 and _geometry(blm) == _expect_grid(n)[0]
    assert np.array_equal(_table(blm), tabs[n])


@pytest.mark.parametrize("which", ["first key of tile 0", "last key of tile 0", "first key of workgroup 0's second tile", "the very last key"])
def test_tile_flag_lookup_finds_the_one_absent_key(pa, oracle, N, est, keys, all_but_first, which):
    """all keys but one inserted, all N2 looked up through the tile flags: the answers are the oracle's for every key and the tally is the
    oracle's count of the absent key's clear probes (every other probe finds its bit set; a probe pass 1 tests itself because its bin is
    full is not tallied: 7 probes among 11 M, of which a few dozen meet a full bin)"""
    a = {"first key of tile 0": 0, "last key of tile 0": TILE - 1, "first key of workgroup 0's second tile": WGS * TILE, "the very last key": N2 - 1}[which]
    if a == 0:
        ob, clear = all_but_first
    else:
        ob = oracle.OracleBloom(M, K)
        ob.add_keys(np.delete(keys, a, axis=0))
        clear = _clear_probes(ob, keys[a:a + 1])
    want = ob.check_keys(keys).astype(np.uint8)
    assert clear > 0 and want[a] == 0 and int((want == 0).sum()) == 1
    blm = pa.BloomFilter(est_elements=est, false_positive_rate=FPR)
    blm.add_many(_dev(np.delete(keys, a, axis=0)))
    assert np.array_equal(_table(blm), ob.bloom)
    blm.set_engine_option("bloom_lookup", 3)
    got = _check(blm, keys)
    assert blm.get_engine_option("pass1_bins_launches") == 2 and _geometry(blm) == (TILE, WGS)
    assert np.array_equal(got, want)
    assert blm.get_engine_option("bloom_lookup_misses") == clear


def test_weighted_cms_add_keeps_each_weight_with_its_key(pa, oracle, N, keys):
    """weights 0 .. 15 in the compact format (PayWeightSmall: the weights travel with the keys, wnext[]): a key's weight differs from the
    weight at the same place of the tile before and of the tile behind, so a weight handed to the wrong tile's key changes a counter"""
    i = np.arange(N2, dtype=np.int64)
    w = ((i + 5 * (i // TILE)) % 16).astype(np.int32)
    assert (w[TILE:] != w[:-TILE]).all() and set(w.tolist()) == set(range(16))
    N.set_option("cms_small_weights", 2)
    cms = pa.CountMinSketch(width=2**20, depth=5)
    cms.add_many(_dev(keys), _dev(w))
    assert cms.get_engine_option("pass1_bins_launches") == 1 and _geometry(cms) == (TILE, WGS)
    oc = oracle.OracleCMS(2**20, 5)
    oc.add_keys(keys, w)
    assert np.array_equal(np.frombuffer(bytes(cms._bins), dtype=np.int32), oc.bins)
    assert cms.elements_added == oc.els_added == int(w.sum())


def test_two_tile_flag_lookups_in_a_row_publish_their_own_tallies(pa, oracle, N, est, keys, absent, all_but_first):
    """The automatic scheme ("bloom_lookup" = 2, choose_scheme in psk_part_bloom_check.hip) reads the tally the previous call published and
    tells a new one from the one it has seen by the launch number in the pinned page.  The expected schemes follow from its thresholds:
      call 1  nothing published yet                                   -> keyed probes (the handle's first mode)
      call 2  call 1 missed nothing: one clean call                   -> keyed probes (tile flags need two clean calls in a row)
      call 3  two clean calls                                         -> tile flags; one absent key among N2: its clear probes are the tally,
                                                                         at most 7 / (N2 x 7) <= 1e-6 of the probes: a third clean call
      call 4  three clean calls                                       -> tile flags; 60 % of 100 000 keys absent: the tally is their clear
                                                                         probes, more than 0.22 of the probes
      call 5  the call before was not clean and missed > 0.22         -> the return trip, which tallies KEYS answered absent
    A tile-flag lookup is the only lookup whose pass 1 goes through the bins, so pass1_bins_launches tells which calls took it; a number in
    the page that did not change with every launch would keep the handle on keyed probes, a tally of another call would not match."""
    ob, clear0 = all_but_first
    blm = pa.BloomFilter(est_elements=est, false_positive_rate=FPR)
    blm.add_many(_dev(keys[1:N2]))
    blm.set_engine_option("bloom_lookup", 2)
    launches = lambda: blm.get_engine_option("pass1_bins_launches")   # noqa: E731
    assert launches() == 1 and blm.get_engine_option("bloom_lookup_misses") == -1
    for _ in range(2):                                                # calls 1 and 2: keyed
        assert _check(blm, keys[1:100_001]).all()
        assert launches() == 1 and blm.get_engine_option("bloom_lookup_misses") == 0
    assert 0 < clear0 <= K and clear0 <= 1e-6 * N2 * K
    assert np.array_equal(_check(blm, keys), ob.check_keys(keys).astype(np.uint8))            # call 3
    assert launches() == 2 and blm.get_engine_option("bloom_lookup_misses") == clear0
    probe = keys[1:100_001].copy()
    probe[np.arange(100_000) % 5 < 3] = absent[np.arange(100_000) % 5 < 3]
    shape = spills(fnv_indices(probe, K, M), 256, 16, bin_capacity(K, 256, True), True, even_tiles=0, tile_tag=True)
    assert shape["bin_spills"] == 0, shape                            # (no probe of this batch is tested by pass 1 itself: the tally is exact)
    clear4 = _clear_probes(ob, probe)
    assert clear4 > 0.22 * probe.shape[0] * K
    assert np.array_equal(_check(blm, probe), ob.check_keys(probe).astype(np.uint8))          # call 4
    assert launches() == 3 and blm.get_engine_option("bloom_lookup_misses") == clear4
    probe5 = keys[200_001:300_001].copy()
    probe5[::3] = absent[: probe5[::3].shape[0]]
    want5 = ob.check_keys(probe5).astype(np.uint8)
    assert np.array_equal(_check(blm, probe5), want5)                                         # call 5
    assert launches() == 3
    assert blm.get_engine_option("bloom_lookup_misses") == int((want5 == 0).sum()) != _clear_probes(ob, probe5)
