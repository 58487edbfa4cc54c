"""Deferred Bloom clear (option lazy_clear): psk_clear only marks a private table clear-pending; the next entry point that touches the
table sweeps it first, except the single-level partitioned insert, whose first apply stores its slices (pass 1's spills wait in a list).
Every case runs with lazy_clear = 1 and = 0 and must give identical tables and answers, equal to the oracle's."""

import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 0x5EED
BIG = dict(est_elements=28005615, false_positive_rate=0.01)   # m = 2^28, k = 7: the bench's filter (single-level partitioned insert)
MID = dict(est_elements=1_000_000, false_positive_rate=0.01)   # m ~ 9.6 Mbit (not a power of two)


@pytest.fixture(scope="module")
def pa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pyprobables_amd

    return pyprobables_amd


@pytest.fixture(autouse=True)
def _restore_option(pa):
    from pyprobables_amd import _native as N

    old = N.get_option("lazy_clear")
    yield
    N.set_option("lazy_clear", old)


def dev_keys(start, n):
    from pyprobables_amd import _native as N

    t = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
    N.check(N.lib().psk_gen_keys16(t.data_ptr(), start, n, SEED, 0, torch.cuda.current_stream().cuda_stream or None))
    return t


def table(blm) -> np.ndarray:
    return np.frombuffer(bytes(blm.bloom), dtype=np.uint8)


def both(fn):
    """run fn() with lazy_clear = 1 and = 0; the two results must be identical"""
    from pyprobables_amd import _native as N

    out = []
    for v in (1, 0):
        N.set_option("lazy_clear", v)
        out.append(fn())
        torch.cuda.synchronize()
    a, b = out
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    return a


def dirty(pa, cfg, n=300_000, start=10**9):
    blm = pa.BloomFilter(**cfg)
    blm.add_many(dev_keys(start, n))
    return blm


def test_option_is_listed_and_settable(pa):
    from pyprobables_amd import _native as N

    for v in (0, 1):
        N.set_option("lazy_clear", v)
        assert N.get_option("lazy_clear") == v


def test_clear_then_read_and_export_are_zero(pa):
    def run():
        blm = dirty(pa, BIG)
        blm.clear()
        t = table(blm)
        assert not t.any()
        assert blm._cnt_number_bits_set() == 0
        return [t[:4096], np.frombuffer(bytes(blm)[:4096], dtype=np.uint8)]

    both(run)


def test_clear_then_check_is_all_false(pa):
    def run():
        blm = dirty(pa, BIG)
        blm.clear()
        keys = dev_keys(10**9, 300_000)   # the keys that were in the table
        got = blm.check_many(keys).cpu().numpy()
        assert not got.any()
        small = blm.check_many(keys[:100]).cpu().numpy()
        assert not small.any()
        return [got, small, table(blm)]

    both(run)


def test_clear_then_small_adds(pa, oracle):
    def run():
        blm = dirty(pa, MID)
        blm.clear()
        keys = oracle.gen_keys16(0, 5_000)
        for k in keys[:50]:
            blm.add(bytes(k))                # per-key adds: host write-combined, direct kernel
        blm.add_many(dev_keys(50, 4_950))    # < 2^16 keys: direct kernel
        ob = oracle.OracleBloom(blm.number_bits, blm.number_hashes)
        ob.add_keys(keys)
        t = table(blm)
        assert np.array_equal(t, ob.bloom)
        return [t]

    both(run)


def test_clear_then_10M_insert_matches_oracle(pa, oracle):
    n = 10_000_000
    ob = oracle.OracleBloom(2**28, 7)
    ob.add_keys(oracle.gen_keys16(0, n))
    want = hashlib.sha256(ob.bloom.tobytes()).hexdigest()
    keys = dev_keys(0, n)

    def run():
        blm = dirty(pa, BIG, n=1_000_000)
        blm.clear()
        blm.add_many(keys)
        t = table(blm)
        assert hashlib.sha256(t.tobytes()).hexdigest() == want
        assert bool(blm.check_many(keys).all())
        return [t]

    both(run)


def test_clear_then_multi_round_insert(pa, oracle):
    from pyprobables_amd import _native as N

    n = 3_000_000
    keys = dev_keys(0, n)
    ob = oracle.OracleBloom(2**28, 7)
    ob.add_keys(oracle.gen_keys16(0, n))
    old = N.get_option("partition_max_keys")

    def run():
        blm = dirty(pa, BIG)
        blm.clear()
        N.set_option("partition_max_keys", 1 << 20)   # rounds of 2^20 keys: the first stores, the others read-modify-write
        try:
            blm.add_many(keys)
        finally:
            N.set_option("partition_max_keys", old)
        t = table(blm)
        assert np.array_equal(t, ob.bloom)
        return [t]

    both(run)


def test_clear_then_all_duplicates_batch(pa, oracle):
    """one key 4M times: nearly every probe overflows its segment and goes through pass 1's spill (the list, in store mode)"""
    n = 4_000_000
    one = dev_keys(7, 1)
    keys = one.expand(n, 16).contiguous()
    ob = oracle.OracleBloom(2**28, 7)
    ob.add_keys(oracle.gen_keys16(7, 1))

    def run():
        blm = dirty(pa, BIG)
        blm.clear()
        blm.add_many(keys)
        t = table(blm)
        assert np.array_equal(t, ob.bloom)
        assert int(np.unpackbits(t).sum()) == ob.bits_set()
        blm.clear()
        blm.add_many(keys[: n // 2])   # a second store-mode insert: the list was reset by the first one
        assert np.array_equal(table(blm), ob.bloom)
        return [t]

    both(run)


def test_table_tensor_after_clear_and_clear_while_exposed(pa, oracle):
    def run():
        blm = dirty(pa, BIG)
        blm.clear()
        t0 = blm.table_tensor.cpu().numpy()   # handing the table out runs the deferred clear first
        assert not t0.any()
        blm.add_many(dev_keys(0, 300_000))
        blm.clear()                           # exposed: cleared at once
        t1 = blm.table_tensor.cpu().numpy()
        assert not t1.any()
        blm._tab.written()                    # the holder is done: clears may be deferred again
        blm.add_many(dev_keys(0, 300_000))
        blm.clear()
        blm.add_many(dev_keys(0, 300_000))
        ob = oracle.OracleBloom(blm.number_bits, blm.number_hashes)
        ob.add_keys(oracle.gen_keys16(0, 300_000))
        t2 = blm.table_tensor.cpu().numpy().view(np.uint8)[: ob.bloom.size]
        assert np.array_equal(t2, ob.bloom)
        return [t0[:1024], t1[:1024], t2]

    both(run)


def test_set_algebra_after_clear(pa, oracle):
    n = 200_000

    def run():
        a, b = dirty(pa, MID), dirty(pa, MID, start=5 * 10**8)
        a.clear()
        b.clear()
        b.add_many(dev_keys(0, n))            # b: cleared, then filled; a: still clear-pending
        u, x = a.union(b), a.intersection(b)
        ob = oracle.OracleBloom(a.number_bits, a.number_hashes)
        ob.add_keys(oracle.gen_keys16(0, n))
        tu, tx = table(u), table(x)
        assert np.array_equal(tu, ob.bloom)
        assert not tx.any()
        assert a.jaccard_index(b) == 0.0
        return [tu, tx]

    both(run)


def test_expanding_bloom_after_clear(pa, oracle):
    n = 20_000

    def run():
        e = pa.ExpandingBloomFilter(est_elements=100_000, false_positive_rate=0.01)
        f = e._blooms[0]
        f.add_many(dev_keys(10**9, 50_000))
        f.clear()                             # the stack's filter is clear-pending; the index ops take its tensor
        e.add_many(dev_keys(0, n))
        ob = oracle.OracleBloom(f.number_bits, f.number_hashes)
        ob.add_keys(oracle.gen_keys16(0, n))
        t = table(f)
        assert np.array_equal(t, ob.bloom)
        assert bool(e.check_many(dev_keys(0, n)).all())
        return [t]

    both(run)


def test_two_clears_in_a_row_and_clear_insert_clear_check(pa, oracle):
    n = 1_000_000
    keys = dev_keys(0, n)

    def run():
        blm = dirty(pa, BIG)
        blm.clear()
        blm.clear()
        assert not table(blm).any()
        blm.clear()
        blm.clear()
        blm.add_many(keys)
        ob = oracle.OracleBloom(2**28, 7)
        ob.add_keys(oracle.gen_keys16(0, n))
        t = table(blm)
        assert np.array_equal(t, ob.bloom)
        blm.clear()
        got = blm.check_many(keys).cpu().numpy()
        assert not got.any()
        bits, hits = blm.check_many_bits(keys)
        assert int(hits) == 0
        blm.add_many(keys)
        blm.clear()
        blm.check_many_begin(keys)
        got2 = blm.check_many_finish().cpu().numpy()
        assert not got2.any()
        return [t, got, got2]

    both(run)
