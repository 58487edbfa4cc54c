"""CuckooFilter without a GPU: the exported names, constructor and setter errors with the reference's messages, the error-rate arithmetic,
the ``random`` state <-> word buffer round trip, the documented limits, and NativeLibraryError where a table would be needed."""

import random
import struct

import numpy as np
import pytest


def test_names_are_exported():
    import pyprobables_amd as pa

    assert {"CuckooFilter", "CuckooFilterFullError"} <= set(pa.__all__)
    assert issubclass(pa.CuckooFilterFullError, pa.ProbablesBaseException)
    assert str(pa.CuckooFilterFullError("The CuckooFilter is currently full")) == "The CuckooFilter is currently full"


def test_abi_prototypes_and_header_name_the_same_entries():
    from pathlib import Path

    from pyprobables_amd import _native as N

    names = {"psk_ck_triples", "psk_ck_check", "psk_ck_present", "psk_ck_place_sweep", "psk_ck_place_apply", "psk_ck_insert", "psk_ck_remove"}
    assert names <= set(N.PROTOTYPES)
    header = (Path(__file__).resolve().parent.parent / "include" / "psk.h").read_text()
    assert all(f"int {n}(" in header for n in names)


@pytest.mark.parametrize("kwargs", [dict(capacity=0), dict(capacity=-5), dict(bucket_size=0), dict(max_swaps=0), dict(capacity="10"), dict(bucket_size=None)])
def test_constructor_rejects_bad_sizes_with_the_reference_message(kwargs):
    import pyprobables_amd as pa

    with pytest.raises(pa.InitializationError) as ex:
        pa.CuckooFilter(**kwargs)
    assert str(ex.value) == "CuckooFilter: capacity, bucket_size, and max_swaps must be an integer greater than 0"


@pytest.mark.parametrize("size", [0, 5, -1])
def test_fingerprint_size_must_be_1_to_4(size):
    import pyprobables_amd as pa

    with pytest.raises(ValueError) as ex:
        pa.CuckooFilter(finger_size=size)
    assert str(ex.value) == "CuckooFilter: fingerprint size must be between 1 and 4"
    cf = pa.CuckooFilter()
    with pytest.raises(ValueError):
        cf.fingerprint_size = size
    assert cf.fingerprint_size == 4


def test_missing_file_is_an_initialization_error(tmp_path):
    import pyprobables_amd as pa

    with pytest.raises(pa.InitializationError) as ex:
        pa.CuckooFilter(filepath=tmp_path / "nothing.cko")
    assert str(ex.value) == "CuckooFilter: failed to load provided file"


def test_default_properties_and_str():
    import pyprobables_amd as pa

    cf = pa.CuckooFilter()
    assert (cf.capacity, cf.bucket_size, cf.max_swaps, cf.expansion_rate, cf.auto_expand) == (10000, 4, 500, 2, True)
    assert (cf.fingerprint_size, cf.fingerprint_size_bits, cf.elements_added, cf.load_factor()) == (4, 32, 0, 0.0)
    assert cf.error_rate == 1 / 2 ** (32 - 3)
    cf.auto_expand = 0
    cf.expansion_rate = 3
    assert cf.auto_expand is False and cf.expansion_rate == 3
    assert str(cf) == ("CuckooFilter:\n\tCapacity: 10000\n\tTotal Bins: 40000\n\tLoad Factor: 0.0%\n\tInserted Elements: 0\n"
                       "\tMax Swaps: 500\n\tExpansion Rate: 3\n\tAuto Expand: False")


@pytest.mark.parametrize("rate,B,bits", [(0.01, 4, 10), (0.00001, 4, 20), (0.05, 1, 6), (0.001, 8, 14), (0.3, 2, 4)])
def test_error_rate_arithmetic(rate, B, bits):
    import math

    import pyprobables_amd as pa

    cf = pa.CuckooFilter.init_error_rate(rate, capacity=100, bucket_size=B)
    assert bits == int(math.ceil(math.log2(1.0 / rate) + math.log2(B) + 1))  # cuckoo.py:522-524
    assert (cf.fingerprint_size_bits, cf.fingerprint_size, cf.error_rate) == (bits, math.ceil(bits / 8), rate)
    plain = pa.CuckooFilter(bucket_size=B, finger_size=2)
    assert plain.error_rate == float(1 / (2 ** (16 - (math.log2(B) + 1))))  # cuckoo.py:518-520


def test_documented_limits():
    import pyprobables_amd as pa

    with pytest.raises(pa.NotSupportedError, match="hash_function"):
        pa.CuckooFilter(hash_function=lambda key: 5)
    with pytest.raises(pa.NotSupportedError, match="32 bits"):
        pa.CuckooFilter.init_error_rate(1e-12)  # 43 fingerprint bits
    with pytest.raises(pa.NotSupportedError, match="bucket_size"):
        pa.CuckooFilter(bucket_size=33)
    assert pa.CuckooFilter(bucket_size=32, hash_function=pa.fnv_1a).bucket_size == 32


def test_random_state_round_trip():
    from pyprobables_amd.cuckoo import state_to_words, words_to_state

    for seed in (0, 1, 2**40):
        random.seed(seed)
        random.gauss(0, 1)  # leaves a gauss_next behind, which the words do not carry
        for _ in range(seed % 7):
            random.random()
        state = random.getstate()
        words = state_to_words(state)
        assert words.dtype == np.uint32 and words.shape == (625,) and words[624] == state[1][624]
        assert words_to_state(words, state) == state
        random.setstate(words_to_state(words.copy(), state))
        assert random.getstate() == state
    with pytest.raises(ValueError):
        words_to_state(np.zeros(624, dtype=np.uint32), state)
    with pytest.raises(ValueError):
        state_to_words((2, (0,) * 625, None))


def test_load_parses_the_footer_and_drops_zero_entries_without_a_device():
    import pyprobables_amd as pa

    rows = [[7, 0, 9], [0, 0, 0], [0, 0, 4], [1, 2, 3]]
    data = b"".join(struct.pack("<3I", *r) for r in rows) + struct.pack("II", 3, 25)
    cf = pa.CuckooFilter.frombytes(data, error_rate=0.01)
    assert (cf.capacity, cf.bucket_size, cf.max_swaps, cf.elements_added) == (4, 3, 25, 6)
    assert cf.fingerprint_size_bits == 10 and cf.error_rate == 0.01
    want = b"".join(struct.pack("<3I", *r) for r in [[7, 9, 0], [0, 0, 0], [4, 0, 0], [1, 2, 3]]) + struct.pack("II", 3, 25)
    assert bytes(cf) == want


def test_no_device_no_table(monkeypatch):
    import pyprobables_amd as pa
    from pyprobables_amd import _native as N

    monkeypatch.setattr(N, "device_count", lambda: 0)  # (what a machine without a GPU reports)
    cf = pa.CuckooFilter(capacity=16)
    for call in (lambda: cf.add("a"), lambda: cf.check("a"), lambda: "a" in cf, lambda: cf.remove("a"), lambda: cf.add_many(["a", "b"]), lambda: cf.expand(),
                 lambda: cf.buckets, lambda: cf.buckets_tensor, lambda: cf.fill_tensor):
        with pytest.raises(N.NativeLibraryError):
            call()
    assert cf.elements_added == 0
