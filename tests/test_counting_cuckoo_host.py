"""CountingCuckooFilter without a GPU: the exported names, the C ABI's declarations, constructor and setter errors with the reference's
messages, properties and ``__str__``, the export format (a fixture's export through ``frombytes`` and back), what a load drops and what
it rejects, and NativeLibraryError where a table would be needed."""

import json
import struct
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import counting_cuckoo_model as M  # noqa: E402

CASES = json.loads((ROOT / "tests" / "golden" / "golden_counting_cuckoo.json").read_text())["cases"]
ENTRIES = {"psk_cck_check", "psk_cck_present", "psk_cck_place_apply", "psk_cck_insert", "psk_cck_add_counts", "psk_cck_remove"}


def test_names_are_exported():
    import pyprobables_amd as pa

    assert {"CountingCuckooFilter", "CountingCuckooBin", "CuckooFilterFullError"} <= set(pa.__all__)
    assert issubclass(pa.CountingCuckooFilter, pa.CuckooFilter)
    b = pa.CountingCuckooBin(7, 3)
    assert (b.finger, b.count) == (7, 3) and 7 in b and 3 not in b and b == pa.CountingCuckooBin(7, 3) and b != pa.CountingCuckooBin(7, 4)
    assert str(b) == "(fingerprint:7 count:3)"


def test_abi_prototypes_and_header_name_the_same_entries():
    from pyprobables_amd import _native as N
    from pyprobables_amd import build as B

    assert ENTRIES <= set(N.PROTOTYPES)
    header = (ROOT / "include" / "psk.h").read_text()
    assert all(f"int {n}(" in header for n in ENTRIES)
    assert "CountingCuckooFilter" in header
    assert "psk_counting_cuckoo.hip" in B.PLAIN_SOURCES
    # every argument the header declares has its ctypes type
    for name in ENTRIES:
        decl = header[header.index(f"int {name}("):]
        assert decl[: decl.index(");")].count(",") + 1 == len(N.PROTOTYPES[name][1]), name


@pytest.mark.parametrize("kwargs", [dict(capacity=0), dict(bucket_size=0), dict(max_swaps=0), dict(capacity="10")])
def test_constructor_rejects_bad_sizes_with_the_reference_message(kwargs):
    import pyprobables_amd as pa

    with pytest.raises(pa.InitializationError) as ex:
        pa.CountingCuckooFilter(**kwargs)
    assert str(ex.value) == "CuckooFilter: capacity, bucket_size, and max_swaps must be an integer greater than 0"


def test_setter_and_file_messages(tmp_path):
    import pyprobables_amd as pa

    with pytest.raises(ValueError) as ex:
        pa.CountingCuckooFilter(finger_size=5)
    assert str(ex.value) == "CountingCuckooFilter: fingerprint size must be between 1 and 4"
    with pytest.raises(pa.InitializationError) as ex:
        pa.CountingCuckooFilter(filepath=tmp_path / "nothing.cck")
    assert str(ex.value) == "CuckooFilter: failed to load provided file"
    with pytest.raises(pa.NotSupportedError, match="hash_function"):
        pa.CountingCuckooFilter(hash_function=lambda key: 5)
    with pytest.raises(pa.NotSupportedError, match="bucket_size"):
        pa.CountingCuckooFilter(bucket_size=33)


def test_default_properties_and_str():
    import pyprobables_amd as pa

    cf = pa.CountingCuckooFilter()
    assert (cf.capacity, cf.bucket_size, cf.max_swaps, cf.expansion_rate, cf.auto_expand) == (10000, 4, 500, 2, True)
    assert (cf.fingerprint_size, cf.fingerprint_size_bits, cf.elements_added, cf.unique_elements, cf.load_factor()) == (4, 32, 0, 0, 0.0)
    assert cf.error_rate == 1 / 2 ** (32 - 3)
    assert str(cf) == ("CountingCuckooFilter:\n\tCapacity: 10000\n\tTotal Bins: 40000\n\tLoad Factor: 0.0%\n\tInserted Elements: 0\n"
                       "\tMax Swaps: 500\n\tExpansion Rate: 2\n\tAuto Expand: True")
    odd = pa.CountingCuckooFilter.init_error_rate(0.01, capacity=100, bucket_size=4)
    assert isinstance(odd, pa.CountingCuckooFilter) and (odd.fingerprint_size_bits, odd.error_rate) == (10, 0.01)


@pytest.mark.parametrize("case", [c for c in CASES if "export_hex" in c], ids=lambda c: c["name"])
def test_fixture_export_round_trip_without_a_device(case, tmp_path):
    """``frombytes`` -> ``bytes()`` of an export the reference wrote: the same bytes unless it holds fingerprint 0, which a load drops
    (then: what the model makes of it); both totals are the reloaded table's"""
    import pyprobables_amd as pa

    data = bytes.fromhex(case["export_hex"])
    back = M.CountingCuckooModel().load(data)
    cf = pa.CountingCuckooFilter.frombytes(data)
    assert bytes(cf) == back.export()
    if "zero_fingerprint" not in case["tags"]:
        assert bytes(cf) == data
    assert (cf.capacity, cf.bucket_size, cf.max_swaps) == (back.capacity, back.bucket_size, back.max_swaps) == (case["capacity"], case["params"]["bucket_size"], case["params"]["max_swaps"])
    assert (cf.elements_added, cf.unique_elements) == (back.elements_added, back.unique_elements)
    assert cf.load_factor() == back.unique_elements / (back.capacity * back.bucket_size)
    path = tmp_path / "f.cck"
    cf.export(path)
    again = pa.CountingCuckooFilter.load_error_rate(0.01, path)
    assert bytes(again) == bytes(cf) and again.fingerprint_size_bits == again._calc_fingerprint_size() and again.error_rate == 0.01
    assert bytes(pa.CountingCuckooFilter(filepath=path)) == bytes(cf)


def pairs(rows, B, max_swaps=25):
    return b"".join(struct.pack(f"<{2 * B}I", *[w for pair in r for w in pair]) for r in rows) + struct.pack("II", B, max_swaps)


def test_load_drops_zero_fingerprint_pairs_wherever_they_stand():
    import pyprobables_amd as pa

    rows = [[(7, 2), (0, 5), (9, 1)], [(0, 0), (0, 0), (0, 0)], [(0, 3), (0, 0), (4, 6)], [(1, 1), (2, 2), (3, 3)]]
    cf = pa.CountingCuckooFilter.frombytes(pairs(rows, 3), error_rate=0.01)
    assert (cf.capacity, cf.bucket_size, cf.max_swaps) == (4, 3, 25)
    assert (cf.elements_added, cf.unique_elements) == (2 + 1 + 6 + 1 + 2 + 3, 6)
    assert cf.fingerprint_size_bits == 10 and cf.error_rate == 0.01
    want = [[(7, 2), (9, 1), (0, 0)], [(0, 0)] * 3, [(4, 6), (0, 0), (0, 0)], [(1, 1), (2, 2), (3, 3)]]
    assert bytes(cf) == pairs(want, 3) == M.CountingCuckooModel().load(pairs(rows, 3)).export()


def test_load_rejects_a_fingerprint_with_count_zero():
    """the reference keeps such a bin and fails with OverflowError when it is removed; here the import is refused"""
    import pyprobables_amd as pa

    with pytest.raises(pa.InitializationError, match="count is 0"):
        pa.CountingCuckooFilter.frombytes(pairs([[(7, 2), (9, 0)], [(0, 0), (0, 0)]], 2))
    assert pa.CountingCuckooFilter.frombytes(pairs([[(7, 2), (0, 0)], [(0, 9), (0, 0)]], 2)).unique_elements == 1
    with pytest.raises(pa.InitializationError):
        pa.CountingCuckooFilter.frombytes(b"\x00\x00")


def test_no_device_no_table(monkeypatch):
    import pyprobables_amd as pa
    from pyprobables_amd import _native as N

    monkeypatch.setattr(N, "device_count", lambda: 0)  # (what a machine without a GPU reports)
    cf = pa.CountingCuckooFilter(capacity=16)
    for call in (lambda: cf.add("a"), lambda: cf.check("a"), lambda: "a" in cf, lambda: cf.remove("a"), lambda: cf.add_many(["a", "b"]), lambda: cf.expand(),
                 lambda: cf.check_many(["a"]), lambda: cf.remove_many(["a"]), lambda: cf.buckets, lambda: cf.bins_tensor, lambda: cf.fill_tensor):
        with pytest.raises(N.NativeLibraryError):
            call()
    assert (cf.elements_added, cf.unique_elements) == (0, 0)
