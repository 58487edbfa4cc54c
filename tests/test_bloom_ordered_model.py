"""The ordered Bloom batch's model (tests/bloom_ordered_model.py) against itself and against the real reference's recorded loop
(tests/golden/golden_bloom_ordered.json).  CPU only."""

import json
from pathlib import Path

import bloom_ordered_model as M

GOLDEN = json.loads((Path(__file__).parent / "golden" / "golden_bloom_ordered.json").read_text())
FOOTER_HEX = 40  # the QQf footer of export_hex()


def case_hashes(c, key):
    k = c["number_hashes"]
    return M.hashes_fnv(key, k) if c["hash"] == "fnv" else M.hashes_digest(key, k, c["hash"])


def case_keys(c):
    return [k if c["type"] == "str" else bytes.fromhex(k) for k in c["keys"]]


def case_start(c) -> set:
    return set() if c["start"] is None else M.table_from_bytes(bytes.fromhex(c["start"][:-FOOTER_HEX]), c["number_bits"])


def test_loop_equals_rule_on_every_3_key_stream_over_a_4_bit_table():
    n = 0
    for start, keys in M.exhaustive_cases():
        want = M.loop(start, keys)
        assert M.rule(start, keys) == want
        assert M.rule(start, keys, chunk=1) == want and M.rule(start, keys, chunk=2) == want  # any ordered cut
        seen_c, table_c, adds = M.loop_conditional(start, keys)
        assert (seen_c, table_c) == want and adds == want[0].count(0)  # the conditional loop: same flags, same table
        n += 1
    assert n == 65536


def test_model_equals_the_reference_recorded_loop():
    names = set()
    for c in GOLDEN["cases"]:
        m, k = c["number_bits"], c["number_hashes"]
        stream = [M.positions(case_hashes(c, key), m, k) for key in case_keys(c)]
        start = case_start(c)
        seen, table = M.loop(start, stream)
        assert seen == c["seen"], c["name"]
        assert M.table_bytes(table, m).hex() == c["export_hex"][:-FOOTER_HEX], c["name"]
        for chunk in (None, 1, 7, 100):
            assert M.rule(start, stream, chunk) == (seen, table), (c["name"], chunk)
        assert c["elements_added"] - c["elements_added_conditional"] == sum(seen)
        names.add(c["name"])
    assert names == {"overfull_m400_k4", "start_from_hex", "bytes_keys", "md5"}
    over = next(c for c in GOLDEN["cases"] if c["name"] == "overfull_m400_k4")
    assert (over["number_bits"], over["number_hashes"]) == (400, 4) and over["seen_at_first_occurrence"] > 0
