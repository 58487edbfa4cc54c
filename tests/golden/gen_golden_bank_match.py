#!/usr/bin/env python3
"""Generate tests/golden/golden_bank_match.json by running the REAL reference's BloomFilter (pyprobables v0.7.0,
probables/blooms/bloom.py:234-272) once per filter of a bank of 70 filters and asking EVERY filter about every probe:
``BloomFilterBank.match_many`` must answer, per key, exactly the set of filters f with ``key in blm[f]``.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_bank_match.py [/root/reference [output file]]

Data only.  70 filters cross the 32- and 64-column word seams of a slice row and leave pad columns 70..127.  Per geometry (both overfilled,
so that false positives occur): the constructor's arguments, number_bits / number_hashes, a pool of keys (["s", text] for str, ["b", hex]
for bytes: mixed, code points above 255, the empty key), per filter the pool indices sent to it, in the order of their add() -- filter 41
gets nothing, pool key 0 goes to three filters --, 60 absent keys, and per probe (every pool key, then every absent key) the reference's answers of all 70 filters
as one hex mask (bit f of the little-endian integer = ``probe in blm[f]``), with the number of false-positive (probe, filter) pairs.
"""

import json
import random
import sys
from pathlib import Path

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

import probables  # noqa: E402
from probables import BloomFilter  # noqa: E402

FILTERS = 70
EMPTY_FILTER = 41
THREE = (0, 33, 69)  # pool key 0 goes to these three filters
# (est_elements, false_positive_rate, keys per filter): overfilled, as in gen_golden_bank.py
GEOMETRIES = [(10, 0.05, 14), (100, 0.01, 120)]
POOL = (96, 300)     # pool keys per geometry: filter f gets `per_filter` of them, chosen at random
ABSENT = 60


def pool_key(g, i):
    if i == 1:
        return ""
    if i % 4 == 0:
        return f"m{g}-bytes-{i}".encode() + bytes([i % 256, 255 - i % 256])[: i % 3]
    if i % 4 == 2:
        return f"m{g}-λ€-{i}" + "\U0001f600" * (i % 2)
    return f"m{g}-key-{i}" + "x" * (i % 7)


def enc(key):
    return ["s", key] if isinstance(key, str) else ["b", key.hex()]


def run(g, est, fpr, per_filter):
    rng = random.Random(7000 + g)
    pool = [pool_key(g, i) for i in range(POOL[g])]
    stream = []
    for f in range(FILTERS):
        if f == EMPTY_FILTER:
            continue
        stream += [(i, f) for i in rng.sample(range(1, len(pool)), per_filter)]
    stream += [(0, f) for f in THREE]
    rng.shuffle(stream)
    blms = [BloomFilter(est, fpr) for _ in range(FILTERS)]
    sent = [set() for _ in range(FILTERS)]
    for i, f in stream:
        blms[f].add(pool[i])
        sent[f].add(i)
    absent = [f"absent-m{g}-{i}" if i % 2 else f"absent-m{g}-{i}".encode() for i in range(ABSENT)]
    masks, fps, none, three = [], 0, 0, 0
    for pi, key in enumerate(pool + absent):
        v = 0
        for f in range(FILTERS):
            a = blms[f].check(key)
            was_sent = pi < len(pool) and pi in sent[f]
            assert a or not was_sent
            fps += int(a and not was_sent)
            v |= int(a) << f
        assert not (v >> EMPTY_FILTER) & 1
        none += v == 0
        three += bin(v).count("1") >= 3
        masks.append(v.to_bytes((FILTERS + 7) // 8, "little").hex())
    assert all((int.from_bytes(bytes.fromhex(masks[0]), "little") >> f) & 1 for f in THREE)
    return {"est": est, "fpr": fpr, "filters": FILTERS, "number_bits": blms[0].number_bits, "number_hashes": blms[0].number_hashes,
            "pool": [enc(k) for k in pool], "sent": [[i for i, f2 in stream if f2 == f] for f in range(FILTERS)], "absent": [enc(k) for k in absent], "masks": masks,
            "false_positives": fps, "match_none": int(none), "match_three_or_more": int(three)}


G = {"reference_version": probables.__version__, "empty_filter": EMPTY_FILTER, "three": list(THREE), "cases": [run(g, *geo) for g, geo in enumerate(GEOMETRIES)]}
assert [(c["number_bits"], c["number_hashes"]) for c in G["cases"]] == [(63, 4), (959, 7)]
assert sum(c["false_positives"] for c in G["cases"]) > 0, "no false-positive (key, filter) pair"
assert sum(c["match_none"] for c in G["cases"]) > 0, "no probe that matches no filter"
assert sum(c["match_three_or_more"] for c in G["cases"]) > 0, "no probe that matches three or more filters"

out = Path(sys.argv[2]) if len(sys.argv) > 2 else Path(__file__).resolve().parent / "golden_bank_match.json"
out.write_text(json.dumps(G, separators=(",", ":")) + "\n")
assert out.stat().st_size < 100_000
print(out, out.stat().st_size, "bytes;", [(c["number_bits"], c["number_hashes"], sum(map(len, c["sent"])),c["false_positives"], c["match_none"], c["match_three_or_more"])
                                         for c in G["cases"]])
