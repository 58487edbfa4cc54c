#!/usr/bin/env python3
"""Generate tests/golden/golden_bank.json by running the REAL reference's BloomFilter (pyprobables v0.7.0,
probables/blooms/bloom.py:234-272) once per filter of a bank: filter f of a BloomFilterBank must be, byte for byte,
``BloomFilter(est_elements, false_positive_rate)`` after ``add()`` of the keys sent to f.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_bank.py [/root/reference [output file]]

Data only.  Per geometry: the constructor's arguments, number_bits / number_hashes, a pool of keys (["s", text] for str, ["b", hex] for
bytes: str and bytes mixed, code points above 255, the empty key), the stream as (pool index, filter) pairs -- filter 3 gets nothing, pool
key 0 goes to two filters, some keys go to one filter twice --, per filter ``bytes(filter).hex()`` and ``elements_added``, and the answers
to a probe list of (pool index or absent key, filter) pairs with the number of false positives among them.  Plus the export of a filter that holds
"spam" and b"eggs" in the smallest geometry.
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

FILTERS = 5
EMPTY_FILTER = 3
# (est_elements, false_positive_rate, keys per filter): the first two are overfilled so that their probe lists meet false positives
GEOMETRIES = [(10, 0.05, 14), (100, 0.01, 120), (1000, 0.001, 40)]


def pool_key(g, i):
    if i == 1:
        return ""
    if i % 4 == 0:
        return f"g{g}-bytes-{i}".encode() + bytes([i % 256, 255 - i % 256])[: i % 3]
    if i % 4 == 2:
        return f"g{g}-λ€-{i}" + "\U0001f600" * (i % 2)
    return f"g{g}-key-{i}" + "x" * (i % 7)


def enc(key):
    return ["s", key] if isinstance(key, str) else ["b", key.hex()]


def run(g, est, fpr, per_filter):
    rng = random.Random(1000 + g)
    used = [f for f in range(FILTERS) if f != EMPTY_FILTER]
    pool = [pool_key(g, i) for i in range(per_filter * len(used))]
    stream = []
    for j, f in enumerate(used):
        mine = list(range(j * per_filter, (j + 1) * per_filter))
        stream += [(i, f) for i in mine]
        stream += [(mine[0], f), (mine[-1], f)]  # repeats: counted by elements_added, no new bits
    stream.append((0, 1))                        # pool key 0 lives in filter 0 and goes to filter 1 as well
    rng.shuffle(stream)
    blms = [BloomFilter(est, fpr) for _ in range(FILTERS)]
    sent = [set() for _ in range(FILTERS)]
    for i, f in stream:
        blms[f].add(pool[i])
        sent[f].add(pool[i])
    absent = [f"absent-{g}-{i}" if i % 2 else f"absent-{g}-{i}".encode() for i in range(100)]
    probes = [(i, i % FILTERS) for i in range(len(pool))] + [(i, (i + 1) % FILTERS) for i in range(0, len(pool), 3)] + [(0, 0), (0, 1), (0, 2)]
    answers, fps = [], 0
    for i, f in probes:
        a = blms[f].check(pool[i])
        assert a or pool[i] not in sent[f]
        fps += int(a and pool[i] not in sent[f])
        answers.append(int(a))
    absent_probes = [(i, i % FILTERS) for i in range(len(absent))]
    absent_answers = []
    for i, f in absent_probes:
        a = blms[f].check(absent[i])
        fps += int(a)
        absent_answers.append(int(a))
    assert fps > 0 or g == 2, "no false positive among the probes"
    assert blms[EMPTY_FILTER].elements_added == 0 and not any(bytes(blms[EMPTY_FILTER])[:-20])
    return {"est": est, "fpr": fpr, "filters": FILTERS, "number_bits": blms[0].number_bits, "number_hashes": blms[0].number_hashes,
            "pool": [enc(k) for k in pool], "stream": [list(p) for p in stream], "export_hex": [bytes(b).hex() for b in blms],
            "elements_added": [b.elements_added for b in blms], "probes": [list(p) for p in probes], "answers": answers,
            "absent": [enc(k) for k in absent], "absent_probes": [list(p) for p in absent_probes], "absent_answers": absent_answers,
            "false_positives": fps}


known = BloomFilter(10, 0.05)
known.add("spam")
known.add(b"eggs")
KNOWN = bytes(known).hex()
assert len(bytes(known)) == 28 and KNOWN.startswith("20008000200074010a00") and KNOWN.endswith("cdcc4c3d"), KNOWN

G = {"reference_version": probables.__version__, "known_spam_eggs": KNOWN, "cases": [run(g, *geo) for g, geo in enumerate(GEOMETRIES)]}
assert [(c["number_bits"], c["number_hashes"]) for c in G["cases"]] == [(63, 4), (959, 7), (14378, 10)]

out = Path(sys.argv[2]) if len(sys.argv) > 2 else Path(__file__).resolve().parent / "golden_bank.json"
out.write_text(json.dumps(G, separators=(",", ":")) + "\n")
print(out, out.stat().st_size, "bytes;", [(c["number_bits"], c["number_hashes"], len(c["stream"]), c["false_positives"]) for c in G["cases"]])
