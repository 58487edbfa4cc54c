#!/usr/bin/env python3
"""Generate tests/golden/golden_bloom_ordered.json by running the REAL reference's BloomFilter (pyprobables v0.7.0,
probables/blooms/bloom.py:234-272) through the stream de-duplication loop

    for key in stream:  seen = key in blm;  blm.add(key)

and through its conditional twin ``if key not in blm: blm.add(key)``.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_bloom_ordered.py [/root/reference]

Data only: every case holds the constructor's arguments (est_elements, false_positive_rate, the hash function's name, a start state as
the hex export of a filter that already holds keys, or null), the keys ("str" as they are, "bytes" as hex), the ``seen`` list, the
filter's ``export_hex()`` after the first loop, number_bits / number_hashes, ``elements_added`` after each of the two loops, and
how many ``seen`` answers fell on a key's first occurrence (false positives of the table, not repeats).  The generator asserts that the two
loops leave the same flags and the same table.
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
from probables.hashes import default_md5  # noqa: E402

HASHES = {"fnv": None, "md5": default_md5}


def stream(kind, n, pool, seed):
    """n draws from a pool of `pool` different keys: heavy repeats"""
    rng = random.Random(seed)
    if kind == "str":
        keys = [f"key-{seed}-{i}-" + "x" * rng.randrange(0, 9) for i in range(pool)]
    else:
        keys = [bytes(rng.randrange(256) for _ in range(rng.randrange(0, 24))) + i.to_bytes(2, "little") for i in range(pool)]
    return [keys[rng.randrange(pool)] for _ in range(n)]


def start_hex(est, fpr, hash_name, n, seed):
    blm = BloomFilter(est, fpr, hash_function=HASHES[hash_name])
    for key in stream("str", n, n, seed):
        blm.add(key)
    return blm.export_hex()


CASES = [
    # est 64 at 5 %: m = 400, k = 4 -- 300 different keys overfill it, so that first occurrences are reported seen
    {"name": "overfull_m400_k4", "est": 64, "fpr": 0.05, "hash": "fnv", "start": None, "type": "str", "keys": stream("str", 580, 300, 1)},
    {"name": "start_from_hex", "est": 200, "fpr": 0.02, "hash": "fnv", "start": start_hex(200, 0.02, "fnv", 150, 2), "type": "str",
     "keys": stream("str", 300, 120, 2)[:150] + stream("str", 150, 150, 2)},  # the second half: keys of the start state itself
    {"name": "bytes_keys", "est": 500, "fpr": 0.01, "hash": "fnv", "start": None, "type": "bytes", "keys": stream("bytes", 400, 180, 3)},
    {"name": "md5", "est": 300, "fpr": 0.03, "hash": "md5", "start": None, "type": "str", "keys": stream("str", 350, 200, 4)},
]


def fresh(c):
    if c["start"] is not None:
        return BloomFilter(hex_string=c["start"], hash_function=HASHES[c["hash"]])
    return BloomFilter(c["est"], c["fpr"], hash_function=HASHES[c["hash"]])


def run(c):
    blm, cond = fresh(c), fresh(c)
    seen, seen_cond, met, first_seen = [], [], set(), 0
    for key in c["keys"]:
        s = key in blm
        blm.add(key)
        seen.append(int(s))
        first_seen += int(s and key not in met)
        met.add(key)
        s2 = key in cond
        if not s2:
            cond.add(key)
        seen_cond.append(int(s2))
    assert seen == seen_cond and blm.export_hex()[:-40] == cond.export_hex()[:-40], "the two loops differ"
    out = dict(c)
    out["keys"] = [k if c["type"] == "str" else k.hex() for k in c["keys"]]
    out.update({"seen": seen, "export_hex": blm.export_hex(), "number_bits": blm.number_bits, "number_hashes": blm.number_hashes,
                "elements_added": blm.elements_added, "elements_added_conditional": cond.elements_added, "seen_at_first_occurrence": first_seen})
    return out


G = {"reference_version": probables.__version__, "cases": [run(c) for c in CASES]}
cs = {c["name"]: c for c in G["cases"]}
# the properties the fixture exists for
assert cs["overfull_m400_k4"]["number_bits"] == 400 and cs["overfull_m400_k4"]["number_hashes"] == 4
assert cs["overfull_m400_k4"]["seen_at_first_occurrence"] > 0, "no false positive at a first occurrence"
assert all(0 < sum(c["seen"]) < len(c["seen"]) for c in cs.values())
assert all(c["elements_added_conditional"] < c["elements_added"] for c in cs.values())

out = Path(__file__).resolve().parent / "golden_bloom_ordered.json"
out.write_text(json.dumps(G, separators=(",", ":")) + "\n")
print(out, out.stat().st_size, "bytes;", {n: (len(c["seen"]), sum(c["seen"]), c["seen_at_first_occurrence"]) for n, c in cs.items()})
