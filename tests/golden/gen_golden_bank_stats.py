#!/usr/bin/env python3
"""Generate tests/golden/golden_bank_stats.json by running the REAL reference's BloomFilter (pyprobables v0.7.0, probables/blooms/bloom.py)
once per filter of a bank of 70 filters and asking it what a bank must answer about its filters as sets: ``estimate_elements`` (340-352),
``current_false_positive_rate`` (361-369), ``jaccard_index`` (430-460), ``union`` (401-428) and ``intersection`` (371-399).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_bank_stats.py [/root/reference [output file]]

Data only.  Per geometry -- (10, 0.05): 63 bits, k = 4; (100, 0.01): 959 bits, k = 7 -- 70 filters are fed 14 / 120 keys each, key i of the pool
being ``key_prefix + str(i)``; "sent" holds the pool indices per filter in the order of their add(), as a list or as ["range", start, stop].
Filter 41 gets nothing, filter 5 forty times its share (every bit set: estimate_elements() == -1), filters 7 and 8 the same keys, filters 20
and 21 one key each, chosen so that the two rows share no bit.  Recorded per filter: elements_added, the bit count, estimate_elements() and
current_false_positive_rate().hex(); the full 70 x 70 matrix of intersection counts; jaccard_index(...).hex() for about 200 chosen pairs; and
for ten groups the row bytes (hex; not export_hex(): the footer cannot pack -1) and elements_added of the chained union and intersection.
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
EMPTY, FULL, SAME, DISJOINT = 41, 5, (7, 8), (20, 21)
GEOMETRIES = [(10, 0.05, 14), (100, 0.01, 120)]  # (est_elements, false_positive_rate, keys per filter)
POOL = (96, 300)
GROUPS = [[3, 9], [10, 11, 12], [17], [EMPTY, 2], [FULL, 30], [6, 6, 13], list(range(FILTERS)), list(SAME), list(DISJOINT), [EMPTY]]


def bits_of(blm):
    return int.from_bytes(bytes(blm._bloom), "little")


def run(g, est, fpr, per_filter):
    rng = random.Random(9000 + g)
    prefix = f"stats-{g}-"
    key = lambda i: prefix + str(i)  # noqa: E731
    sent = []
    for f in range(FILTERS):
        if f == EMPTY:
            sent.append([])
        elif f == FULL:
            sent.append(["range", 1000, 1000 + 40 * per_filter])
        elif f == SAME[1]:
            sent.append(list(sent[SAME[0]]))
        else:
            sent.append(rng.sample(range(POOL[g]), per_filter))
    # two non-empty filters without a common bit: single keys, tried in turn until the rows are disjoint
    first = BloomFilter(est, fpr)
    first.add(key(0))
    for i in range(1, POOL[g]):
        second = BloomFilter(est, fpr)
        second.add(key(i))
        if bits_of(first) & bits_of(second) == 0:
            sent[DISJOINT[0]], sent[DISJOINT[1]] = [0], [i]
            break
    else:
        raise AssertionError("no pair of single keys with disjoint rows")
    blms = []
    for f in range(FILTERS):
        b = BloomFilter(est, fpr)
        s = sent[f]
        for i in (range(s[1], s[2]) if s and s[0] == "range" else s):
            b.add(key(i))
        blms.append(b)
    m, k = blms[0].number_bits, blms[0].number_hashes
    rows = [bits_of(b) for b in blms]
    counts = [bin(r).count("1") for r in rows]
    assert counts[FULL] == m and blms[FULL].estimate_elements() == -1, "filter 5 is not full"
    assert counts[EMPTY] == 0 and rows[SAME[0]] == rows[SAME[1]] and counts[SAME[0]] > 0
    assert rows[DISJOINT[0]] & rows[DISJOINT[1]] == 0 and counts[DISJOINT[0]] > 0 and counts[DISJOINT[1]] > 0
    inter = [[bin(rows[i] & rows[j]).count("1") for j in range(FILTERS)] for i in range(FILTERS)]
    pairs = {(EMPTY, EMPTY), SAME, DISJOINT} | {(f, f) for f in range(FILTERS)}
    pairs |= {(EMPTY, x) for x in (0, FULL, 33)} | {(x, EMPTY) for x in (1, 69)} | {(FULL, x) for x in (0, 7, 41, 69)} | {(x, FULL) for x in (2, 20)}
    while len(pairs) < 200:
        pairs.add((rng.randrange(FILTERS), rng.randrange(FILTERS)))
    jac = []
    for i, j in sorted(pairs):
        v = blms[i].jaccard_index(blms[j])
        union = counts[i] + counts[j] - inter[i][j]
        assert v == (1.0 if union == 0 else inter[i][j] / union)
        jac.append([i, j, float(v).hex()])
    assert blms[EMPTY].jaccard_index(blms[EMPTY]) == 1.0 and blms[EMPTY].jaccard_index(blms[0]) == 0.0
    assert blms[SAME[0]].jaccard_index(blms[SAME[1]]) == 1.0 and blms[DISJOINT[0]].jaccard_index(blms[DISJOINT[1]]) == 0.0
    groups = []
    for members in GROUPS:
        rec = {"members": members}
        for op in ("union", "intersection"):
            res = getattr(blms[members[0]], op)(blms[members[0]])  # (a group of one: the row itself, its count the estimate)
            for f in members[1:]:
                res = getattr(res, op)(blms[f])
            rec[op] = {"row_hex": bytes(res._bloom).hex(), "elements_added": res.elements_added}
            assert res.elements_added == res.estimate_elements()
        groups.append(rec)
    return {"est": est, "fpr": fpr, "filters": FILTERS, "number_bits": m, "number_hashes": k, "key_prefix": prefix, "sent": sent,
            "elements_added": [b.elements_added for b in blms], "bits": counts, "estimate": [b.estimate_elements() for b in blms],
            "fpr_hex": [float(b.current_false_positive_rate()).hex() for b in blms], "intersections": inter, "jaccard_hex": jac, "groups": groups}


G = {"reference_version": probables.__version__, "empty": EMPTY, "full": FULL, "same": list(SAME), "disjoint": list(DISJOINT),
     "cases": [run(g, *geo) for g, geo in enumerate(GEOMETRIES)]}
assert [(c["number_bits"], c["number_hashes"]) for c in G["cases"]] == [(63, 4), (959, 7)]

out = Path(sys.argv[2]) if len(sys.argv) > 2 else Path(__file__).resolve().parent / "golden_bank_stats.json"
out.write_text(json.dumps(G, separators=(",", ":")) + "\n")
assert out.stat().st_size < 100_000, out.stat().st_size
print(out, out.stat().st_size, "bytes;", [(c["number_bits"], c["number_hashes"], len(c["jaccard_hex"]), len(c["groups"])) for c in G["cases"]])
