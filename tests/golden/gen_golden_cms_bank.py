#!/usr/bin/env python3
"""Generate tests/golden/golden_cms_bank.json by running the REAL reference's CountMinSketch (pyprobables v0.7.0,
probables/countminsketch/countminsketch.py:257-288, 342-354, 356-399, 429-453) once per sketch of a bank: sketch s of a CountMinSketchBank
followed by the footer must be, byte for byte, ``bytes(CountMinSketch(width, depth))`` after ``add(key, num_els)`` of the ops sent to s.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_cms_bank.py <checkout of the reference> [output file]

Data only.  Per geometry (width, depth): a pool of keys (["s", text] for str, ["b", hex] for bytes: str and bytes mixed, code points above
255, the empty key), the stream as (pool index, sketch, num_els) triples with repeats -- sketch 3 gets nothing, pool key 0 goes to two
sketches --, per sketch ``bytes(sketch).hex()`` and ``elements_added``, and the answers of CountMinSketch, CountMeanSketch and
CountMeanMinSketch objects fed the same stream to a probe list of (pool index or absent key, sketch) pairs.  A rail case: three adds of
INT32_MAX to one key of one sketch, then one add of 1.  Join folds: groups of recorded member sketches (their exports, some with removes
behind them: negative bins, one on INT32_MIN; one with a bin on INT32_MAX) joined in member order onto an empty sketch, with the export.
"""

import json
import random
import sys
from pathlib import Path

if len(sys.argv) < 2:
    sys.exit(__doc__)
sys.dont_write_bytecode = True
sys.path.insert(0, sys.argv[1])

import probables  # noqa: E402
from probables import CountMeanMinSketch, CountMeanSketch, CountMinSketch  # noqa: E402

SKETCHES = 5
EMPTY_SKETCH = 3
I32_MAX, I32_MIN = 2**31 - 1, -(2**31)
GEOMETRIES = [(8, 3), (7, 3), (64, 5), (100, 4), (16, 1)]  # (7, 3): 21 ints, 3 pad ints in a bank row
KINDS = [("min", CountMinSketch), ("mean", CountMeanSketch), ("mean-min", CountMeanMinSketch)]


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


def run(g, width, depth):
    rng = random.Random(2000 + g)
    used = [s for s in range(SKETCHES) if s != EMPTY_SKETCH]
    per = 12
    pool = [pool_key(g, i) for i in range(per * len(used))]
    stream = []
    for j, s in enumerate(used):
        mine = list(range(j * per, (j + 1) * per))
        stream += [(i, s, rng.choice([1, 1, 1, 2, 5, 0, 1000])) for i in mine]
        stream += [(mine[0], s, 3), (mine[-1], s, 1), (mine[-1], s, 1)]  # repeats
    stream.append((0, 1, 7))  # pool key 0 lives in sketch 0 and goes to sketch 1 as well
    rng.shuffle(stream)
    objs = {name: [cls(width=width, depth=depth) for _ in range(SKETCHES)] for name, cls in KINDS}
    for i, s, w in stream:
        for name, _ in KINDS:
            objs[name][s].add(pool[i], w)
    absent = [f"absent-{g}-{i}" if i % 2 else f"absent-{g}-{i}".encode() for i in range(20)]
    probes = [(i, i % SKETCHES) for i in range(len(pool))] + [(i, (i + 1) % SKETCHES) for i in range(0, len(pool), 3)] + [(0, 0), (0, 1), (0, 2)]
    absent_probes = [(i, i % SKETCHES) for i in range(len(absent))]
    out = {"width": width, "depth": depth, "sketches": SKETCHES, "pool": [enc(k) for k in pool], "stream": [list(t) for t in stream],
           "export_hex": [bytes(c).hex() for c in objs["min"]], "elements_added": [c.elements_added for c in objs["min"]],
           "probes": [list(p) for p in probes], "absent": [enc(k) for k in absent], "absent_probes": [list(p) for p in absent_probes]}
    for name, _ in KINDS:
        if name == "mean-min" and width == 1:
            continue
        out["answers_" + name] = [objs[name][s].check(pool[i]) for i, s in probes]
        out["absent_answers_" + name] = [objs[name][s].check(absent[i]) for i, s in absent_probes]
    assert bytes(objs["min"][0]) == bytes(objs["mean"][0]) == bytes(objs["mean-min"][0])
    assert objs["min"][EMPTY_SKETCH].elements_added == 0 and not any(bytes(objs["min"][EMPTY_SKETCH])[:-16])
    return out


def rail(width, depth):
    objs = {name: cls(width=width, depth=depth) for name, cls in KINDS}
    steps = []
    for w in (I32_MAX, I32_MAX, I32_MAX, 1):
        for c in objs.values():
            c.add("hot", w)
        steps.append({"num_els": w, "export_hex": bytes(objs["min"]).hex(), "elements_added": objs["min"].elements_added,
                      "answers": {name: [c.check("hot"), c.check("cold")] for name, c in objs.items()}})
    return {"width": width, "depth": depth, "key": "hot", "other": "cold", "steps": steps}


def joins(width, depth):
    rng = random.Random(77)
    keys = [f"join-{i}" for i in range(30)]

    def member(adds, removes=(), hot=None):
        c = CountMinSketch(width=width, depth=depth)
        for k, w in adds:
            c.add(keys[k], w)
        for k, w in removes:
            c.remove(keys[k], w)
        if hot is not None:
            c.add(*hot) if hot[1] > 0 else c.remove(hot[0], -hot[1])
        return c

    members = [member([(rng.randrange(30), rng.choice([1, 2, 9])) for _ in range(20)]) for _ in range(4)]
    members.append(member([(0, 5)], hot=("railed", I32_MAX)))                                  # 4: bins on INT32_MAX
    members.append(member([(1, 3), (2, 4)], removes=[(3, 6), (4, 1)]))                         # 5: negative bins
    members.append(member([(5, 2)], removes=[(6, 10)], hot=("sunk", -(2**31))))                # 6: bins on INT32_MIN
    members.append(member([(0, 11), (7, 13)], hot=("railed", 40)))                             # 7: adds onto the railed bins of 4
    members.append(member([(8, 1)], hot=("sunk", 500)))                                        # 8: adds onto the sunk bins of 6
    members.append(member([(9, 2)], hot=("railed", -100)))                                     # 9: removes from the railed bins of 4
    assert max(members[4]._bins) == I32_MAX and min(members[6]._bins) == I32_MIN and min(members[5]._bins) < 0
    groups = [[0, 1], [0, 1, 2, 3], [3, 1, 0, 2], [4, 7, 0], [7, 4, 0], [5, 6, 8, 2], [8, 6, 5], [6, 8], [8, 6], [4, 9], [9, 4], [2]]
    folds = []
    for grp in groups:
        acc = CountMinSketch(width=width, depth=depth)
        for m in grp:
            acc.join(members[m])
        folds.append({"members": grp, "export_hex": bytes(acc).hex(), "elements_added": acc.elements_added})
    return {"width": width, "depth": depth, "members_hex": [bytes(m).hex() for m in members], "folds": folds}


G = {"reference_version": probables.__version__, "cases": [run(g, *geo) for g, geo in enumerate(GEOMETRIES)], "rail": rail(8, 3), "joins": joins(7, 3)}

out = Path(sys.argv[2]) if len(sys.argv) > 2 else Path(__file__).resolve().parent / "golden_cms_bank.json"
out.write_text(json.dumps(G, separators=(",", ":")) + "\n")
print(out, out.stat().st_size, "bytes;", [(c["width"], c["depth"], len(c["stream"])) for c in G["cases"]])
