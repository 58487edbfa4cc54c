#!/usr/bin/env python3
"""Generate tests/golden/golden_cbf_running.json by running the REAL reference's CountingBloomFilter
(pyprobables v0.7.0, probables/blooms/countingbloom.py:125-208) over small ordered streams of add_alt / remove_alt.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_cbf_running.py [/root/reference]

Data only: every case holds m, k, the start counters (sparse), the ops as hash lists with signed weights (w >= 0: add_alt(hashes, w),
w < 0: remove_alt(hashes, -w)), every return value, the final counters (sparse), elements_added, and "ill_formed": a remove found its key
absent (min 0, w > 0) or with less than w.  Streams on which the reference raises OverflowError (an op that moves one counter twice past a
rail) are not part of the fixture: the generator asserts that none does.
"""

import json
import sys
from array import array
from pathlib import Path

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import probables  # noqa: E402
from probables import CountingBloomFilter  # noqa: E402

from cbf_running_model import MAX, sm  # noqa: E402


def fresh(m, k, start):
    blm = CountingBloomFilter(est_elements=10, false_positive_rate=0.05)
    blm._set_values(10, 0.05, k, m, None)
    blm._bloom_length = m
    blm._bloom = array("I", [0]) * m
    for i, v in start:
        blm._bloom[i] = v
    return blm


def distinct_bins(seed, m, k):
    """k different counters of a table of m >= k, from integers alone"""
    got, t = [], 0
    while len(got) < k:
        c = sm(seed * 1009 + t) % m
        t += 1
        if c not in got:
            got.append(c)
    return got


def lift(bins, m, salt):
    """hashes that reduce to the bins: bin + m * (a few multiples), inside 64 bits"""
    return [b + m * (sm(salt * 31 + s) % 1000) for s, b in enumerate(bins)]


def fuzz(name, m, k, n, pool, salt, start=(), wmax=5, removes=0.4, exact=False):
    """keys from a pool with k different counters each; exact: a remove never asks for more than the reference holds (a well-formed stream)"""
    keys = [distinct_bins(salt * 7919 + p, m, k) for p in range(pool)]
    ops, held = [], [0] * pool
    for i in range(n):
        r = sm(salt * 1000003 + i)
        p, w = r % pool, 1 + (r >> 20) % wmax
        if (r >> 40) % 1000 < removes * 1000:
            if exact:
                if held[p] == 0:
                    held[p] += w
                    ops.append((lift(keys[p], m, i), w))
                    continue
                w = min(w, held[p])
                held[p] -= w
            ops.append((lift(keys[p], m, i), -w))
        else:
            held[p] += w
            ops.append((lift(keys[p], m, i), w))
    return {"name": name, "m": m, "k": k, "start": [list(x) for x in start], "ops": [[h, w] for h, w in ops]}


def hand(name, m, k, start, ops):
    return {"name": name, "m": m, "k": k, "start": [list(x) for x in start], "ops": [[list(h), w] for h, w in ops]}


CASES = [
    fuzz("well_formed_k3", 257, 3, 60, 9, 1, exact=True),
    fuzz("well_formed_k7_shared_counters", 31, 7, 60, 5, 2, exact=True),
    fuzz("any_removes_k3", 257, 3, 60, 9, 3),
    fuzz("any_removes_k5_small_table", 17, 5, 60, 6, 4, wmax=9, removes=0.55),
    fuzz("adds_only_k4", 64, 4, 40, 10, 5, removes=0.0),
    fuzz("well_formed_on_a_loaded_table", 101, 3, 50, 7, 6, start=[(i, 1000 + i) for i in range(101)], exact=True),
    # every op probes a counter more than once (m = 3 < k); counters high enough for every remove
    hand("duplicate_probes_m3", 3, 4, [(0, 500), (1, 500), (2, 500)],
         [([0, 1, 2, 3], 5), ([3, 3, 3, 3], 7), ([1, 4, 7, 2], -3), ([0, 0, 1, 1], -2), ([5, 5, 5, 2], 11), ([2, 2, 2, 2], -20), ([0, 1, 2, 0], 1)]),
    hand("duplicate_probes_add_from_zero", 3, 3, [], [([0, 0, 1], 4), ([0, 0, 1], -2), ([2, 2, 2], 9), ([2, 2, 2], -3), ([1, 1, 0], -1)]),
    # the rails: counters that start at MAX - 1 and MAX, adds that reach MAX exactly and adds that pass it, removes on sticky counters
    hand("rails", 8, 2, [(0, MAX - 1), (1, MAX), (2, MAX - 10), (3, 5), (4, MAX - 1)],
         [([0, 3], 1),       # 0 reaches MAX exactly: no clamp
          ([0, 3], -1),      # 0 is sticky now: only 3 moves
          ([1, 3], -2),      # a sticky counter next to a live one
          ([0, 1], -1),      # the minimum is MAX: a no-op that returns MAX
          ([2, 3], 20),      # 2 passes MAX: clamped
          ([2, 3], -20),     # ... and stays there
          ([4, 5], 7),       # 4 passes MAX from MAX - 1
          ([4, 5], -7),
          ([6, 7], 2**31 - 1), ([6, 7], 2**31 - 1), ([6, 7], 1),  # the largest int32 weights: MAX exactly, from zero
          ([6, 7], -1),      # min is MAX
          ([3, 5], 2**31 - 1), ([3, 5], 1), ([3, 5], -(2**31))]),  # ... and the largest remove, INT32_MIN
    hand("absent_remove", 16, 3, [], [([1, 2, 3], 2), ([4, 5, 6], -1), ([1, 2, 3], -1), ([1, 2, 3], 1)]),
    hand("partial_remove", 16, 3, [], [([1, 2, 3], 2), ([1, 2, 3], -5), ([1, 2, 3], 1), ([1, 2, 3], -1)]),
    hand("shared_counter_runs_dry", 16, 2, [], [([1, 2], 3), ([2, 3], 3), ([1, 2], -3), ([2, 3], -3), ([2, 3], -1), ([1, 2], -3)]),
    hand("zero_weights", 16, 2, [(1, 4)], [([1, 2], 0), ([1, 2], -0), ([1, 1], 0), ([3, 4], 0), ([1, 5], 3), ([1, 5], -3)]),
]


def run(c):
    blm = fresh(c["m"], c["k"], c["start"])
    results, ill = [], False
    for h, w in c["ops"]:
        if w >= 0:
            results.append(blm.add_alt(h, w))  # (an OverflowError here ends the generator: such streams are not part of the fixture)
        else:
            mn = blm.check_alt(h[: c["k"]])
            ill |= mn != MAX and mn < -w
            results.append(blm.remove_alt(h, -w))
    out = dict(c)
    out.update({"results": results, "final": [[i, v] for i, v in enumerate(blm._bloom) if v], "elements_added": blm.elements_added, "ill_formed": bool(ill)})
    return out


G = {"reference_version": probables.__version__, "cases": [run(c) for c in CASES]}
cs = G["cases"]
# the properties the fixture exists for
assert any(c["ill_formed"] for c in cs) and any(not c["ill_formed"] and any(w < 0 for _, w in c["ops"]) for c in cs)
assert any(MAX in c["results"] for c in cs), "no op returns MAX"
assert any(c["m"] < c["k"] for c in cs), "no stream of duplicate probes"
assert all(-(2**31) <= w < 2**31 for c in cs for _, w in c["ops"]), "a weight outside int32"

out = Path(__file__).resolve().parent / "golden_cbf_running.json"
out.write_text(json.dumps(G, separators=(",", ":")) + "\n")
print(out, out.stat().st_size, "bytes;", {c["name"]: (len(c["ops"]), c["ill_formed"]) for c in cs})
