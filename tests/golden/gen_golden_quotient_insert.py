#!/usr/bin/env python3
"""Generate tests/golden/golden_quotient_insert.json by running the REAL reference's QuotientFilter
(pyprobables, probables/quotientfilter/quotientfilter.py) through ordered multi-batch add_alt streams into loaded tables.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_quotient_insert.py [/root/reference]

Data only, in the layout of golden_quotient_remove.json (tests/qf_remove_fixture.py reads both): every case has q0, auto_expand and a list of
steps; a step is one stream of 32-bit hashes fed to `add_alt` ("add") or `remove_alt` ("remove") one after the other, and what the
reference holds behind it: the quotient, `elements_added`, `get_hashes()` (null for a completely full table, which the reference cannot
list) and the four arrays written sparsely.  `raised`: the add stream ended in QuotientFilterError (those streams are one hash long, so
nothing was inserted before it).

The cases: batches into clusters over the table's end and over a word seam (q = 5, 6), region boundaries (q = 8), random batches with
duplicates inside and across batches (q = 10), one set in three orders, streams that reach the 0.85 threshold inside a batch / with their
last call / before their first call, removals in between so that the counter is ahead of the true count, and auto_expand=False filled to the
last slot and one hash beyond.
"""

import json
import random
import signal
import sys
from pathlib import Path

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

import probables  # noqa: E402
from probables import QuotientFilter  # noqa: E402
from probables.exceptions import QuotientFilterError  # noqa: E402

SEED = 20241020
rng = random.Random(SEED)


def mk(q, quot, rem):
    return (quot << (32 - q)) | rem


def bits(bitarray, size):
    return np.unpackbits(np.frombuffer(bitarray.bitarray, dtype=np.uint8), bitorder="little")[:size]


def snapshot(qf):
    size = qf.size
    filt = np.frombuffer(qf._filter, dtype={1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[qf._filter.itemsize])[:size]
    occ, cont, sh = (bits(b, size) for b in (qf._is_occupied, qf._is_continuation, qf._is_shifted))
    full = int(((occ | cont | sh) == 0).sum()) == 0
    nz = np.flatnonzero(filt)
    return {"q": qf.quotient, "elements_added": qf.elements_added, "get_hashes": None if full else qf.get_hashes(),
            "filter": [[int(i), int(filt[i])] for i in nz], "occupied": np.flatnonzero(occ).tolist(),
            "continuation": np.flatnonzero(cont).tolist(), "shifted": np.flatnonzero(sh).tolist()}


def _stuck(signum, frame):
    raise AssertionError("the reference did not return")


def scenario(name, q, steps, auto_expand=False):
    qf = QuotientFilter(quotient=q, auto_expand=auto_expand)
    out = []
    signal.signal(signal.SIGALRM, _stuck)
    for op, hashes in steps:
        raised = False
        signal.alarm(600)
        try:
            for h in hashes:
                (qf.add_alt if op == "add" else qf.remove_alt)(h)
        except QuotientFilterError:
            assert op == "add" and len(hashes) == 1
            raised = True
        signal.alarm(0)
        step = {"op": op, "hashes": list(hashes), "raised": raised}
        step.update(snapshot(qf))
        out.append(step)
    return {"name": name, "q0": q, "auto_expand": auto_expand, "steps": out}


def random_set(q, n, small_rem=True, near_end=0.0, avoid=()):
    size, r = 1 << q, 32 - q
    out, avoid = set(), set(avoid)
    while len(out) < n:
        quot = size - 1 - rng.randrange(4) if rng.random() < near_end else rng.randrange(size)
        h = mk(q, quot, rng.randrange(1, 16 if small_rem else 1 << r))
        if h not in avoid:
            out.add(h)
    return sorted(out)


def adds(*batches):
    return [("add", list(b)) for b in batches]


CASES = []

# ---- q = 5: one metadata word, the cluster over the table's end
Q = 5
wrap5 = [mk(Q, 30, 2), mk(Q, 30, 4), mk(Q, 31, 3), mk(Q, 0, 5), mk(Q, 3, 1)]
CASES.append(scenario("q5_batches_over_the_end", Q, adds(wrap5, [mk(Q, 31, 1), mk(Q, 30, 3)], [mk(Q, 0, 1), mk(Q, 1, 1), mk(Q, 29, 9), mk(Q, 30, 1)],
                                                         [mk(Q, 2, 2), mk(Q, 31, 3), mk(Q, 31, 9), mk(Q, 3, 0)])))
CASES.append(scenario("q5_into_empty_slots_and_present", Q, adds(wrap5, [mk(Q, 10, 1), mk(Q, 11, 1), mk(Q, 30, 2)], wrap5, [mk(Q, 10, 0), mk(Q, 10, 2), mk(Q, 10, 1)])))

# ---- q = 6: the seam between the two metadata words
Q = 6
seam6 = [mk(Q, 29, 3), mk(Q, 30, 1), mk(Q, 31, 2), mk(Q, 34, 4), mk(Q, 34, 6), mk(Q, 62, 1), mk(Q, 63, 1)]
CASES.append(scenario("q6_batches_over_the_word_seam", Q, adds(seam6, [mk(Q, 30, 2), mk(Q, 31, 1)], [mk(Q, 29, 1), mk(Q, 33, 1), mk(Q, 34, 5)],
                                                               [mk(Q, 63, 2), mk(Q, 62, 2), mk(Q, 0, 1), mk(Q, 31, 9), mk(Q, 32, 1)])))
base6 = random_set(6, 20, near_end=0.3)
extra6 = random_set(6, 15, near_end=0.3, avoid=base6)
shuffled6 = list(extra6)
rng.shuffle(shuffled6)
for label, order in (("ascending", extra6), ("descending", extra6[::-1]), ("shuffled", shuffled6)):
    CASES.append(scenario(f"q6_one_set_{label}", 6, adds(base6, order)))

# ---- q = 8: where a region ends
Q = 8
cluster8 = [mk(Q, 10, 1), mk(Q, 10, 3), mk(Q, 11, 1), mk(Q, 16, 1), mk(Q, 16, 2)]  # cluster [10..12], 13 - 15 empty, head at 16
CASES.append(scenario("q8_two_into_the_cluster", Q, adds(cluster8, [mk(Q, 10, 2), mk(Q, 12, 1)])))
CASES.append(scenario("q8_three_into_the_cluster", Q, adds(cluster8, [mk(Q, 10, 2), mk(Q, 11, 2), mk(Q, 12, 1)])))
CASES.append(scenario("q8_three_and_quotient_15", Q, adds(cluster8, [mk(Q, 10, 2), mk(Q, 11, 2), mk(Q, 12, 1), mk(Q, 15, 1)])))
domino8 = [mk(Q, 40 + 3 * c + d, 1) for c in range(8) for d in range(2)]
CASES.append(scenario("q8_larger_than_its_cluster_then_domino", Q, adds(cluster8 + domino8, [mk(Q, 12, 9)], [mk(Q, 40, 0)], [mk(Q, 255, 1), mk(Q, 255, 2), mk(Q, 0, 1)])))

# ---- q = 10: random batches, duplicates inside and across batches
base10 = random_set(10, 500, small_rem=False, near_end=0.1)
more10 = random_set(10, 240, small_rem=False, near_end=0.1, avoid=base10)
b1 = more10[:80] + more10[:10] + base10[:10]
b2 = more10[60:160] + more10[100:120]
b3 = more10[160:] + base10[100:105] + more10[:5]
for b in (b1, b2, b3):
    rng.shuffle(b)
CASES.append(scenario("q10_random_batches_with_duplicates", 10, adds(base10, b1, b2, b3)))

# ---- the 0.85 threshold (28 of 32 at q = 5), auto_expand=True
pool5 = random_set(5, 31, near_end=0.2)
rng.shuffle(pool5)
CASES.append(scenario("threshold_reached_inside_a_batch_q5", 5, adds(pool5[:20], pool5[20:30]), auto_expand=True))
CASES.append(scenario("threshold_reached_by_the_last_call_then_first_call_q5", 5, adds(pool5[:20], pool5[20:28], pool5[28:29]), auto_expand=True))
CASES.append(scenario("threshold_then_only_present_hashes_follow_q5", 5, adds(pool5[:20], pool5[20:28] + pool5[:3]), auto_expand=True))
CASES.append(scenario("threshold_not_reached_q5", 5, adds(pool5[:20], pool5[20:27], pool5[:27]), auto_expand=True))
# removals in between: the counter (which a removal does not lower) reaches the threshold with the true count below it
CASES.append(scenario("counter_ahead_of_true_count_q5", 5, [("add", pool5[:20]), ("remove", pool5[:5]), ("add", pool5[20:26]), ("add", pool5[26:30])], auto_expand=True))

# ---- auto_expand=False: to the last slot, and one hash beyond
fill5 = random_set(5, 33, near_end=0.2)
rng.shuffle(fill5)
CASES.append(scenario("fill_to_the_last_slot_q5", 5, adds(fill5[:20], fill5[20:31], fill5[31:32], fill5[32:33])))
CASES.append(scenario("counter_full_with_free_slots_q5", 5, [("add", fill5[:28]), ("remove", fill5[:4]), ("add", fill5[28:32]), ("add", fill5[32:33])]))

by = {c["name"]: c for c in CASES}
# the properties the fixture exists for, by construction
assert {c["q0"] for c in CASES} >= {5, 6, 8, 10}
three = [by[f"q6_one_set_{x}"]["steps"][1] for x in ("ascending", "descending", "shuffled")]
assert all({k: s[k] for k in ("filter", "occupied", "continuation", "shifted")} == {k: three[0][k] for k in ("filter", "occupied", "continuation", "shifted")} for s in three)
assert 0 in by["q5_batches_over_the_end"]["steps"][1]["shifted"]
assert [s["q"] for s in by["threshold_reached_inside_a_batch_q5"]["steps"]] == [5, 6]
assert [(s["q"], s["elements_added"]) for s in by["threshold_reached_by_the_last_call_then_first_call_q5"]["steps"]] == [(5, 20), (5, 28), (6, 29)]
assert [s["q"] for s in by["threshold_then_only_present_hashes_follow_q5"]["steps"]] == [5, 6]
assert [(s["q"], s["elements_added"]) for s in by["threshold_not_reached_q5"]["steps"]] == [(5, 20), (5, 27), (5, 27)]
ca = by["counter_ahead_of_true_count_q5"]["steps"]
assert [(s["q"], s["elements_added"]) for s in ca[:3]] == [(5, 20), (5, 20), (5, 26)] and ca[3]["q"] == 6, [(s["q"], s["elements_added"]) for s in ca]
fl = by["fill_to_the_last_slot_q5"]["steps"]
assert [s["raised"] for s in fl] == [False, False, False, True] and fl[2]["get_hashes"] is None and len(fl[2]["filter"]) == 32 and fl[3]["elements_added"] == 32
cf = by["counter_full_with_free_slots_q5"]["steps"]
assert [s["raised"] for s in cf] == [False, False, False, True] and cf[3]["elements_added"] == 32 and len(cf[3]["get_hashes"]) == 28
assert any(len(st["hashes"]) != len(set(st["hashes"])) for st in by["q10_random_batches_with_duplicates"]["steps"])

G = {"reference_version": probables.__version__, "seed": SEED, "cases": CASES}
out = Path(__file__).resolve().parent / "golden_quotient_insert.json"
lines = ",\n".join(json.dumps(c, separators=(",", ":")) for c in CASES)
out.write_text('{"reference_version":%s,"seed":%d,"cases":[\n%s\n]}\n' % (json.dumps(probables.__version__), SEED, lines))
assert json.loads(out.read_text()) == G
print(out, out.stat().st_size, "bytes;", {c["name"]: [(s["q"], s["elements_added"]) for s in c["steps"]] for c in CASES})
