#!/usr/bin/env python3
"""Generate tests/golden/golden_quotient_remove.json by running the REAL reference's QuotientFilter
(pyprobables, probables/quotientfilter/quotientfilter.py) through add_alt / remove_alt streams built here.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_quotient_remove.py [/root/reference]

Data only.  Every case: q0, auto_expand and a list of steps.  A step is one stream of 32-bit hashes fed to `add_alt` ("add") or to
`remove_alt` ("remove") one after the other, and what the reference holds behind it: the quotient, `elements_added` (the reference's
counter: a removal never decrements it), `get_hashes()`, and the four arrays written sparsely -- `filter` as [slot, remainder] pairs of the
non-zero remainders, `occupied` / `continuation` / `shifted` as the lists of set bits (a table of 2^24 slots stays a few lines).
`raised`: the add stream ended in QuotientFilterError (the streams that do are one hash long, so nothing was inserted before it).

Every step leaves at least one empty slot (on a full table the reference's removal may not return), asserted below together with the
properties each case exists for.
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

SEED = 20241019
rng = random.Random(SEED)


def mk(q, quot, rem):
    return (quot << (32 - q)) | rem


def bits(bitarray, size):
    return np.unpackbits(np.frombuffer(bitarray.bitarray, dtype=np.uint8), bitorder="little")[:size]


def snapshot(qf):
    size = qf.size
    filt = np.frombuffer(qf._filter, dtype={1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[qf._filter.itemsize])[:size]
    occ, cont, sh = (bits(b, size) for b in (qf._is_occupied, qf._is_continuation, qf._is_shifted))
    assert int(((occ | cont | sh) == 0).sum()) >= 1, "a step must leave an empty slot"
    nz = np.flatnonzero(filt)
    return {"q": qf.quotient, "elements_added": qf.elements_added, "get_hashes": qf.get_hashes(),
            "filter": [[int(i), int(filt[i])] for i in nz], "occupied": np.flatnonzero(occ).tolist(),
            "continuation": np.flatnonzero(cont).tolist(), "shifted": np.flatnonzero(sh).tolist()}


def _stuck(signum, frame):
    raise AssertionError("the reference did not return")


def scenario(name, q, steps, auto_expand=False, **extra):
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
    case = {"name": name, "q0": q, "auto_expand": auto_expand, "steps": out}
    case.update(extra)
    return case


def held_after(case):
    """the set the table holds behind each step"""
    s, out = set(), []
    for st in case["steps"]:
        if st["op"] == "add" and not st["raised"]:
            s |= set(st["hashes"])
        elif st["op"] == "remove":
            s -= set(st["hashes"])
        out.append(set(s))
    return out


CASES = []

# ---- q = 5: the whole table is one metadata word
Q = 5
base5 = [mk(Q, 10, r) for r in (1, 2, 3, 4)] + [mk(Q, 11, 5)] + [mk(Q, 12, r) for r in (6, 7)] + [mk(Q, 14, 9)]  # one cluster, slots 10 .. 17
CASES.append(scenario("q5_run_head_with_continuation", Q, [("add", base5), ("remove", [mk(Q, 10, 1)]), ("remove", [mk(Q, 12, 6)])]))
CASES.append(scenario("q5_run_head_without_continuation", Q, [("add", base5), ("remove", [mk(Q, 11, 5)]), ("remove", [mk(Q, 14, 9)])]))
CASES.append(scenario("q5_middle_and_last_of_run", Q, [("add", base5), ("remove", [mk(Q, 10, 2)]), ("remove", [mk(Q, 10, 4)]), ("remove", [mk(Q, 12, 7)])]))
CASES.append(scenario("q5_whole_run", Q, [("add", base5), ("remove", [mk(Q, 10, r) for r in (3, 1, 4, 2)]), ("remove", [mk(Q, 12, 7), mk(Q, 12, 6)])]))
CASES.append(scenario("q5_whole_cluster", Q, [("add", base5 + [mk(Q, 25, 1), mk(Q, 25, 2)]), ("remove", base5[::-1]), ("remove", [mk(Q, 25, 2), mk(Q, 25, 1)])]))
# 10, 10, 11, 13 sit in slots 10 .. 13; without the second 10 slot 12 falls empty and 13 starts a cluster of its own
split5 = [mk(Q, 10, 1), mk(Q, 10, 2), mk(Q, 11, 3), mk(Q, 13, 4), mk(Q, 13, 5)]
CASES.append(scenario("q5_split_cluster", Q, [("add", split5), ("remove", [mk(Q, 10, 2)])]))
wrap5 = [mk(Q, 30, r) for r in (1, 2, 3)] + [mk(Q, 31, r) for r in (4, 5, 6)] + [mk(Q, 0, r) for r in (7, 8)] + [mk(Q, 2, 9)]
CASES.append(scenario("q5_wrapped_cluster", Q, [("add", wrap5), ("remove", [mk(Q, 31, 4), mk(Q, 0, 8)]), ("remove", [mk(Q, 30, 1), mk(Q, 30, 2), mk(Q, 30, 3)]),
                                                ("remove", [mk(Q, 0, 7), mk(Q, 31, 6)]), ("add", [mk(Q, 31, 1), mk(Q, 30, 9)]), ("remove", [mk(Q, 2, 9), mk(Q, 31, 5)])]))
CASES.append(scenario("q5_absent_and_duplicates", Q, [("add", base5), ("remove", [mk(Q, 10, 0), mk(Q, 10, 9), mk(Q, 12, 5), mk(Q, 3, 3), mk(Q, 13, 9), mk(Q, 31, 0), 0, 0xFFFFFFFF]),
                                                      ("remove", [mk(Q, 10, 2), mk(Q, 10, 2), mk(Q, 13, 1), mk(Q, 12, 7), mk(Q, 10, 2), mk(Q, 12, 7)]), ("remove", [])]))

# ---- q = 6: two metadata words
Q = 6
cross6 = [mk(Q, 29, 3)] + [mk(Q, 30, r) for r in (1, 2)] + [mk(Q, 31, r) for r in (1, 2, 3)] + [mk(Q, 32, 4)] + [mk(Q, 33, r) for r in (5, 6)]  # slots 29 .. 37
CASES.append(scenario("q6_cluster_over_word_boundary", Q, [("add", cross6), ("remove", [mk(Q, 31, 2), mk(Q, 30, 1)]), ("remove", [mk(Q, 33, 5), mk(Q, 29, 3)]),
                                                           ("remove", [mk(Q, 31, 1), mk(Q, 31, 3), mk(Q, 32, 4)])]))
two6 = [mk(Q, 3, r) for r in (1, 2, 3)] + [mk(Q, 4, 4)] + [mk(Q, 20, r) for r in (5, 6)] + [mk(Q, 21, 7), mk(Q, 21, 8)] + [mk(Q, 40, 1), mk(Q, 40, 2), mk(Q, 41, 3)]
CASES.append(scenario("q6_two_clusters_in_one_word", Q, [("add", two6), ("remove", [mk(Q, 21, 7), mk(Q, 3, 2), mk(Q, 40, 1), mk(Q, 20, 5), mk(Q, 4, 4)])]))
wrap6 = [mk(Q, 62, r) for r in (1, 2)] + [mk(Q, 63, r) for r in (3, 4, 5)] + [mk(Q, 0, 6), mk(Q, 0, 7), mk(Q, 1, 8)]
CASES.append(scenario("q6_wrapped_cluster", Q, [("add", wrap6), ("remove", [mk(Q, 63, 3), mk(Q, 0, 6), mk(Q, 62, 2)]), ("remove", [mk(Q, 62, 1), mk(Q, 63, 5)])]))


def random_set(q, n, small_rem=False, near_end=0.0):
    size, r = 1 << q, 32 - q
    out = set()
    while len(out) < n:
        quot = size - 1 - rng.randrange(4) if rng.random() < near_end else rng.randrange(size)
        out.add(mk(q, quot, rng.randrange(16 if small_rem else 1 << r)))
    return sorted(out)


def random_case(name, q, load, batches, width=None, **kw):
    hs = random_set(q, int((1 << q) * load), **kw)
    rng.shuffle(hs)
    steps, left = [("add", list(hs))], list(hs)
    for frac in batches:
        k = max(1, int(len(left) * frac))
        gone = rng.sample(left, k)
        absent = [h ^ 1 for h in gone[: max(1, k // 4)]] + [rng.getrandbits(32) for _ in range(max(1, k // 4))]
        batch = gone + absent + gone[:2]
        rng.shuffle(batch)
        steps.append(("remove", batch))
        dropped = set(gone)
        left = [h for h in left if h not in dropped]
    steps.append(("add", rng.sample(hs, min(len(hs), 5))))  # an add after the removes: some come back, some are still there
    return scenario(name, q, steps, **({"width": width} if width else {}))


CASES.append(random_case("q6_random_load0.8", 6, 0.8, (0.3, 0.3, 0.5), small_rem=True, near_end=0.3))
CASES.append(random_case("q5_random_load0.9", 5, 0.9, (0.2, 0.5), small_rem=True, near_end=0.3))

# ---- q = 10: one run of 300 (a cluster of a single quotient), and the 32-bit remainder width
Q = 10
long10 = [mk(Q, 700, r) for r in rng.sample(range(1 << 22), 300)]
s10 = sorted(long10)
CASES.append(scenario("q10_one_run_of_300", Q, [("add", long10), ("remove", [s10[0], s10[-1], s10[150]] + rng.sample(s10[1:-1], 100)), ("remove", s10[:40]),
                                                 ("remove", s10)], width=32))
CASES.append(random_case("q10_width32_random", 10, 0.7, (0.25, 0.4), near_end=0.1, width=32))
# ---- the other two remainder widths
CASES.append(random_case("q16_width16_random", 16, 0.02, (0.3,), near_end=0.3, width=16))
h24 = random_set(24, 300, near_end=0.5) + [mk(24, 5000, r) for r in range(1, 40)]
CASES.append(scenario("q24_width8", 24, [("add", h24), ("remove", rng.sample(h24, 120) + [mk(24, 5000, 200), mk(24, 77, 1)])], width=8))

# ---- the counter: `_elements_added` counts inserts, a removal never decrements it, only a resize resets it
d = [mk(3, quot, 1 + quot) for quot in (0, 2, 3, 5, 6, 7)]
e = [mk(3, 1, 9), mk(3, 4, 9), mk(3, 1, 10)]
# 6 in, 3 out, 2 in: the second of the two adds starts at a counter of 7 / 8 >= 0.85 (true load 4 / 8) and doubles the table
CASES.append(scenario("counter_doubles_at_half_load_q3", 3, [("add", d), ("remove", d[:3]), ("add", e[:2])], auto_expand=True))
# the resize reset the counter: behind it the stream is judged on true counts (13 held at its end: one short of q = 4's threshold of 14, which
# a counter that kept the three removals would have passed), and the second doubling comes in the next stream, two removals early again
more = [rng.getrandbits(32) for _ in range(20)]
CASES.append(scenario("counter_second_doubling_on_true_counts_q3", 3, [("add", d), ("remove", d[:3]), ("add", e + more[:7]), ("remove", more[:2]), ("add", more[7:])],
                      auto_expand=True))
# no expansion: the counter reaches the size with three slots free
CASES.append(scenario("counter_insufficient_space_with_free_slots_q3", 3, [("add", d), ("remove", d[:3]), ("add", e[:2]), ("add", [e[2]]), ("remove", [d[3]]), ("add", [e[2]])]))

by = {c["name"]: c for c in CASES}
# the properties the fixture exists for, by construction
for c in CASES:
    sets = held_after(c)
    for st, s in zip(c["steps"], sets):
        assert sorted(st["get_hashes"]) == sorted(s), (c["name"], st["op"])
assert by["q5_whole_run"]["steps"][1]["occupied"] == [11, 12, 14] and by["q5_whole_cluster"]["steps"][2]["occupied"] == []
sp = by["q5_split_cluster"]["steps"]
assert sp[0]["shifted"] == [11, 12, 14] and sp[1]["shifted"] == [14] and sp[1]["filter"] == [[10, 1], [11, 3], [13, 4], [14, 5]]
assert 0 in by["q5_wrapped_cluster"]["steps"][0]["shifted"] and 0 in by["q6_wrapped_cluster"]["steps"][0]["shifted"]
assert {31, 32} <= set(by["q6_cluster_over_word_boundary"]["steps"][0]["shifted"])
assert by["q10_one_run_of_300"]["steps"][0]["continuation"] == list(range(701, 1000))
assert {c.get("width") for c in CASES} >= {8, 16, 32}
c1, c2, c3 = (by[n]["steps"] for n in ("counter_doubles_at_half_load_q3", "counter_second_doubling_on_true_counts_q3", "counter_insufficient_space_with_free_slots_q3"))
assert [(s["q"], s["elements_added"]) for s in c1] == [(3, 6), (3, 6), (4, 5)], [(s["q"], s["elements_added"]) for s in c1]
assert [(s["q"], s["elements_added"]) for s in c2] == [(3, 6), (3, 6), (4, 13), (4, 13), (5, 24)], [(s["q"], s["elements_added"]) for s in c2]
assert [s["raised"] for s in c3] == [False, False, False, True, False, True] and c3[3]["elements_added"] == 8 and len(c3[3]["get_hashes"]) == 5

G = {"reference_version": probables.__version__, "seed": SEED, "cases": CASES}
out = Path(__file__).resolve().parent / "golden_quotient_remove.json"
lines = ",\n".join(json.dumps(c, separators=(",", ":")) for c in CASES)
out.write_text('{"reference_version":%s,"seed":%d,"cases":[\n%s\n]}\n' % (json.dumps(probables.__version__), SEED, lines))
assert json.loads(out.read_text()) == G
print(out, out.stat().st_size, "bytes;", {c["name"]: [(s["q"], s["elements_added"], len(s["get_hashes"])) for s in c["steps"]] for c in CASES})
