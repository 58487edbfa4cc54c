#!/usr/bin/env python3
"""Generate tests/golden/golden_quotient.json by running the REAL reference's QuotientFilter
(pyprobables, probables/quotientfilter/quotientfilter.py) over hash streams built here.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_quotient.py [/root/reference]

Data only.  Every case: the 32-bit hash stream in order, q, the reference's four arrays after the stream (`filter`, `occupied`,
`continuation`, `shifted`), `get_hashes()` (null for a full table: the reference's walk to the first empty slot runs off the table),
and `check_alt` answers for a probe list that mixes present and absent hashes.  `expand_cases`: streams into an auto-expanding filter
that starts at q0, with the quotient and the arrays it ends with.
"""

import json
import random
import sys
from pathlib import Path

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

import probables  # noqa: E402
from probables import QuotientFilter  # noqa: E402

SEED = 20240611
rng = random.Random(SEED)


def mk(q, quot, rem):
    return (quot << (32 - q)) | rem


def random_stream(q, load):
    """`int(load * size)` distinct hashes (the whole table at load 1.0): ~30 % of them in the last four quotients (clusters that wrap past the
    last slot), remainders from a small pool for q <= 6 (long runs, neighbours by remainder), then ~25 % duplicates mixed in"""
    size, r = 1 << q, 32 - q
    want = size if load == 1.0 else int(size * load)
    seen = []
    while len(set(seen)) < want:
        quot = size - 1 - rng.randrange(4) if rng.random() < 0.3 else rng.randrange(size)
        rem = rng.randrange(16 if q <= 6 else 1 << r)
        seen.append(mk(q, quot, rem))
    distinct = list(dict.fromkeys(seen))
    stream = distinct + [rng.choice(distinct) for _ in range(max(2, want // 4))]
    head = stream[: want // 2]  # (duplicates only after part of the set is in: they meet a non-empty table)
    tail = stream[want // 2:]
    rng.shuffle(tail)
    return head + tail


def probes_for(q, stream):
    size, r = 1 << q, 32 - q
    s = sorted(set(stream))
    pick = s if len(s) <= 24 else rng.sample(s, 24)
    out = list(pick)
    out += [h ^ 1 for h in pick]                                   # the neighbouring remainder of an occupied quotient
    out += [mk(q, h >> r, (1 << r) - 1) for h in pick[:8]]         # past the end of a run
    out += [mk(q, h >> r, 0) for h in pick[:8]]                    # in front of a run
    out += [mk(q, quot, rng.randrange(1 << r)) for quot in range(0, size, max(1, size // 16))]
    out += [mk(q, size - 1, 5), mk(q, 0, 5), 0, 0xFFFFFFFF]
    return out


def arrays(qf):
    n = qf.size
    return {"filter": list(qf._filter), "occupied": [qf._is_occupied[i] for i in range(n)],
            "continuation": [qf._is_continuation[i] for i in range(n)], "shifted": [qf._is_shifted[i] for i in range(n)]}


def run(name, q, stream, **extra):
    qf = QuotientFilter(quotient=q, auto_expand=False)
    for h in stream:
        qf.add_alt(h)
    full = qf.elements_added == qf.size
    try:
        listed = qf.get_hashes()
    except IndexError:  # no empty slot to start from
        assert full
        listed = None
    probes = probes_for(q, stream)
    out = {"name": name, "q": q, "stream": stream, "elements_added": qf.elements_added, "get_hashes": listed, "probes": probes,
           "answers": [bool(qf.check_alt(p)) for p in probes]}
    out.update(arrays(qf))
    out.update(extra)
    # what the case was built for (asserted below over the whole set)
    qs = [h >> (32 - q) for h in sorted(set(stream))]
    out["max_run"] = max(qs.count(x) for x in set(qs))
    out["wrapped"] = out["shifted"][0] == 1  # slot 0 holds an element of another quotient: only a cluster that passed the last slot puts one there
    out["duplicates"] = len(stream) - len(set(stream))
    out["load"] = qf.elements_added / qf.size
    return out


CASES = []
for q in (3, 4, 6, 10):
    for load in (0.3, 0.6, 0.85, 1.0):
        CASES.append(run(f"random_q{q}_load{load}", q, random_stream(q, load)))

# every key in ONE quotient: a single run (in the middle of the table; at its end, wrapping)
CASES.append(run("one_quotient_middle_q4", 4, [mk(4, 9, x) for x in (7, 3, 3, 11, 1, 250, 7, 64)]))
CASES.append(run("one_quotient_last_q6", 6, [mk(6, 63, x) for x in rng.sample(range(1 << 26), 20)]))
# runs of 4+ equal quotients side by side (every insert shifts the runs behind it)
CASES.append(run("long_runs_q6", 6, [mk(6, quot, rem) for rem in (9, 2, 30, 4, 17) for quot in (10, 11, 12, 14, 40)]))
# a cluster of the last four quotients that wraps over slot 0 and pushes the runs of quotients 0 and 1
CASES.append(run("wrap_pushes_head_q4", 4, [mk(4, 0, 8), mk(4, 1, 3), mk(4, 15, 1), mk(4, 14, 2), mk(4, 13, 9), mk(4, 15, 7), mk(4, 12, 4), mk(4, 14, 6),
                                            mk(4, 15, 2), mk(4, 13, 1), mk(4, 0, 2), mk(4, 15, 9)]))
# one set, three orders
base = random_stream(6, 0.6)
CASES.append(run("orders_q6_forward", 6, base, same_set_as="orders_q6_forward"))
CASES.append(run("orders_q6_reversed", 6, base[::-1], same_set_as="orders_q6_forward"))
shuffled = base[:]
rng.shuffle(shuffled)
CASES.append(run("orders_q6_shuffled", 6, shuffled, same_set_as="orders_q6_forward"))


def run_expand(name, q0, stream):
    qf = QuotientFilter(quotient=q0, auto_expand=True)
    for h in stream:
        qf.add_alt(h)
    out = {"name": name, "q0": q0, "stream": stream, "q": qf.quotient, "elements_added": qf.elements_added, "get_hashes": qf.get_hashes()}
    out.update(arrays(qf))
    return out


def distinct_hashes(n):
    out = set()
    while len(out) < n:
        out.add(rng.getrandbits(32))
    return list(out)


# q0 = 3: 8 slots, load 7 / 8 >= 0.85 > 6 / 8 -- the 7th distinct hash reaches the threshold, the NEXT call (any hash) resizes
d7 = distinct_hashes(7)
d40 = distinct_hashes(40)
EXPAND = [
    run_expand("threshold_at_last_key", 3, d7),                                # no call follows: stays at q = 3
    run_expand("threshold_at_second_to_last_key_then_duplicate", 3, d7 + [d7[2]]),  # the duplicate's call resizes
    run_expand("threshold_at_second_to_last_key_then_new", 3, d7 + [d7[0] ^ 0x10101]),
    run_expand("duplicates_before_threshold", 3, d7[:6] + d7[:6] + [d7[6]]),   # duplicates do not count towards the load
    run_expand("several_doublings", 3, d40 + d40[:5]),
    run_expand("several_doublings_ends_on_threshold", 3, d40[:28]),            # q = 5 holds 28 > 27.2: reached at the last key
]

G = {"reference_version": probables.__version__, "seed": SEED, "cases": CASES, "expand_cases": EXPAND}
cs = CASES
# the properties the fixture exists for, by construction
assert {c["q"] for c in cs} >= {3, 4, 6, 10}
for q in (3, 4, 6, 10):
    loads = sorted(c["load"] for c in cs if c["q"] == q and c["name"].startswith("random"))
    assert loads[-1] == 1.0 and len(loads) == 4, loads
assert all(c["duplicates"] > 0 for c in cs if c["name"].startswith("random"))
assert sum(c["max_run"] > 2 for c in cs) >= 8
assert sum(c["wrapped"] for c in cs) >= 6, [c["name"] for c in cs if c["wrapped"]]
assert any(c["max_run"] == c["elements_added"] and c["elements_added"] >= 5 for c in cs)  # every key in one quotient
assert any(c["get_hashes"] is None for c in cs)
same = [c for c in cs if c.get("same_set_as")]
assert len(same) == 3 and all(c["filter"] == same[0]["filter"] and c["stream"] != same[0]["stream"] for c in same[1:])
assert all(any(c["answers"]) and not all(c["answers"]) for c in cs)
assert [e["q"] for e in EXPAND[:4]] == [3, 4, 4, 3], [e["q"] for e in EXPAND]
assert EXPAND[4]["q"] > 5 and EXPAND[5]["q"] == 5

out = Path(__file__).resolve().parent / "golden_quotient.json"
lines = ",\n".join(json.dumps(c, separators=(",", ":")) for c in CASES)
elines = ",\n".join(json.dumps(c, separators=(",", ":")) for c in EXPAND)
out.write_text('{"reference_version":%s,"seed":%d,"cases":[\n%s\n],"expand_cases":[\n%s\n]}\n' % (json.dumps(probables.__version__), SEED, lines, elines))
assert json.loads(out.read_text()) == G
print(out, out.stat().st_size, "bytes;", {c["name"]: (c["elements_added"], c["max_run"], c["wrapped"]) for c in cs}, [e["q"] for e in EXPAND])
