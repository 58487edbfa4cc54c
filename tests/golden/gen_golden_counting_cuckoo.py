#!/usr/bin/env python3
"""Generate tests/golden/golden_counting_cuckoo.json by running the REAL reference's CountingCuckooFilter (pyprobables,
probables/cuckoo/countingcuckoo.py).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_counting_cuckoo.py [/root/reference]

Data only.  Every case: the constructor parameters (``finger_size`` bytes, or ``error_rate`` + the ``finger_bits`` that
``init_error_rate`` makes of it), the integer `seed` handed to ``random.seed`` before the first op, the keys (``f"{prefix}{i}"`` for
i < nkeys), the op stream (``a<key index>`` = add, ``r<key index>`` = remove, comma separated: long runs of adds with about 40 % repeats,
so that one run holds repeats on both sides of an expansion), the returns of the removes in op order (one 0 / 1 each), the export (hex up
to 512 bytes, its sha256 always), ``elements_added``, ``unique_elements``, the final capacity, the index of the op that raised
CuckooFilterFullError and its message (null: none), ``check`` of every key and of the 32 probes ``f"absent-{i}"``, and the sha256 of the
625 words of ``random.getstate()`` afterwards.  `tags` says what the case exercises (tests/test_counting_cuckoo_model.py holds the fixture
to its quotas).  The model (tests/counting_cuckoo_model.py) has to agree with the reference before a case is recorded.
"""

import hashlib
import json
import random
import sys
from pathlib import Path

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

from probables import CountingCuckooFilter  # noqa: E402
from probables.exceptions import CuckooFilterFullError  # noqa: E402

import counting_cuckoo_model as M  # noqa: E402

pick = random.Random(20250311)  # chooses the cases; the cases themselves run on the global `random`, seeded per case
ABSENT = [f"absent-{i}" for i in range(32)]
RATES = [(0.3, 2), (0.05, 1), (0.01, 4), (0.001, 8), (0.2, 4), (0.1, 3), (0.04, 2)]  # (error_rate, bucket_size): widths that are no whole bytes


def candidate(seed, wide=None):
    B = wide or pick.choice([1, 2, 3, 4, 8])
    cap = pick.choice([5, 13, pick.randrange(5, 40), pick.randrange(5, 40), pick.randrange(40, 258)])
    if wide:
        cap = pick.randrange(5, 9)
    p = {
        "capacity": cap,
        "bucket_size": B,
        "max_swaps": pick.choice([1, 2, 5, 20, 100, 500]),
        "expansion_rate": pick.choice([2, 2, 3]),
        "auto_expand": pick.random() < 0.6,
    }
    if wide is None and pick.random() < 0.2:
        p["error_rate"], p["bucket_size"] = pick.choice(RATES)
        B = p["bucket_size"]
    else:
        p["finger_size"] = pick.choice([1, 1, 2, 3, 4])
    slots = cap * B
    nkeys = min(max(4, int(slots * pick.choice([0.5, 0.9, 1.1, 1.4]))), 110)
    prefix = pick.choice(["", "k", "key-", "é"])
    with_removes = pick.random() < 0.3
    ops, added = [], []
    nxt = 0
    while nxt < nkeys and len(ops) < 230:
        if added and pick.random() < 0.4:
            ops.append(("a", pick.choice(added)))  # a repeat
        else:
            ops.append(("a", nxt))
            added.append(nxt)
            nxt += 1
        if with_removes and pick.random() < 0.04:
            k = pick.choice(added)
            ops += [("r", k)] * pick.choice([1, 2, 5])  # often more removes than the key has counts
            ops += [("r", pick.randrange(nkeys)) for _ in range(pick.randrange(4))]
    return {"seed": seed, "params": p, "prefix": prefix, "nkeys": nkeys, "ops": ops}


def run(c):
    p = dict(c["params"])
    keys = [f"{c['prefix']}{i}" for i in range(c["nkeys"])]
    random.seed(c["seed"])
    before = random.getstate()
    cko = CountingCuckooFilter.init_error_rate(**p) if "error_rate" in p else CountingCuckooFilter(**p)
    bits = cko.fingerprint_size_bits
    if "error_rate" in p:
        c["params"]["finger_bits"] = bits
        assert bits % 8
    rets, err_at, err = [], None, None
    for at, (op, k) in enumerate(c["ops"]):
        try:
            if op == "a":
                cko.add(keys[k])
            else:
                rets.append(int(cko.remove(keys[k])))
        except CuckooFilterFullError as ex:
            err_at, err = at, str(ex)
            break
    after = random.getstate()
    data = bytes(cko)
    checks = [cko.check(k) for k in keys]
    absent = [cko.check(k) for k in ABSENT]

    # the model, from the same start, op by op (what the tags are read from): it must agree before the case is worth recording
    m = M.CountingCuckooModel(p["capacity"], p["bucket_size"], p["max_swaps"], p["expansion_rate"], p["auto_expand"], bits, M.MT19937(before))
    tags, mrets, merr_at, merr = set(), [], None, None
    seg_repeats, true_seen = set(), set()  # fingerprints repeated since the last failed walk of this run of adds; fingerprints a remove took
    for at, (op, k) in enumerate(c["ops"]):
        fp = m.fingerprint(keys[k])
        if op == "r":
            seg_repeats = set()
            unique = m.unique_elements
            r = m.remove(keys[k])
            mrets.append(int(r))
            if r:
                true_seen.add(fp)
            elif fp in true_seen:
                tags.add("remove_beyond")
            if m.unique_elements < unique:
                tags.add("bin_emptied")
            continue
        repeat, had = m._where(fp) is not None, len(m.leftovers)
        try:
            m.add(keys[k])
        except M.Full as ex:
            merr_at, merr = at, str(ex)
        if repeat:
            seg_repeats.add(fp)
        if len(m.leftovers) > had:  # (the first one is the walk of this add, any other an expansion's)
            if m.leftovers[had][0] in seg_repeats:
                tags.add("leftover_counted")
            seg_repeats = set()
        if merr is not None:
            break
    assert (m.export(), m.elements_added, m.unique_elements, m.capacity, merr_at, merr) == (data, cko.elements_added, cko.unique_elements, cko.capacity, err_at, err), c["seed"]
    assert m.rng.getstate() == after and mrets == rets, c["seed"]
    assert [m.check(k) for k in keys] == checks and [m.check(k) for k in ABSENT] == absent, c["seed"]

    fps = {}
    for op, k in c["ops"]:
        fps.setdefault(m.fingerprint(keys[k]), set()).add(k)
    first = M.CountingCuckooModel(p["capacity"], finger_bits=bits)
    if after != before:
        tags.add("draws")
    if cko.capacity != p["capacity"]:
        tags.add("expands")
    if err == M.FULL:
        tags.add("full")
    if err == M.EXPAND_FAILED:
        tags.add("expand_failed")
    if m.count_resets:
        tags.add("count_reset")
    if any(len(v) > 1 for v in fps.values()):
        tags.add("shared_fingerprint")
    if any(len(set(first.indices(fp))) == 1 for fp in fps):
        tags.add("same_index")
    if any(op == "r" for op, _ in c["ops"]):
        tags.add("removes")
    if 0 in fps:
        tags.add("zero_fingerprint")
    out = {
        "name": f"s{c['seed']}_c{p['capacity']}x{p['bucket_size']}",
        "seed": c["seed"],
        "params": c["params"],
        "prefix": c["prefix"],
        "nkeys": c["nkeys"],
        "ops": ",".join(f"{op}{k}" for op, k in c["ops"]),
        "remove_returns": "".join(map(str, rets)),
        "export_sha256": hashlib.sha256(data).hexdigest(),
        "elements_added": cko.elements_added,
        "unique_elements": cko.unique_elements,
        "capacity": cko.capacity,
        "error_index": err_at,
        "error": err,
        "checks": checks,
        "absent": absent,
        "state_sha256": M.state_digest(after),
        "tags": sorted(tags),
    }
    if len(data) <= 512:
        out["export_hex"] = data.hex()
    return out


QUOTA = {"draws": 24, "expands": 7, "full": 5, "expand_failed": 2, "removes": 8, "shared_fingerprint": 5, "same_index": 5, "count_reset": 5,
         "leftover_counted": 5, "bin_emptied": 5, "remove_beyond": 5, "zero_fingerprint": 2}


def main():
    cases, have, by_b, rate3, odd = [], dict.fromkeys(QUOTA, 0), dict.fromkeys([1, 2, 3, 4, 8, 16, 32], 0), 0, 0
    need_b = {1: 4, 2: 4, 3: 4, 4: 4, 8: 4, 16: 2, 32: 2}
    seed = 0
    while (len(cases) < 64 or any(have[t] < q for t, q in QUOTA.items()) or any(by_b[b] < q for b, q in need_b.items()) or rate3 < 1 or odd < 8):
        seed += 1
        wide = next((b for b in (16, 32) if by_b[b] < need_b[b]), None) if seed % 5 == 0 else None
        c = run(candidate(seed, wide))
        B = c["params"]["bucket_size"]
        r3 = "expands" in c["tags"] and c["params"]["expansion_rate"] == 3
        is_odd = "error_rate" in c["params"]
        wanted = any(have[t] < QUOTA[t] for t in c["tags"]) or by_b[B] < need_b[B] or (r3 and rate3 < 1) or (is_odd and odd < 8)
        if not wanted and len(cases) >= 64:
            continue
        cases.append(c)
        by_b[B] += 1
        rate3 += r3
        odd += is_odd
        for t in c["tags"]:
            have[t] += 1
        assert seed < 5000

    path = HERE / "golden_counting_cuckoo.json"
    path.write_text(json.dumps({"cases": cases}, separators=(",", ":")).replace('},{"name"', '},\n{"name"') + "\n")
    size = path.stat().st_size
    print(path, size, "bytes;", len(cases), "cases;", have, by_b, "rate3", rate3, "odd widths", odd)
    assert size < 200_000


if __name__ == "__main__":
    main()
