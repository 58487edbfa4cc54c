#!/usr/bin/env python3
"""Generate tests/golden/golden_cuckoo.json by running the REAL reference's CuckooFilter (pyprobables, probables/cuckoo/cuckoo.py).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_cuckoo.py [/root/reference]

Data only.  Every case: the constructor parameters, the integer `seed` handed to ``random.seed`` before the first op, the keys
(``f"{prefix}{i}"`` for i < nkeys), the op stream (``a<key index>`` = add, ``r<key index>`` = remove, comma separated), the returns of the
removes in op order (one 0 / 1 each), the export (hex up to 512 bytes, its sha256 always), ``elements_added``, the final capacity, the
index of the op that raised CuckooFilterFullError and its message (null: none), and the sha256 of the 625 words of ``random.getstate()``
afterwards.  `tags` says what the case exercises (tests/test_cuckoo_model.py holds the fixture to its quotas).  `kat` is the reference's
own known-answer test (tests/cuckoo_test.py:248-266).
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

from probables import CuckooFilter  # noqa: E402
from probables.exceptions import CuckooFilterFullError  # noqa: E402

import cuckoo_model as M  # noqa: E402

pick = random.Random(20241017)  # chooses the cases; the cases themselves run on the global `random`, seeded per case


def candidate(seed):
    B = pick.choice([1, 2, 3, 4, 8])
    cap = pick.choice([5, 13, pick.randrange(5, 40), pick.randrange(5, 40), pick.randrange(40, 258)])
    slots = cap * B
    p = {
        "capacity": cap,
        "bucket_size": B,
        "max_swaps": pick.choice([1, 2, 5, 20, 100, 500]),
        "expansion_rate": pick.choice([2, 2, 3]),
        "auto_expand": pick.random() < 0.5,
        "finger_size": pick.choice([1, 1, 2, 3, 4]),
    }
    nkeys = min(max(4, int(slots * pick.choice([0.5, 0.9, 1.0, 1.3]))), 220)
    prefix = pick.choice(["", "k", "key-", "é"])
    with_removes = pick.random() < 0.3
    ops = []
    for i in range(nkeys):
        ops.append(("a", i))
        if pick.random() < 0.1:
            ops.append(("a", pick.randrange(i + 1)))  # a repeat
        if with_removes and pick.random() < 0.25:
            ops.append(("r", pick.randrange(nkeys)))
    return {"seed": seed, "params": p, "prefix": prefix, "nkeys": nkeys, "ops": ops}


def run(c):
    p = c["params"]
    keys = [f"{c['prefix']}{i}" for i in range(c["nkeys"])]
    random.seed(c["seed"])
    before = random.getstate()
    cko = CuckooFilter(**p)
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
    # the model, from the same start: it must agree before the case is worth recording
    m = M.CuckooModel(p["capacity"], p["bucket_size"], p["max_swaps"], p["expansion_rate"], p["auto_expand"], p["finger_size"] * 8, M.MT19937(before))
    mrets, merr_at, merr = M.run_ops(m, keys, [list(o) for o in c["ops"]])
    assert (m.export(), m.elements_added, m.capacity, merr_at, merr) == (data, cko.elements_added, cko.capacity, err_at, err), c["seed"]
    assert m.rng.getstate() == after and [int(r) for r in mrets if r is not None] == rets

    fps = {}
    for op, k in c["ops"]:
        fps.setdefault(m.fingerprint(keys[k]), set()).add(k)
    first = M.CuckooModel(p["capacity"], finger_bits=p["finger_size"] * 8)
    tags = []
    if after != before:
        tags.append("draws")
    if cko.capacity != p["capacity"]:
        tags.append("expands")
    if err == M.FULL:
        tags.append("full")
    if err == M.EXPAND_FAILED:
        tags.append("expand_failed")
    if p["finger_size"] == 1 and any(len(v) > 1 for v in fps.values()):
        tags.append("shared_fingerprint")
    if any(len(set(first.indices(fp))) == 1 for fp in fps):
        tags.append("same_index")
    if any(op == "r" for op, _ in c["ops"]):
        tags.append("removes")
    out = {
        "name": f"s{c['seed']}_c{p['capacity']}x{p['bucket_size']}",
        "seed": c["seed"],
        "params": p,
        "prefix": c["prefix"],
        "nkeys": c["nkeys"],
        "ops": ",".join(f"{op}{k}" for op, k in c["ops"]),
        "remove_returns": "".join(map(str, rets)),
        "export_sha256": hashlib.sha256(data).hexdigest(),
        "elements_added": cko.elements_added,
        "capacity": cko.capacity,
        "error_index": err_at,
        "error": err,
        "state_sha256": M.state_digest(after),
        "tags": tags,
    }
    if len(data) <= 512:
        out["export_hex"] = data.hex()
    return out


QUOTA = {"draws": 24, "expands": 7, "full": 7, "expand_failed": 3, "shared_fingerprint": 7, "same_index": 7, "removes": 8}


def main():
    cases, have, by_b, rate3 = [], dict.fromkeys(QUOTA, 0), dict.fromkeys([1, 2, 3, 4, 8], 0), 0
    seed = 0
    while len(cases) < 64 or any(have[t] < q for t, q in QUOTA.items()) or min(by_b.values()) < 4 or rate3 < 2:
        seed += 1
        c = run(candidate(seed))
        B = c["params"]["bucket_size"]
        r3 = "expands" in c["tags"] and c["params"]["expansion_rate"] == 3
        wanted = any(have[t] < QUOTA[t] for t in c["tags"]) or by_b[B] < 4 or (r3 and rate3 < 2)
        if not wanted and (len(cases) >= 64 or len(c["ops"]) > 600):
            continue
        if len(cases) >= 90 and not wanted:
            continue
        cases.append(c)
        by_b[B] += 1
        rate3 += r3
        for t in c["tags"]:
            have[t] += 1
        assert seed < 5000

    random.seed(0)
    cko = CuckooFilter()
    for i in range(1000):
        cko.add(str(i))
    kat = {"keys": "str(i) for i < 1000", "md5": hashlib.md5(bytes(cko)).hexdigest(), "elements_added": cko.elements_added}
    assert kat["md5"] == "1371760d4ee9ccbe83e0144919750140"

    path = HERE / "golden_cuckoo.json"
    path.write_text(json.dumps({"kat": kat, "cases": cases}, separators=(",", ":")).replace('},{"name"', '},\n{"name"') + "\n")
    print(path, path.stat().st_size, "bytes;", len(cases), "cases;", have, by_b, "rate3", rate3)


if __name__ == "__main__":
    main()
