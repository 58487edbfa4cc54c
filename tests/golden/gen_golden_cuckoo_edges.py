#!/usr/bin/env python3
"""Generate tests/golden/golden_cuckoo_edges.json by running the REAL reference's CuckooFilter (pyprobables, probables/cuckoo/cuckoo.py)
where golden_cuckoo.json does not go: fingerprint widths that are no whole bytes and buckets of 5 .. 32 fingerprints.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_cuckoo_edges.py [/root/reference]

Data only, the records of gen_golden_cuckoo.py with three differences.  The filter is built by ``CuckooFilter.init_error_rate``: `params`
holds ``error_rate`` instead of ``finger_size``, and beside it ``finger_bits``, the width that rate gave the reference (no constructor
argument).  ``probe_answers`` holds one 0 / 1 per probe, ``check`` asked after the last op: the case's keys in order, then ``probes_absent``
keys ``f"{prefix}absent{i}"``.  And the tags: ``odd_width`` (a width that is no multiple of 8), ``zero_fingerprint`` (a key whose
fingerprint is 0 is added, removed -- the return is among `remove_returns` -- added again as the last op and so checked among the probes),
``draws`` / ``expands`` / ``full`` / ``expand_failed`` / ``removes`` as in golden_cuckoo.json.  tests/test_cuckoo_model.py holds the
fixture to the quotas below.
"""

import hashlib
import json
import math
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

pick = random.Random(20241018)  # chooses the cases; the cases themselves run on the global `random`, seeded per case

BUCKETS = [5, 6, 7, 12, 16, 31, 32]
RATES = [0.9, 0.5, 0.3, 0.1, 0.05, 0.01, 0.001, 1e-4, 1e-5, 1e-6, 1e-7, 3e-8, 1e-8]
WIDTHS = [4, 10, 14, 21, 25, 29, 8, 16, 24, 32]  # every one of them is in the file: six that are no whole bytes, and the four that are
ABSENT = 40


def width_of(rate, B):
    return int(math.ceil(math.log2(1.0 / rate) + math.log2(B) + 1))


def candidate(seed, want_width=None):
    while True:
        B, rate = pick.choice(BUCKETS), pick.choice(RATES)
        if width_of(rate, B) <= 32 and want_width in (None, width_of(rate, B)):
            break
    cap = pick.randrange(3, min(40, 320 // B) + 1)
    p = {
        "capacity": cap,
        "bucket_size": B,
        "max_swaps": pick.choice([1, 2, 5, 20, 100, 500]),
        "expansion_rate": pick.choice([2, 2, 3]),
        "auto_expand": pick.random() < 0.5,
        "error_rate": rate,
    }
    nkeys = max(4, int(cap * B * pick.choice([0.5, 0.9, 1.0, 1.3])))
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
    bits = width_of(p["error_rate"], p["bucket_size"])
    # a key whose fingerprint is 0: removed half way, added again at the very end
    zero = next((i for i, k in enumerate(keys) if M.fnv_1a(k) & ((1 << bits) - 1) == 0), None)
    if zero is not None:
        at = max(len(c["ops"]) // 2, c["ops"].index(("a", zero)) + 1)
        c["ops"] = c["ops"][:at] + [("r", zero)] + c["ops"][at:] + [("a", zero)]
    probes = keys + [f"{c['prefix']}absent{i}" for i in range(ABSENT)]

    random.seed(c["seed"])
    before = random.getstate()
    cko = CuckooFilter.init_error_rate(**p)
    assert cko.fingerprint_size_bits == bits
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
    answers = [int(cko.check(k)) for k in probes]
    assert random.getstate() == after
    # the model, from the same start: it must agree before the case is worth recording
    m = M.CuckooModel(p["capacity"], p["bucket_size"], p["max_swaps"], p["expansion_rate"], p["auto_expand"], bits, M.MT19937(before))
    mrets, merr_at, merr = M.run_ops(m, keys, [list(o) for o in c["ops"]])
    assert (m.export(), m.elements_added, m.capacity, merr_at, merr) == (data, cko.elements_added, cko.capacity, err_at, err), c["seed"]
    assert m.rng.getstate() == after and [int(r) for r in mrets if r is not None] == rets
    assert m.buckets == [list(b) for b in cko.buckets] and [int(m.check(k)) for k in probes] == answers

    tags = []
    if after != before:
        tags.append("draws")
    if cko.capacity != p["capacity"]:
        tags.append("expands")
    if err == M.FULL:
        tags.append("full")
    if err == M.EXPAND_FAILED:
        tags.append("expand_failed")
    if any(op == "r" for op, _ in c["ops"]):
        tags.append("removes")
    if zero is not None and err is None and answers[zero] == 1:
        tags.append("zero_fingerprint")
    if bits % 8:
        tags.append("odd_width")
    out = {
        "name": f"s{c['seed']}_c{p['capacity']}x{p['bucket_size']}_w{bits}",
        "seed": c["seed"],
        "params": {**p, "finger_bits": bits},
        "prefix": c["prefix"],
        "nkeys": c["nkeys"],
        "ops": ",".join(f"{op}{k}" for op, k in c["ops"]),
        "remove_returns": "".join(map(str, rets)),
        "probes_absent": ABSENT,
        "probe_answers": "".join(map(str, answers)),
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


QUOTA = {"draws": 14, "expands": 5, "full": 5, "removes": 6, "zero_fingerprint": 4, "odd_width": 12}
DRAWS_PER_BUCKET = 2


def main():
    cases, have, draws_by_b, widths = [], dict.fromkeys(QUOTA, 0), dict.fromkeys(BUCKETS, 0), dict.fromkeys(WIDTHS, 0)
    seed = 0

    def short():
        return any(have[t] < q for t, q in QUOTA.items()) or min(draws_by_b.values()) < DRAWS_PER_BUCKET or min(widths.values()) < 1

    while short():
        seed += 1
        missing = [w for w, n in widths.items() if n < 1]
        c = run(candidate(seed, missing[0] if missing and seed % 2 else None))
        B, bits = c["params"]["bucket_size"], c["params"]["finger_bits"]
        drew = "draws" in c["tags"]
        wanted = any(have[t] < QUOTA[t] for t in c["tags"]) or (drew and draws_by_b[B] < DRAWS_PER_BUCKET) or widths.get(bits, 1) < 1
        if not wanted:
            continue
        cases.append(c)
        draws_by_b[B] += drew
        if bits in widths:
            widths[bits] += 1
        for t in c["tags"]:
            if t in have:
                have[t] += 1
        assert seed < 5000 and len(cases) < 70

    path = HERE / "golden_cuckoo_edges.json"
    path.write_text(json.dumps({"cases": cases}, separators=(",", ":")).replace('},{"name"', '},\n{"name"') + "\n")
    print(path, path.stat().st_size, "bytes;", len(cases), "cases;", have, draws_by_b, widths)


if __name__ == "__main__":
    main()
