"""The sequential model (tests/counting_cuckoo_model.py) IS the reference's counting cuckoo filter: on every case of
tests/golden/golden_counting_cuckoo.json (written by tests/golden/gen_golden_counting_cuckoo.py from the real reference) and, where the
reference is at hand, on 300 random op streams fed to the live class -- bins, both totals, the op that raises, the remove returns, the
counts ``check`` gives and the final ``random.getstate()``.  No case is left out."""

import hashlib
import json
import math
import os
import random
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import counting_cuckoo_model as M  # noqa: E402

PATH = ROOT / "tests" / "golden" / "golden_counting_cuckoo.json"
CASES = json.loads(PATH.read_text())["cases"]
ABSENT = [f"absent-{i}" for i in range(32)]
REF = Path(os.environ.get("PYPROBABLES_REFERENCE", "/root/reference"))
QUOTA = {"draws": 24, "expands": 7, "full": 5, "expand_failed": 2, "removes": 8, "shared_fingerprint": 5, "same_index": 5, "count_reset": 5,
         "leftover_counted": 5, "bin_emptied": 5, "remove_beyond": 5, "zero_fingerprint": 2}


def tagged(tag):
    return [c for c in CASES if tag in c["tags"]]


def bits_of(p):
    if "error_rate" in p:
        assert p["finger_bits"] == math.ceil(math.log2(1.0 / p["error_rate"]) + math.log2(p["bucket_size"]) + 1)
        return p["finger_bits"]
    return p["finger_size"] * 8


def test_fixture_keeps_its_quotas():
    assert len(CASES) >= 64 and len({c["name"] for c in CASES}) == len(CASES) and PATH.stat().st_size < 200_000
    for tag, quota in QUOTA.items():
        assert len(tagged(tag)) >= quota, tag
    assert any(c["params"]["expansion_rate"] == 3 for c in tagged("expands"))
    assert sum(c["error"] == M.FULL for c in CASES) >= 5 and sum(c["error"] == M.EXPAND_FAILED for c in CASES) >= 2
    sizes = [c["params"]["bucket_size"] for c in CASES]
    assert set(sizes) >= {1, 2, 3, 4, 8} and sizes.count(16) >= 2 and sizes.count(32) >= 2
    assert all(5 <= c["params"]["capacity"] <= 257 for c in CASES)
    assert {c["params"]["finger_size"] for c in CASES if "finger_size" in c["params"]} == {1, 2, 3, 4}
    assert sum("error_rate" in c["params"] and bits_of(c["params"]) % 8 != 0 for c in CASES) >= 8
    for c in CASES:
        assert len(c["checks"]) == c["nkeys"] and len(c["absent"]) == 32
        adds = [o[0] == "a" for o in c["ops"].split(",")]
        assert max(len(run) for run in "".join("a" if a else " " for a in adds).split()) >= 4


def run_model(case):
    p = case["params"]
    random.seed(case["seed"])
    start = random.getstate()
    m = M.CountingCuckooModel(p["capacity"], p["bucket_size"], p["max_swaps"], p["expansion_rate"], p["auto_expand"], bits_of(p), M.MT19937(start))
    keys = [f"{case['prefix']}{i}" for i in range(case["nkeys"])]
    ops = [(o[0], int(o[1:])) for o in case["ops"].split(",")]
    rets, err_at, err = M.run_ops(m, keys, ops)
    return m, keys, ops, rets, err_at, err, start


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_equals_reference_fixture(case):
    m, keys, ops, rets, err_at, err, start = run_model(case)
    data = m.export()
    assert (err_at, err) == (case["error_index"], case["error"])
    assert "".join(str(int(r)) for r in rets if r is not None) == case["remove_returns"]
    if "export_hex" in case:
        assert data.hex() == case["export_hex"]
    assert hashlib.sha256(data).hexdigest() == case["export_sha256"]
    assert (m.elements_added, m.unique_elements, m.capacity) == (case["elements_added"], case["unique_elements"], case["capacity"])
    assert [m.check(k) for k in keys] == case["checks"] and [m.check(k) for k in ABSENT] == case["absent"]
    assert M.state_digest(m.rng.getstate()) == case["state_sha256"]
    # the tags say what the case really does
    assert ("draws" in case["tags"]) == (m.rng.draws > 0) == (m.rng.getstate() != start)
    assert ("expands" in case["tags"]) == (m.capacity != case["params"]["capacity"]) == (m.expansions > 0)
    assert ("count_reset" in case["tags"]) == (m.count_resets > 0)
    assert ("full" in case["tags"]) == (err == M.FULL) and ("expand_failed" in case["tags"]) == (err == M.EXPAND_FAILED)
    assert ("zero_fingerprint" in case["tags"]) == any(m.fingerprint(keys[k]) == 0 for _, k in ops)
    assert m.unique_elements == sum(map(len, m.buckets))
    # a reloaded export holds what the table held, fingerprint 0 aside; its total is the sum of the counts
    back = M.CountingCuckooModel(rng=None).load(data)
    assert back.bins() == [[b for b in row if b[0]] for row in m.bins()]
    assert back.elements_added == sum(c for row in back.bins() for _, c in row)


def test_an_expansion_loses_counts():
    """capacity 5 x 2, each of 8 keys three times, then 32 more keys: both totals end at the number of bins, the counts sum to more, and
    the tripled key whose bin had to walk during an expansion answers 1 (countingcuckoo.py:247, :235-241)"""
    random.seed(0)
    m = M.CountingCuckooModel(5, 2, rng=M.MT19937(random.getstate()))
    for _ in range(3):
        for i in range(8):
            m.add(f"k{i}")
    assert (m.elements_added, m.unique_elements) == (24, 8)
    for i in range(8, 40):
        m.add(f"k{i}")
    assert (m.elements_added, m.unique_elements, m.capacity, m.count_resets) == (40, 40, 40, 1)
    assert sum(c for row in m.bins() for _, c in row) == 54
    assert [m.check(f"k{i}") for i in range(8)] == [3, 3, 1, 3, 3, 3, 3, 3]


@pytest.mark.skipif(not (REF / "probables" / "cuckoo" / "countingcuckoo.py").is_file(), reason="the reference checkout is not present")
def test_model_equals_live_reference_on_random_streams():
    sys.path.insert(0, str(REF))
    try:
        from probables import CountingCuckooFilter
        from probables.exceptions import CuckooFilterFullError
    finally:
        sys.path.remove(str(REF))
    pick = random.Random(7)
    seen = {"expands": 0, "full": 0, "count_reset": 0}
    for trial in range(300):
        B, cap = pick.choice([1, 2, 3, 4, 8]), pick.randrange(3, 40)
        p = dict(capacity=cap, bucket_size=B, max_swaps=pick.choice([1, 3, 20, 200]), expansion_rate=pick.choice([2, 3]), auto_expand=pick.random() < 0.6,
                 finger_size=pick.choice([1, 2, 4]))
        nkeys = max(4, int(cap * B * pick.choice([0.6, 1.0, 1.5])))
        keys = [f"t{trial}-{i}" for i in range(nkeys)]
        ops = []
        for i in range(nkeys):
            ops.append(("a", i))
            while pick.random() < 0.4:
                ops.append(("a", pick.randrange(i + 1)))
            if pick.random() < 0.1:
                ops += [("r", pick.randrange(nkeys))] * pick.randrange(1, 4)
        random.seed(trial)
        start = random.getstate()
        ref = CountingCuckooFilter(**p)
        rets, err_at, err = [], None, None
        for at, (op, k) in enumerate(ops):
            try:
                rets.append(ref.add(keys[k]) if op == "a" else ref.remove(keys[k]))
            except CuckooFilterFullError as ex:
                err_at, err = at, str(ex)
                break
        after = random.getstate()
        m = M.CountingCuckooModel(cap, B, p["max_swaps"], p["expansion_rate"], p["auto_expand"], p["finger_size"] * 8, M.MT19937(start))
        assert M.run_ops(m, keys, ops) == (rets, err_at, err), trial
        assert (m.export(), m.elements_added, m.unique_elements, m.capacity) == (bytes(ref), ref.elements_added, ref.unique_elements, ref.capacity), trial
        assert m.rng.getstate() == after and [m.check(k) for k in keys] == [ref.check(k) for k in keys], trial
        assert m.bins() == [[(b.finger, b.count) for b in row] for row in ref.buckets], trial
        seen["expands"] += m.expansions > 0
        seen["full"] += err == M.FULL
        seen["count_reset"] += m.count_resets > 0
    assert all(v >= 5 for v in seen.values()), seen
