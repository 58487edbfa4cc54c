"""The sequential model (tests/cuckoo_model.py) IS the reference's cuckoo filter: on every case of tests/golden/golden_cuckoo.json (written
by tests/golden/gen_golden_cuckoo.py from the real reference) and, where the reference is at hand, on a few hundred random cases fed to
the live class -- buckets, counts, the op that raises and the final ``random.getstate()``.  No case is left out."""

import hashlib
import json
import os
import random
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import cuckoo_model as M  # noqa: E402

FIXTURE = json.loads((ROOT / "tests" / "golden" / "golden_cuckoo.json").read_text())
CASES = FIXTURE["cases"]
REF = Path(os.environ.get("PYPROBABLES_REFERENCE", "/root/reference"))


def tagged(tag):
    return [c for c in CASES if tag in c["tags"]]


def test_fixture_keeps_its_properties():
    assert len(CASES) >= 60 and len({c["name"] for c in CASES}) == len(CASES)
    assert (ROOT / "tests" / "golden" / "golden_cuckoo.json").stat().st_size < 200_000
    assert len(tagged("draws")) >= 20
    assert len(tagged("expands")) >= 5 and any(c["params"]["expansion_rate"] == 3 for c in tagged("expands"))
    assert sum(c["error"] == M.FULL for c in CASES) >= 5 and sum(c["error"] == M.EXPAND_FAILED for c in CASES) >= 2
    assert len(tagged("shared_fingerprint")) >= 5 and all(c["params"]["finger_size"] == 1 for c in tagged("shared_fingerprint"))
    assert len(tagged("same_index")) >= 5 and len(tagged("removes")) >= 5
    assert {c["params"]["bucket_size"] for c in CASES} >= {1, 2, 3, 4, 8}
    assert FIXTURE["kat"]["md5"] == "1371760d4ee9ccbe83e0144919750140"


def run_model(case):
    p = case["params"]
    random.seed(case["seed"])
    start = random.getstate()
    m = M.CuckooModel(p["capacity"], p["bucket_size"], p["max_swaps"], p["expansion_rate"], p["auto_expand"], p["finger_size"] * 8, M.MT19937(start))
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
    assert (m.elements_added, m.capacity) == (case["elements_added"], case["capacity"])
    assert M.state_digest(m.rng.getstate()) == case["state_sha256"]
    # the tags say what the case really does
    assert ("draws" in case["tags"]) == (m.rng.draws > 0) == (m.rng.getstate() != start)
    assert ("expands" in case["tags"]) == (m.capacity != case["params"]["capacity"])
    if "shared_fingerprint" in case["tags"]:
        used = {k for _, k in ops}
        assert len({m.fingerprint(keys[k]) for k in used}) < len(used)
    if "same_index" in case["tags"]:
        first = M.CuckooModel(case["params"]["capacity"], finger_bits=case["params"]["finger_size"] * 8)
        assert any(len(set(first.indices(first.fingerprint(keys[k])))) == 1 for _, k in ops)
    # a reloaded export holds what the table held, fingerprint 0 aside
    again = M.CuckooModel(finger_bits=m.finger_bits).load(data)
    assert again.buckets == [[fp for fp in b if fp] for b in m.buckets] and again.max_swaps == m.max_swaps


def test_known_answer_of_the_reference():
    random.seed(123)
    m = M.CuckooModel(rng=M.MT19937(random.getstate()))
    for i in range(1000):
        m.add(str(i))
    assert hashlib.md5(m.export()).hexdigest() == FIXTURE["kat"]["md5"] and m.rng.draws == 0
    assert m.elements_added == FIXTURE["kat"]["elements_added"]


def test_mt19937_is_pythons_generator():
    random.seed(99)
    g = M.MT19937(random.getstate())
    for n in (1, 2, 3, 4, 8, 1000, 2**31 - 1):
        assert [g.randbelow(n) for _ in range(700)] == [random.randrange(n) for _ in range(700)]
    assert g.getstate() == random.getstate()


def test_model_equals_live_reference_on_random_cases():
    if not (REF / "probables").is_dir():
        pytest.skip("the reference checkout is not on this machine")
    sys.path.insert(0, str(REF))
    try:
        from probables import CuckooFilter
        from probables.exceptions import CuckooFilterFullError
    finally:
        sys.path.remove(str(REF))
    pick = random.Random(11)
    kicked = expanded = raised = 0
    for run in range(300):
        p = dict(capacity=pick.randrange(5, 258), bucket_size=pick.choice([1, 2, 3, 4, 8]), max_swaps=pick.choice([1, 3, 20, 500]),
                 expansion_rate=pick.choice([2, 3]), auto_expand=pick.random() < 0.5, finger_size=pick.randrange(1, 5))
        n = min(int(p["capacity"] * p["bucket_size"] * pick.choice([0.6, 1.0, 1.2])) + 2, 400)
        keys = [f"r{run}-{i}" for i in range(n)]
        ops = []
        for i in range(n):
            ops.append(("a", i))
            if pick.random() < 0.15:
                ops.append(("r", pick.randrange(n)))
        random.seed(run)
        m = M.CuckooModel(p["capacity"], p["bucket_size"], p["max_swaps"], p["expansion_rate"], p["auto_expand"], p["finger_size"] * 8, M.MT19937(random.getstate()))
        ref = CuckooFilter(**p)
        want, err_at, err = [], None, None
        for at, (op, k) in enumerate(ops):
            try:
                want.append(ref.add(keys[k]) if op == "a" else ref.remove(keys[k]))
            except CuckooFilterFullError as ex:
                err_at, err = at, str(ex)
                break
        assert M.run_ops(m, keys, ops) == (want, err_at, err), p
        assert (m.export(), m.elements_added, m.capacity) == (bytes(ref), ref.elements_added, ref.capacity), p
        assert m.rng.getstate() == random.getstate(), p
        kicked += m.kicks > 0
        expanded += m.capacity != p["capacity"]
        raised += err is not None
    assert kicked >= 100 and expanded >= 10 and raised >= 10
