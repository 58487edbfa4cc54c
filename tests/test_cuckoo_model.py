"""The sequential model (tests/cuckoo_model.py) IS the reference's cuckoo filter: on every case of tests/golden/golden_cuckoo.json and
tests/golden/golden_cuckoo_edges.json (written by tests/golden/gen_golden_cuckoo.py and gen_golden_cuckoo_edges.py from the real
reference; the second holds the widths that are no whole bytes and the buckets of 5 .. 32) and, where the reference is at hand, on a few
hundred random cases fed to the live class -- buckets, counts, the op that raises and the final ``random.getstate()``.  No case is left out."""

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

import cuckoo_model as M  # noqa: E402

FIXTURE = json.loads((ROOT / "tests" / "golden" / "golden_cuckoo.json").read_text())
CASES = FIXTURE["cases"]
EDGES_PATH = ROOT / "tests" / "golden" / "golden_cuckoo_edges.json"
EDGES = json.loads(EDGES_PATH.read_text())["cases"]
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


def test_edges_fixture_keeps_its_properties():
    def edged(tag):
        return [c for c in EDGES if tag in c["tags"]]

    assert len({c["name"] for c in EDGES}) == len(EDGES) and EDGES_PATH.stat().st_size < 200_000
    for B in (5, 6, 7, 12, 16, 31, 32):
        assert sum(c["params"]["bucket_size"] == B for c in edged("draws")) >= 2, B
    assert len(edged("draws")) >= 14 and len(edged("expands")) >= 5 and len(edged("full")) >= 5 and len(edged("removes")) >= 6
    assert len(edged("zero_fingerprint")) >= 4 and len(edged("odd_width")) >= 12
    assert sum(c["error"] == M.FULL for c in EDGES) >= 5
    assert {c["params"]["finger_bits"] for c in EDGES} >= {4, 10, 14, 21, 25, 29, 8, 16, 24, 32}
    assert all(3 <= c["params"]["capacity"] <= 40 and "finger_size" not in c["params"] for c in EDGES)
    assert any(c["nkeys"] >= 1.3 * c["params"]["capacity"] * c["params"]["bucket_size"] - 1 for c in EDGES)
    for c in EDGES:
        assert len(c["probe_answers"]) == c["nkeys"] + c["probes_absent"] and set(c["probe_answers"]) <= {"0", "1"}
    assert any("1" in c["probe_answers"][c["nkeys"]:] for c in EDGES) and any("0" in c["probe_answers"][:c["nkeys"]] for c in EDGES)


def bits_of(p):
    """the fingerprint width of a fixture's `params`: whole bytes in golden_cuckoo.json, what the error rate gave in golden_cuckoo_edges.json"""
    if "error_rate" in p:
        assert p["finger_bits"] == math.ceil(math.log2(1.0 / p["error_rate"]) + math.log2(p["bucket_size"]) + 1)
        return p["finger_bits"]
    return p["finger_size"] * 8


def run_model(case):
    p = case["params"]
    random.seed(case["seed"])
    start = random.getstate()
    m = M.CuckooModel(p["capacity"], p["bucket_size"], p["max_swaps"], p["expansion_rate"], p["auto_expand"], bits_of(p), M.MT19937(start))
    keys = [f"{case['prefix']}{i}" for i in range(case["nkeys"])]
    ops = [(o[0], int(o[1:])) for o in case["ops"].split(",")]
    rets, err_at, err = M.run_ops(m, keys, ops)
    return m, keys, ops, rets, err_at, err, start


@pytest.mark.parametrize("case", CASES + EDGES, ids=[c["name"] for c in CASES + EDGES])
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
        first = M.CuckooModel(case["params"]["capacity"], finger_bits=bits_of(case["params"]))
        assert any(len(set(first.indices(first.fingerprint(keys[k])))) == 1 for _, k in ops)
    if "probe_answers" in case:  # golden_cuckoo_edges.json: lookups, and what its own tags say
        probes = keys + [f"{case['prefix']}absent{i}" for i in range(case["probes_absent"])]
        assert "".join(str(int(m.check(k))) for k in probes) == case["probe_answers"]
        assert ("odd_width" in case["tags"]) == (m.finger_bits % 8 != 0)
        assert ("full" in case["tags"]) == (err == M.FULL) and ("removes" in case["tags"]) == any(op == "r" for op, _ in ops)
        if "zero_fingerprint" in case["tags"]:
            z = next(k for k in range(len(keys)) if m.fingerprint(keys[k]) == 0)
            assert ops[-1] == ("a", z) and ops.count(("r", z)) >= 1 and ops.index(("a", z)) < ops.index(("r", z)) and err is None
            assert case["probe_answers"][z] == "1" and any(0 in b for b in m.buckets)
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
    kicked = expanded = raised = wide = 0
    widths = set()
    for run in range(300):
        p = dict(capacity=pick.randrange(5, 258), bucket_size=pick.choice([1, 2, 3, 4, 8]), max_swaps=pick.choice([1, 3, 20, 500]),
                 expansion_rate=pick.choice([2, 3]), auto_expand=pick.random() < 0.5, finger_size=pick.randrange(1, 5))
        bits, make = p["finger_size"] * 8, CuckooFilter
        if run % 3 == 2:  # a width from an error rate, in buckets of up to 32
            p["bucket_size"], p["capacity"] = pick.choice([5, 6, 7, 12, 16, 17, 31, 32]), pick.randrange(3, 41)
            while True:
                p["error_rate"] = pick.choice([0.9, 0.5, 0.3, 0.1, 0.05, 0.01, 0.001, 1e-4, 1e-5, 1e-6, 1e-7, 3e-8, 1e-8])
                bits = math.ceil(math.log2(1.0 / p["error_rate"]) + math.log2(p["bucket_size"]) + 1)
                if bits <= 32:
                    break
            del p["finger_size"]
            make = CuckooFilter.init_error_rate
            widths.add(bits)
            wide += p["bucket_size"] >= 16
        n = min(int(p["capacity"] * p["bucket_size"] * pick.choice([0.6, 1.0, 1.2])) + 2, 400)
        keys = [f"r{run}-{i}" for i in range(n)]
        ops = []
        for i in range(n):
            ops.append(("a", i))
            if pick.random() < 0.15:
                ops.append(("r", pick.randrange(n)))
        random.seed(run)
        m = M.CuckooModel(p["capacity"], p["bucket_size"], p["max_swaps"], p["expansion_rate"], p["auto_expand"], bits, M.MT19937(random.getstate()))
        ref = make(**p)
        assert ref.fingerprint_size_bits == bits
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
    assert wide >= 20 and len(widths) >= 12 and sum(w % 8 != 0 for w in widths) >= 8
