"""The canonical-layout model (tests/qf_model.py) IS the reference's quotient filter: on every case of tests/golden/golden_quotient.json
(written by tests/golden/gen_golden_quotient.py from the real reference) and, where the reference is at hand, on a few hundred random
permutations of random sets fed to the live class.  No case is left out: there is no exclusion predicate."""

import json
import os
import random
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import qf_model as M  # noqa: E402

FIXTURE = json.loads((ROOT / "tests" / "golden" / "golden_quotient.json").read_text())
CASES, EXPAND = FIXTURE["cases"], FIXTURE["expand_cases"]
REF = Path(os.environ.get("PYPROBABLES_REFERENCE", "/root/reference"))  # the checkout the generator scripts default to


def assert_arrays(case, hashes, q):
    filt, occ, cont, sh = M.canonical(hashes, q)
    assert filt.tolist() == case["filter"]
    assert occ.tolist() == case["occupied"]
    assert cont.tolist() == case["continuation"]
    assert sh.tolist() == case["shifted"]


def test_fixture_keeps_its_properties():
    assert {c["q"] for c in CASES} >= {3, 4, 6, 10}
    for q in (3, 4, 6, 10):
        size = 1 << q
        assert {int(size * 0.3), int(size * 0.6), int(size * 0.85), size} <= {c["elements_added"] for c in CASES if c["q"] == q}
        assert any(c["load"] == 1.0 and c["get_hashes"] is None for c in CASES if c["q"] == q)
    assert sum(c["duplicates"] > 0 for c in CASES) >= 16
    assert sum(c["max_run"] > 2 for c in CASES) >= 8 and sum(c["wrapped"] for c in CASES) >= 6
    assert any(c["max_run"] == c["elements_added"] >= 5 for c in CASES)
    assert len({tuple(c["stream"]) for c in CASES if c.get("same_set_as")}) == 3
    assert all(len(c["occupied"]) == 1 << c["q"] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_equals_reference_fixture(case):
    q = case["q"]
    assert_arrays(case, case["stream"], q)
    assert len(set(case["stream"])) == case["elements_added"]
    if case["get_hashes"] is None:
        with pytest.raises(ValueError):
            M.reference_order(case["stream"], q)
    else:
        assert M.reference_order(case["stream"], q) == case["get_hashes"]
        assert sorted(case["get_hashes"]) == M.sorted_hashes(case["stream"])
    assert M.contains(case["stream"], case["probes"]) == case["answers"]


@pytest.mark.parametrize("case", EXPAND, ids=[c["name"] for c in EXPAND])
def test_model_expand_rule_equals_reference_fixture(case):
    assert M.final_quotient(case["stream"], case["q0"]) == case["q"]
    assert_arrays(case, case["stream"], case["q"])
    assert M.reference_order(case["stream"], case["q"]) == case["get_hashes"]


def test_model_equals_live_reference_on_random_permutations():
    if not (REF / "probables").is_dir():
        pytest.skip("the reference checkout is not on this machine")
    sys.path.insert(0, str(REF))
    try:
        from probables import QuotientFilter
    finally:
        sys.path.remove(str(REF))
    rng = random.Random(7)
    runs = 0
    for q, sets, perms in ((3, 30, 4), (4, 30, 4), (5, 20, 3), (7, 10, 2)):
        size, r = 1 << q, 32 - q
        for s in range(sets):
            n = rng.choice([size, size - 1, rng.randrange(1, size + 1), rng.randrange(1, size + 1)])
            hs = set()
            while len(hs) < n:
                quot = size - 1 - rng.randrange(4) if rng.random() < 0.35 else rng.randrange(size)
                hs.add((quot << r) | rng.randrange(8 if s % 2 else 1 << r))
            want = tuple(a.tolist() for a in M.canonical(hs, q))
            for _ in range(perms):
                stream = list(hs) + rng.sample(sorted(hs), min(3, n))
                rng.shuffle(stream)
                qf = QuotientFilter(quotient=q, auto_expand=False)
                for h in stream:
                    qf.add_alt(h)
                got = (list(qf._filter), *([bits[i] for i in range(size)] for bits in (qf._is_occupied, qf._is_continuation, qf._is_shifted)))
                assert got == want, (q, stream)
                if n < size:
                    assert qf.get_hashes() == M.reference_order(hs, q)
                runs += 1
    assert runs >= 300
