"""tests/golden/golden_quotient_insert.json (written by tests/golden/gen_golden_quotient_insert.py from the real reference) for the tests that
read it; the layout is golden_quotient_remove.json's, so tests/qf_remove_fixture.py's helpers serve both."""

from __future__ import annotations

import json
from pathlib import Path

from qf_remove_fixture import dense, held_after, same_tables  # noqa: F401

ROOT = Path(__file__).resolve().parent.parent
PATH = ROOT / "tests" / "golden" / "golden_quotient_insert.json"
FIXTURE = json.loads(PATH.read_text())
CASES = FIXTURE["cases"]
IDS = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}


def in_place_steps(case):
    """-> [(held before, step, held after)] of the add steps into a loaded table that keep the quotient and raise nothing"""
    out, before, q = [], frozenset(), case["q0"]
    for st, held in zip(case["steps"], held_after(case)):
        if st["op"] == "add" and not st["raised"] and before and st["q"] == q:
            out.append((before, st, held))
        before, q = held, st["q"]
    return out
