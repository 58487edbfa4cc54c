"""tests/golden/golden_quotient_remove.json (written by tests/golden/gen_golden_quotient_remove.py from the real reference) for the tests
that read it: the cases, each step's arrays made dense, and the set a table holds behind each step."""

from __future__ import annotations

import json
from pathlib import Path

import numpy as np

import qf_model as M

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = json.loads((ROOT / "tests" / "golden" / "golden_quotient_remove.json").read_text())
CASES = FIXTURE["cases"]
IDS = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}


def dense(step):
    """-> (filter, occupied, continuation, shifted) of a step as tests/qf_model.canonical gives them"""
    q = step["q"]
    size = 1 << q
    filt = np.zeros(size, dtype=M.remainder_dtype(q))
    if step["filter"]:
        at = np.asarray(step["filter"], dtype=np.int64)
        filt[at[:, 0]] = at[:, 1]
    out = [filt]
    for name in ("occupied", "continuation", "shifted"):
        a = np.zeros(size, dtype=np.uint8)
        a[np.asarray(step[name], dtype=np.int64)] = 1
        out.append(a)
    return tuple(out)


def held_after(case):
    """the set of hashes the table holds behind each step (a stream that raised inserted nothing: those are one hash long)"""
    s, out = set(), []
    for st in case["steps"]:
        if st["op"] == "add" and not st["raised"]:
            s |= set(st["hashes"])
        elif st["op"] == "remove":
            s -= set(st["hashes"])
        out.append(frozenset(s))
    return out


def same_tables(got, want) -> bool:
    return all(np.array_equal(g, w) for g, w in zip(got, want)) and all(g.dtype == w.dtype for g, w in zip(got, want))
