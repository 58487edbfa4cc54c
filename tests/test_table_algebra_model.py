"""The numpy model of the table algebra (tests/table_algebra_model.py) IS the reference's: it reproduces every case of
tests/golden/golden_table_algebra.json (written by tests/golden/gen_golden_table_algebra.py from the real reference) exactly -- the join with
its frozen rails and both joins in a row, `elements_added` at INT64_MIN / INT64_MAX, union / intersection / jaccard_index in both directions,
the OverflowError exactly where a sum passes 2^32 - 1, and the saturating add / remove on a table that came out of the algebra.  The GPU file
(tests/test_gpu_table_algebra.py) may therefore use the model at sizes the reference is too slow for."""

import json
import math
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import table_algebra_model as M  # noqa: E402

PATH = ROOT / "tests" / "golden" / "golden_table_algebra.json"
G = json.loads(PATH.read_text())
OVERFLOW = {"type": "OverflowError", "message": "unsigned int is greater than maximum"}


def by_name(cases):
    return [pytest.param(c, id=c["name"]) for c in cases]


def estimate_elements(bits_set: int, m: int, k: int) -> int:
    """bloom.py:340-352"""
    if bits_set >= m:
        return -1
    return int(-(m / k) * math.log(1 - bits_set / m))


def test_fixture_holds_every_branch():
    assert PATH.stat().st_size < 200_000 and G["reference_version"] == "0.7.0"
    jb = {b["name"]: (b["self"], b["second"]) for b in G["join_branches"]}
    for rail in (M.I32_MAX, M.I32_MIN):       # self on each rail against a positive, a negative and a zero second
        seconds = [o for s, o in jb.values() if s == rail]
        assert any(o > 0 for o in seconds) and any(o < 0 for o in seconds) and 0 in seconds
    sums = [s + o for s, o in jb.values() if s not in (M.I32_MAX, M.I32_MIN)]
    assert {M.I32_MAX, M.I32_MAX + 1, M.I32_MIN, M.I32_MIN - 1, 0} <= set(sums)
    assert jb["min_plus_min"] == (M.I32_MIN, M.I32_MIN) and jb["max_plus_max"] == (M.I32_MAX, M.I32_MAX)
    for c in G["join"]:                       # every case holds every branch; the ends of elements_added occur
        assert set(c["branches"]) == set(jb)
    ends = {c["joined_elements_added"] for c in G["join"]} | {c["joined_twice_elements_added"] for c in G["join"]}
    assert {M.I64_MAX, M.I64_MIN} <= ends
    cb = {b["name"]: (b["a"], b["b"]) for b in G["cbf_branches"]}
    assert sum(a + b == M.U32_MAX and a and b for a, b in cb.values()) >= 3
    assert (0, M.U32_MAX) in cb.values() and (M.U32_MAX, 0) in cb.values()
    assert any(a >= 2**31 > b > 0 for a, b in cb.values()) and any(b >= 2**31 > a > 0 for a, b in cb.values())
    assert any(a >= 2**31 and b >= 2**31 for a, b in cb.values())
    assert sum(c["union_error"] is not None for c in G["cbf"]) >= 3 and sum(c["union_error"] is None for c in G["cbf"]) >= 5


@pytest.mark.parametrize("case", by_name(G["join"]))
def test_join_as_recorded(case):
    a, b = case["a_bins"], case["b_bins"]
    once = M.join(a, b)
    assert once.tolist() == case["joined_bins"]
    assert M.join(once, b).tolist() == case["joined_twice_bins"]      # bins that reached a rail in the first join stay frozen
    e1 = M.join_elements(case["a_elements_added"], case["b_elements_added"])
    assert e1 == case["joined_elements_added"]
    assert M.join_elements(e1, case["b_elements_added"]) == case["joined_twice_elements_added"]
    assert (case["b_bins_after"], case["b_elements_added_after"]) == (b, case["b_elements_added"])
    for name, x, y, r in zip(case["branches"], a, b, case["joined_bins"]):
        if "frozen" in name:
            assert r == x, name
        if name.startswith("sum_exactly") or name.startswith("cancel_") and "minus_one" not in name:
            assert r == x + y, name


@pytest.mark.parametrize("case", by_name(G["cbf"]))
def test_union_intersection_jaccard_as_recorded(case):
    a, b, m, k = case["a_table"], case["b_table"], case["m"], case["k"]
    assert (case["a_table_after"], case["b_table_after"]) == (a, b)
    assert (M.nonzero(a), M.nonzero(b)) == (case["a_bits_set"], case["b_bits_set"])
    assert (M.jaccard(a, b), M.jaccard(b, a), M.jaccard(a, a)) == (case["jaccard"], case["jaccard_ba"], case["jaccard_self"])
    for op, fn in (("union", M.add_u32), ("intersection", M.intersect)):
        for tag, (x, y) in (("", (a, b)), ("_ba", (b, a))):
            tab, overflowed = fn(x, y)
            if overflowed:                     # the class turns a non-zero tally into the reference's exception
                assert case[f"{op}{tag}_error"] == OVERFLOW and case[f"{op}{tag}_table"] is None
                continue
            assert case[f"{op}{tag}_error"] is None
            assert tab.tolist() == case[f"{op}{tag}_table"]
            assert estimate_elements(M.nonzero(tab), m, k) == case[f"{op}{tag}_elements_added"]
    if case["union_error"] is None:            # union as two sums onto a cleared table, as the class does it
        first, ov = M.add_u32(np.zeros(m, dtype=np.int64), a)
        assert ov == 0 and M.add_u32(first, b)[0].tolist() == case["union_table"]


def fnv_1a(key: str, seed: int = 0) -> int:
    """hashes.py:86-103"""
    h = (14695981039346656037 + 31 * seed) & (2**64 - 1)
    for c in map(ord, key):
        h = ((h ^ c) * 1099511628211) & (2**64 - 1)
    return h


def default_hashes(key: str, depth: int):
    """hashes.py:71-83 default_fnv_1a"""
    return [fnv_1a(key, i) for i in range(depth)]


@pytest.mark.parametrize("case", by_name(G["cbf_follow_on"]))
def test_adds_onto_a_union_or_intersection_as_recorded(case):
    fn = M.add_u32 if case["op"] == "union" else M.intersect
    tab, ov = fn(case["a_table"], case["b_table"])
    assert ov == 0 and tab.tolist() == case["result_table"]
    m, delta, els = len(tab), np.zeros(len(tab), dtype=np.int64), case["result_elements_added"]
    k = next(c["k"] for c in G["cbf"])
    for op in case["ops"]:
        idx = [h % m for h in default_hashes(op["key"], k)]
        one = np.zeros(m, dtype=np.int64)
        np.add.at(one, idx, op["count"])
        # countingbloom.py:146-155: the value returned is the min over the k cells of min(before + count, rail), `before` read up front
        before = M.cbf_add_delta(tab, delta)
        assert min(min(int(before[i]) + op["count"], M.U32_MAX) for i in idx) == op["returned"]
        delta += one
        els = min(els + op["count"], M.U64_MAX)
        assert els == op["elements_added"]
    assert M.cbf_add_delta(tab, delta).tolist() == case["final_table"]       # saturating adds commute: one delta for the whole stream
    assert els == case["final_elements_added"]
    if "small" not in case["name"]:
        assert M.U32_MAX in case["final_table"] and M.U32_MAX in case["final_checks"]
        assert int((tab + delta).max()) > M.U32_MAX                          # a wrapping add would have passed the rail here
    else:
        assert int((tab + delta).max()) < 2**31


@pytest.mark.parametrize("case", by_name(G["cms_follow_on"]))
def test_adds_and_removes_onto_a_join_as_recorded(case):
    bins = M.join(case["a_bins"], case["b_bins"])
    assert bins.tolist() == case["joined_bins"]
    els = M.join_elements(case["a_elements_added"], case["b_elements_added"])
    assert els == case["joined_elements_added"]
    w = case["width"]
    for op in case["ops"]:
        idx = [h % w + i * w for i, h in enumerate(default_hashes(op["key"], case["depth"]))]
        one = np.zeros(len(bins), dtype=np.int64)
        np.add.at(one, idx, op["count"])
        bins = M.cms_add_delta(bins, one) if op["op"] == "add" else M.cms_remove_delta(bins, one)
        els = M.join_elements(els, op["count"] if op["op"] == "add" else -op["count"])
        assert min(int(bins[i]) for i in idx) == op["returned"]              # query 'min' over the cells after the update
        assert els == op["elements_added"]
    assert bins.tolist() == case["final_bins"] and els == case["final_elements_added"]
    rail = M.I32_MAX if "max" in case["name"] else M.I32_MIN
    assert rail in case["final_bins"] and rail in case["final_checks"]


def test_counts_on_single_bit_words():
    """popcount, non-zero and OR over slices have no reference counterpart of their own beyond bloom.py:552-557 / countingbloom.py:302-304:
    stated on words whose only set bit is the top one, the low one, and on full words"""
    words = [0x80000000, 1, 0xFFFFFFFF, 0, 0x80000001, 0x7FFFFFFF]
    assert M.popcount(words) == sum(bin(w).count("1") for w in words) == 1 + 1 + 32 + 0 + 2 + 31
    assert M.nonzero(words) == 5
    assert M.or_slices(words, 3).tolist() == [0x80000000 | 0xFFFFFFFF | 0x80000001, 1 | 0 | 0x7FFFFFFF]
    assert M.or_slices(words, 1).tolist() == words
    assert M.table_or(words, words[::-1]).tolist() == [a | b for a, b in zip(words, words[::-1])]
    assert M.table_and(words, words[::-1]).tolist() == [a & b for a, b in zip(words, words[::-1])]
    assert M.jaccard_counts([0x80000000, 0, 1, 0], [0x80000000, 0xFFFFFFFF, 0, 0]) == (3, 1)
