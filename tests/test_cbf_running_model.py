"""tests/cbf_running_model.py against the real reference (tests/golden/golden_cbf_running.json) and against itself: the (a, p) maps compose
associatively and describe the loop, the optimistic scan plus its verification rule is exact, chunk seams do not matter."""

import itertools
import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import cbf_running_model as M  # noqa: E402

CASES = json.loads((ROOT / "tests" / "golden" / "golden_cbf_running.json").read_text())["cases"]


def load(case):
    table = np.zeros(case["m"], dtype=np.int64)
    for i, v in case["start"]:
        table[i] = v
    bins = [[h % case["m"] for h in hashes[: case["k"]]] for hashes, _ in case["ops"]]
    return table, bins, [w for _, w in case["ops"]]


def final_of(case):
    t = np.zeros(case["m"], dtype=np.int64)
    for i, v in case["final"]:
        t[i] = v
    return t


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_loop_of_the_model_is_the_reference(case):
    table, bins, w = load(case)
    tally = M.new_tally()
    assert M.serial(table, bins, w, tally) == case["results"]
    assert (table == final_of(case)).all()
    assert tally["added"] - tally["removed"] == case["elements_added"]


@pytest.mark.parametrize("cap", [1, 2, 7, 1000])
@pytest.mark.parametrize("vectorised", [False, True])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_chunked_executor_is_the_reference(case, cap, vectorised):
    table, bins, w = load(case)
    ref_table, ref_tally = table.copy(), M.new_tally()
    M.serial(ref_table, bins, w, ref_tally)
    out, tally, fast, replayed = M.execute(table, np.array(bins, dtype=np.int64) if vectorised else bins, np.array(w, dtype=np.int64) if vectorised else w, cap, vectorised)
    assert out == case["results"]
    assert (table == final_of(case)).all()
    assert tally == ref_tally
    assert fast + replayed == -(-len(bins) // cap)
    if not case["ill_formed"]:
        assert replayed == 0, "a stream whose removes are all full must not be flagged"


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_verification_flags_exactly_the_ill_formed_streams(case):
    table, bins, w = load(case)
    for scan in (M.scan_chunk_maps, lambda t, b, x: M.scan_chunk(t, np.array(b, dtype=np.int64), np.array(x, dtype=np.int64))):
        res = scan(table, bins, w)
        assert res[-2] == case["ill_formed"]


def test_both_scans_agree_value_for_value():
    for case in CASES:
        table, bins, w = load(case)
        out1, final, f1, t1 = M.scan_chunk_maps(table, bins, w)
        out2, cs, vals, f2, t2 = M.scan_chunk(table, np.array(bins, dtype=np.int64), np.array(w, dtype=np.int64))
        assert f1 == f2 and t1 == t2
        if not f1:  # (a flagged chunk's values are never used)
            assert out1 == [int(x) for x in out2]
            assert final == {int(c): int(v) for c, v in zip(cs, vals)}


def test_an_op_is_its_map_and_composition_is_composition():
    """on a toy rail, exhaustively: a sequence of adds and FULL removes applied step by step equals its composed map, from every start"""
    rail = 9
    steps = [M.add_map(w) for w in (0, 1, 3, 9, 12)] + [M.remove_map(w) for w in (0, 1, 2, 4)]
    for seq in itertools.product(steps, repeat=3):
        f = M.IDENTITY
        for g in seq:
            f = M.combine(f, g)
        for x in range(rail + 1):
            v, ok = x, True
            for a, p in seq:
                if p == M.NONE:  # a full remove: defined where the counter holds enough (or is sticky)
                    ok &= v == rail or v + a >= 0
                    v = rail if v == rail else v + a
                else:
                    v = min(v + a, rail)
            if ok:
                assert M.apply(f, x, rail) == v, (seq, x)


def test_composition_is_associative_on_random_triples_with_the_rails():
    edge = [0, 1, 2, 2**31 - 1, 2**31, M.MAX - 1, M.MAX]

    def rnd_map(r):
        w = edge[r % len(edge)] if (r >> 8) & 1 else (r >> 16) % 2**32
        c = 1 + (r >> 50) % 3
        return M.op_map(w if (r >> 9) & 1 else -w, c)

    for t in range(3000):
        f, g, h = (rnd_map(M.sm(3 * t + j)) for j in range(3))
        lhs, rhs = M.combine(M.combine(f, g), h), M.combine(f, M.combine(g, h))
        assert lhs == rhs
        for x in edge + [M.sm(t) % 2**32]:
            assert M.apply(lhs, x) == M.apply(rhs, x)
    assert M.combine(M.IDENTITY, M.add_map(5)) == M.add_map(5) == M.combine(M.add_map(5), M.IDENTITY)
    assert M.combine(M.IDENTITY, M.remove_map(5)) == M.remove_map(5) == M.combine(M.remove_map(5), M.IDENTITY)


def test_the_duplicate_probe_rules_flag_what_the_loop_does_differently():
    """an op that moves one counter twice: the loop wraps where the scan would clamp or go below zero -- flagged, and only then"""
    for start, w, want in ((M.MAX - 3, 2, True), (M.MAX - 4, 2, False), (M.MAX - 1, 2, False), (3, -2, True), (4, -2, False), (M.MAX, -2, False)):
        table = np.array([start, 7], dtype=np.int64)
        res = M.scan_chunk_maps(table, [[0, 0]], [w])
        assert res[2] == want, (start, w)
        ref = table.copy()
        out = M.serial(ref, [[0, 0]], [w])
        got, tally, fast, replayed = M.execute(table, [[0, 0]], [w], 4)
        assert got == out and (table == ref).all() and replayed == int(want)
