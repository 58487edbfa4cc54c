"""tests/signed_running_model.py IS the reference's ordered stream of adds and removes: the composition law of clamp-add maps by brute
force on toy rails, and the numpy model of a whole batch on every case of tests/golden/golden_signed_running.json (written by
tests/golden/gen_golden_signed_running.py from the real reference) and, where the reference is at hand, on a few hundred random streams
with tables preloaded near both int32 rails and elements_added near both int64 rails."""

import hashlib
import itertools
import json
import random
import struct
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import hitters_recipe as R  # noqa: E402
import signed_running_model as M  # noqa: E402
from test_quotient_model import REF  # noqa: E402  (where the reference checkout is looked for: PYPROBABLES_REFERENCE, or that module's default)

CASES = json.loads((ROOT / "tests" / "golden" / "golden_signed_running.json").read_text())["cases"]
TOY = (-4, 3)
FOOTER = struct.Struct("IIq")


# ------------------------------------------------------------------ the law, by brute force
STARTS = range(TOY[0], TOY[1] + 1)
_toy: dict = {}


def toy_table():
    """every sequence ws of up to 4 weights in [-9, 9] -> (ws folded from the left into one map, the clamp loop's value after ws for
    every start value, its clamp count for every start value); a sequence is built on the one that is shorter by its last weight"""
    if not _toy:
        _toy[()] = (M.identity(TOY), tuple(STARTS), (0,) * len(STARTS))
        for n in range(1, 5):
            for ws in itertools.product(range(-9, 10), repeat=n):
                f, vals, clamps = _toy[ws[:-1]]
                w = ws[-1]
                raw = [v + w for v in vals]
                _toy[ws] = (M.combine(f, M.op_map(w, TOY)), tuple(M.clamp(v, *TOY) for v in raw),
                            tuple(c + (v < TOY[0] or v > TOY[1]) for c, v in zip(clamps, raw)))
    return _toy


def test_combine_is_associative_on_toy_rails():
    """every sequence of up to 4 weights in [-9, 9]: however its ops are bracketed the composed map is the same triple, and that map is
    the clamp loop on every start value"""
    table = toy_table()
    image: dict = {}  # a triple -> its values on every start value (there are few distinct triples)

    def values(f):
        if f not in image:
            image[f] = tuple(M.apply(f, x) for x in STARTS)
        return image[f]

    for ws, (folded, want, _) in table.items():
        assert values(folded) == want, ws
        for a, b in itertools.combinations(range(len(ws) + 1), 2):  # three consecutive stretches [0, a) [a, b) [b, end)
            f, g, h = table[ws[:a]][0], table[ws[a:b]][0], table[ws[b:]][0]
            fg_h = M.combine(M.combine(f, g), h)
            assert fg_h == M.combine(f, M.combine(g, h)), (ws, a, b)
            assert values(fg_h) == want, (ws, a, b)  # (the triple may differ from `folded`; the map may not)


def test_scan_equals_the_clamp_loop_on_toy_rails():
    """values and clamp count, every sequence and start value: op i's value is clamp(F_exclusive(x) + w_i) with F_exclusive the scanned
    map of the ops in front of it, and the op counts as a clamp when that unclamped sum lies strictly outside the rails.  A value that
    lands exactly on a rail is no clamp"""
    table = toy_table()
    for ws, (_, want, clamps) in table.items():
        if not ws:
            continue
        front, _, clamps_front = table[ws[:-1]]
        raw = [M.apply(front, x) + ws[-1] for x in STARTS]
        assert tuple(M.clamp(v, *TOY) for v in raw) == want, ws
        assert tuple(c + (v < TOY[0] or v > TOY[1]) for c, v in zip(clamps_front, raw)) == clamps, ws
    for ws in itertools.islice(table, 0, None, 61):  # the two whole-sequence forms of the model, on a sample
        for x in STARTS:
            assert M.scanned(x, ws, TOY) == M.sequential(x, ws, TOY), (ws, x)
            if ws:
                assert (M.sequential(x, ws, TOY)[0][-1], M.sequential(x, ws, TOY)[1]) == (table[ws][1][x - TOY[0]], table[ws][2][x - TOY[0]])
    assert M.sequential(0, (-4, -1, 3), TOY) == ([-4, -4, -1], 1)


def test_batch_model_equals_the_clamp_loop_on_toy_rails():
    """the numpy batch on toy rails against a dict-of-bins loop, a few hundred random streams"""
    rng = random.Random(5)
    for _ in range(300):
        width, depth, n = rng.choice((1, 2, 3, 7)), rng.choice((1, 2, 3)), rng.randrange(0, 40)
        h = np.array([[rng.randrange(2**64) for _ in range(depth)] for _ in range(n)], dtype=np.uint64).reshape(n, depth)
        w = [rng.randrange(-9, 10) for _ in range(n)]
        t0 = [rng.randrange(TOY[0], TOY[1] + 1) for _ in range(width * depth)]
        e0, erails = rng.randrange(-20, 21), (-20, 20)
        res, table, els, clamps = M.signed_batch(width, depth, h, w, ("min", "mean"), t0, e0, TOY, erails)
        bins, want, wc, e = list(t0), {"min": [], "mean": []}, 0, e0
        for i in range(n):
            vals = []
            for s in range(depth):
                at = int(h[i, s]) % width + s * width
                v = bins[at] + w[i]
                wc += v < TOY[0] or v > TOY[1]
                bins[at] = M.clamp(v, *TOY)
                vals.append(bins[at])
            e = M.clamp(e + w[i], *erails)
            want["min"].append(min(vals))
            want["mean"].append(sum(vals) // depth)
        assert (res["min"].tolist(), res["mean"].tolist(), table.tolist(), els, clamps) == (want["min"], want["mean"], bins, e, wc)


# ------------------------------------------------------------------ the fixture
def test_fixture_keeps_its_properties():
    assert {c["query"] for c in CASES} == {"min", "mean", "mean-min"}
    assert {c["cls"].partition(":")[0] for c in CASES} == {"CountMinSketch", "CountMeanSketch", "CountMeanMinSketch", "StreamThreshold"}
    assert all(c["n"] <= 3000 and 8 <= c["width"] <= 1000 and 1 <= c["depth"] <= 5 for c in CASES)
    assert {c["depth"] for c in CASES} >= {1, 5} and {c["width"] for c in CASES} >= {8, 1000}
    assert any(c["preload"] and c["preload"]["bins"] == "both" and c["clamps"] for c in CASES)
    assert any(c["query"] == "mean-min" and c["negative_bins"] and c["els_not_monotone"] for c in CASES)
    assert all(c["tracked"] for c in CASES if "tracked" in c) and any(c.get("pops", 0) for c in CASES)
    assert any(c["els_clamps"][0] for c in CASES) and any(c["els_clamps"][1] for c in CASES)


def case_model(case):
    keys, w = R.stream_keys(case), M.stream_weights(case)
    p = case["preload"]
    res, table, els, clamps = M.signed_batch(case["width"], case["depth"], M.fnv_matrix(keys, case["depth"]), w, case["query"], M.preload_bins(case),
                                            p["elements_added"] if p else 0)
    return keys, w, res[case["query"]], table, els, clamps


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_equals_reference_fixture(case):
    keys, w, res, table, els, clamps = case_model(case)
    assert M.results_sha(res) == case["results_sha256"] and res[:8].tolist() == case["results_head"]
    assert (els, clamps) == (case["elements_added"], case["clamps"])
    export = table.astype(np.int32).tobytes() + FOOTER.pack(case["width"], case["depth"], els)
    assert hashlib.sha256(export).hexdigest() == case["export_sha256"]
    if case["bins"] is not None:
        assert table.tolist() == case["bins"]
    if "tracked" in case:
        assert R.dict_pairs(case, M.threshold_dict({}, keys, w.tolist(), res, case["param"])) == case["tracked"]


# ------------------------------------------------------------------ the live reference
def test_model_equals_live_reference_on_random_streams():
    if not (REF / "probables").is_dir():
        pytest.skip("the reference checkout is not on this machine")
    sys.path.insert(0, str(REF))
    try:
        import probables
    finally:
        sys.path.remove(str(REF))
    classes = [(probables.CountMinSketch, "min"), (probables.CountMeanSketch, "mean"), (probables.CountMeanMinSketch, "mean-min"), (probables.StreamThreshold, "min")]
    rng = random.Random(11)
    big = (M.I32[1], -M.I32[1], M.I32[0], 0, 1, -1)
    for it in range(240):
        cls, query = classes[it % 4]
        width, depth, n = rng.choice((2, 3, 8, 50)), rng.randrange(1, 6), rng.randrange(0, 60)
        keys = ["k%d" % rng.randrange(12) for _ in range(n)]
        w = [rng.choice(big) if rng.random() < 0.4 else rng.randrange(-2**31, 2**31) if rng.random() < 0.3 else rng.randrange(-5, 6) for _ in range(n)]
        near = rng.choice(("hi", "lo", "both", "zero"))
        cells = width * depth
        t0 = [{"hi": M.I32[1] - rng.randrange(4), "lo": M.I32[0] + rng.randrange(4), "zero": rng.randrange(-3, 4)}[near if near != "both" else ("hi", "lo")[j % 2]]
              for j in range(cells)]
        # (mean-min computes elements_added - bin: Python integers on both sides, so the int64 rails are fair game here too)
        e0 = rng.choice((M.I64[1] - rng.randrange(6), M.I64[0] + rng.randrange(6), rng.randrange(-10, 10)))
        image = np.array(t0, dtype=np.int32).tobytes() + FOOTER.pack(width, depth, e0)
        thr = rng.choice((1, 5, 2**31 - 4))
        sk = cls.frombytes(image, threshold=thr) if cls is probables.StreamThreshold else cls.frombytes(image)
        sk.query_type = query  # (frombytes leaves 'min' whatever the class)
        want = [sk.add(k, x) if x >= 0 else sk.remove(k, -x) for k, x in zip(keys, w)]
        res, table, els, _ = M.signed_batch(width, depth, M.fnv_matrix(keys, depth), w if n else None, query, t0, e0)
        assert res[query].tolist() == want, (it, query)
        assert table.tolist() == list(sk._bins) and els == sk.elements_added
        if cls is probables.StreamThreshold:
            assert list(M.threshold_dict({}, keys, w, want, thr).items()) == list(sk.meets_threshold.items())
