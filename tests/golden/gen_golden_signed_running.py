#!/usr/bin/env python3
"""Generate tests/golden/golden_signed_running.json by running the REAL reference's CountMinSketch family and StreamThreshold
(pyprobables v0.7.0, probables/countminsketch/countminsketch.py:257-321, :775-835) over mixed add / remove streams: op i is
``add(key_i, w_i)`` for ``w_i >= 0`` and ``remove(key_i, -w_i)`` for ``w_i < 0``.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_signed_running.py /path/to/pyprobables   (or PYPROBABLES_REFERENCE)

Data only: every case's recipe (tests/signed_running_model.py, tests/hitters_recipe.py) and what the reference produced for it --
sha256 of the per-op return values (int64 LE), sha256 of the final export bytes, the final bins of the small tables, elements_added, how
many (op, row) pairs clamped, the tracked dict of a StreamThreshold as an ordered list of pairs.
"""

import hashlib
import json
import os
import sys
from pathlib import Path

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ["PYPROBABLES_REFERENCE"]
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import probables  # noqa: E402

import hitters_recipe as R  # noqa: E402
import signed_running_model as M  # noqa: E402

I64_MAX, I64_MIN = M.I64[1], M.I64[0]


def case(name, cls, width, depth, n, pool, salt, weights, key_kind="str", param=None, preload=None):
    return {"name": name, "cls": cls, "param": param, "width": width, "depth": depth, "n": n, "R": pool, "salt": salt, "key_kind": key_kind,
            "weights": weights, "preload": preload}


CASES = [
    case("cms_min_unit", "CountMinSketch", 1000, 5, 3000, 800, 21, "unit"),
    case("cms_min_depth1_tiny", "CountMinSketch", 8, 1, 700, 40, 22, "small", "key16"),
    case("cmean_small_even_depth", "CountMeanSketch", 64, 4, 3000, 500, 23, "small"),
    case("cmeanmin_small", "CountMeanMinSketch", 256, 3, 3000, 600, 24, "small", "key16"),
    case("cmeanmin_unit_even_depth", "CountMeanMinSketch", 9, 2, 1500, 100, 25, "unit"),
    case("cms_rails_both", "CountMinSketch", 8, 2, 2000, 30, 26, "rail", "str", None, {"bins": "both", "below": 3, "elements_added": I64_MAX - 10}),
    case("cmean_rails_low", "CountMeanSketch", 16, 3, 2000, 60, 27, "rail", "key16", None, {"bins": "lo", "below": 5, "elements_added": I64_MIN + 10}),
    case("cmeanmin_rails_high", "CountMeanMinSketch", 32, 5, 1000, 90, 28, "rail", "str", None, {"bins": "hi", "below": 2, "elements_added": 12345}),
    case("st_min_unit", "StreamThreshold", 1000, 5, 3000, 300, 29, "unit", "str", 3),
    case("st_mean_small_key16", "StreamThreshold:mean", 500, 4, 3000, 400, 30, "small", "key16", 12),
    case("st_meanmin_small", "StreamThreshold:mean-min", 128, 3, 2500, 300, 31, "small", "str", 8),
    case("st_add_then_remove", "StreamThreshold", 300, 4, 3000, 200, 32, "add_then_remove", "key16", 60),
    case("st_one_key", "StreamThreshold", 1000, 5, 1200, 1, 33, "add_then_remove", "str", 500),
]
CLASSES = {"CountMinSketch": probables.CountMinSketch, "CountMeanSketch": probables.CountMeanSketch, "CountMeanMinSketch": probables.CountMeanMinSketch}


def run(c):
    image = M.preload_bytes(c)
    name, _, query = c["cls"].partition(":")
    if name == "StreamThreshold":
        sk = probables.StreamThreshold.frombytes(image, threshold=c["param"]) if image else probables.StreamThreshold(threshold=c["param"], width=c["width"], depth=c["depth"])
        if query:
            sk.query_type = query
    else:
        sk = CLASSES[name].frombytes(image) if image else CLASSES[name](width=c["width"], depth=c["depth"])
        sk.query_type = {"CountMinSketch": "min", "CountMeanSketch": "mean", "CountMeanMinSketch": "mean-min"}[name]  # (frombytes leaves 'min')
    keys, w = R.stream_keys(c), M.stream_weights(c).tolist()
    before = list(sk._bins)
    results, clamps, pops, els_seen, els_high, els_low = [], 0, 0, [], 0, 0
    hashes = M.fnv_matrix(keys, c["depth"])
    for i, (k, x) in enumerate(zip(keys, w)):
        for s in range(c["depth"]):  # an (op, row) pair clamps when the unclamped value lies strictly outside the rails
            v = sk._bins[int(hashes[i, s]) % c["width"] + s * c["width"]] + x
            clamps += v > M.I32[1] or v < M.I32[0]
        els_high += sk.elements_added + x > I64_MAX
        els_low += sk.elements_added + x < I64_MIN
        held = name == "StreamThreshold" and k in sk.meets_threshold
        results.append(sk.add(k, x) if x >= 0 else sk.remove(k, -x))
        pops += held and k not in sk.meets_threshold
        els_seen.append(sk.elements_added)
    raw = bytes(sk)
    out = dict(c)
    out.update({"query": sk.query_type, "results_sha256": M.results_sha(results), "results_head": results[:8], "export_sha256": hashlib.sha256(raw).hexdigest(),
                "elements_added": sk.elements_added, "clamps": clamps, "els_clamps": [els_low, els_high], "negative_bins": sum(1 for b in sk._bins if b < 0),
                "els_not_monotone": any(a > b for a, b in zip(els_seen, els_seen[1:])) and any(a < b for a, b in zip(els_seen, els_seen[1:])),
                "bins": list(sk._bins) if len(before) <= 600 else None})
    if name == "StreamThreshold":
        out.update({"tracked": R.dict_pairs(c, sk.meets_threshold), "pops": pops})
    return out


G = {"reference_version": probables.__version__, "seed": R.SEED, "cases": [run(c) for c in CASES]}
cs = G["cases"]
# the properties the fixture exists for
assert {c["query"] for c in cs} == {"min", "mean", "mean-min"} and {c["query"] for c in cs if "tracked" in c} == {"min", "mean", "mean-min"}
assert any(c["clamps"] > 0 and c["preload"] and c["preload"]["bins"] == b for c in cs for b in ("both",)), "no case clamps at both rails"
assert all(c["clamps"] > 0 for c in cs if c["preload"]), "a preloaded case never clamps"
assert any(c["query"] == "mean-min" and c["negative_bins"] and c["els_not_monotone"] for c in cs), "no mean-min case with negative bins"
assert all(c["tracked"] for c in cs if "tracked" in c) and any(c.get("pops", 0) > 0 for c in cs), "a dict is empty, or nothing is ever popped"
assert any(c["els_clamps"][0] for c in cs) and any(c["els_clamps"][1] for c in cs), "elements_added never clamps at one of the int64 rails"

out = Path(__file__).resolve().parent / "golden_signed_running.json"
out.write_text(json.dumps(G, indent=1) + "\n")
print(out, out.stat().st_size, "bytes;", {c["name"]: (c["clamps"], c["negative_bins"], c.get("pops"), len(c.get("tracked", []))) for c in cs})
