#!/usr/bin/env python3
"""Generate tests/golden/golden_hitters.json by running the REAL reference's StreamThreshold / HeavyHitters
(pyprobables v0.7.0, probables/countminsketch/countminsketch.py:532-843) over the streams of tests/hitters_recipe.py.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_hitters.py [/root/reference]

Data only: every case's recipe and what the reference produced for it -- sha256 of the per-op return values (int64 LE), sha256 of the
final export bytes, elements_added, the tracked dict as an ordered list of pairs.
"""

import hashlib
import json
import sys
from pathlib import Path

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import probables  # noqa: E402
from probables import HeavyHitters, StreamThreshold  # noqa: E402

import hitters_recipe as R  # noqa: E402


def case(name, cls, param, width, depth, n, pool, salt, key_kind="str", weighted=False, query="min", preload=None):
    return {"name": name, "cls": cls, "param": param, "width": width, "depth": depth, "n": n, "R": pool, "salt": salt, "key_kind": key_kind,
            "weighted": weighted, "query": query, "preload": preload}


CASES = [
    case("st_min_str", "StreamThreshold", 40, 1000, 5, 20000, 5000, 1),
    case("st_mean_key16_even_depth", "StreamThreshold", 150, 4096, 4, 20000, 3000, 2, "key16", True, "mean"),
    case("st_meanmin_str", "StreamThreshold", 60, 2048, 4, 20000, 4000, 3, "str", True, "mean-min"),
    case("st_meanmin_odd_depth", "StreamThreshold", 25, 777, 3, 8000, 2000, 4, "key16", False, "mean-min"),
    case("st_tiny_table", "StreamThreshold", 600, 4, 2, 3000, 400, 5),
    case("st_saturating", "StreamThreshold", R.I32_MAX - 20, 64, 3, 6000, 300, 6, "key16", True, "min", {"below": 40, "elements_added": 12345}),
    case("st_one_key", "StreamThreshold", 2500, 1000, 5, 5000, 1, 7),
    case("hh_str", "HeavyHitters", 20, 1000, 5, 30000, 5000, 8),
    case("hh_key16_weighted_even_depth", "HeavyHitters", 50, 3000, 4, 30000, 8000, 9, "key16", True),
    case("hh_mean", "HeavyHitters", 10, 512, 3, 10000, 1500, 10, "str", True, "mean"),
    case("hh_one_key", "HeavyHitters", 5, 1000, 5, 3000, 1, 11, "key16"),
    case("hh_large", "HeavyHitters", 100, 65536, 5, 200000, 50000, 12, "key16"),
]


def run(c):
    image = R.preload_bytes(c)
    if c["cls"] == "StreamThreshold":
        sk = StreamThreshold.frombytes(image, threshold=c["param"]) if image else StreamThreshold(threshold=c["param"], width=c["width"], depth=c["depth"])
        tracked = lambda: sk.meets_threshold  # noqa: E731
    else:
        sk = HeavyHitters.frombytes(image, num_hitters=c["param"]) if image else HeavyHitters(num_hitters=c["param"], width=c["width"], depth=c["depth"])
        tracked = lambda: sk.heavy_hitters  # noqa: E731
    sk.query_type = c["query"]
    keys, w = R.stream_keys(c), R.stream_weights(c)
    results, evictions = [], 0
    for i, k in enumerate(keys):
        before = set(tracked()) if c["cls"] == "HeavyHitters" and len(tracked()) >= c["param"] else None
        results.append(sk.add(k, 1 if w is None else int(w[i])))
        if before is not None and before - set(tracked()):
            evictions += 1
    raw = bytes(sk)
    bins = raw[: 4 * c["width"] * c["depth"]]
    saturated = sum(1 for j in range(0, len(bins), 4) if bins[j:j + 4] == b"\xff\xff\xff\x7f")
    # keys whose FINAL estimate reaches the threshold although the reference never recorded them (only an order-exact result tells)
    late = 0
    if c["cls"] == "StreamThreshold":
        late = sum(1 for k in dict.fromkeys(keys) if k not in sk.meets_threshold and sk.check(k) >= c["param"])
    out = dict(c)
    out.update({"results_sha256": R.results_sha(results), "export_sha256": hashlib.sha256(raw).hexdigest(), "elements_added": sk.elements_added,
                "tracked": R.dict_pairs(c, tracked()), "evictions_when_full": evictions, "saturated_bins": saturated, "late_keys": late})
    return out


G = {"reference_version": probables.__version__, "seed": R.SEED, "cases": [run(c) for c in CASES]}
cs = G["cases"]
# the properties the fixture exists for
assert any(c["cls"] == "StreamThreshold" and c["late_keys"] > 0 for c in cs), "(a) no case separates order-exact results from the final table"
assert any(c["cls"] == "HeavyHitters" and c["evictions_when_full"] > 0 for c in cs), "(b) no eviction from a full list"
assert any(c["saturated_bins"] > 0 for c in cs), "(c) no bin saturates"
assert {c["query"] for c in cs if c["cls"] == "StreamThreshold"} == {"min", "mean", "mean-min"}
assert all(c["tracked"] for c in cs), "a case tracks nothing"

out = Path(__file__).resolve().parent / "golden_hitters.json"
out.write_text(json.dumps(G, indent=1) + "\n")
print(out, out.stat().st_size, "bytes;", {c["name"]: (len(c["tracked"]), c["evictions_when_full"], c["saturated_bins"], c["late_keys"]) for c in cs})
