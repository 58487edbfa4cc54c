#!/usr/bin/env python3
"""Generate tests/golden/golden_table_algebra.json by running the REAL reference (pyprobables v0.7.0).

The table algebra at its rails: CountMinSketch.join (countminsketch.py:356-399) with bins frozen on INT32_MIN / INT32_MAX, sums that land
exactly on a rail and one past it, `elements_added` clamping at INT64_MIN / INT64_MAX and a second join of the same operand;
CountingBloomFilter.union / intersection / jaccard_index (countingbloom.py:210-300) with sums of exactly 2^32 - 1, 0 against 2^32 - 1 and
counters with the top bit set; what the reference does when a sum passes 2^32 - 1; and what `add` / `remove` do to a table that came out of
the algebra with counters a few counts under a rail.  The cells are set directly (`_bins[i] = ...`, `_bloom[i] = ...`).  Run in the build
container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_table_algebra.py [/root/reference]

Data only: the cell values put in and the outputs the reference produced.
"""

import json
import sys
from pathlib import Path

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

import probables  # noqa: E402
from probables import CountingBloomFilter, CountMinSketch  # noqa: E402

I32_MIN, I32_MAX = -(2**31), 2**31 - 1
U32_MAX = 2**32 - 1
I64_MIN, I64_MAX = -(2**63), 2**63 - 1
TOP = 2**31

G = {"reference_version": probables.__version__}

# ------------------------------------------------------------------ CountMinSketch.join
WIDTH, DEPTH = 8, 5
# name -> (self bin, second bin): every branch of countminsketch.py:381-391
JOIN_BRANCHES = [
    ("max_frozen_second_positive", I32_MAX, 5),
    ("max_frozen_second_negative", I32_MAX, -5),
    ("max_frozen_second_zero", I32_MAX, 0),
    ("min_frozen_second_positive", I32_MIN, 5),
    ("min_frozen_second_negative", I32_MIN, -5),
    ("min_frozen_second_zero", I32_MIN, 0),
    ("sum_exactly_max", I32_MAX - 7, 7),
    ("sum_exactly_min", I32_MIN + 7, -7),
    ("sum_one_past_max", I32_MAX - 7, 8),
    ("sum_one_past_min", I32_MIN + 7, -8),
    ("min_plus_min", I32_MIN, I32_MIN),
    ("max_plus_max", I32_MAX, I32_MAX),
    ("max_frozen_second_min", I32_MAX, I32_MIN),
    ("min_frozen_second_max", I32_MIN, I32_MAX),
    ("zero_plus_max", 0, I32_MAX),
    ("zero_plus_min", 0, I32_MIN),
    ("one_plus_max", 1, I32_MAX),
    ("minus_one_plus_min", -1, I32_MIN),
    ("near_max_plus_max", I32_MAX - 1, I32_MAX),
    ("near_min_plus_min", I32_MIN + 1, I32_MIN),
    ("cancel_small", 12345, -12345),
    ("cancel_large", I32_MAX - 1, -(I32_MAX - 1)),
    ("cancel_min_side", I32_MIN + 1, I32_MAX),
    ("cancel_to_minus_one", I32_MAX, I32_MIN),          # self is frozen: no cancelling on a rail
    ("second_join_reaches_max", I32_MAX - 12, 7),       # 7 short after the first join, clamped by the second
    ("second_join_reaches_min", I32_MIN + 12, -7),
    ("second_join_exactly_max", I32_MAX - 14, 7),
    ("second_join_exactly_min", I32_MIN + 14, -7),
    ("half_plus_half", 2**30, 2**30),                   # 2^31: one past INT32_MAX
    ("minus_half_plus_minus_half", -(2**30), -(2**30)),  # exactly INT32_MIN
    ("small_positive", 3, 4),
    ("small_negative", -3, -4),
    ("zero_zero", 0, 0),
]


def cms_with(bins, els):
    c = CountMinSketch(width=WIDTH, depth=DEPTH)
    for i, v in enumerate(bins):
        c._bins[i] = v
    c._CountMinSketch__elements_added = els
    return c


def join_case(name, a_els, b_els, rotate):
    n = WIDTH * DEPTH
    pairs = [JOIN_BRANCHES[(i + rotate) % len(JOIN_BRANCHES)] for i in range(n)]
    a, b = cms_with([p[1] for p in pairs], a_els), cms_with([p[2] for p in pairs], b_els)
    a.join(b)
    first, first_els = list(a._bins), a.elements_added
    a.join(b)
    return {
        "name": name, "width": WIDTH, "depth": DEPTH, "branches": [p[0] for p in pairs],
        "a_bins": [p[1] for p in pairs], "b_bins": [p[2] for p in pairs], "a_elements_added": a_els, "b_elements_added": b_els,
        "joined_bins": first, "joined_elements_added": first_els,
        "joined_twice_bins": list(a._bins), "joined_twice_elements_added": a.elements_added,
        "b_bins_after": list(b._bins), "b_elements_added_after": b.elements_added,
    }


G["join_branches"] = [{"name": n, "self": s, "second": o} for n, s, o in JOIN_BRANCHES]
G["join"] = [
    join_case("elements_plain", 1000, 234, 0),
    join_case("elements_clamp_at_int64_max", I64_MAX - 3, 10, 0),          # clamps in the first join
    join_case("elements_clamp_at_int64_min", I64_MIN + 3, -10, 0),
    join_case("elements_exactly_int64_max", I64_MAX - 10, 10, 17),         # exact in the first join, clamped by the second
    join_case("elements_exactly_int64_min", I64_MIN + 10, -10, 17),
    join_case("elements_cancel", 2**40, -(2**40), 17),
]

# ------------------------------------------------------------------ CountingBloomFilter.union / intersection / jaccard_index
EST, FPR = 10, 0.05
# name -> (a counter, b counter): no sum passes 2^32 - 1
CBF_BRANCHES = [
    ("sum_exactly_max", U32_MAX - 5, 5),
    ("sum_exactly_max_top_bit_left", TOP, TOP - 1),
    ("sum_exactly_max_top_bit_right", TOP - 1, TOP),
    ("zero_against_max", 0, U32_MAX),
    ("max_against_zero", U32_MAX, 0),
    ("top_bit_left_only_word", TOP, 1),
    ("top_bit_right_only_word", 1, TOP),
    ("top_bit_left_against_zero", TOP, 0),
    ("top_bit_right_against_zero", 0, TOP),
    ("top_bit_left_plus_small", TOP + 123, 7),
    ("top_bit_right_plus_small", 7, TOP + 123),
    ("one_under_max", U32_MAX - 1, 0),
    ("just_under_top_bit_both", TOP - 1, TOP - 1),    # 2^32 - 2: the largest sum of two counters below 2^31
    ("small_both", 3, 4),
    ("small_left", 9, 0),
    ("small_right", 0, 9),
    ("zero_zero", 0, 0),
    ("one_one", 1, 1),
]
# counters >= 2^31 on BOTH sides pass 2^32 - 1 when summed: they are recorded for jaccard_index and the bit count, and as the overflow case
JACCARD_BRANCHES = CBF_BRANCHES + [
    ("top_bit_both", TOP, TOP),
    ("top_bit_both_plus_small", TOP + 5, TOP + 9),
    ("max_both", U32_MAX, U32_MAX),
    ("max_against_top_bit", U32_MAX, TOP),
    ("top_bit_against_max", TOP, U32_MAX),
    ("max_against_one", U32_MAX, 1),
]


def cbf_with(vals):
    f = CountingBloomFilter(est_elements=EST, false_positive_rate=FPR)
    for i, v in enumerate(vals):
        f._bloom[i] = v
    return f


def outcome(fn):
    try:
        res = fn()
    except Exception as ex:  # noqa: BLE001  (the type and the message are the record)
        return None, {"type": type(ex).__name__, "message": str(ex)}
    return res, None


def cbf_case(name, branches, rotate, a_els=0, b_els=0):
    m = CountingBloomFilter(est_elements=EST, false_positive_rate=FPR).number_bits
    pairs = [branches[(i + rotate) % len(branches)] for i in range(m)]
    a, b = cbf_with([p[1] for p in pairs]), cbf_with([p[2] for p in pairs])
    a.elements_added, b.elements_added = a_els, b_els
    case = {
        "name": name, "est_elements": EST, "fpr": FPR, "m": a.number_bits, "k": a.number_hashes, "branches": [p[0] for p in pairs],
        "a_table": list(a.bloom), "b_table": list(b.bloom), "a_elements_added": a_els, "b_elements_added": b_els,
        "jaccard": a.jaccard_index(b), "jaccard_ba": b.jaccard_index(a), "jaccard_self": a.jaccard_index(a),
        "a_bits_set": a._cnt_number_bits_set(), "b_bits_set": b._cnt_number_bits_set(),
    }
    for op in ("union", "intersection"):
        for tag, (x, y) in (("", (a, b)), ("_ba", (b, a))):
            res, err = outcome(lambda x=x, y=y, op=op: getattr(x, op)(y))
            case[f"{op}{tag}_error"] = err
            case[f"{op}{tag}_table"] = None if res is None else list(res.bloom)
            case[f"{op}{tag}_elements_added"] = None if res is None else res.elements_added
    case["a_table_after"], case["b_table_after"] = list(a.bloom), list(b.bloom)
    return case


G["cbf_branches"] = [{"name": n, "a": a, "b": b} for n, a, b in JACCARD_BRANCHES]
G["cbf"] = [
    cbf_case("rails", CBF_BRANCHES, 0, 5, 6),
    cbf_case("rails_rotated", CBF_BRANCHES, 11),
    cbf_case("only_top_bit_words", [("top_bit_left_against_zero", TOP, 0), ("top_bit_right_against_zero", 0, TOP), ("zero_zero", 0, 0)], 0),
    cbf_case("only_ones", [("one_one", 1, 1), ("small_left", 1, 0), ("zero_zero", 0, 0)], 0),
    cbf_case("max_against_zero_everywhere", [("max_against_zero", U32_MAX, 0)], 0),
    # a sum passes 2^32 - 1: the reference's array('I') store raises
    cbf_case("overflow_top_bit_both", JACCARD_BRANCHES, 0),
    cbf_case("overflow_by_one_in_one_cell", [("small_both", 3, 4)] * 40 + [("max_against_one", U32_MAX, 1)] + [("small_both", 3, 4)] * 40, 0),
    cbf_case("overflow_everywhere", [("max_both", U32_MAX, U32_MAX)], 0),
]

# ------------------------------------------------------------------ the state the algebra leaves: add / remove on its result
KEYS = [f"key-{i}" for i in range(12)]


def cbf_follow_on(name, op, near, counts):
    """both operands hold `near` // 2 (rounded both ways) except in three cells that hold small counters and three that hold zero: the result stands a few
    counts under 2^32 - 1 nearly everywhere; then add(key, count) per key"""
    m = CountingBloomFilter(est_elements=EST, false_positive_rate=FPR).number_bits
    av = [0 if i % 21 == 0 else (3 if i % 21 == 10 else near // 2) for i in range(m)]
    bv = [0 if i % 21 == 0 else (4 if i % 21 == 10 else near - near // 2) for i in range(m)]
    a, b = cbf_with(av), cbf_with(bv)
    res = getattr(a, op)(b)
    case = {"name": name, "op": op, "est_elements": EST, "fpr": FPR, "a_table": av, "b_table": bv, "result_table": list(res.bloom),
            "result_elements_added": res.elements_added, "ops": []}
    for key, cnt in zip(KEYS, counts):
        ret = res.add(key, cnt)
        case["ops"].append({"op": "add", "key": key, "count": cnt, "returned": ret, "elements_added": res.elements_added})
    case["final_table"] = list(res.bloom)
    case["final_elements_added"] = res.elements_added
    case["final_checks"] = [res.check(k) for k in KEYS]
    return case


G["cbf_follow_on"] = [
    cbf_follow_on("union_three_under_the_rail", "union", U32_MAX - 3, [2, 3, 7, 5, 2, 4, 6, 2, 3, 7, 5, 2]),
    cbf_follow_on("intersection_three_under_the_rail", "intersection", U32_MAX - 3, [2, 3, 7, 5, 2, 4, 6, 2, 3, 7, 5, 2]),
    cbf_follow_on("union_five_under_the_rail", "union", U32_MAX - 5, [2, 5, 3, 2, 5, 2, 7, 3, 6, 4, 5, 6]),
    cbf_follow_on("union_of_small_counters", "union", 40, [2, 3, 7, 5, 2, 4, 6, 2, 3, 7, 5, 2]),
    cbf_follow_on("intersection_of_small_counters", "intersection", 40, [2, 3, 7, 5, 2, 4, 6, 2, 3, 7, 5, 2]),
]


def cms_follow_on(name, rail_sign, ops):
    """every bin of the join stands 3 under INT32_MAX (rail_sign > 0) or 3 over INT32_MIN (< 0); then the ops"""
    n = WIDTH * DEPTH
    half = 2**30
    av = [half if rail_sign > 0 else -half] * n
    bv = [half - 4 if rail_sign > 0 else -half + 3] * n
    a, b = cms_with(av, 100), cms_with(bv, 50)
    a.join(b)
    case = {"name": name, "width": WIDTH, "depth": DEPTH, "a_bins": av, "b_bins": bv, "a_elements_added": 100, "b_elements_added": 50,
            "joined_bins": list(a._bins), "joined_elements_added": a.elements_added, "ops": []}
    for (op, cnt), key in zip(ops, KEYS):
        ret = getattr(a, op)(key, cnt)
        case["ops"].append({"op": op, "key": key, "count": cnt, "returned": ret, "elements_added": a.elements_added})
    case["final_bins"] = list(a._bins)
    case["final_elements_added"] = a.elements_added
    case["final_checks"] = [a.check(k) for k in KEYS]
    return case


G["cms_follow_on"] = [
    cms_follow_on("adds_three_under_int32_max", 1, [("add", c) for c in (2, 3, 7, 5, 2, 4, 6, 2, 3, 7, 5, 2)]),
    cms_follow_on("removes_three_over_int32_min", -1, [("remove", c) for c in (2, 3, 7, 5, 2, 4, 6, 2, 3, 7, 5, 2)]),
    cms_follow_on("adds_then_removes_under_int32_max", 1, [("add", 2), ("add", 7), ("remove", 3), ("add", 5), ("remove", 2), ("add", 6),
                                                           ("add", 2), ("remove", 7), ("add", 3), ("add", 4), ("remove", 5), ("add", 2)]),
    cms_follow_on("removes_then_adds_over_int32_min", -1, [("remove", 2), ("remove", 7), ("add", 3), ("remove", 5), ("add", 2), ("remove", 6),
                                                           ("remove", 2), ("add", 7), ("remove", 3), ("remove", 4), ("add", 5), ("remove", 2)]),
]

out = Path(__file__).resolve().parent / "golden_table_algebra.json"
out.write_text(json.dumps(G, indent=0, ensure_ascii=True))
print("wrote", out, out.stat().st_size, "bytes")
