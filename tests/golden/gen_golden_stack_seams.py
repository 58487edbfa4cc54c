#!/usr/bin/env python3
"""Generate tests/golden/golden_stack_seams.json by running the REAL reference's ExpandingBloomFilter / RotatingBloomFilter
(pyprobables v0.7.0, probables/blooms/expandingbloom.py) through add_alt with CHOSEN hashes: a hash is the wanted bit position itself
(``hash % number_bits`` leaves it alone), so every stream below is built on purpose to land on one seam of the ordered batch add.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_stack_seams.py [/root/reference]

Data only.  Per case: the parameters (m and k read from the reference's first filter), the ops ("a1.2.3" add_alt, "f1.2.3" add_alt with
force, "push", "pop"), after every op [filters, per-filter counts, elements_added], the final export in hex, check_alt of every key used and
of 16 unused bit sets.  A case built with frombytes carries the loaded image in "load".  Every case carries tags; a tag is only kept when
its predicate (below, over tests/stack_model.py) holds, a case is only recorded after the model agreed with the reference on every field,
and every tag has at least QUOTA cases."""

import copy
import json
import sys
from pathlib import Path

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import probables  # noqa: E402
from probables import ExpandingBloomFilter, RotatingBloomFilter  # noqa: E402

from stack_model import StackModel  # noqa: E402

QUOTA = 2
TAGS = ["room_th_candidate_is_last", "one_more_candidate_than_room", "full_then_reported_run", "covered_by_several", "repeated_bit_in_key",
        "force_across_growth", "rotation_drops_holder", "queue_of_one", "loaded_count_above_est", "single_key_tail"]
FPR = {1: 0.5, 3: 0.125, 5: 0.03125}  # exact in float32 (the footer stores a float); k = 1, 3, 5 at est_elements 4, 5 and 10


def sm(x):
    x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return x ^ (x >> 31)


def a(*keys):
    return [("a", list(k)) for k in keys]


def f(*keys):
    return [("f", list(k)) for k in keys]


PUSH, POP = [("push", None)], [("pop", None)]


def disjoint(m, k):
    """D(i): key i of a family of keys with no bit in common"""
    def D(i):
        assert (i + 1) * k <= m, "no room for that many disjoint keys"
        return list(range(i * k, (i + 1) * k))
    return D


# ---------------------------------------------------------------- the cases: name, est, k, queue, declared tags, ops(m, k, D)
def c_room_exact_ebf(m, k, D):      # est 4, k 3, m 18
    return f(D(0)) + a(D(0), D(1), D(2), D(3)) + PUSH + a(D(4), D(0), D(5), D(5))


def c_room_exact_rbf(m, k, D):      # est 5, k 1, m 8, queue 2
    return a(D(0), D(1), D(2), D(3), D(4)) + f(D(1)) + a(D(1), D(5), D(6), D(0))


def c_one_more_ebf(m, k, D):        # est 4, k 3
    return a(D(0), D(1), D(2), D(3), D(4)) + f(D(5)) + a(D(5), D(0), D(4))


def c_one_more_rbf(m, k, D):        # est 5, k 5, m 37, queue 3
    return a(D(0), D(1), D(0), D(2), D(3), D(4)) + f(D(5)) + a(D(5), D(5)) + PUSH + a(D(6), D(0)) + POP + a(D(0))


def c_full_reported_ebf(m, k, D):   # est 4, k 3
    return f(D(0), D(1), D(2), D(3)) + a(D(0), D(1), D(0), D(2), D(4), D(1), D(5))


def c_full_reported_rbf(m, k, D):   # est 4, k 1, m 6, queue 2
    return f(D(0), D(1), D(2), D(3)) + a(D(3), D(3), D(0), D(4), D(4), D(1))


def c_covered_k3(m, k, D):          # est 10, k 3, m 44
    return f([9, 9, 40]) + a([1, 2, 9], [3, 4, 9], [1, 3, 9], [1, 3, 5], [2, 4, 40], [5, 1, 2])


def c_covered_k5(m, k, D):          # est 5, k 5, m 37
    return a(D(0), D(1), [0, 5, 1, 6, 2], [0, 5, 1, 6, 12]) + PUSH + a([10, 11, 0, 1, 2], [12, 10, 11, 5, 6], D(3))


def c_repeated_k3(m, k, D):         # est 4, k 3
    return a([1, 1, 2], [3, 3, 3], [1, 2, 2], [2, 3, 1], [3, 4, 4]) + f([4, 4, 4]) + a([5, 5, 5], [5, 5, 4], [6, 6, 6], [6, 5, 5])


def c_repeated_k5(m, k, D):         # est 5, k 5, queue 2
    return a([7, 7, 7, 7, 7], [7, 8, 7, 8, 7], [8, 8, 8, 8, 8], [9, 9, 9, 9, 7]) + f([7, 7, 7, 7, 7], [7, 7, 8, 8, 9], [1, 1, 1, 1, 1]) + a([1, 7, 1, 7, 1])


def c_force_ebf(m, k, D):           # est 4, k 3
    return a(D(0), D(1)) + f(D(0), D(0), D(1), D(2), D(3)) + PUSH + f(D(0)) + a(D(0), D(4)) + f(D(4), D(4), D(4), D(4))


def c_force_rbf(m, k, D):           # est 5, k 1, queue 2
    return a(D(0)) + f(D(0), D(0), D(0), D(1), D(1), D(2), D(0), D(0), D(0), D(0), D(0), D(3)) + a(D(0), D(3), D(1))


def c_drops_holder_q2(m, k, D):     # est 4, k 3, m 18, queue 2: X = D(0) lives in the oldest filter only
    return f(D(0), D(1), D(2), D(3)) + a(D(0), D(4), D(5), [0, 1, 12], [3, 4, 15], [6, 7, 13], D(0), D(1))


def c_drops_holder_q1(m, k, D):     # est 4, k 3, queue 1
    return f(D(0), D(1), D(2), D(3)) + a(D(0), D(4), D(0), D(0), D(1))


def c_queue_of_one_k1(m, k, D):     # est 5, k 1, m 8, queue 1
    return a(D(0), D(1), D(2), D(3), D(4), D(0), D(5), D(0), D(5)) + PUSH + a(D(5), D(6)) + f(D(6), D(6), D(6), D(6), D(1))


def c_loaded_one(m, k, D):          # est 4, k 3, queue 2: loaded with D(0), D(1) and a count of 7
    return a(D(2), D(3), D(4), D(5), D(0)) + f(D(0), D(0)) + a([0, 3, 6], [0, 3, 6])


def c_loaded_two(m, k, D):          # est 5, k 1, queue 2: two filters, the newest at est + 1
    return a(D(2), D(0), D(3), D(4), D(5), D(6), D(6)) + f(D(1))


def c_tail_ebf(m, k, D):            # est 4, k 3: [.. room-th candidate | one key]: room 0 in the first batch, room left in the last
    return a(D(0), D(1), D(2), D(3), D(4)) + f(D(5)) + a([0, 1, 13], [0, 1, 13], [15, 16, 0])


def c_tail_rbf(m, k, D):            # est 10, k 3, m 44, queue 3
    return a(*[D(i) for i in range(11)]) + f(*[D(11)] * 9) + a(D(0), D(1), D(13))


CASES = [
    ("room_exact_ebf", "ebf", 4, 3, None, ["room_th_candidate_is_last"], c_room_exact_ebf, None),
    ("room_exact_rbf_k1", "rbf", 5, 1, 2, ["room_th_candidate_is_last"], c_room_exact_rbf, None),
    ("one_more_ebf", "ebf", 4, 3, None, ["one_more_candidate_than_room", "single_key_tail"], c_one_more_ebf, None),
    ("one_more_rbf_k5_q3", "rbf", 5, 5, 3, ["one_more_candidate_than_room"], c_one_more_rbf, None),
    ("full_reported_ebf", "ebf", 4, 3, None, ["full_then_reported_run"], c_full_reported_ebf, None),
    ("full_reported_rbf_k1", "rbf", 4, 1, 2, ["full_then_reported_run"], c_full_reported_rbf, None),
    ("covered_k3_est10", "ebf", 10, 3, None, ["covered_by_several", "repeated_bit_in_key"], c_covered_k3, None),
    ("covered_k5", "ebf", 5, 5, None, ["covered_by_several"], c_covered_k5, None),
    ("repeated_k3", "ebf", 4, 3, None, ["repeated_bit_in_key"], c_repeated_k3, None),
    ("repeated_k5_rbf", "rbf", 5, 5, 2, ["repeated_bit_in_key"], c_repeated_k5, None),
    ("force_ebf", "ebf", 4, 3, None, ["force_across_growth"], c_force_ebf, None),
    ("force_rbf_k1", "rbf", 5, 1, 2, ["force_across_growth"], c_force_rbf, None),
    ("drops_holder_q2", "rbf", 4, 3, 2, ["rotation_drops_holder"], c_drops_holder_q2, None),
    ("drops_holder_q1", "rbf", 4, 3, 1, ["rotation_drops_holder", "queue_of_one"], c_drops_holder_q1, None),
    ("queue_of_one_k1", "rbf", 5, 1, 1, ["queue_of_one"], c_queue_of_one_k1, None),
    ("loaded_one_filter", "rbf", 4, 3, 2, ["loaded_count_above_est"], c_loaded_one, {"filters": [([0, 1], 7)], "elements_added": 9}),
    ("loaded_two_filters_k1", "rbf", 5, 1, 2, ["loaded_count_above_est"], c_loaded_two, {"filters": [([0], 5), ([1], 6)], "elements_added": 11}),
    ("tail_ebf", "ebf", 4, 3, None, ["single_key_tail", "one_more_candidate_than_room"], c_tail_ebf, None),
    ("tail_rbf_est10_q3", "rbf", 10, 3, 3, ["single_key_tail", "one_more_candidate_than_room"], c_tail_rbf, None),
]


# ---------------------------------------------------------------- the reference
def make_ref(kind, est, fpr, queue):
    if kind == "rbf":
        return RotatingBloomFilter(est_elements=est, false_positive_rate=fpr, max_queue_size=queue)
    return ExpandingBloomFilter(est_elements=est, false_positive_rate=fpr)


def ref_state(ref):
    return [len(ref._blooms), [int(b.elements_added) for b in ref._blooms], int(ref.elements_added)]


def loaded(kind, est, fpr, queue, load, D):
    """a stack whose filters hold the given disjoint keys and CLAIM the given counts: written by the reference, read back with frombytes"""
    ref = make_ref(kind, est, fpr, queue)
    for j, (keys, count) in enumerate(load["filters"]):
        if j:
            ref._blooms.append(make_ref(kind, est, fpr, queue)._blooms[0])
        for i in keys:
            ref._blooms[-1].add_alt(D(i))
        ref._blooms[-1]._els_added = count
    ref._added_elements = load["elements_added"]
    raw = bytes(ref)
    return RotatingBloomFilter.frombytes(raw, max_queue_size=queue), raw


# ---------------------------------------------------------------- tag predicates, over the model
def runs_of(ops):
    """maximal runs of adds of one kind: what a caller would hand over as ONE batch; -> (first op, one past the last, kind)"""
    out, i = [], 0
    while i < len(ops):
        j = i
        while j < len(ops) and ops[j][0] == ops[i][0] and ops[i][0] in "af":
            j += 1
        j = max(j, i + 1)
        out.append((i, j, ops[i][0]))
        i = j
    return out


def room_of(mod):
    c = mod.filters[-1][1]
    if mod.queue is None:
        return max(0, mod.est - c)
    return mod.est - c if c <= mod.est else None


def tail_room(mod, keys):
    """walk the batch as the ordered add cuts it (a chunk ends right after the room-th key that is absent at the chunk's start, a full
    newest filter is replaced at the first absent key); -> the room seen when exactly ONE key is left for a chunk of its own, or -1"""
    mod, s, n = copy.deepcopy(mod), 0, len(keys)
    while n - s > 1:
        room = room_of(mod)
        cand = [not mod.check_alt(key) for key in keys[s:]]
        if room == 0:
            if not any(cand):
                return -1
            s += cand.index(True)
            mod._make_room()
            continue
        if room is None or sum(cand) <= room:
            e = n - s
        else:
            e = [i for i, c in enumerate(cand) if c][room - 1] + 1
        for key in keys[s:s + e]:
            mod.add_alt(key)
        s += e
    return room_of(mod) if n - s == 1 else -1


def tags_of(case, start_model):
    found, tails = set(), set()
    mod, ops = copy.deepcopy(start_model), case["ops"]
    if case["load"] is not None and mod.filters[-1][1] > mod.est:
        found.add("loaded_count_above_est")
    for lo, hi, kind in runs_of(ops):
        if kind not in "af":
            getattr(mod, kind)()
            continue
        keys = [bits for _, bits in ops[lo:hi]]
        if any(len(set(bits)) < len(bits) for bits in keys):
            found.add("repeated_bit_in_key")
        at_start = copy.deepcopy(mod)
        room = room_of(mod)
        absent = [not at_start.check_alt(bits) for bits in keys]
        if kind == "a":
            if room and sum(absent) == room and hi - lo > 1:
                found.add("room_th_candidate_is_last")
            if room and sum(absent) == room + 1:
                found.add("one_more_candidate_than_room")
            if room == 0 and len(keys) >= 3 and not any(absent[:2]) and any(absent):
                found.add("full_then_reported_run")
            t = tail_room(mod, keys)
            if len(keys) > 1 and t >= 0:
                tails.add(0 if t == 0 else 1)
        inserted_by, held, grown = [], {}, False  # per key: the bits it set (None: skipped); key -> the oldest filter, when it alone reported it
        for i, bits in enumerate(keys):
            before, count = list(mod.filters), mod.filters[-1][1]
            oldest_only = all(b in before[0][0] for b in bits) and not any(all(b in g[0] for b in bits) for g in before[1:])
            mod.add_alt(bits, kind == "f")
            grew = mod.filters[-1] is not before[-1]
            did = grew or mod.filters[-1][1] != count
            if grew:
                grown = True
                if kind == "f" and 0 < i < len(keys) - 1:
                    found.add("force_across_growth")
                if mod.queue == 1:
                    found.add("queue_of_one")
            if kind == "a" and not did and absent[i] and not grown:
                clear = {b for b in bits if b not in at_start.filters[-1][0]}
                setters = [got for got in inserted_by if got and got & clear]
                if len(setters) >= 2 and not any(clear <= got for got in setters):
                    found.add("covered_by_several")
            key = tuple(bits)
            if kind == "a" and did and key in held and not any(g is held[key] for g in mod.filters):
                found.add("rotation_drops_holder")  # counted while the oldest filter held it, inserted once that filter was gone
            if kind == "a" and not did and oldest_only and mod.queue is not None:
                held[key] = before[0]
            inserted_by.append(set(bits) if did else None)
    if tails:
        found.add("single_key_tail")
    return found, tails


# ---------------------------------------------------------------- run one case through the reference and the model
def op_text(op):
    return op[0] if op[0] in ("push", "pop") else op[0] + ".".join(str(b) for b in op[1])


def run(name, kind, est, k_want, queue, declared, build, load):
    fpr = FPR[k_want]
    ref = make_ref(kind, est, fpr, queue)
    m, k = int(ref._blooms[0].number_bits), int(ref._blooms[0].number_hashes)
    assert k == k_want, (name, k)
    D = disjoint(m, k)
    load_hex = None
    if load is not None:
        ref, raw = loaded(kind, est, fpr, queue, load, D)
        load_hex = raw.hex()
        bits = [[b for i in keys for b in D(i)] for keys, _ in load["filters"]]
        mod = StackModel.from_state(m, k, est, queue, fpr, [(bs, c) for bs, (_, c) in zip(bits, load["filters"])], load["elements_added"])
        assert mod.export() == raw == bytes(ref), name
    else:
        mod = StackModel(m, k, est, queue, fpr)
    ops = build(m, k, D)
    assert all(op[1] is None or (len(op[1]) == k and all(0 <= b < m for b in op[1])) for op in ops), name
    case = {"name": name, "kind": kind, "est_elements": est, "fpr": fpr, "queue": queue, "m": m, "k": k, "load": load_hex, "ops": ops}
    found, tails = tags_of(case, mod)
    assert set(declared) <= found, (name, "declared", declared, "found", sorted(found))
    trace = []
    for op, bits in ops:
        for obj in (ref, mod):
            if op in ("push", "pop"):
                getattr(obj, op)()
            else:
                obj.add_alt(list(bits), op == "f")
        trace.append(ref_state(ref))
        assert [mod.state()[x] for x in ("filters", "counts", "elements_added")] == trace[-1], (name, op, bits)  # the model is the reference
    raw = bytes(ref)
    assert mod.export() == raw, name
    used = sorted({tuple(bits) for op, bits in ops if bits is not None})
    unused, t = [], 0
    while len(unused) < 16:
        cand = tuple(int(sm(len(name) * 7919 + 31 * t + j) % m) for j in range(k))
        t += 1
        assert t < 10_000, (name, "every bit set of this table is in use")
        if cand not in used:
            unused.append(cand)
    checks = {"used": [[list(u), bool(ref.check_alt(list(u)))] for u in used], "unused": [[list(u), bool(ref.check_alt(list(u)))] for u in unused]}
    for part in checks.values():
        assert all(mod.check_alt(bits) == want for bits, want in part), name
    case.update({"ops": [op_text(op) for op in ops], "tags": sorted(found), "tails": sorted(tails), "trace": trace, "hex": raw.hex(), "check": checks})
    return case


G = {"reference_version": probables.__version__, "quota": QUOTA, "tags": TAGS, "cases": [run(*c) for c in CASES]}
cs = G["cases"]
per_tag = {t: [c["name"] for c in cs if t in c["tags"]] for t in TAGS}
assert all(len(v) >= QUOTA for v in per_tag.values()), per_tag
assert {c["est_elements"] for c in cs} == {4, 5, 10} and {c["k"] for c in cs} == {1, 3, 5} and {c["queue"] for c in cs} == {None, 1, 2, 3}
assert {t for c in cs for t in c["tails"]} == {0, 1}, "single_key_tail needs a tail taken with room 0 and one with room left"
assert any(any(x is False for _, x in c["check"]["used"]) for c in cs), "no used key was ever dropped again"
assert any(any(x for _, x in c["check"]["unused"]) for c in cs) and any(not all(x for _, x in c["check"]["unused"]) for c in cs)

out = Path(__file__).resolve().parent / "golden_stack_seams.json"
out.write_text(json.dumps(G, separators=(",", ":")) + "\n")
assert out.stat().st_size < 200_000, out.stat().st_size
print(out, out.stat().st_size, "bytes")
for t, v in per_tag.items():
    print(f"  {t}: {v}")
