"""tests/stack_model.py against the real reference (tests/golden/golden_stack_seams.json: chosen bit positions on the seams of the ordered
batch add), the tag quotas of that fixture, and the power of the resolver inputs: three deliberate mistakes in the loop each change the
expected flags of an exhaustive or hand-made case, so a kernel that made them could not pass tests/test_gpu_stack_kernels.py."""

import json
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import stack_model as M  # noqa: E402

G = json.loads((ROOT / "tests" / "golden" / "golden_stack_seams.json").read_text())
CASES = G["cases"]


def parse(op):
    if op in ("push", "pop"):
        return op, None
    return op[0], [int(x) for x in op[1:].split(".")]


def start_model(case):
    """the stack the case begins with: fresh, or the loaded image taken apart"""
    m, k, est = case["m"], case["k"], case["est_elements"]
    if case["load"] is None:
        return M.StackModel(m, k, est, case["queue"], case["fpr"])
    raw, nbytes = bytes.fromhex(case["load"]), (m + 7) // 8
    size, est_l, added, fpr = M.StackModel._FOOTER.unpack(raw[-M.StackModel._FOOTER.size:])
    assert (est_l, fpr) == (est, case["fpr"])
    filters = []
    for j in range(size):
        part = raw[j * (8 + nbytes):(j + 1) * (8 + nbytes)]
        filters.append(([b for b in range(m) if part[8 + (b >> 3)] >> (b & 7) & 1], M.StackModel._COUNT.unpack(part[:8])[0]))
    mod = M.StackModel.from_state(m, k, est, case["queue"], fpr, filters, added)
    assert mod.export() == raw
    return mod


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_model_replays_every_case_op_by_op(case):
    mod = start_model(case)
    assert len(case["trace"]) == len(case["ops"])
    for op, want in zip(case["ops"], case["trace"]):
        kind, bits = parse(op)
        if bits is None:
            getattr(mod, kind)()
        else:
            mod.add_alt(bits, kind == "f")
        assert [len(mod.filters), mod.counts(), mod.elements_added] == want, op
    assert mod.export().hex() == case["hex"]
    for part in ("used", "unused"):
        assert [mod.check_alt(bits) for bits, _ in case["check"][part]] == [want for _, want in case["check"][part]]
    assert len(case["check"]["unused"]) == 16
    assert sorted(tuple(b) for b, _ in case["check"]["used"]) == sorted({tuple(parse(op)[1]) for op in case["ops"] if parse(op)[1] is not None})


def test_the_tag_quotas_hold():
    assert G["quota"] >= 2 and len(G["tags"]) == 10
    for tag in G["tags"]:
        assert sum(tag in c["tags"] for c in CASES) >= G["quota"], tag
    tails = {t for c in CASES if "single_key_tail" in c["tags"] for t in c["tails"]}
    assert tails == {0, 1}  # a one-key last chunk taken with room 0, and one taken with room left
    assert {c["est_elements"] for c in CASES} == {4, 5, 10} and {c["queue"] for c in CASES} == {None, 1, 2, 3}
    ks = {c["k"] for c in CASES}
    assert 1 in ks and 3 in ks and max(ks) >= 5
    assert all(c["queue"] == 1 for c in CASES if "queue_of_one" in c["tags"])
    assert all(c["load"] is not None and c["kind"] == "rbf" for c in CASES if "loaded_count_above_est" in c["tags"])


def test_the_model_pops_and_pushes_like_the_reference():
    mod = M.StackModel(18, 3, 4, queue=1)
    with pytest.raises(ValueError, match="unusable system"):
        mod.pop()
    mod.push()
    assert len(mod.filters) == 1
    mod = M.StackModel(18, 3, 4)
    mod.push()
    assert len(mod.filters) == 2 and mod.export()[-M.StackModel._FOOTER.size:] == M.StackModel._FOOTER.pack(2, 4, 0, 0.0)


# ---- the resolver inputs tell these mistakes apart
def non_candidates_claim(table_bits, idx, present):
    table, flags = set(table_bits), []
    for bits, p in zip(idx, present):
        new = not all(b in table for b in bits)
        table.update(bits)  # (wrong: a key another filter reports sets nothing)
        flags.append(int(new and not p))
    return flags


def starting_table_ignored(table_bits, idx, present):
    return M.resolve((), idx, present)


def repeated_bit_is_two_claims(table_bits, idx, present):
    """a key's second probe of a clear bit taken for a rival's: a key only wins through a clear bit it names once"""
    table, flags = set(table_bits), []
    for bits, p in zip(idx, present):
        won = not p and any(b not in table and bits.count(b) == 1 for b in bits)
        if won:
            table.update(bits)
        flags.append(int(won))
    return flags


@pytest.mark.parametrize("wrong", [non_candidates_claim, starting_table_ignored, repeated_bit_is_two_claims], ids=lambda f: f.__name__)
def test_each_mistake_changes_a_hand_made_and_an_exhaustive_case(wrong):
    hand = [c["name"] for c in M.HAND_CASES if wrong(c["table"], c["idx"], c["present"]) != M.resolve(c["table"], c["idx"], c["present"])]
    stripe = next((t for t, (bits, idx, present) in enumerate(M.exhaustive_stripes()) if wrong(bits, idx, present) != M.resolve(bits, idx, present)), None)
    print(wrong.__name__, "changes", hand, "and first the exhaustive stripe", stripe)
    assert hand and stripe is not None
