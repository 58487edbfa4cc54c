"""tests/qf_insert_model.py -- the step model of the in-place insertion (``psk_qf_add_alt``) -- against ``qf_model.canonical``:

* every old / new / absent assignment of a small pool of hashes at 8 and at 16 slots, the pools chosen so that clusters cross the table's end;
* random splits at 32 and 64 slots, with long runs, packed clusters and batches that hold present hashes.

A union that leaves an empty slot must be taken and give the canonical table of the union; one that does not fit must be refused with the
table untouched; one that fills the table to the last slot may be either (a region that comes round to its own start is refused).

No GPU."""

import itertools
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import qf_insert_fixture as G  # noqa: E402
import qf_insert_model as I  # noqa: E402
import qf_model as M  # noqa: E402


def mk(q, quot, rem):
    return (quot << (32 - q)) | rem


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def check_split(q, old, batch, order=None):
    """`batch` (sorted, distinct; may hold hashes of `old`) into the canonical table of `old` -> 1 if the model took it"""
    size = 1 << q
    t = I.table_of(M.canonical(old, q), q)
    before = t.copy()
    union = set(old) | set(batch)
    added, status = I.add_in_place(t, batch, order)
    if status:
        assert len(union) >= size, (q, old, batch)
        assert same(t.arrays(), before.arrays()) and added == 0, (q, old, batch)
        return 0
    assert len(union) <= size, (q, old, batch)
    assert added == len(union) - len(set(old)), (q, old, batch)
    assert same(t.arrays(), M.canonical(union, q)), (q, old, batch)
    return 1


POOLS = {
    3: [mk(3, 6, 1), mk(3, 6, 2), mk(3, 7, 1), mk(3, 7, 2), mk(3, 0, 1), mk(3, 0, 2), mk(3, 1, 1), mk(3, 3, 1)],
    4: [mk(4, 13, 2), mk(4, 14, 1), mk(4, 14, 2), mk(4, 15, 1), mk(4, 15, 2), mk(4, 15, 3), mk(4, 0, 1), mk(4, 0, 2), mk(4, 2, 1)],
}


@pytest.mark.parametrize("q", [3, 4])
def test_every_assignment_of_a_pool_over_the_tables_end(q):
    pool, taken, fit = POOLS[q], 0, 0
    for assign in itertools.product((0, 1, 2), repeat=len(pool)):  # 0: absent, 1: old, 2: new
        old = [h for h, a in zip(pool, assign) if a == 1]
        new = [h for h, a in zip(pool, assign) if a == 2]
        taken += check_split(q, old, new)
        fit += len(old) + len(new) < 1 << q
    assert fit <= taken  # every union that leaves an empty slot is taken (check_split: a refusal needs a union of at least `size`)


def random_split(rng, q):
    size, r = 1 << q, 32 - q
    kind = rng.randrange(4)
    n = min(rng.randrange(1, size), 28 if kind == 1 else size)  # (kind 1 has 50 distinct hashes to draw from)
    hs = set()
    while len(hs) < n:
        if kind == 0:
            quot = rng.randrange(size)
        elif kind == 1:  # packed clusters: few quotients
            quot = rng.choice([1, 2, size // 2, size - 3, size - 1]) + rng.randrange(2)
        elif kind == 2:  # near the end, so that clusters wrap
            quot = size - 1 - rng.randrange(6) if rng.random() < 0.6 else rng.randrange(size)
        else:  # long runs
            quot = rng.choice([3, size - 2, size // 3])
        hs.add(mk(q, quot % size, rng.randrange(1, 40 if kind == 3 else 6)))
    hs = sorted(hs)
    rng.shuffle(hs)
    k = rng.randrange(0, len(hs) + 1)
    old, new = hs[:k], hs[k:]
    present = rng.sample(old, rng.randrange(0, min(len(old), 4) + 1)) if old else []
    return old, sorted(set(new) | set(present))


@pytest.mark.parametrize("q,count", [(5, 2500), (6, 1500)])
def test_random_splits(q, count):
    rng = random.Random(1000 + q)
    taken = 0
    for i in range(count):
        old, batch = random_split(rng, q)
        order = (lambda n: rng.sample(range(n), n)) if i % 2 else None  # the head lanes in any order
        taken += check_split(q, old, batch, order)
    assert taken >= count * 0.95


def test_batch_of_present_hashes_only_and_empty_batch():
    old = [mk(5, 30, 1), mk(5, 30, 2), mk(5, 31, 1), mk(5, 0, 1), mk(5, 9, 4)]
    t = I.table_of(M.canonical(old, 5), 5)
    before = t.copy()
    assert I.add_in_place(t, sorted(old)) == (0, 0) and same(t.arrays(), before.arrays())
    assert I.add_in_place(t, []) == (0, 0)


def test_regions_end_where_the_issue_says():
    """cluster [10..12], 13 - 15 empty, head at 16 (q = 8): two new hashes end the region at 14, three arrive at 15 with carry 1 and stop in
    front of 16, a fourth of quotient 15 pushes the head"""
    q = 8
    old = [mk(q, 10, 1), mk(q, 10, 3), mk(q, 11, 1), mk(q, 16, 1), mk(q, 16, 2)]
    t = I.table_of(M.canonical(old, q), q)
    for batch, end in (([mk(q, 10, 2), mk(q, 12, 1)], 15), ([mk(q, 10, 2), mk(q, 11, 2), mk(q, 12, 1)], 16),
                       ([mk(q, 10, 2), mk(q, 11, 2), mk(q, 12, 1), mk(q, 15, 1)], 19)):
        bs = [I.group_start(t, h >> (32 - q)) for h in batch]
        assert bs[0] == 10 and I.is_leader(t, batch, bs, 0)
        w = I.walk(t, batch, bs, 0)
        assert (w.b + w.end, w.added) == (end, len(batch))
        assert check_split(q, old, batch) == 1


# ------------------------------------------------------------------ tests/golden/golden_quotient_insert.json: the live reference's tables
def test_fixture_keeps_its_properties():
    assert {c["q0"] for c in G.CASES} >= {5, 6, 8, 10} and G.PATH.stat().st_size <= (G.PATH.parent / "golden_quotient_remove.json").stat().st_size
    by = G.BY_NAME
    three = [by[f"q6_one_set_{x}"]["steps"][1] for x in ("ascending", "descending", "shuffled")]
    assert all(G.same_tables(G.dense(s), G.dense(three[0])) for s in three) and len({tuple(s["hashes"]) for s in three}) == 3
    assert [s["q"] for s in by["threshold_reached_inside_a_batch_q5"]["steps"]] == [5, 6]
    assert [(s["q"], s["elements_added"]) for s in by["threshold_reached_by_the_last_call_then_first_call_q5"]["steps"]] == [(5, 20), (5, 28), (6, 29)]
    assert [s["q"] for s in by["counter_ahead_of_true_count_q5"]["steps"]] == [5, 5, 5, 6]
    fill = by["fill_to_the_last_slot_q5"]["steps"]
    assert [s["raised"] for s in fill] == [False, False, False, True] and len(fill[2]["filter"]) == 32 and fill[2]["get_hashes"] is None
    free = by["counter_full_with_free_slots_q5"]["steps"]
    assert free[3]["raised"] and len(free[3]["get_hashes"]) == 28
    assert any(len(st["hashes"]) != len(set(st["hashes"])) for st in by["q10_random_batches_with_duplicates"]["steps"])
    assert sum(len(G.in_place_steps(c)) for c in G.CASES) >= 25


@pytest.mark.parametrize("case", G.CASES, ids=G.IDS)
def test_fixture_steps_are_canonical_and_the_model_reaches_them_in_place(case):
    for st, held in zip(case["steps"], G.held_after(case)):
        assert G.same_tables(M.canonical(held, st["q"]), G.dense(st)), (case["name"], st["hashes"][:8])
        if st["get_hashes"] is not None:
            assert st["get_hashes"] == M.reference_order(held, st["q"])
    for before, st, held in G.in_place_steps(case):
        q = st["q"]
        t = I.table_of(M.canonical(before, q), q)
        added, status = I.add_in_place(t, sorted(set(st["hashes"])))
        if status:
            assert len(held) == 1 << q, (case["name"], st["hashes"][:8])  # only the last slot may be refused
        else:
            assert added == len(held) - len(before) and same(t.arrays(), G.dense(st)), (case["name"], st["hashes"][:8])


@pytest.mark.parametrize("case", G.CASES, ids=G.IDS)
def test_fixture_counters_follow_plan_add(case):
    pytest.importorskip("torch")
    from pyprobables_amd.exceptions import QuotientFilterError
    from pyprobables_amd.quotientfilter import plan_add

    q, held, stale = case["q0"], set(), 0
    for st in case["steps"]:
        if st["op"] == "remove":
            gone = held & set(st["hashes"])
            held -= gone
            stale += len(gone)
        elif st["hashes"]:
            seen, counts = set(held), []
            for h in st["hashes"]:
                seen.add(h)
                counts.append(len(seen))
            try:
                q, stale = plan_add(q, len(held), stale, counts, case["auto_expand"])
                held = seen
                assert not st["raised"]
            except QuotientFilterError:
                assert st["raised"]
        assert (q, len(held) + stale) == (st["q"], st["elements_added"]), (case["name"], st["hashes"][:8])
