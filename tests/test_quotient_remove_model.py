"""Removal in the reference's quotient filter, on every step of tests/golden/golden_quotient_remove.json (written by
tests/golden/gen_golden_quotient_remove.py from the real reference) and, where the reference is at hand, on random add / remove streams
fed to the live class:

* behind a removal the four arrays are tests/qf_model.canonical(remaining set) -- the table is still a function of the set it holds, which
  is what makes a batch removal exact however it is carried out;
* the reference's counter (`elements_added`) and quotient follow the host-side rule of pyprobables_amd/quotientfilter.py: held + stale,
  stale = the successful removals since the last resize (``plan_add``).

The second half holds tests/qf_remove_model.py -- the step model of the two kernels behind ``psk_qf_remove_alt`` -- against ``canonical``: two
exhaustive walks over the table's end, every case of tests/qf_remove_edges.py with the property the case is there for, random tables
repaired in two list orders, and the loop and index bounds on arrays that are no quotient filter's.

No GPU: only the package's host functions are used."""

import itertools
import os
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import qf_model as M  # noqa: E402
import qf_remove_edges as E  # noqa: E402
import qf_remove_fixture as F  # noqa: E402
import qf_remove_model as R  # noqa: E402

REF = Path(os.environ.get("PYPROBABLES_REFERENCE", "/root/reference"))  # the checkout the generator scripts default to


def counts_after(held: set, stream):
    seen, out = set(held), []
    for h in stream:
        seen.add(h)
        out.append(len(seen))
    return out


class CounterModel:
    """the host side of the class without its table: a set, and the two counters"""

    def __init__(self, q, auto_expand):
        self.q, self.auto, self.held, self.stale = q, auto_expand, set(), 0

    def add(self, stream) -> bool:
        from pyprobables_amd.exceptions import QuotientFilterError
        from pyprobables_amd.quotientfilter import plan_add

        if not stream:
            return False
        try:
            q, self.stale = plan_add(self.q, len(self.held), self.stale, counts_after(self.held, stream), self.auto)
        except QuotientFilterError:
            return True
        self.q = q
        self.held |= set(stream)
        return False

    def remove(self, stream) -> int:
        gone = self.held & set(stream)
        self.held -= gone
        self.stale += len(gone)
        return len(gone)

    @property
    def elements_added(self):
        return len(self.held) + self.stale


def test_fixture_keeps_its_properties():
    names = set(F.BY_NAME)
    assert {c["q0"] for c in F.CASES} >= {3, 5, 6, 10, 16, 24} and {c.get("width") for c in F.CASES} >= {8, 16, 32}
    assert {"q5_run_head_with_continuation", "q5_run_head_without_continuation", "q5_middle_and_last_of_run", "q5_whole_run", "q5_whole_cluster",
            "q5_split_cluster", "q5_wrapped_cluster", "q5_absent_and_duplicates", "q6_cluster_over_word_boundary", "q6_two_clusters_in_one_word",
            "q6_wrapped_cluster", "q10_one_run_of_300", "counter_doubles_at_half_load_q3", "counter_second_doubling_on_true_counts_q3",
            "counter_insufficient_space_with_free_slots_q3"} <= names
    for c in F.CASES:
        for st in c["steps"]:
            occ, cont, sh = (set(st[k]) for k in ("occupied", "continuation", "shifted"))
            assert len(occ | cont | sh) < 1 << st["q"], "every step keeps an empty slot"
    wrapped = F.BY_NAME["q5_wrapped_cluster"]["steps"][0]
    assert {h >> 27 for h in wrapped["hashes"]} >= {30, 31, 0} and 0 in wrapped["shifted"]
    assert F.BY_NAME["q10_one_run_of_300"]["steps"][0]["continuation"] == list(range(701, 1000))
    assert F.BY_NAME["q5_whole_run"]["steps"][1]["occupied"] == [11, 12, 14]
    split = F.BY_NAME["q5_split_cluster"]["steps"]
    assert split[0]["shifted"] == [11, 12, 14] and split[1]["shifted"] == [14]
    assert any(len(st["hashes"]) != len(set(st["hashes"])) for c in F.CASES for st in c["steps"] if st["op"] == "remove")
    c1 = F.BY_NAME["counter_doubles_at_half_load_q3"]["steps"]
    assert [(s["q"], s["elements_added"], len(s["get_hashes"])) for s in c1] == [(3, 6, 6), (3, 6, 3), (4, 5, 5)]
    c3 = F.BY_NAME["counter_insufficient_space_with_free_slots_q3"]["steps"]
    assert [s["raised"] for s in c3] == [False, False, False, True, False, True] and len(c3[3]["get_hashes"]) == 5


@pytest.mark.parametrize("case", F.CASES, ids=F.IDS)
def test_every_step_is_the_canonical_table_of_the_remaining_set(case):
    for st, held in zip(case["steps"], F.held_after(case)):
        assert F.same_tables(M.canonical(held, st["q"]), F.dense(st)), (case["name"], st["op"], st["hashes"][:8])
        assert st["get_hashes"] == M.reference_order(held, st["q"])


@pytest.mark.parametrize("case", F.CASES, ids=F.IDS)
def test_counter_rule_gives_the_references_elements_added_and_quotient(case):
    torch = pytest.importorskip("torch")  # noqa: F841 -- plan_add counts with it
    m = CounterModel(case["q0"], case["auto_expand"])
    for st, held in zip(case["steps"], F.held_after(case)):
        if st["op"] == "add":
            assert m.add(st["hashes"]) == st["raised"]
        else:
            m.remove(st["hashes"])
        assert (m.q, m.elements_added, m.held) == (st["q"], st["elements_added"], held), (case["name"], st["op"])


def test_model_and_counter_rule_equal_live_reference_on_random_streams():
    pytest.importorskip("torch")
    if not (REF / "probables").is_dir():
        pytest.skip("the reference checkout is not on this machine")
    sys.path.insert(0, str(REF))
    try:
        from probables import QuotientFilter
    finally:
        sys.path.remove(str(REF))
    rng = random.Random(11)
    checked = 0
    for q, streams in ((3, 60), (4, 60), (5, 40), (7, 20), (10, 4)):
        for s in range(streams):
            auto = s % 3 == 0
            qf = QuotientFilter(quotient=q, auto_expand=auto)
            m = CounterModel(q, auto)
            for _ in range(6):
                size = 1 << qf.quotient
                # every table keeps an empty slot: an expanding filter doubles before it fills; without expansion the reference's counter (which
                # removals do not lower) stays below the size, and so no insert raises in these streams
                room = size - 1 - qf.elements_added
                n = rng.randrange(0, int(size * rng.choice([0.2, 0.5, 0.9])) + 1)
                n = n if auto else max(0, min(n, room))
                add = []
                for _ in range(n):
                    quot = size - 1 - rng.randrange(3) if rng.random() < 0.35 else rng.randrange(size)
                    add.append((quot << (32 - qf.quotient)) | rng.randrange(8 if s % 2 else 1 << (32 - qf.quotient)))
                for h in add:
                    qf.add_alt(h)
                assert m.add(add) is False
                have = sorted(m.held)
                gone = rng.sample(have, rng.randrange(0, len(have) + 1)) if have else []
                absent = [h ^ 1 for h in gone[:3]] + [rng.getrandbits(32) for _ in range(3)]
                batch = gone + absent + gone[:2]
                rng.shuffle(batch)
                for h in batch:
                    qf.remove_alt(h)
                m.remove(batch)
                assert (qf.quotient, qf.elements_added) == (m.q, m.elements_added), (q, s)
                size = 1 << qf.quotient
                got = (list(qf._filter), *([b[i] for i in range(size)] for b in (qf._is_occupied, qf._is_continuation, qf._is_shifted)))
                assert got == tuple(a.tolist() for a in M.canonical(m.held, qf.quotient)), (q, s, batch)
                checked += 1
    assert checked >= 1000


# ------------------------------------------------------------------ tests/qf_remove_model.py: the two kernels step by step, against canonical
def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def check_removal(q, held, batch, order=None):
    """`batch` (any order, duplicates and absent hashes allowed) out of the canonical table of `held` -> the model's run"""
    held = set(held)
    assert len(held) < 1 << q, "the in-place removal asks for an empty slot"
    t = R.table_of(M.canonical(held, q), q)
    run = R.remove_in_place(t, batch, order)
    rest = held - set(batch)
    where = (q, sorted(held), list(batch))
    assert same(t.arrays(), M.canonical(rest, q)), where
    assert run.removed == len(held) - len(rest), where
    assert R.scratch_is_zero(t, run), where
    assert run.longest <= (1 << q) + 1, where
    return run


RING_POOL = [(30, 1), (30, 2), (31, 1), (31, 2), (0, 1), (0, 2), (1, 1), (3, 1)]  # (quotient of the LAST slots / the first, remainder)


@pytest.mark.parametrize("q", [5, 6])
def test_model_every_assignment_on_the_ring(q):
    """eight hashes round the table's end, each absent (and asked for), kept or removed: 3^8 tables.  At q = 6 the metadata is two words and
    the end of the table is the seam between the second and the first."""
    size = 1 << q
    pool = [E.m(q, (quot + size - 32) % size if quot >= 30 else quot, rem) for quot, rem in RING_POOL]
    assert {h >> (32 - q) for h in pool} == {size - 2, size - 1, 0, 1, 3}
    dirty = 0
    for assign in itertools.product((0, 1, 2), repeat=len(pool)):
        held = [h for h, a in zip(pool, assign) if a]
        batch = [h for h, a in zip(pool, assign) if a != 1]
        dirty += len(check_removal(q, held, batch).starts)
    assert dirty >= 3 ** len(pool)


EDGE_HITS = {"dead_head_run_survives": 1, "head_run_dies_next_run_falls_home": 2, "gap_splits_cluster_in_three": 2, "whole_cluster": 3,
             "seam_31_32_dead_each_side": 2, "three_words_shift_by_one": 1, "three_words_last_only": 1, "two_clusters_one_word": 2,
             "three_clusters_middle_untouched": 2, "over_the_end_dead_each_side": 2, "over_the_end_head_dies": 1, "over_the_end_shifted_head_dies": 1,
             "over_the_end_occupied_scan_wraps": 1, "over_the_end_only_wrapped_part": 2,
             "next_occupied_two_words_on": 2, "long_run_first_middle_last": 3, "absent_only": 0, "remainder_zero_and_max": 2, "one_empty_slot_ring": 4,
             "one_empty_slot_shifted_ring": 3, "domino_heads": 341, "domino_seconds": 341, "domino_alternate": 341, "quads_middle_two": 408,
             "width_q23_r9": 100, "width_q16_r16": 100, "width_q15_r17": 100}


def only(f):
    """the one dirty cluster of a case that has one -> (start, cluster)"""
    ((b, c),) = f["clusters"].items()
    return b, c


def most_words(f):
    return E.most_dirty_starts_in_one_word(f)


def starts_of(q, held):
    return sorted(set(E.layout(held, q)[2].tolist()))


def edge_property(name, q, held, gone, f, before, after):
    """the reason the case is in the table, read off canonical(held) and canonical(rest)"""
    size = 1 << q
    rest = sorted(set(held) - set(gone))
    if name == "dead_head_run_survives":
        return only(f)[1]["dead"] == [0] and after[1][10] == 1 and after[0][10] == 2
    if name == "head_run_dies_next_run_falls_home":
        return only(f)[1]["dead"] == [0, 1] and before[3][11] == 1 and (after[1][10], after[1][11], after[3][11], after[0][11]) == (0, 1, 0, 1)
    if name == "gap_splits_cluster_in_three":
        # six slots in a row, heads at 10, 13 and 15; the two dead slots leave gaps at 12 and 14, and 11's run falls home and heads a cluster
        return sorted(f["slot"].values()) == list(range(10, 16)) and sorted(f["clusters"]) == [10, 13] and f["all_starts"] == [10, 13, 15] \
            and sorted(E.layout(rest, q)[1].tolist()) == [10, 11, 13, 15] and starts_of(q, rest) == [10, 11, 13, 15]
    if name == "whole_cluster":
        b, c = only(f)
        return c["dead"] == list(range(c["length"])) and not any(a[10:13].any() for a in after) and starts_of(q, rest) == [20]
    if name == "seam_31_32_dead_each_side":
        b, c = only(f)
        dead = [c["slots"][o] for o in c["dead"]]
        return c["words"] == [0, 1] and min(dead) < 32 <= max(dead)
    if name == "three_words_shift_by_one":
        b, c = only(f)
        return len(c["words"]) >= 3 and c["dead"] == [0] and not any(a[103] for a in (after[0], after[2], after[3])) \
            and bool(after[0][28:103].all()) and bool(after[3][30:103].all())
    if name == "three_words_last_only":
        b, c = only(f)
        differ = np.flatnonzero((before[0] != after[0]) | (before[2] != after[2]) | (before[3] != after[3])).tolist()
        return len(c["words"]) >= 3 and c["dead"] == [c["length"] - 1] and differ == [103]
    if name == "two_clusters_one_word":
        return sorted(f["clusters"]) == [3, 20] and most_words(f) == 2
    if name == "three_clusters_middle_untouched":
        return sorted(f["clusters"]) == [3, 20] and f["all_starts"] == [3, 10, 20]
    if name == "over_the_end_head_dies":  # a cluster of one in front of the cluster that goes over the end: its slot empties, the neighbour stays
        b, c = only(f)
        return (b, c["dead"], c["length"]) == (254, [0], 1) and f["all_starts"] == [254, 255] and same(before[0][:3], after[0][:3]) and after[1][254] == 0
    if name.startswith("over_the_end"):
        b, c = only(f)
        dead = [c["slots"][o] for o in c["dead"]]
        if not c["wraps"]:
            return False
        if name == "over_the_end_dead_each_side":
            return min(dead) < b <= max(dead)
        if name == "over_the_end_shifted_head_dies":
            return c["dead"] == [0] and c["length"] == 5
        if name == "over_the_end_occupied_scan_wraps":  # from quotient 254 the next occupied bit is in word 0: the scan leaves the last word empty-handed
            return b == 254 and not before[1][255] and before[1][0] == 1 and c["length"] == 5 and c["dead"] == [1]
        return max(dead) < b
    if name == "next_occupied_two_words_on":
        b, c = only(f)
        return not before[1][32:64].any() and before[1][:32].sum() == 1 and before[1][85] == 1 and c["length"] == 82 and c["dead"] == [79, 80]
    if name == "long_run_first_middle_last":
        b, c = only(f)
        return c["dead"] == [0, 39, 79] and c["length"] == 80 and before[2].sum() == 79
    if name == "absent_only":
        return f["hits"] == 0 and not f["clusters"] and same(before, after)
    if name == "remainder_zero_and_max":
        return before[0][10] == 0 and before[1][10] == 1 and before[0][12] == 0 and before[3][12] == 1 and after[0][10] == E.RMAX8 and after[0][12] == E.RMAX8
    if name == "one_empty_slot_ring":
        return f["empty"] == 1 and not before[3].any() and sorted(c["length"] for c in f["clusters"].values()) == [1, 1, 1, 1]
    if name == "one_empty_slot_shifted_ring":
        b, c = only(f)
        return f["empty"] == 1 and c["length"] == 255 and c["wraps"] and c["dead"] == [0, 127, 254] and before[3].sum() == 254
    if name in E.SHARED_WORD_CASES:
        # (four slots and a gap are five: a word of 32 slots has room for six or seven such clusters, not ten)
        need = 6 if name == "quads_middle_two" else 10
        return most_words(f) >= need and any(len(c["words"]) == 2 for c in f["clusters"].values()) and len(f["clusters"]) == (204 if need == 6 else 341)
    if name in E.WIDTH_CASES:
        r = 32 - q
        rmax = (1 << r) - 1
        kept = set(rest)
        around = all(E.m(q, quot, 0) in kept and E.m(q, quot, rmax) in kept and E.m(q, quot, 1) in set(gone) for quot in (size - 1, 0, size - 150, 60))
        third = 0.25 <= f["hits"] / len(held) <= 0.45
        return before[0].dtype == {9: np.uint16, 16: np.uint16, 17: np.uint32}[r] and around and third and any(c["wraps"] for c in f["clusters"].values()) \
            and max(c["length"] for c in f["clusters"].values()) >= 40 and 300 <= len(held) <= 400 and sum(h >> r == size - 20 for h in held) >= 40
    raise KeyError(name)


def test_edge_table_has_the_cases_the_gpu_runs():
    assert set(E.NAMES) == set(EDGE_HITS) and len(E.NAMES) == 27
    assert {E.CASES[n][0] for n in E.NAMES} == {8, 10, 15, 16, 23}


@pytest.mark.parametrize("name", E.NAMES)
def test_model_on_every_edge_case(name):
    q, held, gone = E.CASES[name]
    f = E.facts(q, held, gone)
    assert f["empty"] >= 1 and len(set(held)) == len(held)
    assert f["hits"] >= EDGE_HITS[name] and (f["hits"] == EDGE_HITS[name] or name in E.WIDTH_CASES)
    rest = set(held) - set(gone)
    before, after = M.canonical(held, q), M.canonical(rest, q)
    assert edge_property(name, q, held, gone, f, before, after), name
    for order in (None, lambda n: range(n - 1, -1, -1)):
        t = R.table_of(before, q)
        run = R.remove_in_place(t, sorted(set(gone)), order)
        assert same(t.arrays(), after), name
        assert run.removed == f["hits"] and sorted(run.starts) == sorted(f["clusters"]) and R.scratch_is_zero(t, run)
        assert run.longest <= (1 << q) + 1


def random_table(rng, q):
    size = 1 << q
    kind = rng.randrange(4)
    n = min(rng.randrange(1, size), 40 if kind == 1 else size - 1)
    hs = set()
    while len(hs) < n:
        if rng.random() < 0.3:  # near the end, so that clusters come round it
            quot = size - 1 - rng.randrange(4)
        elif kind == 1:  # packed clusters: few quotients
            quot = rng.choice([1, 2, size // 2, 31, 32]) + rng.randrange(2)
        elif kind == 3:  # long runs
            quot = rng.choice([3, size // 3, 30])
        else:
            quot = rng.randrange(size)
        hs.add(E.m(q, quot % size, rng.randrange(0, 80 if kind == 3 else 6)))
    held = sorted(hs)
    gone = rng.sample(held, rng.randrange(0, len(held) + 1))
    absent = [h ^ 1 for h in gone[:4]] + [rng.getrandbits(32) for _ in range(3)]
    batch = gone + absent + gone[:3]  # duplicates are counted once
    rng.shuffle(batch)
    return held, batch


@pytest.mark.parametrize("q,count", [(5, 1500), (6, 1200), (7, 800), (8, 500)])
def test_model_random_tables_in_two_list_orders(q, count):
    rng = random.Random(2000 + q)
    for _ in range(count):
        held, batch = random_table(rng, q)
        a = check_removal(q, held, batch)
        b = check_removal(q, held, batch, lambda n: rng.sample(range(n), n))
        assert sorted(a.starts) == sorted(b.starts) and len(set(a.starts)) == len(a.starts)


def test_model_counts_a_hash_once_and_takes_the_empty_batch():
    held = [E.m(5, 30, 1), E.m(5, 30, 2), E.m(5, 31, 1), E.m(5, 0, 1), E.m(5, 9, 0)]
    run = check_removal(5, held, [held[1], held[1], held[4], held[1], held[4] ^ 1])
    assert run.removed == 2 and sorted(run.starts) == [9, 30]
    t = R.table_of(M.canonical(held, 5), 5)
    assert R.remove_in_place(t, []).removed == 0 and same(t.arrays(), M.canonical(held, 5))


@pytest.mark.parametrize("q", [5, 6, 7])
def test_model_stays_bounded_on_arrays_that_are_no_quotient_filters(q):
    """the kernels' promise for a caller's garbage: some table, every loop over after at most size + 1 steps, no index outside the arrays
    (``Dev`` raises on one).  This is checked here and only here: such arrays are never handed to the GPU."""
    size, words, r = 1 << q, 1 << (q - 5), 32 - q
    rng = np.random.default_rng(q)
    longest = 0
    for i in range(400):
        if i % 4 == 3:  # a real table with a few bits flipped
            held = rng.choice(1 << 12, size=int(rng.integers(1, size)), replace=False).astype(np.uint64) << np.uint64(20)
            filt, *meta = M.canonical(held, q)
            meta = [R.pack(a) for a in meta]
            for a in meta:
                a[rng.integers(words)] ^= np.uint32(1 << int(rng.integers(32)))
            held = held.tolist()
        else:
            density = (0.1, 0.5, 0.9)[i % 3]
            filt = rng.integers(0, 4 if i % 2 else 1 << 24, size=size).astype(M.remainder_dtype(q))
            meta = [R.pack(rng.random(size) < density) for _ in range(3)]
            held = []
        t = R.Table(filt, *meta, q)
        batch = [int(h) for h in held[: size // 2]] + [int(h) for h in rng.integers(0, 2**32, size=size)]
        batch += [E.m(q, int(s), int(t.filter[int(s)])) for s in rng.integers(0, size, size=size)]  # remainders that are there: hits
        run = R.remove_in_place(t, batch)
        assert run.longest <= size + 1, (q, i, run.longest)
        longest = max(longest, run.longest)
    assert longest >= size // 2  # the walks did go far
