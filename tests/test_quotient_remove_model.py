"""Removal in the reference's quotient filter, on every step of tests/golden/golden_quotient_remove.json (written by
tests/golden/gen_golden_quotient_remove.py from the real reference) and, where the reference is at hand, on random add / remove streams
fed to the live class:

* behind a removal the four arrays are tests/qf_model.canonical(remaining set) -- the table is still a function of the set it holds, which
  is what makes a batch removal exact however it is carried out;
* the reference's counter (`elements_added`) and quotient follow the host-side rule of pyprobables_amd/quotientfilter.py: held + stale,
  stale = the successful removals since the last resize (``plan_add``).

No GPU: only the package's host functions are used."""

import os
import random
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import qf_model as M  # noqa: E402
import qf_remove_fixture as F  # noqa: E402

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
