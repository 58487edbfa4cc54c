"""In-place insertion into a loaded QuotientFilter on the GPU: psk_qf_add_alt itself and the class's ``_add_policy`` paths, against
tests/golden/golden_quotient_insert.json and golden_quotient_remove.json (the live reference's tables) and tests/qf_model.canonical (tied to the
reference by tests/test_quotient_model.py).
All comparisons are exact equality.  Small shapes: the bug classes live at 32-slot word seams, cluster boundaries and the table's end."""

import itertools
import random
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import qf_insert_fixture as G  # noqa: E402
import qf_model as M  # noqa: E402
import qf_remove_fixture as F  # noqa: E402

POLICIES = ("local", "rebuild")


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def pa(torch):
    import pyprobables_amd

    return pyprobables_amd


def mk(q, quot, rem):
    return (quot << (32 - q)) | rem


def dev_u32(torch, values):
    a = np.asarray(values, dtype=np.uint64).astype(np.uint32)
    return torch.from_numpy(a.view(np.int32)).cuda()


def tables(qf):
    t = qf.tables()
    return t["filter"], t["occupied"], t["continuation"], t["shifted"]


class AbiTable:
    """the four arrays and the scratch as a caller of include/psk.h would hold them"""

    def __init__(self, torch, q, capacity):
        r = 32 - q
        self.torch, self.q, self.size = torch, q, 1 << q
        self.udt = np.uint8 if r <= 8 else (np.uint16 if r <= 16 else np.uint32)
        self.filter = torch.zeros(self.size, dtype={np.uint8: torch.uint8, np.uint16: torch.int16, np.uint32: torch.int32}[self.udt], device="cuda")
        self.words = max(self.size // 32, 1)
        self.occ, self.cont, self.sh = (torch.zeros(self.words, dtype=torch.int32, device="cuda") for _ in range(3))
        self.scratch = torch.zeros(2 * self.words + 2 + capacity, dtype=torch.int32, device="cuda")  # zeroed once: every call hands it back zeroed
        self.result = torch.full((2,), -7, dtype=torch.int32, device="cuda")
        self.tiles = torch.empty(capacity // 1024 + 2, dtype=torch.int32, device="cuda")

    def args(self):
        return (self.q, self.filter.data_ptr(), self.occ.data_ptr(), self.cont.data_ptr(), self.sh.data_ptr())

    def build(self, hashes):
        from pyprobables_amd import _native as N

        hs = dev_u32(self.torch, sorted(hashes))
        N.check(N.lib().psk_qf_build(self.q, hs.data_ptr() if hs.numel() else None, hs.numel(), *self.args()[1:], self.tiles.data_ptr(), 0, None))

    def add(self, hashes):
        """-> (added, status)"""
        from pyprobables_amd import _native as N

        hs = dev_u32(self.torch, sorted(set(hashes)))
        N.check(N.lib().psk_qf_add_alt(*self.args(), hs.data_ptr() if hs.numel() else None, hs.numel(), self.scratch.data_ptr(), self.result.data_ptr(), 0, None))
        added, status = self.result.tolist()
        assert not bool(self.scratch[: 2 * self.words + 2].any().item()), "the scratch comes back zeroed"
        return added, status

    def tables(self):
        out = [self.filter.cpu().numpy().view(self.udt)]
        for t in (self.occ, self.cont, self.sh):
            out.append(np.unpackbits(t.cpu().numpy().view(np.uint8), bitorder="little")[: self.size])
        return tuple(out)


def abi_split(torch, t, q, old, new, must_take=True):
    """build `old`, add `new` in place, compare with the canonical table of the union"""
    t.build(old)
    before = None if must_take else t.tables()
    added, status = t.add(new)
    union = set(old) | set(new)
    if status:
        assert not must_take and len(union) >= 1 << q, (old, new)
        assert added == 0 and F.same_tables(t.tables(), before), (old, new)
        return
    assert added == len(union) - len(set(old)), (old, new)
    assert F.same_tables(t.tables(), M.canonical(union, q)), (old, new)


# ------------------------------------------------------------------ the C ABI
def test_abi_every_assignment_on_the_ring_q5(torch):
    """seven hashes with quotients {30, 31, 0, 1} and two remainders: every old / new / absent assignment, 3^7 tables, each built with psk_qf_build
    and extended with psk_qf_add_alt"""
    q = 5
    pool = [mk(q, 30, 1), mk(q, 30, 2), mk(q, 31, 1), mk(q, 31, 2), mk(q, 0, 1), mk(q, 0, 2), mk(q, 1, 1)]
    t = AbiTable(torch, q, 16)
    for assign in itertools.product((0, 1, 2), repeat=len(pool)):
        abi_split(torch, t, q, [h for h, a in zip(pool, assign) if a == 1], [h for h, a in zip(pool, assign) if a == 2])


Q8 = 8
CLUSTER = [mk(Q8, 10, 1), mk(Q8, 10, 3), mk(Q8, 11, 1), mk(Q8, 16, 1), mk(Q8, 16, 2)]  # cluster [10..12], 13 - 15 empty, head at 16
DOMINO = [mk(Q8, 40 + 3 * c + d, 1) for c in range(8) for d in range(2)]  # 8 clusters of two slots, one empty slot between neighbours
BOUNDARIES = {
    "two_into_cluster_region_ends_at_14": (CLUSTER, [mk(Q8, 10, 2), mk(Q8, 12, 1)]),
    "three_into_cluster_carry_arrives_at_15": (CLUSTER, [mk(Q8, 10, 2), mk(Q8, 11, 2), mk(Q8, 12, 1)]),
    "three_and_quotient_15_pushes_the_head_at_16": (CLUSTER, [mk(Q8, 10, 2), mk(Q8, 11, 2), mk(Q8, 12, 1), mk(Q8, 15, 1)]),
    "larger_than_every_element_of_its_cluster": (CLUSTER, [mk(Q8, 12, 9)]),
    "larger_than_its_cluster_in_front_of_the_next_head": (CLUSTER + [mk(Q8, 13, 1), mk(Q8, 13, 2)], [mk(Q8, 14, 9)]),
    "domino_through_8_clusters": (DOMINO, [mk(Q8, 40, 0)]),
    "two_regions_in_one_word": (CLUSTER + [mk(Q8, 24, 1), mk(Q8, 24, 2)], [mk(Q8, 10, 2), mk(Q8, 25, 1)]),
    "one_region_across_three_words": ([mk(Q8, 28 + i // 2, 1 + i % 2) for i in range(76)], [mk(Q8, 28, 0), mk(Q8, 50, 0)]),
    "over_the_tables_end_absorbing_slot_0": ([mk(Q8, 254, 1), mk(Q8, 254, 2), mk(Q8, 255, 1), mk(Q8, 2, 1)], [mk(Q8, 254, 3), mk(Q8, 255, 2), mk(Q8, 0, 1), mk(Q8, 1, 1)]),
    "wrapped_cluster_new_hashes_at_its_far_end": ([mk(Q8, 254, 1), mk(Q8, 254, 2), mk(Q8, 255, 1), mk(Q8, 255, 2), mk(Q8, 0, 1)], [mk(Q8, 0, 2), mk(Q8, 1, 1), mk(Q8, 253, 1)]),
    "only_present_hashes": (CLUSTER, [mk(Q8, 10, 3), mk(Q8, 16, 1)]),
    "run_in_front_inside_behind": ([mk(Q8, 10, 1), mk(Q8, 12, 1), mk(Q8, 12, 5), mk(Q8, 14, 1)], [mk(Q8, 11, 1), mk(Q8, 11, 2), mk(Q8, 12, 3), mk(Q8, 13, 1), mk(Q8, 14, 0), mk(Q8, 14, 2)]),
    "into_empty_slots_only": (CLUSTER, [mk(Q8, 13, 1), mk(Q8, 14, 1), mk(Q8, 100, 1), mk(Q8, 255, 1), mk(Q8, 0, 1)]),
}


@pytest.mark.parametrize("name", list(BOUNDARIES))
def test_abi_chosen_boundaries_q8(torch, name):
    old, new = BOUNDARIES[name]
    abi_split(torch, AbiTable(torch, Q8, 16), Q8, old, new)


def random_hashes(rng, q, n, near_end=0.2, small_rem=False):
    size, r = 1 << q, 32 - q
    out = set()
    while len(out) < n:
        quot = size - 1 - rng.randrange(6) if rng.random() < near_end else rng.randrange(size)
        out.add(mk(q, quot, rng.randrange(16 if small_rem else 1 << r)))
    return sorted(out)


@pytest.mark.parametrize("q,n", [(10, 800), (16, 4000), (24, 4000)])
def test_abi_remainder_widths(torch, q, n):
    rng = random.Random(q)
    hs = random_hashes(rng, q, n, near_end=0.3 if q == 10 else 0.05, small_rem=q == 10)
    hs += [mk(q, 77, r) for r in range(1, 60)]  # one long run
    rng.shuffle(hs)
    k = len(hs) * 2 // 3
    abi_split(torch, AbiTable(torch, q, len(hs)), q, hs[:k], hs[k:] + hs[:50])


def test_abi_refusals_and_the_empty_batch(torch):
    from pyprobables_amd import _native as N

    L = N.lib()
    t = AbiTable(torch, 5, 64)
    old = [mk(5, i, 1) for i in range(0, 30)]
    t.build(old)
    before = t.tables()
    assert t.add([]) == (0, 0) and F.same_tables(t.tables(), before)
    hs = dev_u32(torch, [1, 2])
    assert L.psk_qf_add_alt(4, *t.args()[1:], hs.data_ptr(), 2, t.scratch.data_ptr(), t.result.data_ptr(), 0, None) == N.PSK_EINVAL
    assert L.psk_qf_add_alt(*t.args(), None, 2, t.scratch.data_ptr(), t.result.data_ptr(), 0, None) == N.PSK_EINVAL
    assert L.psk_qf_add_alt(*t.args(), hs.data_ptr(), 2, t.scratch.data_ptr(), None, 0, None) == N.PSK_EINVAL
    assert F.same_tables(t.tables(), before)
    added, status = t.add([mk(5, 3, 2), mk(5, 17, 2), mk(5, 31, 2)])  # 30 + 3 > 32
    assert status != 0 and added == 0 and F.same_tables(t.tables(), before)
    assert t.add([mk(5, 3, 2)]) == (1, 0) and F.same_tables(t.tables(), M.canonical(old + [mk(5, 3, 2)], 5))


# ------------------------------------------------------------------ the class
def filter_with(pa, q, hashes, policy, auto_expand=False):
    qf = pa.QuotientFilter(quotient=q, auto_expand=auto_expand, device=0)
    qf._add_policy = policy
    if len(hashes):
        qf.add_alt_many(hashes)
    return qf


def assert_holds(qf, held, q):
    assert qf.quotient == q and qf.elements_held == len(held)
    assert F.same_tables(tables(qf), M.canonical(held, q))
    assert sorted(qf.get_hashes()) == sorted(held)
    assert qf.validate_metadata()
    s = qf._remove_scratch
    assert s is None or not bool(s[: 2 * qf.occupied_tensor.numel() + 2].any().item())


def run_case(pa, case, policy, record=False):
    """the case through the class; every step compared with what the reference held -> the calls recorded"""
    qf = filter_with(pa, case["q0"], [], policy, case["auto_expand"])
    calls = recording(qf) if record else []
    for st, held in zip(case["steps"], F.held_after(case)):
        if st["op"] == "add" and st["raised"]:
            before = tables(qf)
            with pytest.raises(pa.QuotientFilterError, match="insufficient space"):
                qf.add_alt_many(st["hashes"])
            assert F.same_tables(tables(qf), before)
        elif st["op"] == "add":
            qf.add_alt_many(st["hashes"])
        else:
            qf.remove_alt_many(st["hashes"])
        where = (case["name"], st["op"], st["hashes"][:8])
        assert F.same_tables(tables(qf), F.dense(st)), where
        assert (qf.quotient, qf.elements_added, qf.elements_held) == (st["q"], st["elements_added"], len(held)), where
        if st["get_hashes"] is not None:
            assert qf.get_hashes() == st["get_hashes"], where
        probes = sorted(set(st["hashes"]) | held)
        if probes:
            assert qf.check_alt_many(probes).tolist() == [h in held for h in probes], where
    return calls


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("case", G.CASES + F.CASES, ids=G.IDS + F.IDS)
def test_class_equals_reference_fixtures_under_both_add_policies(pa, case, policy):
    run_case(pa, case, policy)


@pytest.mark.parametrize("case", [c for c in G.CASES if G.in_place_steps(c)], ids=[c["name"] for c in G.CASES if G.in_place_steps(c)])
def test_abi_equals_reference_fixture(torch, case):
    """the add steps into a loaded table that keep the quotient, through psk_qf_add_alt itself (the scratch comes back zeroed: AbiTable.add)"""
    for before, st, held in G.in_place_steps(case):
        q = st["q"]
        t = AbiTable(torch, q, len(st["hashes"]) + len(before))
        t.build(before)
        added, status = t.add(st["hashes"])
        if status:
            assert len(held) == 1 << q  # only a table filled to the last slot may be refused
            assert added == 0 and F.same_tables(t.tables(), M.canonical(before, q))
        else:
            assert added == len(held) - len(before) and F.same_tables(t.tables(), F.dense(st)), (case["name"], st["hashes"][:8])


def test_forced_local_falls_back_as_the_fixture_says(pa):
    """a stream that reaches the threshold, a batch that fills the table, "insufficient space": forced "local" hands them to the rebuild and
    the results are the reference's (run_case compares every step)"""
    calls = run_case(pa, G.BY_NAME["threshold_reached_inside_a_batch_q5"], "local", record=True)
    assert calls == [("_add_rebuild", None), ("_add_local", False), ("_add_rebuild", None)]
    calls = run_case(pa, G.BY_NAME["threshold_reached_by_the_last_call_then_first_call_q5"], "local", record=True)
    assert [c[0] for c in calls] == ["_add_rebuild", "_add_local", "_add_rebuild", "_add_local", "_add_rebuild"] and not calls[1][1] and not calls[3][1]
    calls = run_case(pa, G.BY_NAME["threshold_not_reached_q5"], "local", record=True)
    assert calls == [("_add_rebuild", None), ("_add_local", True), ("_add_local", True)]
    calls = run_case(pa, G.BY_NAME["fill_to_the_last_slot_q5"], "local", record=True)  # 20, 31 (in place), 32 (the last slot), one beyond (raises)
    assert calls[:4] == [("_add_rebuild", None), ("_add_local", True), ("_add_local", False), ("_add_rebuild", None)] and len(calls) == 4
    calls = run_case(pa, G.BY_NAME["q10_random_batches_with_duplicates"], "local", record=True)
    assert calls == [("_add_rebuild", None)] + [("_add_local", True)] * 3


@pytest.fixture(scope="module")
def q16_sets():
    rng = random.Random(16)
    hs = random_hashes(rng, 16, 50000, near_end=0.02)
    rng.shuffle(hs)
    return hs[:40000], hs[40000:]


@pytest.mark.parametrize("batches", [1, 10])
@pytest.mark.parametrize("policy", POLICIES)
def test_class_q16_random(pa, q16_sets, policy, batches):
    old, new = q16_sets
    rng = random.Random(batches)
    stream = new + old[:1000] + new[:500]
    rng.shuffle(stream)
    qf = filter_with(pa, 16, old, policy)
    step = len(stream) // batches
    for i in range(batches):
        qf.add_alt_many(stream[i * step:] if i == batches - 1 else stream[i * step:(i + 1) * step])
    assert_holds(qf, set(old) | set(new), 16)
    assert qf.elements_added == 50000
    assert qf.check_alt_many(new[:2000] + [h ^ 1 for h in new[:50] if h ^ 1 not in set(old) | set(new)]).tolist()[:2000] == [True] * 2000


def test_class_alternating_add_and_remove_on_one_scratch(pa, q16_sets):
    old, new = q16_sets
    rng = random.Random(5)
    qf = filter_with(pa, 16, old, "local")
    qf._remove_policy = "local"
    held = set(old)
    for i in range(10):
        add = new[i * 1000:(i + 1) * 1000]
        qf.add_alt_many(add)
        held |= set(add)
        assert_holds(qf, held, 16)
        gone = rng.sample(sorted(held), 700)
        assert qf.remove_alt_many(gone) == 700
        held -= set(gone)
        assert_holds(qf, held, 16)


def test_grid_cap_q22(pa, torch):
    """more new hashes than 4096 x 256 lanes"""
    q, n_old, n_new = 22, 1 << 20, 4096 * 256 + 12345
    g = torch.Generator(device="cpu").manual_seed(22)
    hs = torch.unique(torch.randint(0, 2**32, (n_old + n_new + 50000,), generator=g, dtype=torch.int64))
    hs = hs[torch.randperm(hs.numel(), generator=g)][: n_old + n_new]
    old, new = hs[:n_old], hs[n_old:]
    qf = filter_with(pa, q, old.cuda(), "local")
    ran = []
    inner = qf._add_local
    qf._add_local = lambda bits: ran.append(inner(bits)) or ran[-1]
    qf.add_alt_many(new.cuda())
    assert ran == [True]
    assert qf.elements_held == n_old + n_new and qf.quotient == q
    assert bool(qf.check_alt_many(hs.cuda()).all().item())
    ref = filter_with(pa, q, hs.cuda(), "rebuild")
    assert all(bool((a == b).all().item()) for a, b in zip((qf.filter_tensor, qf.occupied_tensor, qf.continuation_tensor, qf.shifted_tensor),
                                                           (ref.filter_tensor, ref.occupied_tensor, ref.continuation_tensor, ref.shifted_tensor)))


def recording(qf):
    calls = []
    for name in ("_add_local", "_add_rebuild"):
        inner = getattr(qf, name)

        def wrapped(bits, _inner=inner, _name=name):
            out = _inner(bits)
            calls.append((_name, out))
            return out

        setattr(qf, name, wrapped)
    return calls


def test_auto_takes_both_add_paths_by_batch_size(pa, monkeypatch):
    import pyprobables_amd.quotientfilter as Q

    rng = random.Random(3)
    hs = random_hashes(rng, 10, 600)
    qf = filter_with(pa, 10, hs[:400], "auto")
    calls = recording(qf)
    qf.add_alt_many(hs[:3])  # a table below 2^ADD_LOCAL_MIN_QUOTIENT slots rebuilds whatever the batch
    assert calls == [("_add_rebuild", None)] and Q.ADD_LOCAL_MIN_QUOTIENT > 10
    del calls[:]
    monkeypatch.setattr(Q, "ADD_LOCAL_MIN_QUOTIENT", 5)
    monkeypatch.setattr(Q, "ADD_LOCAL_MAX_FRACTION", 0.25)
    qf.add_alt_many(hs[400:500])  # 100 <= 0.25 * 400
    assert calls == [("_add_local", True)]
    monkeypatch.setattr(Q, "ADD_LOCAL_MAX_FRACTION", 0.01)
    qf.add_alt_many(hs[500:])  # 100 > 0.01 * 500
    assert calls == [("_add_local", True), ("_add_rebuild", None)]
    assert_holds(qf, set(hs), 10)


def test_forced_local_still_rebuilds_where_it_must(pa):
    rng = random.Random(9)
    # q = 3, 4 and an empty filter
    for q in (3, 4):
        hs = random_hashes(rng, q, 5, small_rem=True)
        qf = filter_with(pa, q, hs[:3], "local")
        calls = recording(qf)
        qf.add_alt_many(hs[3:])
        assert [c[0] for c in calls] == ["_add_rebuild"]
        assert_holds(qf, set(hs), q)
    qf = pa.QuotientFilter(quotient=6, auto_expand=False, device=0)
    qf._add_policy = "local"
    calls = recording(qf)
    hs = random_hashes(rng, 6, 64, small_rem=True)
    qf.add_alt_many(hs[:40])
    assert [c[0] for c in calls] == ["_add_rebuild"]
    qf.add_alt_many(hs[40:63])  # one slot stays empty: in place
    assert calls[1:] == [("_add_local", True)]
    assert_holds(qf, set(hs[:63]), 6)
    qf.add_alt_many(hs[63:])  # the last slot: the build places a full table
    assert calls[2:] == [("_add_local", False), ("_add_rebuild", None)]
    assert qf.elements_held == 64 and F.same_tables(tables(qf), M.canonical(hs, 6))
    # insufficient space: nothing changes
    before = tables(qf)
    with pytest.raises(pa.QuotientFilterError, match="insufficient space"):
        qf.add_alt_many([hs[0] ^ 1 if hs[0] ^ 1 not in hs else hs[0] ^ 2])
    assert F.same_tables(tables(qf), before) and (qf.elements_held, qf.elements_added) == (64, 64)
    # a stream that reaches the load threshold goes the old way and doubles the table where the reference does
    hs = random_hashes(rng, 5, 30, small_rem=True)
    qf = filter_with(pa, 5, hs[:20], "local", auto_expand=True)
    calls = recording(qf)
    qf.add_alt_many(hs[20:])
    assert [c[0] for c in calls] == ["_add_local", "_add_rebuild"] and calls[0][1] is False
    ref = filter_with(pa, 5, hs[:20], "rebuild", auto_expand=True)
    ref.add_alt_many(hs[20:])
    assert qf.quotient == ref.quotient == 6 and qf.elements_added == ref.elements_added
    assert_holds(qf, set(hs), 6)


def test_per_key_add_and_merge_go_in_place(pa):
    qf = pa.QuotientFilter(quotient=8, device=0)
    qf._add_policy = "local"
    qf.add_many([f"key{i}" for i in range(100)])
    calls = recording(qf)
    qf.add("another")
    qf.add_alt(12345)
    other = pa.QuotientFilter(quotient=8, device=0)
    other.add_many([f"more{i}" for i in range(20)])
    qf.merge(other)
    assert calls == [("_add_local", True)] * 3
    assert qf.check("another") and qf.check_alt(12345) and all(qf.check_many([f"more{i}" for i in range(20)]))
    assert F.same_tables(tables(qf), M.canonical(qf.get_hashes(), 8))
