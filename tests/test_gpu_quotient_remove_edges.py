"""psk_qf_remove_alt at its seams, its ring and its grid caps: the tables of tests/qf_remove_edges.py (which tests/test_quotient_remove_model.py
runs through the host model of the two kernels and checks for the property each is there for), an exhaustive walk over the table's end, the
class under ``_remove_policy = "local"``, one scratch across table sizes and both in-place paths, and a batch with more hashes and more dirty
clusters than the launches have lanes.

The reference everywhere is tests/qf_model.canonical(the remaining set) -- never the package's own rebuild path.  All comparisons are exact
equality.  What only the GPU can show is here: lanes that repair clusters in one metadata word at the same time, the masks, the strides."""

import itertools
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import qf_model as M  # noqa: E402
import qf_remove_edges as E  # noqa: E402
import qf_remove_fixture as F  # noqa: E402
from qf_remove_model import pack  # noqa: E402


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


def dev_u32(torch, values):
    a = np.asarray(values, dtype=np.uint64).astype(np.uint32)
    return torch.from_numpy(a.view(np.int32)).cuda()


class AbiTable:
    """the four arrays and the removal scratch as a caller of include/psk.h would hold them"""

    def __init__(self, torch, q, capacity):
        r = 32 - q
        self.torch, self.q, self.size = torch, q, 1 << q
        self.udt = np.uint8 if r <= 8 else (np.uint16 if r <= 16 else np.uint32)
        self.filter = torch.zeros(self.size, dtype={np.uint8: torch.uint8, np.uint16: torch.int16, np.uint32: torch.int32}[self.udt], device="cuda")
        self.words = self.size // 32
        self.occ, self.cont, self.sh = (torch.zeros(self.words, dtype=torch.int32, device="cuda") for _ in range(3))
        self.scratch = torch.zeros(2 * self.words + 2 + capacity, dtype=torch.int32, device="cuda")  # zeroed once: every call hands it back zeroed
        self.count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        self.tiles = torch.empty(capacity // 1024 + 2, dtype=torch.int32, device="cuda")
        self.capacity = capacity

    def args(self):
        return (self.q, self.filter.data_ptr(), self.occ.data_ptr(), self.cont.data_ptr(), self.sh.data_ptr())

    def build_dev(self, hs):
        """`hs`: sorted distinct hashes, an int32 device tensor"""
        from pyprobables_amd import _native as N

        assert hs.numel() <= self.capacity
        N.check(N.lib().psk_qf_build(self.q, hs.data_ptr() if hs.numel() else None, hs.numel(), *self.args()[1:], self.tiles.data_ptr(), 0, None))

    def remove_dev(self, hs):
        from pyprobables_amd import _native as N

        assert hs.numel() <= self.capacity
        N.check(N.lib().psk_qf_remove_alt(*self.args(), hs.data_ptr() if hs.numel() else None, hs.numel(), self.scratch.data_ptr(), self.count.data_ptr(), 0, None))

    def check_dev(self, hs):
        from pyprobables_amd import _native as N

        out = self.torch.empty(hs.numel(), dtype=self.torch.uint8, device="cuda")
        N.check(N.lib().psk_qf_check_alt(*self.args(), hs.data_ptr() if hs.numel() else None, hs.numel(), out.data_ptr(), 0, None))
        return out

    def build(self, hashes):
        self.build_dev(dev_u32(self.torch, sorted(set(hashes))))

    def remove(self, hashes) -> int:
        self.remove_dev(dev_u32(self.torch, sorted(set(hashes))))
        return int(self.count.item())

    def check(self, hashes) -> list:
        return self.check_dev(dev_u32(self.torch, hashes)).cpu().numpy().astype(bool).tolist()

    def scratch_is_zero(self) -> bool:
        return not bool(self.scratch[: 2 * self.words + 2].any().item())

    def arrays(self):
        bits = lambda t: np.unpackbits(t.cpu().numpy().view(np.uint8), bitorder="little")[: self.size]  # noqa: E731
        return self.filter.cpu().numpy().view(self.udt), bits(self.occ), bits(self.cont), bits(self.sh)


def abi_remove(t, q, held, gone):
    """build `held`, remove `gone` in place; everything the call promises, against the canonical table of the rest -> that table"""
    held = set(held)
    rest = held - set(gone)
    t.build(held)
    removed = t.remove(gone)
    want = M.canonical(rest, q)
    assert F.same_tables(t.arrays(), want)
    assert removed == len(held) - len(rest)
    assert t.scratch_is_zero()
    probes = sorted(held | set(gone))
    assert t.check(probes) == [h in rest for h in probes]
    return want


# ------------------------------------------------------------------ the C ABI
def test_abi_every_assignment_on_the_ring_q5(torch):
    """seven hashes with quotients {30, 31, 0, 1} and two remainders, each absent, kept or removed: 3^7 tables, each built with psk_qf_build and
    cut down with psk_qf_remove_alt.  Two hashes that are in no table go into every batch, and so does what the assignment left out.
    One upload and one flag per table: the expected arrays, count, scratch and lookups travel with the hashes and are compared on the device;
    a table that differs is read back and compared again for the message."""
    q = 5
    pool = [E.m(q, 30, 1), E.m(q, 30, 2), E.m(q, 31, 1), E.m(q, 31, 2), E.m(q, 0, 1), E.m(q, 0, 2), E.m(q, 1, 1)]
    never = [E.m(q, 31, 3), E.m(q, 2, 1)]
    probes = sorted(pool + never)
    t = AbiTable(torch, q, 16)
    for assign in itertools.product((0, 1, 2), repeat=len(pool)):
        held = sorted(h for h, a in zip(pool, assign) if a)
        batch = sorted([h for h, a in zip(pool, assign) if a != 1] + never)
        rest = {h for h, a in zip(pool, assign) if a == 1}
        want = M.canonical(rest, q)
        tail = [want[0].astype(np.uint64), *(pack(a).astype(np.uint64) for a in want[1:]), [len(held) - len(rest)], [0] * 4, [h in rest for h in probes]]
        dev = dev_u32(torch, np.concatenate([np.asarray(x, dtype=np.uint64) for x in (held, batch, probes, *tail)]))
        a, b, c = len(held), len(held) + len(batch), len(held) + len(batch) + len(probes)
        t.build_dev(dev[:a])
        t.remove_dev(dev[a:b])
        found = t.check_dev(dev[b:c])
        got = torch.cat([t.filter, t.occ, t.cont, t.sh, t.count, t.scratch[:4], found.to(torch.int32)])
        if not torch.equal(got, dev[c:]):
            assert F.same_tables(t.arrays(), want), (held, batch)
            assert int(t.count.item()) == len(held) - len(rest) and t.scratch_is_zero(), (held, batch)
            assert found.cpu().numpy().astype(bool).tolist() == [h in rest for h in probes], (held, batch)
            raise AssertionError((held, batch))


@pytest.mark.parametrize("name", E.NAMES)
def test_abi_edge_case(torch, name):
    q, held, gone = E.CASES[name]
    abi_remove(AbiTable(torch, q, max(len(held), len(set(gone)))), q, held, gone)


# ------------------------------------------------------------------ the class
def tables(qf):
    t = qf.tables()
    return t["filter"], t["occupied"], t["continuation"], t["shifted"]


def scratch_is_zero(qf) -> bool:
    s = qf._remove_scratch
    return s is not None and not bool(s[: 2 * qf.occupied_tensor.numel() + 2].any().item())


def local_filter(pa, q, hashes):
    """a filter that holds `hashes` and takes both in-place paths whenever they apply -> (filter, the in-place calls it made)"""
    qf = pa.QuotientFilter(quotient=q, auto_expand=False, device=0)
    qf.add_alt_many(hashes)
    qf._remove_policy = qf._add_policy = "local"
    calls = []
    for name in ("_remove_local", "_add_local"):
        inner = getattr(qf, name)
        setattr(qf, name, lambda bits, _inner=inner, _name=name: (calls.append(_name), _inner(bits))[1])
    return qf, calls


def assert_holds(qf, held, q):
    assert qf.quotient == q and qf.elements_held == len(held)
    assert F.same_tables(tables(qf), M.canonical(held, q))
    assert sorted(qf.get_hashes()) == sorted(held)
    assert qf.validate_metadata() and scratch_is_zero(qf)


@pytest.mark.parametrize("name", E.NAMES)
def test_class_local_edge_case_equals_the_abi(pa, torch, name):
    q, held, gone = E.CASES[name]
    rest = set(held) - set(gone)
    qf, calls = local_filter(pa, q, held)
    assert qf.remove_alt_many(gone + gone[:2]) == len(held) - len(rest) and calls == ["_remove_local"]
    assert_holds(qf, rest, q)
    t = AbiTable(torch, q, max(len(held), len(set(gone))))
    t.build(held)
    t.remove(gone)
    assert F.same_tables(tables(qf), t.arrays())


def test_class_one_scratch_across_sizes_and_both_in_place_paths(pa):
    rng = np.random.default_rng(812)
    hs = np.unique(rng.integers(0, 2**32, size=3400, dtype=np.uint64)).tolist()
    assert len(hs) >= 3300
    qf, calls = local_filter(pa, 8, hs[:150])
    held = set(hs[:150])
    assert qf.remove_alt_many(hs[:60] + hs[3000:3010]) == 60  # q = 8: a scratch of 2 * 8 + 2 + 1024 words
    held -= set(hs[:60])
    assert_holds(qf, held, 8)
    small = qf._remove_scratch
    qf.resize(12)  # forgets the scratch; the table is built anew
    assert F.same_tables(tables(qf), M.canonical(held, 12)) and qf._remove_scratch is None
    qf.add_alt_many(hs[150:3000])  # in place, on a scratch sized for the batch
    held |= set(hs[150:3000])
    assert calls[-1] == "_add_local"
    assert_holds(qf, held, 12)
    assert qf._remove_scratch is not small and qf._remove_scratch.numel() == 2 * 128 + 2 + 2850
    scratch = qf._remove_scratch
    assert qf.remove_alt_many(hs[100:2100] + hs[3000:3100]) == 2000  # a batch that fits the scratch the insertion left
    held -= set(hs[100:2100])
    assert_holds(qf, held, 12)
    assert qf._remove_scratch is scratch
    assert qf.remove_alt_many(hs[:3300]) == len(held)  # one that does not: everything goes
    assert_holds(qf, set(), 12)
    assert qf._remove_scratch is not scratch
    qf.add_alt_many(hs[:40])  # an empty filter bulk-builds ...
    qf.add_alt_many(hs[40:900])  # ... and this goes in place
    assert qf.remove_alt_many(hs[20:500]) == 480
    assert_holds(qf, set(hs[:20] + hs[500:900]), 12)
    assert calls == ["_remove_local", "_add_local", "_remove_local", "_remove_local", "_add_local", "_remove_local"]


# ------------------------------------------------------------------ more hashes, and more dirty clusters, than 4096 x 256 lanes
LANES = 4096 * 256


@pytest.fixture(scope="module")
def grid_cap_sets():
    """q = 23 at load 0.31: 2.65 M draws, 1.4 M of the distinct ones removed; how many clusters that dirties is counted on the CPU"""
    rng = np.random.default_rng(23)
    hs = np.unique(rng.integers(0, 2**32, size=2_650_000, dtype=np.uint64))
    rng.shuffle(hs)
    gone, rest = hs[:1_400_000], hs[1_400_000:]
    more = rng.integers(0, 2**32, size=4000, dtype=np.uint64)
    absent = more[~np.isin(more, hs)][:1000]
    batch = np.concatenate([gone, absent, gone[:1000]])
    rng.shuffle(batch)
    sorted_hs, _, start = E.layout(hs, 23)
    dirty = np.unique(start[np.isin(sorted_hs, gone.astype(np.int64))]).size
    return {"held": hs, "gone": gone, "rest": rest, "absent": absent, "batch": batch, "dirty": int(dirty), "clusters": int(np.unique(start).size)}


def test_class_local_grid_caps_q23(grid_cap_sets, pa):
    s = grid_cap_sets
    assert s["gone"].size > LANES and s["absent"].size == 1000 and s["batch"].size == s["gone"].size + 2000
    assert s["dirty"] > LANES, s["dirty"]  # (1 223 115 of 2 132 382 clusters with this draw)
    qf, calls = local_filter(pa, 23, s["held"])
    assert qf.elements_held == s["held"].size
    assert qf.remove_alt_many(s["batch"]) == s["gone"].size and calls == ["_remove_local"]
    assert (qf.elements_held, qf.elements_added) == (s["rest"].size, s["held"].size)
    assert F.same_tables(tables(qf), M.canonical(s["rest"], 23))
    assert qf.validate_metadata() and scratch_is_zero(qf)
    assert not qf.check_alt_many(s["batch"]).any() and qf.check_alt_many(s["rest"]).all()
