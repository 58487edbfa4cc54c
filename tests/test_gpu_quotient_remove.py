"""QuotientFilter.remove_many / remove_alt_many on the GPU: every step of tests/golden/golden_quotient_remove.json (the real reference's
tables) through the class under both removal paths and through psk_qf_remove_alt itself, then the shapes the fixture is too small for
against tests/qf_model.py (which tests/test_quotient_remove_model.py ties to the reference's removal).  All comparisons are exact equality."""

import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

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


def dev_u32(torch, values):
    a = np.asarray(values, dtype=np.uint64).astype(np.uint32)
    return torch.from_numpy(a.view(np.int32)).cuda()


def tables(qf):
    t = qf.tables()
    return t["filter"], t["occupied"], t["continuation"], t["shifted"]


def scratch_is_zero(qf) -> bool:
    """the part of the class's scratch the kernels read as bitmaps and cursor (the list behind it is written before it is read)"""
    s = qf._remove_scratch
    return s is None or not bool(s[: 2 * qf.occupied_tensor.numel() + 2].any().item())


def filter_with(pa, q, hashes, policy, auto_expand=False):
    qf = pa.QuotientFilter(quotient=q, auto_expand=auto_expand, device=0)
    qf._remove_policy = policy
    if len(hashes):
        qf.add_alt_many(hashes)
    return qf


def assert_holds(qf, held, q):
    """the table is the canonical one of `held`, and says so through every reading call"""
    assert qf.quotient == q and qf.elements_held == len(held)
    assert F.same_tables(tables(qf), M.canonical(held, q))
    assert sorted(qf.get_hashes()) == sorted(held)
    assert qf.validate_metadata() and scratch_is_zero(qf)


# ------------------------------------------------------------------ the fixture, through the class
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("case", F.CASES, ids=F.IDS)
def test_class_equals_reference_fixture(pa, case, policy):
    qf = filter_with(pa, case["q0"], [], policy, case["auto_expand"])
    before = frozenset()
    for st, held in zip(case["steps"], F.held_after(case)):
        if st["op"] == "add" and st["raised"]:
            with pytest.raises(pa.QuotientFilterError, match="insufficient space"):
                qf.add_alt_many(st["hashes"])
        elif st["op"] == "add":
            qf.add_alt_many(st["hashes"])
        else:
            assert qf.remove_alt_many(st["hashes"]) == len(before & set(st["hashes"]))
        where = (case["name"], st["op"], st["hashes"][:8])
        assert F.same_tables(tables(qf), F.dense(st)), where
        assert (qf.quotient, qf.elements_added, qf.elements_held) == (st["q"], st["elements_added"], len(held)), where
        assert qf.load_factor == st["elements_added"] / (1 << st["q"])
        assert qf.get_hashes() == st["get_hashes"], where
        probes = sorted(set(st["hashes"]) | held)
        if probes:
            assert qf.check_alt_many(probes).tolist() == [h in held for h in probes], where
        assert scratch_is_zero(qf), where
        before = held


# ------------------------------------------------------------------ the fixture, through the C ABI
class AbiTable:
    """the four arrays and the removal scratch as a caller of include/psk.h would hold them"""

    def __init__(self, torch, q, capacity):
        r = 32 - q
        self.torch, self.q, self.size = torch, q, 1 << q
        self.udt = np.uint8 if r <= 8 else (np.uint16 if r <= 16 else np.uint32)
        self.filter = torch.zeros(self.size, dtype={np.uint8: torch.uint8, np.uint16: torch.int16, np.uint32: torch.int32}[self.udt], device="cuda")
        self.words = max(self.size // 32, 1)
        self.occ, self.cont, self.sh = (torch.zeros(self.words, dtype=torch.int32, device="cuda") for _ in range(3))
        self.scratch = torch.zeros(2 * self.words + 2 + capacity, dtype=torch.int32, device="cuda")  # zeroed once: every call hands it back zeroed
        self.count = torch.full((1,), -7, dtype=torch.int32, device="cuda")

    def build(self, hashes):
        from pyprobables_amd import _native as N

        hs = dev_u32(self.torch, sorted(hashes))
        tiles = self.torch.empty(hs.numel() // 1024 + 2, dtype=self.torch.int32, device="cuda")
        N.check(N.lib().psk_qf_build(self.q, hs.data_ptr() if hs.numel() else None, hs.numel(), self.filter.data_ptr(), self.occ.data_ptr(), self.cont.data_ptr(),
                                     self.sh.data_ptr(), tiles.data_ptr(), 0, None))

    def remove(self, hashes) -> int:
        from pyprobables_amd import _native as N

        hs = dev_u32(self.torch, sorted(set(hashes)))
        N.check(N.lib().psk_qf_remove_alt(self.q, self.filter.data_ptr(), self.occ.data_ptr(), self.cont.data_ptr(), self.sh.data_ptr(),
                                          hs.data_ptr() if hs.numel() else None, hs.numel(), self.scratch.data_ptr(), self.count.data_ptr(), 0, None))
        return int(self.count.item())

    def arrays(self):
        bits = lambda t: np.unpackbits(t.cpu().numpy().view(np.uint8), bitorder="little")[: self.size]  # noqa: E731
        return self.filter.cpu().numpy().view(self.udt), bits(self.occ), bits(self.cont), bits(self.sh)


ABI_CASES = [c for c in F.CASES if c["q0"] >= 5]


@pytest.mark.parametrize("case", ABI_CASES, ids=[c["name"] for c in ABI_CASES])
def test_abi_equals_reference_fixture(torch, case):
    assert not case["auto_expand"]
    t = AbiTable(torch, case["q0"], max(len(st["hashes"]) for st in case["steps"]))
    before = frozenset()
    for st, held in zip(case["steps"], F.held_after(case)):
        if st["op"] == "add":
            t.build(held)  # (an add is a rebuild: the removal that follows meets the table the bulk build left)
        else:
            assert t.remove(st["hashes"]) == len(before & set(st["hashes"]))
            assert not bool(t.scratch[: 2 * t.words + 2].any().item())
        assert F.same_tables(t.arrays(), F.dense(st)), (case["name"], st["op"], st["hashes"][:8])
        before = held


def test_abi_refuses_the_tables_it_does_not_take(torch):
    from pyprobables_amd import _native as N

    t = AbiTable(torch, 5, 4)
    args = (t.filter.data_ptr(), t.occ.data_ptr(), t.cont.data_ptr(), t.sh.data_ptr())
    hs = dev_u32(torch, [1, 2])
    L = N.lib()
    assert L.psk_qf_remove_alt(4, *args, hs.data_ptr(), 2, t.scratch.data_ptr(), t.count.data_ptr(), 0, None) == N.PSK_EINVAL  # one replicated word
    assert L.psk_qf_remove_alt(5, *args, None, 2, t.scratch.data_ptr(), t.count.data_ptr(), 0, None) == N.PSK_EINVAL
    assert L.psk_qf_remove_alt(5, *args, hs.data_ptr(), 2, t.scratch.data_ptr(), None, 0, None) == N.PSK_EINVAL
    assert L.psk_qf_remove_alt(5, *args, None, 0, None, t.count.data_ptr(), 0, None) == 0 and int(t.count.item()) == 0  # an empty batch


# ------------------------------------------------------------------ q = 16 against the model
@pytest.fixture(scope="module")
def big():
    """40 000 distinct hashes at q = 16 (load 0.61), 10 000 of them to remove and 1 000 that are not there; the canonical tables before and after"""
    rng = np.random.default_rng(20241019)
    hs = np.unique(rng.integers(0, 2**32, size=60000, dtype=np.uint64))
    rng.shuffle(hs)
    have, absent = hs[:40000], hs[40000:41000]
    gone = have[:10000]
    batch = np.concatenate([gone, absent])
    rng.shuffle(batch)
    rest = set(have[10000:].tolist())
    return {"have": have, "batch": batch, "rest": rest, "want": M.canonical(rest, 16)}


@pytest.mark.parametrize("batches", (1, 10))
@pytest.mark.parametrize("policy", POLICIES)
def test_q16_equals_model(pa, big, policy, batches):
    qf = filter_with(pa, 16, big["have"], policy)
    removed = sum(qf.remove_alt_many(part) for part in np.array_split(big["batch"], batches))
    assert removed == 10000 and (qf.elements_held, qf.elements_added) == (30000, 40000)
    assert F.same_tables(tables(qf), big["want"]) and scratch_is_zero(qf)
    assert sorted(qf.get_hashes()) == sorted(big["rest"])
    assert qf.check_alt_many(big["batch"]).sum() == 0 and qf.check_alt_many(big["have"][10000:]).all()


def test_auto_takes_both_paths_by_batch_size(pa, big, monkeypatch):
    import pyprobables_amd.quotientfilter as Q

    calls = []
    for name in ("_remove_local", "_remove_rebuild"):
        monkeypatch.setattr(Q.QuotientFilter, name, lambda self, gone, _f=getattr(Q.QuotientFilter, name), _n=name: (calls.append(_n), _f(self, gone))[1])
    monkeypatch.setattr(Q, "REMOVE_LOCAL_MAX_FRACTION", 0.125)  # 5 000 of 40 000 held: in place; 6 000 of the ~35 500 left: rebuild
    qf = filter_with(pa, 16, big["have"], "auto")
    assert qf.remove_alt_many(big["batch"][:5000]) + qf.remove_alt_many(big["batch"][5000:]) == 10000
    assert calls == ["_remove_local", "_remove_rebuild"] and F.same_tables(tables(qf), big["want"])


# ------------------------------------------------------------------ the tables the in-place path does not take, under "auto"
def test_full_table_gives_the_canonical_table_of_the_rest(pa):
    rng = np.random.default_rng(3)
    hs = [int((quot << 27) | rem) for quot, rem in zip(rng.integers(0, 32, size=32), rng.permutation(1 << 20)[:32])]
    qf = filter_with(pa, 5, hs, "auto")
    assert qf.elements_held == qf.size == 32
    assert qf.remove_alt_many(hs[:5] + [hs[0] ^ 1]) == 5
    assert_holds(qf, set(hs[5:]), 5)
    assert (qf.elements_added, qf.load_factor) == (32, 1.0)
    full = filter_with(pa, 5, hs, "local")
    assert full.remove_alt_many(hs[30:]) == 2  # forced, a full table still rebuilds
    assert_holds(full, set(hs[:30]), 5)


@pytest.mark.parametrize("q", (3, 4))
def test_one_word_tables(pa, q):
    size, r = 1 << q, 32 - q
    hs = [((size - 1) << r) | 5, ((size - 1) << r) | 9, ((size - 2) << r) | 1, 7, 8, (2 << r) | 3]  # a cluster over the table's end
    qf = filter_with(pa, q, hs, "auto")
    assert qf.remove_alt_many([hs[0], 7, (3 << r) | 3]) == 2
    assert_holds(qf, set(hs) - {hs[0], 7}, q)
    assert qf.remove_alt_many(hs) == 4
    assert_holds(qf, set(), q)
    assert qf.elements_added == 6 and qf.remove_alt_many(hs) == 0


# ------------------------------------------------------------------ the surface
@pytest.mark.parametrize("policy", POLICIES)
def test_add_after_remove_and_counters(pa, policy):
    rng = np.random.default_rng(8)
    hs = np.unique(rng.integers(0, 2**32, size=150, dtype=np.uint64)).tolist()
    qf = filter_with(pa, 8, hs[:120], policy)
    assert qf.remove_alt_many(hs[:50]) == 50 and (qf.elements_held, qf.elements_added) == (70, 120)
    qf.add_alt_many(hs[40:60] + hs[120:130])  # 10 come back, 10 were there, 10 are new
    assert_holds(qf, set(hs[40:130]), 8)
    assert (qf.elements_held, qf.elements_added, qf.load_factor) == (90, 140, 140 / 256)
    qf.resize(9)  # any resize forgets the removals
    assert_holds(qf, set(hs[40:130]), 9)
    assert (qf.elements_held, qf.elements_added) == (90, 90)
    with pytest.raises(pa.NotSupportedError):
        qf.remove_alt(hs[40])


@pytest.mark.parametrize("policy", POLICIES)
def test_device_and_host_inputs_keys_and_hashes(pa, torch, policy):
    keys = [f"key-{i:04d}" for i in range(400)]  # 8 bytes each
    h = [pa.hashes.fnv_1a_32(k, 0) for k in keys]
    qf = pa.QuotientFilter(quotient=10, device=0)
    qf._remove_policy = policy
    qf.add_many(keys)
    assert qf.elements_held == len(set(h)) == 400
    assert qf.remove_many(keys[:100] + ["nobody", keys[0]]) == 100  # a host list
    fixed = np.frombuffer("".join(keys[100:200]).encode(), dtype=np.uint8).reshape(100, 8)
    assert qf.remove_many(torch.from_numpy(fixed.copy()).cuda()) == 100  # device keys
    assert qf.remove_alt_many(dev_u32(torch, h[200:300] + h[200:205] + h[:3])) == 100  # a device tensor of hashes: duplicates, and three already gone
    assert qf.remove_alt_many(np.asarray(h[:300], dtype=np.uint32)) == 0 and qf.remove_alt_many(h[:3]) == 0  # numpy, ints: nothing left of these
    assert qf.remove_alt_many(h[300]) == 1 and qf.remove_many(keys[301]) == 1  # one hash, one key
    assert_holds(qf, set(h[302:]), 10)
    assert (qf.elements_added, qf.elements_held) == (400, 98)
    assert not qf.check_many(keys[:302]).any() and qf.check_many(keys[302:]).all()


@pytest.mark.parametrize("policy", POLICIES + ("auto",))
def test_empty_batch_and_empty_filter(pa, torch, policy):
    qf = filter_with(pa, 6, [], policy)
    assert qf.remove_alt_many([1, 2, 3]) == 0 and qf.remove_many([]) == 0
    qf.add_alt_many([5 << 26, (5 << 26) | 1])
    want = tables(qf)
    assert qf.remove_alt_many([]) == 0 and qf.remove_alt_many(torch.empty(0, dtype=torch.int32, device="cuda")) == 0 and qf.remove_many([]) == 0
    assert F.same_tables(tables(qf), want) and (qf.elements_held, qf.elements_added) == (2, 2) and scratch_is_zero(qf)
