"""QuotientFilter on the GPU: every case of tests/golden/golden_quotient.json (the real reference's tables) through the C ABI and through
the class, and the shapes the fixtures are too small for against tests/qf_model.py (which tests/test_quotient_model.py ties to the
reference).  All comparisons are exact equality."""

import json
import random
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import qf_model as M  # noqa: E402

FIXTURE = json.loads((ROOT / "tests" / "golden" / "golden_quotient.json").read_text())
CASES, EXPAND = FIXTURE["cases"], FIXTURE["expand_cases"]
BY_NAME = {c["name"]: c for c in CASES}
IDS = [c["name"] for c in CASES]


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
    """the four arrays as a caller of include/psk.h would hold them"""

    def __init__(self, torch, q):
        r = 32 - q
        self.torch, self.q, self.size = torch, q, 1 << q
        self.udt = np.uint8 if r <= 8 else (np.uint16 if r <= 16 else np.uint32)
        self.filter = torch.full((self.size,), 7, dtype={np.uint8: torch.uint8, np.uint16: torch.int16, np.uint32: torch.int32}[self.udt], device="cuda")
        words = max(self.size // 32, 1)
        self.occ, self.cont, self.sh = (torch.full((words,), -1, dtype=torch.int32, device="cuda") for _ in range(3))  # (build overwrites: not zeroed here)

    def args(self):
        return (self.q, self.filter.data_ptr(), self.occ.data_ptr(), self.cont.data_ptr(), self.sh.data_ptr())

    def build(self, hashes):
        from pyprobables_amd import _native as N

        hs = dev_u32(self.torch, sorted(set(int(h) for h in hashes)))
        scratch = self.torch.empty(hs.numel() // 1024 + 2, dtype=self.torch.int32, device="cuda")
        N.check(N.lib().psk_qf_build(self.q, hs.data_ptr() if hs.numel() else None, hs.numel(), self.filter.data_ptr(), self.occ.data_ptr(), self.cont.data_ptr(),
                                     self.sh.data_ptr(), scratch.data_ptr(), 0, None))
        self.n = hs.numel()
        return self

    def arrays(self):
        bits = lambda t: np.unpackbits(t.cpu().numpy().view(np.uint8), bitorder="little")[: self.size]  # noqa: E731
        return self.filter.cpu().numpy().view(self.udt), bits(self.occ), bits(self.cont), bits(self.sh)

    def check_alt(self, probes):
        from pyprobables_amd import _native as N

        p = dev_u32(self.torch, probes)
        out = self.torch.empty(p.numel(), dtype=self.torch.uint8, device="cuda")
        N.check(N.lib().psk_qf_check_alt(*self.args(), p.data_ptr() if p.numel() else None, p.numel(), out.data_ptr(), 0, None))
        return out.cpu().numpy().astype(bool).tolist()

    def decode(self):
        """-> (hashes in slot order, first empty slot or None)"""
        from pyprobables_amd import _native as N

        t, L = self.torch, N.lib()
        words = self.occ.numel()
        counts = t.empty((3, words), dtype=t.int64, device="cuda")
        marks = t.empty(2, dtype=t.int32, device="cuda")
        N.check(L.psk_qf_decode(*self.args(), counts.data_ptr(), marks.data_ptr(), None, 0, 0, None))
        inc = t.cumsum(counts, dim=1).contiguous()
        assert int(inc[2, -1]) == self.n
        out = t.full((self.n + 1,), -1, dtype=t.int32, device="cuda")
        N.check(L.psk_qf_decode(*self.args(), inc.data_ptr(), marks.data_ptr(), out.data_ptr(), self.n, 0, None))
        got = out.cpu().numpy().view(np.uint32).tolist()
        assert got[-1] == 0xFFFFFFFF  # nothing written past out_cap
        e = int(marks[1].item()) & 0xFFFFFFFF
        return got[:-1], (None if e == 0xFFFFFFFF else e)


def reference_arrays(case):
    return case["filter"], case["occupied"], case["continuation"], case["shifted"]


def class_arrays(qf):
    t = qf.tables()
    return t["filter"], t["occupied"], t["continuation"], t["shifted"]


def model_arrays(hashes, q):
    return M.canonical(hashes, q)


def same(got, want) -> bool:
    """the four arrays, element for element"""
    return len(got) == len(want) == 4 and all(np.array_equal(np.asarray(g, dtype=np.int64), np.asarray(w, dtype=np.int64)) for g, w in zip(got, want))


# ------------------------------------------------------------------ the reference's own tables
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture_through_the_c_abi(torch, case):
    tab = AbiTable(torch, case["q"]).build(case["stream"])
    assert same(tab.arrays(), reference_arrays(case))
    assert tab.check_alt(case["probes"]) == case["answers"]
    listed, first_empty = tab.decode()
    assert sorted(listed) == sorted(set(case["stream"]))
    if case["get_hashes"] is None:
        assert first_empty is None
    else:  # slot order from the first empty slot on is the reference's own walk
        used = np.array(case["occupied"]) | np.array(case["continuation"]) | np.array(case["shifted"])
        rank = int(used[:first_empty].sum())
        assert listed[rank:] + listed[:rank] == case["get_hashes"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture_through_the_class(pa, case):
    qf = pa.QuotientFilter(quotient=case["q"], auto_expand=False)
    qf.add_alt_many(case["stream"])
    assert same(class_arrays(qf), reference_arrays(case))
    assert qf.elements_added == case["elements_added"] and qf.quotient == case["q"]
    assert qf.get_hashes() == (case["get_hashes"] if case["get_hashes"] is not None else sorted(set(case["stream"])))
    assert qf.check_alt_many(case["probes"]).tolist() == case["answers"]
    assert [qf.check_alt(p) for p in case["probes"][:6]] == case["answers"][:6]
    assert qf.validate_metadata()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture_in_two_batches_goes_through_decode_and_rebuild(pa, case):
    stream = case["stream"]
    for cut in (1, len(stream) // 2):
        qf = pa.QuotientFilter(quotient=case["q"], auto_expand=False)
        qf.add_alt_many(stream[:cut])
        qf.add_alt_many(stream[cut:])
        assert same(class_arrays(qf), reference_arrays(case)), cut
        assert qf.elements_added == case["elements_added"]


def test_one_set_in_three_orders_gives_one_table(pa):
    fwd, rev, shuf = BY_NAME["orders_q6_forward"], BY_NAME["orders_q6_reversed"], BY_NAME["orders_q6_shuffled"]
    assert rev["stream"] == fwd["stream"][::-1] and sorted(shuf["stream"]) == sorted(fwd["stream"])
    tables = []
    for c in (fwd, rev, shuf):
        qf = pa.QuotientFilter(quotient=6, auto_expand=False)
        qf.add_alt_many(c["stream"])
        tables.append(class_arrays(qf))
    assert same(tables[0], tables[1]) and same(tables[1], tables[2]) and same(tables[2], reference_arrays(fwd))


@pytest.mark.parametrize("case", EXPAND, ids=[c["name"] for c in EXPAND])
def test_auto_expand_lands_on_the_reference_quotient(pa, case):
    stream = case["stream"]
    for cuts in ((), (len(stream) // 2,), (1, len(stream) - 1)):
        qf = pa.QuotientFilter(quotient=case["q0"])
        edges = [0, *cuts, len(stream)]
        for a, b in zip(edges, edges[1:]):
            qf.add_alt_many(stream[a:b])
        assert qf.quotient == case["q"], cuts
        assert same(class_arrays(qf), reference_arrays(case))
        assert qf.elements_added == case["elements_added"] and qf.get_hashes() == case["get_hashes"]


def test_per_key_calls_match_the_batch(pa):
    case = BY_NAME["wrap_pushes_head_q4"]
    qf = pa.QuotientFilter(quotient=4, auto_expand=False)
    for h in case["stream"]:
        qf.add_alt(h)
    assert same(class_arrays(qf), reference_arrays(case))
    assert list(qf.hashes()) == case["get_hashes"]


def test_no_room_raises_before_the_table_changes(pa):
    case = BY_NAME["random_q3_load0.6"]
    qf = pa.QuotientFilter(quotient=3, auto_expand=False)
    qf.add_alt_many(case["stream"])
    more = [h ^ 0x5A5A5A for h in range(1, 8)]
    with pytest.raises(pa.QuotientFilterError) as ex:
        qf.add_alt_many(more)
    assert str(ex.value) == "Unable to insert the element due to insufficient space"
    assert same(class_arrays(qf), reference_arrays(case)) and qf.elements_added == case["elements_added"]


def test_resize_and_merge(pa):
    case = BY_NAME["random_q6_load0.6"]
    hs = sorted(set(case["stream"]))
    qf = pa.QuotientFilter(quotient=6, auto_expand=False)
    qf.add_alt_many(case["stream"])
    with pytest.raises(pa.QuotientFilterError, match="Unable to shrink"):
        qf.resize(5)
    with pytest.raises(pa.QuotientFilterError, match="between 3 and 31; 32 was provided"):
        qf.resize(32)
    qf.resize()
    assert qf.quotient == 7 and same(class_arrays(qf), model_arrays(hs, 7)) and qf.elements_added == len(hs)
    qf.resize(10)
    assert same(class_arrays(qf), model_arrays(hs, 10))
    other = pa.QuotientFilter(quotient=8, auto_expand=False)
    extra = [0x01020304, 0xFFFFFFF0, hs[0], 77]
    other.add_alt_many(extra)
    qf.merge(other)
    assert same(class_arrays(qf), model_arrays(hs + extra, 10)) and qf.elements_added == len(set(hs + extra))
    with pytest.raises(pa.QuotientFilterError, match="Hash functions do not match"):
        qf.merge(pa.QuotientFilter(quotient=8, hash_function=lambda key, seed: 5))


# ------------------------------------------------------------------ shapes the fixtures are too small for, against the model
def mk(q, quot, rem):
    return (quot << (32 - q)) | rem


def assert_matches_model(torch, q, hashes, probes_absent):
    hashes = sorted(set(hashes))
    tab = AbiTable(torch, q).build(hashes)
    assert same(tab.arrays(), model_arrays(hashes, q))
    listed, _ = tab.decode()
    assert sorted(listed) == hashes
    held = set(hashes)
    absent = [p for p in probes_absent if p not in held]
    step = max(1, len(hashes) // 4000)
    assert all(tab.check_alt(hashes[::step])) and not any(tab.check_alt(absent))
    return tab


def neighbours(q, hashes, rng, count=2000):
    """absent probes that share quotients with the set: the remainder next door, the ends of the remainder range, random ones"""
    pick = rng.sample(hashes, min(count, len(hashes)))
    r = 32 - q
    return [h ^ 1 for h in pick] + [(h >> r << r) | ((1 << r) - 1) for h in pick[:200]] + [h >> r << r for h in pick[:200]] + [rng.getrandbits(32) for _ in range(count)]


@pytest.mark.parametrize("n", [1024 + 6, 2048 + 7, 4096], ids=["just_over_one_scan_block", "just_over_two", "full"])
def test_block_carry_seam_q12(torch, n):
    rng = random.Random(n)
    hs = set()
    while len(hs) < n:  # dense stretches so that the prefix max is carried across the tile boundaries
        hs.add(mk(12, rng.choice([rng.randrange(4096), 900 + rng.randrange(300), 2000 + rng.randrange(100)]), rng.randrange(1 << 20)))
    hs = sorted(hs)
    assert_matches_model(torch, 12, hs, neighbours(12, hs, rng))


def test_wrapped_tail_pushes_more_than_a_block_of_head_elements(torch):
    rng = random.Random(5)
    tail = {mk(12, 4095 - rng.randrange(4), rng.randrange(1 << 20)) for _ in range(1500)}  # ~1500 elements in the last four slots' quotients
    head = {mk(12, quot, rng.randrange(1 << 20)) for quot in range(0, 1300)}               # one per quotient: each is pushed by the carry
    hs = sorted(tail | head)
    pos = M.positions(np.array(hs, dtype=np.int64), 12)
    assert pos[-1] - 4096 > 1024 and int((pos[: len(head)] != np.arange(len(head))).sum()) > 1024
    assert_matches_model(torch, 12, hs, neighbours(12, hs, rng))


def test_runs_and_clusters_that_straddle_metadata_words(torch):
    rng = random.Random(6)
    hs = [mk(8, 30, x) for x in (5, 9, 11, 200, 4000)]                                         # one run over slots 30 .. 34
    hs += [mk(8, quot, rng.randrange(1 << 24)) for quot in range(70, 76) for _ in range(20)]   # one cluster over ~120 slots
    hs += [mk(8, 255, x) for x in range(40)]                                                   # a run that wraps from the last word into the first
    tab = assert_matches_model(torch, 8, hs, neighbours(8, hs, rng, 150))
    assert tab.check_alt([mk(8, 30, 4000), mk(8, 30, 4001), mk(8, 31, 5), mk(8, 75, 0), mk(8, 0, 3)]) == [True, False, False, mk(8, 75, 0) in hs, False]


def test_all_keys_in_one_quotient(torch):
    rng = random.Random(8)
    hs = [mk(10, 500, x) for x in rng.sample(range(1 << 22), 300)]
    assert_matches_model(torch, 10, hs, neighbours(10, hs, rng, 300))


@pytest.mark.parametrize("q,n", [(24, 200_000), (20, 300_000), (10, 700)], ids=["uint8_r8", "uint16_r12", "uint32_r22"])
def test_each_remainder_width(torch, q, n):
    rng = np.random.default_rng(q)
    hs = np.unique(rng.integers(0, 1 << 32, size=n, dtype=np.uint64)).tolist()
    assert_matches_model(torch, q, hs, neighbours(q, hs, random.Random(q)))


def test_full_table_q8(torch):
    rng = random.Random(9)
    hs = set()
    while len(hs) < 256:
        hs.add(mk(8, rng.choice([rng.randrange(256), 250 + rng.randrange(6)]), rng.randrange(64)))
    hs = sorted(hs)
    tab = assert_matches_model(torch, 8, hs, neighbours(8, hs, rng, 256))
    assert tab.decode()[1] is None


def test_smallest_tables_q3(torch):
    rng = random.Random(10)
    for n in range(0, 9):
        hs = sorted({mk(3, rng.choice([7, 6, rng.randrange(8)]), rng.randrange(4)) for _ in range(40)})[:n] if n < 8 else [mk(3, 7, x) for x in range(8)]
        assert_matches_model(torch, 3, hs, [mk(3, quot, rem) for quot in range(8) for rem in range(6)])


def test_q31_one_bit_remainders(torch):
    """r = 1: the uint8 class at its narrowest, 2^31 slots; compared where the set lives (both ends of the table, the tail wrapping)"""
    rng = random.Random(31)
    q, size = 31, 1 << 31
    hs = sorted({mk(q, quot, rem) for quot in [*range(0, 3000, 3), *range(size - 1200, size), *[size - 1 - rng.randrange(50) for _ in range(200)]] for rem in (0, 1)
                 if rng.random() < 0.8})
    tab = AbiTable(torch, q).build(hs)
    a = np.array(hs, dtype=np.int64)
    pos = M.positions(a, q)
    assert pos[-1] >= size  # the tail wraps
    p = torch.from_numpy(pos % size).cuda()
    qs = a >> 1
    bit = lambda t, at: ((t[at >> 5] >> (at & 31)) & 1).cpu().numpy()  # noqa: E731
    assert np.array_equal(tab.filter[p].cpu().numpy(), (a & 1).astype(np.uint8))
    assert np.array_equal(bit(tab.cont, p), np.concatenate([[0], qs[1:] == qs[:-1]]).astype(np.int32))
    assert np.array_equal(bit(tab.sh, p), (pos % size != qs).astype(np.int32))
    assert bit(tab.occ, torch.from_numpy(qs).cuda()).all()
    pc = lambda t: int(sum(((t >> s) & 1).sum().item() for s in range(32)))  # noqa: E731
    assert pc(tab.occ) == len(set(qs.tolist())) and pc(tab.sh) == int((pos % size != qs).sum()) and pc(tab.cont) == int((qs[1:] == qs[:-1]).sum())
    assert int(tab.filter.sum(dtype=torch.int64).item()) == int((a & 1).sum())
    present = set(hs)
    probes = [h ^ 1 for h in hs[:500]] + [h ^ 1 for h in hs[-500:]] + [mk(q, size // 2, 1), 0, 2**32 - 1]
    assert tab.check_alt(hs[:300] + hs[-300:]) == [True] * 600
    assert tab.check_alt(probes) == [x in present for x in probes]
    listed, _ = tab.decode()
    assert sorted(listed) == hs


def test_empty_filter(pa, torch):
    qf = pa.QuotientFilter(quotient=7)
    assert qf.check_many(["a", "b", "c"]).tolist() == [False] * 3
    assert qf.check_alt_many(dev_u32(torch, [0, 5, 2**32 - 1])).tolist() == [False] * 3
    assert qf.get_hashes() == [] and list(qf.hashes()) == [] and qf.elements_added == 0
    tab = AbiTable(torch, 7).build([])
    assert same(tab.arrays(), model_arrays([], 7)) and tab.decode() == ([], 0)
    qf.add_many([])
    assert qf.elements_added == 0 and "a" not in qf


# ------------------------------------------------------------------ hashing on the device
def test_key_layouts_hash_like_fnv_1a_32(pa, torch):
    from pyprobables_amd import _native as N
    from pyprobables_amd.hashes import fnv_1a_32
    from pyprobables_amd.keys import pack_keys

    rng = np.random.default_rng(4)
    batches = {
        "fixed16": rng.integers(0, 256, size=(1500, 16), dtype=np.uint8),
        "fixed8": rng.integers(0, 256, size=(1500, 8), dtype=np.uint8),
        "fixed32": rng.integers(0, 256, size=(300, 32), dtype=np.uint8),
        "fixed12": rng.integers(0, 256, size=(300, 12), dtype=np.uint8),
        "fixed5": rng.integers(0, 256, size=(700, 5), dtype=np.uint8),
    }
    for name, a in batches.items():
        want = [fnv_1a_32(bytes(row), 0) for row in a]
        for keys in (a, torch.from_numpy(a).cuda()):
            b = pack_keys(keys)
            if b.where == N.DEVICE:
                out = torch.empty(b.n, dtype=torch.int32, device="cuda")
                N.check(N.lib().psk_qf_hash(*b.args(), N.DEVICE, out.data_ptr(), 0, None))
                got = out.cpu().numpy().view(np.uint32).tolist()
            else:
                out = np.empty(b.n, dtype=np.uint32)
                N.check(N.lib().psk_qf_hash(*b.args(), N.HOST, out.ctypes.data, 0, None))
                got = out.tolist()
            assert got == want, name
    ragged = [bytes(rng.integers(0, 256, size=int(ln), dtype=np.uint8)) for ln in rng.integers(0, 70, size=900)]
    blob = np.frombuffer(b"".join(ragged), dtype=np.uint8).copy()
    offs = np.concatenate([[0], np.cumsum([len(k) for k in ragged])]).astype(np.uint64)
    want = [fnv_1a_32(k, 0) for k in ragged]
    qf = pa.QuotientFilter(quotient=12)
    for keys in (ragged, (blob, offs), (torch.from_numpy(blob).cuda(), torch.from_numpy(offs.view(np.int64)).cuda())):
        assert qf._hash_keys(keys).cpu().numpy().view(np.uint32).tolist() == want
    words = ["", "a", "foobar", "héllo", "€uro", "日本語のキー", "x" * 37]
    assert qf._hash_keys(words).cpu().numpy().view(np.uint32).tolist() == [fnv_1a_32(w, 0) for w in words]


def test_keys_end_to_end(pa, torch):
    from pyprobables_amd.hashes import fnv_1a_32

    rng = np.random.default_rng(12)
    keys = rng.integers(0, 256, size=(5000, 16), dtype=np.uint8)
    absent = rng.integers(0, 256, size=(5000, 16), dtype=np.uint8)
    hs = [fnv_1a_32(bytes(k), 0) for k in keys]
    qf = pa.QuotientFilter(quotient=10)  # grows on the way
    qf.add_many(torch.from_numpy(keys[:3000]).cuda())
    qf.add_many(keys[3000:])
    q = qf.quotient
    assert q == M.final_quotient(hs, 10) and same(class_arrays(qf), model_arrays(hs, q))
    assert qf.check_many(torch.from_numpy(keys).cuda()).all().item() and qf.check_many(keys).all()
    want_absent = [fnv_1a_32(bytes(k), 0) in set(hs) for k in absent]
    assert qf.check_many(absent).tolist() == want_absent
    small = pa.QuotientFilter(quotient=3)
    for w in ("alpha", "beta", "gamma"):
        small.add(w)
    assert "alpha" in small and small.check("beta") and "delta" not in small and small.elements_added == 3
    custom = pa.QuotientFilter(quotient=8, hash_function=lambda key, seed: fnv_1a_32(key, 0) ^ 0xFFFF)
    custom.add_many(["alpha", "beta"])
    assert custom.check_many(["alpha", "beta", "gamma"]).tolist() == [True, True, False]
    assert sorted(custom.get_hashes()) == sorted(fnv_1a_32(w, 0) ^ 0xFFFF for w in ("alpha", "beta"))
