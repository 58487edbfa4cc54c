"""The ordered Bloom batch (csrc/psk_bloom_ordered.hip, ``BloomFilter.add_many_ordered``): the loop ``seen = key in blm; blm.add(key)`` as a
batch.  Every comparison is exact and against the model (tests/bloom_ordered_model.py: the plain loop in Python integers) or against the
real reference's recorded loop (tests/golden/golden_bloom_ordered.json): the ``seen`` flags, the number of new keys, ``elements_added`` and
the table byte for byte."""

import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import bloom_ordered_model as M  # noqa: E402
import edge_hashes as E  # noqa: E402

GOLDEN = json.loads((ROOT / "tests" / "golden" / "golden_bloom_ordered.json").read_text())
FOOTER = 20  # bytes of the QQf footer


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def N(torch):
    from pyprobables_amd import _native

    _native.lib()
    return _native


@pytest.fixture(scope="module")
def pa(torch):
    import pyprobables_amd

    return pyprobables_amd


# ---------------------------------------------------------------- the C ABI on a handle of the test's own
class Handle:
    def __init__(self, N, m, k):
        self.N, self.m, self.k = N, int(m), int(k)
        self.h = C.c_void_p()
        N.check(N.lib().psk_bloom_create(self.m, self.k, 0, None, C.byref(self.h)))

    def close(self):
        if self.h:
            self.N.check(self.N.lib().psk_destroy(self.h))
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def add(self, hashes):
        a = np.ascontiguousarray(hashes, dtype=np.uint64)
        if a.shape[0]:
            self.N.check(self.N.lib().psk_bloom_add(self.h, self.N.KEYS_HASHES, a.ctypes.data, None, a.shape[0], a.shape[1], self.N.HOST, None))

    def running(self, hashes, chunk=0, device=False, torch=None, want_new=True):
        """-> (seen uint8[n], number of new keys or None)"""
        N, L = self.N, self.N.lib()
        a = np.ascontiguousarray(hashes, dtype=np.uint64)
        n, w = a.shape
        if device:
            t = torch.from_numpy(a.view(np.int64)).cuda()
            seen = torch.full((max(n, 1),), 9, dtype=torch.uint8, device="cuda")
            new = torch.full((1,), 77, dtype=torch.int64, device="cuda")
            N.check(L.psk_bloom_add_running(self.h, N.KEYS_HASHES, t.data_ptr() if n else None, None, n, w, N.DEVICE, chunk, seen.data_ptr(),
                                            new.data_ptr() if want_new else None, None))
            torch.cuda.synchronize()
            return seen[:n].cpu().numpy(), (int(new.item()) if want_new else None)
        seen = np.full(max(n, 1), 9, dtype=np.uint8)
        new = C.c_uint64(77)
        N.check(L.psk_bloom_add_running(self.h, N.KEYS_HASHES, a.ctypes.data if n else None, None, n, w, N.HOST, chunk, seen.ctypes.data,
                                        C.addressof(new) if want_new else None, None))
        return seen[:n], (int(new.value) if want_new else None)

    def table(self) -> bytes:
        out = np.empty((self.m + 7) // 8, dtype=np.uint8)
        self.N.check(self.N.lib().psk_read_table(self.h, out.ctypes.data, out.size, None))
        return out.tobytes()

    def scratch(self):
        b = (C.c_uint64 * 3)()
        self.N.check(self.N.lib().psk_scratch_bytes(self.h, b))
        return int(b[0])


def check_against_loop(hd, start: set, idx, got_seen, got_new):
    """the engine's answers for the stream of position rows ``idx`` from table ``start`` against the model's plain loop; -> table after"""
    seen, table = M.loop(start, idx)
    assert got_seen.tolist() == seen
    if got_new is not None:
        assert got_new == seen.count(0)
    assert hd.table() == M.table_bytes(table, hd.m)
    return table


# ---------------------------------------------------------------- 1. exhaustive, in one call
@pytest.fixture(scope="module")
def exhaustive():
    """all 65 536 cases, case c on bits [4c, 4c + 4): start positions, the 196 608 keys' positions case-major, the model's flags and table"""
    start, rows, seen = [], [], []
    table = set()
    for c, (s, keys) in enumerate(M.exhaustive_cases()):
        base = 4 * c
        start += [base + b for b in s]
        rows += [(base + a, base + b) for a, b in keys]
        sn, t = M.loop(s, keys)
        seen += sn
        table.update(base + b for b in t)
    m = 262144
    assert len(rows) == 196608 and max(max(r) for r in rows) < m
    return {"m": m, "start": np.array(start, dtype=np.int64), "idx": np.array(rows, dtype=np.int64), "seen": np.array(seen, dtype=np.uint8),
            "table": M.table_bytes(table, m)}


@pytest.mark.parametrize("order", ["case_major", "key_major"])
@pytest.mark.parametrize("chunk", [0, 1000])
def test_exhaustive_4bit_space_in_one_call(torch, N, exhaustive, order, chunk):
    x = exhaustive
    m = x["m"]
    # key-major: the first keys of all cases, then the second keys, then the third -- the cases are independent, so each keeps its own order
    perm = np.arange(196608) if order == "case_major" else np.arange(196608).reshape(65536, 3).T.reshape(-1)
    h = E.lift(x["idx"][perm], m, seed=3)
    with Handle(N, m, 2) as hd:
        hd.add(E.lift(np.stack([x["start"], x["start"]], axis=1), m, seed=4))
        seen, new = hd.running(h, chunk=chunk, device=True, torch=torch)
        want = x["seen"][perm]
        assert np.array_equal(seen, want)
        assert new == int((want == 0).sum())
        assert hd.table() == x["table"]


# ---------------------------------------------------------------- 2. k = 1 and k = 64
@pytest.mark.parametrize("k,m", [(1, 97), (64, 1 << 12), (64, 4099)])
def test_k_1_and_k_64(torch, N, k, m):
    rng = np.random.default_rng(k + m)
    pool = rng.integers(0, m, size=(40, k))
    idx = pool[rng.integers(0, 40, size=300)]
    for device in (False, True):
        with Handle(N, m, k) as hd:
            seen, new = hd.running(E.lift(idx, m, seed=1), device=device, torch=torch)
            check_against_loop(hd, set(), idx.tolist(), seen, new)


# ---------------------------------------------------------------- 3. positions past 2^32
def test_positions_past_2_pow_32(torch, N):
    m, k = (1 << 32) + 4096, 2
    P = 1 << 32
    empty_marker = P - 1  # the 32-bit map's "empty": an ordinary bit here
    rows = [
        (5, 6), (5 + P, 6 + P),              # p and p + 2^32 in one chunk: strangers
        (5, 6), (5 + P, 6 + P),              # ... and both seen the second time
        (empty_marker, empty_marker), (empty_marker, 7), (empty_marker, empty_marker),
        (P, P + 4095), (0, 4095), (P, 0), (m - 1, m - 1), (m - 1, P - 2), (P - 2, P - 2),
        (100, 100 + P), (100 + P, 100 + P), (100, 100),
    ]
    idx = np.array(rows, dtype=np.int64)
    hashes = np.stack([E.any_how(idx[:, 0], m, seed=1), E.any_how(idx[:, 1], m, seed=2)], axis=1)
    assert np.array_equal(E.indices(hashes, m, k), idx)
    seen_want, table = M.loop(set(), rows)
    assert seen_want[:4] == [0, 0, 1, 1] and seen_want[4:7] == [0, 0, 1]
    for device in (False, True):
        with Handle(N, m, k) as hd:
            seen, new = hd.running(hashes, device=device, torch=torch)
            assert seen.tolist() == seen_want and new == seen_want.count(0)
            got = np.frombuffer(hd.table(), dtype=np.uint8)
            want = np.zeros((m + 7) // 8, dtype=np.uint8)
            E.bloom_table(m, np.array(sorted(table), dtype=np.int64), want)
            assert np.array_equal(got, want)


# ---------------------------------------------------------------- 4. seams
def test_repeats_across_chunk_seams(torch, N):
    chunk, m, k = 64, 1 << 16, 3
    n = 5 * chunk
    rng = np.random.default_rng(5)
    idx = rng.integers(0, m, size=(n, k))
    for d in (chunk - 1, chunk, chunk + 1):  # a key and its repeat at distance d, from several places of every chunk
        for lo in range(0, n - d, 37):
            idx[lo + d] = idx[lo]
    for device in (False, True):
        with Handle(N, m, k) as hd:
            seen, new = hd.running(E.lift(idx, m, seed=6), chunk=chunk, device=device, torch=torch)
            check_against_loop(hd, set(), idx.tolist(), seen, new)
            assert 0 < int(seen.sum()) < n


def test_chunks_that_insert_nothing_and_maps_of_changing_size(torch, N):
    """a chunk whose keys are all present leaves the map empty (no settle work, no fill in front of the next chunk); calls with other
    chunk sizes on the same handle use other parts of the same map: whatever was left behind must never be taken for an entry"""
    m, k = 1 << 15, 3
    rng = np.random.default_rng(13)
    table = set()
    with Handle(N, m, k) as hd:
        for call, (chunk, n) in enumerate([(256, 700), (16, 100), (256, 700), (64, 640), (1, 40), (512, 512), (0, 3000)]):
            fresh = rng.integers(0, m, size=(n, k))
            old = np.array(sorted(table) or [0], dtype=np.int64)[rng.integers(0, max(len(table), 1), size=(n, k))]  # present for sure
            idx = fresh.copy()
            per_chunk = max(chunk, 1) if chunk else n
            for c in range(0, n, per_chunk):  # every other chunk holds nothing but present keys
                if (c // per_chunk) % 2 == 1 and table:
                    idx[c:c + per_chunk] = old[c:c + per_chunk]
            seen, new = hd.running(E.lift(idx, m, seed=call), chunk=chunk, device=bool(call % 2), torch=torch)
            table = check_against_loop(hd, table, idx.tolist(), seen, new)


# ---------------------------------------------------------------- 5. one slot under contention
def test_one_key_100000_times(torch, N):
    m, k, n = 1 << 20, 3, 100_000
    h = np.tile(E.lift(np.array([[123, 456789, 7]]), m, seed=7), (n, 1))
    with Handle(N, m, k) as hd:
        seen, new = hd.running(h, chunk=n, device=True, torch=torch)
        assert seen[0] == 0 and seen[1:].all() and new == 1
        assert hd.table() == M.table_bytes({123, 456789, 7}, m)


# ---------------------------------------------------------------- 6. the smallest map
@pytest.mark.parametrize("chunk,k", [(1, 2), (1, 1), (3, 2)])
def test_smallest_map_walks_wrap(torch, N, chunk, k):
    """chunk_keys = 1: a map of 2 k slots (the power of two above it), every walk starts near its end"""
    m, n = 5003, 2000
    rng = np.random.default_rng(chunk * 10 + k)
    idx = rng.integers(0, m, size=(n, k))
    idx[n // 2:] = idx[rng.integers(0, n // 2, size=n - n // 2)]
    with Handle(N, m, k) as hd:
        seen, new = hd.running(E.lift(idx, m, seed=8), chunk=chunk, device=True, torch=torch)
        check_against_loop(hd, set(), idx.tolist(), seen, new)


# ---------------------------------------------------------------- 7. n = 0, n = 1
def test_n_0_and_n_1(torch, N):
    m, k = 1000, 3
    for device in (False, True):
        with Handle(N, m, k) as hd:
            hd.add(E.lift(np.array([[1, 2, 3]]), m))
            before = hd.table()
            seen, new = hd.running(np.zeros((0, k), dtype=np.uint64), device=device, torch=torch)
            assert seen.size == 0 and new == 0 and hd.table() == before
            for row, want in (([1, 2, 3], 1), ([1, 2, 4], 0), ([1, 2, 4], 1)):
                seen, new = hd.running(E.lift(np.array([row]), m), device=device, torch=torch)
                assert seen.tolist() == [want] and new == 1 - want
            seen, new = hd.running(E.lift(np.array([[9, 9, 9]]), m), device=device, torch=torch, want_new=False)  # new_out may be NULL
            assert seen.tolist() == [0] and new is None
            assert hd.table() == M.table_bytes({1, 2, 3, 4, 9}, m)


# ---------------------------------------------------------------- 8. 2^18 + 3 keys at the default chunk
def test_2_pow_18_plus_3_keys_half_repeats(torch, N):
    m, k, n = 1 << 24, 3, (1 << 18) + 3
    rng = np.random.default_rng(9)
    idx = rng.integers(0, m, size=(n, k))
    rep = rng.permutation(n)[: n // 2]
    idx[rep] = idx[rng.integers(0, n, size=n // 2)]  # half of the keys repeat another one (in front or behind)
    with Handle(N, m, k) as hd:
        base = hd.scratch()
        seen, new = hd.running(E.lift(idx, m, seed=10), device=True, torch=torch)
        grown = hd.scratch()
        assert 16 << 21 <= grown - base <= 64 << 20  # the map of the default chunk: 2^21 slots of 16 bytes, counted as the handle's scratch
        check_against_loop(hd, set(), idx.tolist(), seen, new)
        hd.running(E.lift(idx[:100], m, seed=10), device=True, torch=torch)
        assert hd.scratch() >= grown  # grows only
        N.check(N.lib().psk_release_scratch(hd.h))
        assert hd.scratch() == 0


# ---------------------------------------------------------------- 9. layouts, through the Python class
def _fixed(n, width, seed):
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 256, size=(n // 2, width), dtype=np.uint8)
    return pool[rng.integers(0, n // 2, size=n)]


def _strings(n, seed, as_bytes):
    rng = np.random.default_rng(seed)
    pool = ["k%d-%s" % (i, "y" * int(rng.integers(0, 40))) for i in range(n // 2)]
    keys = [pool[int(i)] for i in rng.integers(0, n // 2, size=n)]
    return [s.encode() for s in keys] if as_bytes else keys


def _plain_keys(keys):
    """the keys of any batch form as a list of bytes / str"""
    if isinstance(keys, tuple):
        blob, offs = keys
        return [bytes(blob[int(offs[i]):int(offs[i + 1])]) for i in range(len(offs) - 1)]
    if isinstance(keys, np.ndarray):
        return [bytes(r) for r in keys]
    return list(keys)


def _to_device(torch, keys):
    if isinstance(keys, tuple):
        return (torch.from_numpy(keys[0]).cuda(), torch.from_numpy(keys[1].view(np.int64)).cuda())
    return torch.from_numpy(keys).cuda()


def _ragged(n, seed):
    rng = np.random.default_rng(seed)
    pool = [bytes(rng.integers(0, 256, size=int(rng.integers(0, 50)), dtype=np.uint8)) for _ in range(n // 2)]
    keys = [pool[int(i)] for i in rng.integers(0, n // 2, size=n)]
    offs = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in keys], out=offs[1:])
    return (np.frombuffer(b"".join(keys), dtype=np.uint8).copy(), offs)


def custom_hash(key, depth):
    """a hash function the engine does not know: evaluated on the host, per key"""
    return [(M.fnv_1a(key, 1000 + 3 * i) ^ 0x5555) % M.U64 for i in range(depth)]


N_KEYS = 320
LAYOUTS = {
    "n_by_8": lambda: _fixed(N_KEYS, 8, 1),
    "n_by_16": lambda: _fixed(N_KEYS, 16, 2),
    "n_by_32": lambda: _fixed(N_KEYS, 32, 3),
    "n_by_13": lambda: _fixed(N_KEYS, 13, 4),
    "ragged": lambda: _ragged(N_KEYS, 5),
    "list_str": lambda: _strings(N_KEYS, 6, False),
    "list_bytes": lambda: _strings(N_KEYS, 7, True),
}
HASHERS = ["fnv", "md5", "sha256", "custom"]
_HASH_CACHE = {}


def _stream_hashes(layout, hasher, k):
    """the model's hashes of a layout's keys, once per (layout, hasher)"""
    key = (layout, hasher)
    if key not in _HASH_CACHE:
        keys = LAYOUTS[layout]()
        plain = _plain_keys(keys)
        if hasher == "fnv":
            hs = [M.hashes_fnv(x, k) for x in plain]
        elif hasher == "custom":
            hs = [custom_hash(x, k) for x in plain]
        else:
            hs = [M.hashes_digest(x, k, hasher) for x in plain]
        _HASH_CACHE[key] = (keys, hs)
    return _HASH_CACHE[key]


def _hash_function(pa, hasher):
    from pyprobables_amd import hashes as H

    return {"fnv": None, "md5": H.default_md5, "sha256": H.default_sha256, "custom": custom_hash}[hasher]


def _run_class_case(torch, pa, shape, layout, hasher):
    blm0 = pa.BloomFilter(*shape, hash_function=_hash_function(pa, hasher))
    m, k = blm0.number_bits, blm0.number_hashes
    assert m == E.bloom_bits(*shape)
    keys, hs = _stream_hashes(layout, hasher, 7)
    assert k == 7
    stream = [M.positions(h, m, k) for h in hs]
    seen, table = M.loop(set(), stream)
    want_bytes = M.table_bytes(table, m)
    assert 0 < sum(seen) < len(seen)
    wheres = ["host"] if isinstance(keys, list) else ["host", "device"]  # (lists of str / bytes are host objects)
    for where in wheres:
        batch = _to_device(torch, keys) if where == "device" else keys
        for count_seen in (True, False):
            blm = blm0 if (where, count_seen) == ("host", True) else pa.BloomFilter(*shape, hash_function=_hash_function(pa, hasher))
            got = blm.add_many_ordered(batch, count_seen=count_seen)
            if where == "device":
                assert got.dtype == torch.bool and got.is_cuda
                got = got.cpu().numpy()
            assert got.dtype == np.bool_ and got.astype(np.uint8).tolist() == seen
            assert blm.elements_added == (len(seen) if count_seen else seen.count(0))
            assert bytes(blm)[:-FOOTER] == want_bytes


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("shape", [E.BLOOM_2P28, E.BLOOM_NP2], ids=["pow2", "np2"])
def test_layouts_host_and_device_both_counts(torch, pa, shape, layout):
    _run_class_case(torch, pa, shape, layout, "fnv")


@pytest.mark.parametrize("hasher", ["md5", "sha256", "custom"])
@pytest.mark.parametrize("shape", [E.BLOOM_2P28, E.BLOOM_NP2], ids=["pow2", "np2"])
def test_digest_and_custom_hash_functions(torch, pa, shape, hasher):
    # (a custom Python hash function is called per key on the host: lists only; the digest kernels also take byte matrices, host or device)
    for layout in (["list_str"] if hasher == "custom" else ["list_str", "n_by_16"]):
        _run_class_case(torch, pa, shape, layout, hasher)


def test_add_alt_many_ordered_host_and_device(torch, pa):
    blm = pa.BloomFilter(1000, 0.01)
    m, k = blm.number_bits, blm.number_hashes
    rng = np.random.default_rng(11)
    idx = rng.integers(0, m, size=(150, k))[rng.integers(0, 150, size=400)]
    h = E.lift(idx, m, seed=12)
    seen, table = M.loop(set(), idx.tolist())
    for dev in (False, True):
        for count_seen in (True, False):
            b = pa.BloomFilter(1000, 0.01)
            got = b.add_alt_many_ordered(torch.from_numpy(h.view(np.int64)).cuda() if dev else h, count_seen=count_seen)
            got = got.cpu().numpy() if dev else got
            assert got.astype(np.uint8).tolist() == seen
            assert b.elements_added == (400 if count_seen else seen.count(0))
            assert bytes(b)[:-FOOTER] == M.table_bytes(table, m)


# ---------------------------------------------------------------- 10. state
def test_state_clear_pending_adds_check_and_twin(torch, pa):
    shape = (5000, 0.01)
    blm, twin = pa.BloomFilter(*shape), pa.BloomFilter(*shape)
    m, k = blm.number_bits, blm.number_hashes
    old = _strings(200, 20, False)
    blm.add_many(old)
    blm.clear()  # (deferred inside the engine: it must reach the table in front of the batch)
    pending = _strings(60, 21, False)
    for key in pending:  # per-key adds wait on the host: flushed first
        blm.add(key)
        twin.add(key)
    keys = _strings(500, 22, False) + pending[:20]
    start = set()
    for key in pending:
        start.update(M.positions(M.hashes_fnv(key, k), m, k))
    stream = [M.positions(M.hashes_fnv(key, k), m, k) for key in keys]
    seen, table = M.loop(start, stream)
    got = blm.add_many_ordered(keys)
    assert got.astype(np.uint8).tolist() == seen and all(seen[-20:])
    assert blm.elements_added == len(pending) + len(keys)
    assert bytes(blm)[:-FOOTER] == M.table_bytes(table, m)
    assert blm.check_many(keys).all()
    twin.add_many(keys)
    assert bytes(twin) == bytes(blm)  # the same table and the same count
    # clear() immediately in front of the call, nothing in between
    blm.clear()
    seen0, table0 = M.loop(set(), stream)
    assert blm.add_many_ordered(keys, count_seen=False).astype(np.uint8).tolist() == seen0
    assert blm.elements_added == seen0.count(0) and bytes(blm)[:-FOOTER] == M.table_bytes(table0, m)


def test_counting_bloom_keeps_its_own_ordered_methods(torch, pa):
    cbf = pa.CountingBloomFilter(100, 0.05)
    out = cbf.add_many_ordered(["a", "b", "a"])
    assert np.asarray(out).tolist() == [1, 1, 2]  # counts, not flags


# ---------------------------------------------------------------- 11. the reference's recorded loop, end to end
@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_fixture_cases_end_to_end(torch, pa, case):
    from pyprobables_amd import hashes as H

    hf = {"fnv": None, "md5": H.default_md5}[case["hash"]]
    keys = case["keys"] if case["type"] == "str" else [bytes.fromhex(x) for x in case["keys"]]
    for count_seen, added in ((True, case["elements_added"]), (False, case["elements_added_conditional"])):
        blm = pa.BloomFilter(hex_string=case["start"], hash_function=hf) if case["start"] else pa.BloomFilter(case["est"], case["fpr"], hash_function=hf)
        assert (blm.number_bits, blm.number_hashes) == (case["number_bits"], case["number_hashes"])
        got = blm.add_many_ordered(keys, count_seen=count_seen)
        assert got.astype(np.uint8).tolist() == case["seen"]
        assert blm.elements_added == added
        assert blm.export_hex()[:-2 * FOOTER] == case["export_hex"][:-2 * FOOTER]
        if count_seen:
            assert blm.export_hex() == case["export_hex"]
