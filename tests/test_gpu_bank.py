"""BloomFilterBank on the GPU: every route into the table (ids / direct atomics, ids / sort + grouped build, offsets / grouped build; the build's
routes 0 auto, 1 LDS image, 2 global atomics; host and device keys; every key layout) leaves the same rows, and the rows are the reference's:
byte for byte what the REAL reference exported per filter (tests/golden/golden_bank.json) and, at sizes the reference is too slow for, what
the numpy model (tests/bank_model.py, checked against that fixture in tests/test_bank_host.py) computes.  The C ABI is driven directly where
the Python layer would refuse the arguments (ids beyond the bank) or cannot express them (chosen hashes, a table in the middle of a tensor)."""

import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import bank_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

G = json.loads((ROOT / "tests" / "golden" / "golden_bank.json").read_text())
SENTINEL = 0x5A5AA5A5


@pytest.fixture(scope="module")
def pa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pyprobables_amd

    return pyprobables_amd


@pytest.fixture(scope="module")
def N(pa):
    from pyprobables_amd import _native

    return _native


def _dev(a):
    a = np.ascontiguousarray(a)  # (unsigned words travel as the signed tensors of the same bits)
    return torch.from_numpy(a.view({np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype))).cuda()


def dec(e):
    return e[1] if e[0] == "s" else bytes.fromhex(e[1])


def code_points(keys):
    """mixed str / bytes keys -> (uint32 blob, uint64 offsets): a str by code point, bytes by value -- what the reference's FNV walks"""
    parts = [np.array(list(map(ord, k)) if isinstance(k, str) else list(bytes(k)), dtype=np.uint32) for k in keys]
    offs = np.zeros(len(keys) + 1, dtype=np.uint64)
    np.cumsum([p.size for p in parts], out=offs[1:])
    blob = np.concatenate(parts) if offs[-1] else np.zeros(1, dtype=np.uint32)
    return blob.astype(np.uint32), offs


def ragged_bytes(keys):
    offs = np.zeros(len(keys) + 1, dtype=np.uint64)
    np.cumsum([len(k) for k in keys], out=offs[1:])
    blob = np.frombuffer(b"".join(keys), dtype=np.uint8).copy()
    return (blob if blob.size else np.zeros(1, dtype=np.uint8)), offs


def rows_of(bank):
    return bank.table_tensor.cpu().numpy().view(np.uint8).reshape(bank.num_filters, bank.row_bytes)


def grouped(ids, F):
    """stable order by filter and the offsets of the groups"""
    ids = np.asarray(ids)
    order = np.argsort(ids, kind="stable")
    offs = np.zeros(F + 1, dtype=np.int64)
    np.cumsum(np.bincount(ids, minlength=F), out=offs[1:])
    return order, offs


# every way into the table for DEVICE keys: (policy, ids or offsets, the build's route)
DEVICE_WAYS = [("direct", "ids", 0), ("direct", "offsets", 0)] + [("grouped", how, r) for how in ("ids", "offsets") for r in (0, 1, 2)]


def fill(bank, give, ids, policy, how, route, alt=False, split=None, dev_offs=False):
    """send keys (give(index array) -> what add_many takes) with filter `ids` into the bank along one way"""
    bank._add_policy, bank._route, bank._split = policy, route, split
    add = bank.add_alt_many if alt else bank.add_many
    if how == "ids":
        add(give(np.arange(len(ids))), ids)
    else:
        order, offs = grouped(ids, bank.num_filters)
        add(give(order), filter_offsets=torch.from_numpy(offs).cuda() if dev_offs else offs)
    bank._add_policy, bank._route, bank._split = "auto", 0, None


# ------------------------------------------------------------------ the golden streams
@pytest.fixture(scope="module")
def golden_cases():
    out = []
    for c in G["cases"]:
        pool = [dec(e) for e in c["pool"]]
        idx = np.array([i for i, _ in c["stream"]])
        ids = np.array([f for _, f in c["stream"]])
        nbytes = (c["number_bits"] + 7) // 8
        want = np.zeros((c["filters"], M.row_bytes(c["number_bits"])), dtype=np.uint8)
        for f, hx in enumerate(c["export_hex"]):
            want[f, :nbytes] = np.frombuffer(bytes.fromhex(hx)[:nbytes], dtype=np.uint8)
        out.append({"c": c, "pool": pool, "idx": idx, "ids": ids, "want": want})
    return out


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_golden_streams_every_route(pa, golden_cases, ci):
    g = golden_cases[ci]
    c, pool, idx, ids, want = g["c"], g["pool"], g["idx"], g["ids"], g["want"]
    F = c["filters"]

    def new():
        b = pa.BloomFilterBank(F, c["est"], c["fpr"])
        assert (b.number_bits, b.number_hashes, b.row_bytes) == (c["number_bits"], c["number_hashes"], want.shape[1])
        return b

    def give_list(sel):
        return [pool[idx[j]] for j in sel]

    def give_dev(sel):
        blob, offs = code_points([pool[idx[j]] for j in sel])
        return (_dev(blob), _dev(offs))

    banks = []
    for how in ("ids", "offsets"):  # host keys always go direct
        b = new()
        fill(b, give_list, ids, "auto", how, 0)
        banks.append(b)
    b = new()  # host keys, device ids
    b.add_many(give_list(np.arange(len(ids))), torch.from_numpy(ids).cuda())
    banks.append(b)
    for policy, how, route in DEVICE_WAYS:
        for ids_where in ("host", "device"):
            b = new()
            the_ids = torch.from_numpy(ids).cuda() if ids_where == "device" and how == "ids" else ids
            fill(b, give_dev, the_ids, policy, how, route, split=None if route == 0 else 3, dev_offs=ids_where == "device")
            banks.append(b)
    for b in banks:
        assert np.array_equal(rows_of(b), want)
        assert b.elements_added.tolist() == c["elements_added"]
    b = banks[-1]
    for f in range(F):  # the contract: the export of filter f is the reference's, footer and all
        assert bytes(b.filter(f)) == bytes.fromhex(c["export_hex"][f])
    # lookups: the reference's answers, false positives included, host and device
    pi, pf = np.array([i for i, _ in c["probes"]]), np.array([f for _, f in c["probes"]])
    got = b.check_many([pool[i] for i in pi], pf)
    assert isinstance(got, np.ndarray) and got.dtype == np.bool_ and got.astype(int).tolist() == c["answers"]
    blob, offs = code_points([pool[i] for i in pi])
    got = b.check_many((_dev(blob), _dev(offs)), torch.from_numpy(pf).cuda())
    assert got.is_cuda and got.dtype == torch.bool and got.cpu().numpy().astype(int).tolist() == c["answers"]
    absent = [dec(e) for e in c["absent"]]
    ai, af = np.array([i for i, _ in c["absent_probes"]]), np.array([f for _, f in c["absent_probes"]])
    got = b.check_many([absent[i] for i in ai], af).astype(int).tolist()
    assert got == c["absent_answers"]
    sent = set(map(tuple, c["stream"]))
    assert sum(got) + sum(a for a, (i, f) in zip(c["answers"], c["probes"]) if (i, f) not in sent) == c["false_positives"]
    # the same key under two ids answers per row: pool key 0 went to filters 0 and 1 only
    assert b.check_many([pool[0]] * 3, [0, 1, 3]).tolist() == [True, True, False]


def test_known_two_key_export(pa):
    bank = pa.BloomFilterBank(2, 10, 0.05)
    bank.add_many(["spam", b"eggs"], [1, 1])
    raw = bytes(bank.filter(1))
    assert raw.hex() == G["known_spam_eggs"] and len(raw) == 28
    assert not rows_of(bank)[0].any() and bank.elements_added.tolist() == [0, 2]


# ------------------------------------------------------------------ every key layout, against the model
def _layout(name, rng, n):
    """-> (host form, device form, (n, k)-hash function of the model, alt)"""
    if name.startswith("fixed"):
        L = int(name[5:])
        keys = rng.integers(0, 256, (n, L), dtype=np.uint8)
        return (lambda s: keys[s]), (lambda s: _dev(keys[s])), (lambda k: M.hashes_fixed(keys, k)), False
    if name == "ragged":
        keys = [bytes(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8)) for _ in range(n)]
        keys[5] = b""

        def dev(s):
            blob, offs = ragged_bytes([keys[j] for j in s])
            return (_dev(blob), _dev(offs))
        return (lambda s: [keys[j] for j in s]), dev, (lambda k: M.hashes_list(keys, k)), False
    if name == "codepoints":
        keys = ["".join(chr(int(x)) for x in rng.choice([65, 233, 955, 8364, 128512], int(rng.integers(0, 12)))) + str(i) for i in range(n)]

        def dev(s):
            blob, offs = code_points([keys[j] for j in s])
            return (_dev(blob), _dev(offs))
        return (lambda s: [keys[j] for j in s]), dev, (lambda k: M.hashes_list(keys, k)), False
    h = rng.integers(0, 2**63, (n, 12), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 12), dtype=np.uint64)
    return (lambda s: h[s]), (lambda s: _dev(h[s])), (lambda k: h[:, :k]), True


@pytest.mark.parametrize("layout", ["fixed16", "fixed8", "fixed32", "fixed13", "fixed20", "ragged", "codepoints", "hashes"])
def test_every_layout_every_route(pa, layout):
    rng = np.random.default_rng(11)
    F, n = 37, 3000
    host, dev, hashes, alt = _layout(layout, rng, n)
    ids = rng.integers(0, F, n)
    ids[ids == 9] = 10  # an empty filter
    new = lambda: pa.BloomFilterBank(F, 100, 0.01)  # noqa: E731
    b0 = new()
    m, k = b0.number_bits, b0.number_hashes
    assert (m, k, b0.row_bytes) == (959, 7, 128)
    want = M.bank_rows(F, m, k, hashes(k), ids)
    banks = []
    for how in ("ids", "offsets"):
        b = new()
        fill(b, host, ids, "auto", how, 0, alt)
        banks.append(b)
    for policy, how, route in DEVICE_WAYS:
        b = new()
        fill(b, dev, torch.from_numpy(ids).cuda() if how == "ids" else ids, policy, how, route, alt, split=2 if route == 1 else None, dev_offs=route == 2)
        banks.append(b)
    for b in banks:
        assert np.array_equal(rows_of(b), want)
        assert b.elements_added.tolist() == np.bincount(ids, minlength=F).tolist()
    # lookups along both sides; every key under its own id and under its neighbour's
    b = banks[-1]
    check = b.check_alt_many if alt else b.check_many
    for shift in (0, 1):
        pid = (ids + shift) % F
        model = M.bank_check(want, m, k, hashes(k), pid)
        assert np.array_equal(check(host(np.arange(n)), pid), model)
        assert np.array_equal(check(dev(np.arange(n)), torch.from_numpy(pid).cuda()).cpu().numpy(), model)
    assert model.sum() < n  # (some answers are False)


def test_one_filter_is_a_bloomfilter(pa, oracle):
    keys = oracle.gen_keys16(0, 5000)
    bank = pa.BloomFilterBank(1, 4000, 0.01)
    blm = pa.BloomFilter(4000, 0.01)
    bank._add_policy = "grouped"
    bank.add_many(torch.from_numpy(keys).cuda(), filter_offsets=[0, 5000])
    blm.add_many(torch.from_numpy(keys).cuda())
    assert bytes(bank.filter(0)) == bytes(blm)
    ob = oracle.OracleBloom(blm.number_bits, blm.number_hashes)
    ob.add_keys(keys)
    assert np.array_equal(rows_of(bank)[0, : ob.bloom.size], ob.bloom)
    assert bank.split_for() > 1  # (a bank of fewer filters than twice the CUs splits each filter's segment)


def test_chunked_calls(pa):
    rng = np.random.default_rng(2)
    F, n = 11, 2500
    keys = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    rag = [bytes(r[: 1 + i % 16]) for i, r in enumerate(keys)]
    ids = rng.integers(0, F, n)
    for give, hashes in ((lambda: keys, M.hashes_fixed(keys, 7)), (lambda: _dev(keys), M.hashes_fixed(keys, 7)), (lambda: rag, M.hashes_list(rag, 7)),
                         (lambda: tuple(map(_dev, ragged_bytes(rag))), M.hashes_list(rag, 7))):
        bank = pa.BloomFilterBank(F, 100, 0.01)
        bank._CHUNK = 1000  # three engine calls per batch
        bank.add_many(give(), ids)
        want = M.bank_rows(F, 959, 7, hashes, ids)
        assert np.array_equal(rows_of(bank), want)
        got = bank.check_many(give(), (ids + 1) % F)
        got = got.cpu().numpy() if hasattr(got, "is_cuda") else got
        assert np.array_equal(got, M.bank_check(want, 959, 7, hashes, (ids + 1) % F))


# ------------------------------------------------------------------ through the C ABI
def c_add(N, tab, F, m, k, layout, data, n, key_len, ids, offsets=None):
    N.check(N.lib().psk_bank_add(tab, F, m, k, layout, data.data_ptr(), offsets.data_ptr() if offsets is not None else None, n, key_len, N.DEVICE,
                                 ids.data_ptr(), torch.cuda.current_device(), None))


def c_check(N, tab, F, m, k, layout, data, n, key_len, ids):
    out = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    N.check(N.lib().psk_bank_check(tab, F, m, k, layout, data.data_ptr(), None, n, key_len, N.DEVICE, ids.data_ptr(), out.data_ptr(),
                                   torch.cuda.current_device(), None))
    return out.cpu().numpy()


def c_build(N, tab, F, m, k, layout, data, n, key_len, seg, perm, split, route, offsets=None):
    return N.lib().psk_bank_build(tab, F, m, k, layout, data.data_ptr(), offsets.data_ptr() if offsets is not None else None, n, key_len, seg.data_ptr(),
                                  perm.data_ptr() if perm is not None else None, split, route, torch.cuda.current_device(), None)


def test_row_isolation_at_the_16_byte_row(pa, N):
    """m = 63, k = 4, 64 filters in the MIDDLE of a larger tensor: the words in front and behind stay, pad bit 63 of every row stays clear,
    ids F and F + 1 are skipped by the updates and answer 0"""
    rng = np.random.default_rng(4)
    F, m, k, n, guard = 64, 63, 4, 4000, 8
    assert N.lib().psk_bank_row_bytes(m) == 16
    keys = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    ids = rng.integers(0, F + 2, n)
    ids[:4] = [F, F + 1, 0, F - 1]
    h = M.hashes_fixed(keys, k)
    want = M.bank_rows(F, m, k, h, ids)  # (the model skips ids >= F)
    dkeys, dids = _dev(keys), _dev(ids.astype(np.uint32))
    inside = ids < F
    order = np.argsort(np.where(inside, ids, F), kind="stable")  # the keys of the bank's filters first, grouped; the skipped ones behind seg[F]
    seg = np.zeros(F + 1, dtype=np.uint64)
    np.cumsum(np.bincount(ids[inside], minlength=F), out=seg[1:])
    assert seg[F] < n
    calls = [lambda tab: c_add(N, tab, F, m, k, N.KEYS_FIXED, dkeys, n, 16, dids)]
    for route in (0, 1, 2):
        for split in (1, 3):
            calls.append(lambda tab, route=route, split=split: N.check(
                c_build(N, tab, F, m, k, N.KEYS_FIXED, dkeys, n, 16, _dev(seg), _dev(order.astype(np.uint32)), split, route)))
    for call in calls:
        big = torch.full((guard + F * 4 + guard,), SENTINEL, dtype=torch.int32, device="cuda")
        big[guard:guard + F * 4] = 0
        tab = big.data_ptr() + 4 * guard
        call(tab)
        torch.cuda.synchronize()
        got = big.cpu().numpy().view(np.uint32)
        assert (got[:guard] == SENTINEL).all() and (got[-guard:] == SENTINEL).all()
        rows = got[guard:-guard].reshape(F, 4)
        assert not (rows[:, 1] >> 31).any() and not rows[:, 2:].any()  # bit 63 and the pad words
        assert np.array_equal(rows.view(np.uint8).reshape(F, 16), want)
        ans = c_check(N, tab, F, m, k, N.KEYS_FIXED, dkeys, n, 16, dids)
        assert np.array_equal(ans.astype(bool), M.bank_check(want, m, k, h, ids))
        assert not ans[~inside].any() and ans[inside].all()
        # a key that IS in row 0 answers 0 under ids F and F + 1
        j = int(np.flatnonzero(ids == 0)[0])
        three = _dev(np.repeat(keys[j:j + 1], 3, axis=0))
        assert c_check(N, tab, F, m, k, N.KEYS_FIXED, three, 3, 16, _dev(np.array([0, F, F + 1], dtype=np.uint32))).tolist() == [1, 0, 0]


def test_workgroup_seams(pa):
    """segments of 0 .. 1000 keys, parts that do not divide, a second call into the same rows; ragged keys through perm"""
    rng = np.random.default_rng(6)
    sizes = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
    F = len(sizes)
    ids = np.repeat(np.arange(F), sizes)
    rng.shuffle(ids)
    n = ids.size
    keys = [bytes(rng.integers(0, 256, int(rng.integers(1, 30)), dtype=np.uint8)) for _ in range(n)]
    more = [bytes(rng.integers(0, 256, int(rng.integers(1, 30)), dtype=np.uint8)) for _ in range(n)]
    dk, dm = tuple(map(_dev, ragged_bytes(keys))), tuple(map(_dev, ragged_bytes(more)))
    new = lambda: pa.BloomFilterBank(F, 1000, 0.001)  # noqa: E731
    b0 = new()
    m, k = b0.number_bits, b0.number_hashes
    assert (m, k, b0.row_bytes) == (14378, 10, 1808)
    first = M.bank_rows(F, m, k, M.hashes_list(keys, k), ids)
    both = M.bank_rows(F, m, k, M.hashes_list(more, k), ids, rows=first)
    assert not first[0].any() and (both != first).any()
    for split in (1, 2, 3, 7):
        for route in (0, 1, 2):
            b = new()
            b._add_policy, b._route, b._split = "grouped", route, split
            b.add_many(dk, torch.from_numpy(ids).cuda())
            assert np.array_equal(rows_of(b), first), (split, route)
            b.add_many(dm, torch.from_numpy(ids).cuda())
            assert np.array_equal(rows_of(b), both), (split, route)
            assert b.elements_added.tolist() == [2 * s for s in sizes]


def test_auto_route_threshold(pa, N):
    """route 0 sends a part with keys * k * R below the row's words straight to the row: just below and just above give the same table"""
    from pyprobables_amd.bank import BANK_ROUTE_R

    rng = np.random.default_rng(8)
    m, k = 14378, 10
    words = M.row_bytes(m) // 4
    at = -(-words // (k * BANK_ROUTE_R))  # the first part size that takes the image
    assert (at - 1) * k * BANK_ROUTE_R < words <= at * k * BANK_ROUTE_R and at > 2
    sizes = [at - 1, at, at + 1, 1]
    F = len(sizes)
    n = sum(sizes)
    keys = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    ids = np.repeat(np.arange(F), sizes)
    want = M.bank_rows(F, m, k, M.hashes_fixed(keys, k), ids)
    seg = np.zeros(F + 1, dtype=np.uint64)
    np.cumsum(sizes, out=seg[1:])
    for route in (0, 1, 2):
        tab = torch.zeros(F * words, dtype=torch.int32, device="cuda")
        N.check(c_build(N, tab.data_ptr(), F, m, k, N.KEYS_FIXED, _dev(keys), n, 16, _dev(seg), None, 1, route))
        assert np.array_equal(tab.cpu().numpy().view(np.uint8).reshape(F, -1), want), route


@pytest.mark.parametrize("m", [524288, 524287, 524303])
@pytest.mark.parametrize("k", [1, 64])
def test_lds_cap_with_chosen_hashes(pa, N, m, k):
    """rows of 65536 bytes (a power of two and a Barrett modulus) fill the image exactly; 65552 bytes are over the cap: route 0 goes through
    atomics, route 1 is refused.  Chosen hashes set bits 0, 31, 32, m - 1 and the last word's bits in the first and the last row."""
    rng = np.random.default_rng(m + k)
    F = 3
    rb = M.row_bytes(m)
    assert rb == (65552 if m == 524303 else 65536)
    last_word = ((m - 1) >> 5) * 32
    bits = np.array([0, 31, 32, m - 1] + list(range(last_word, m)) + [int(x) for x in rng.integers(0, m, 200)], dtype=np.uint64)
    q = rng.integers(0, (2**64 - m) // m, bits.size, dtype=np.uint64)
    h = bits + q * np.uint64(m)
    assert np.array_equal(h % np.uint64(m), bits)
    h = np.concatenate([h, rng.choice(h, (-h.size) % k)]).reshape(-1, k)
    hh = np.concatenate([h, h])  # every key into the first and into the last row, grouped
    ids = np.repeat([0, F - 1], h.shape[0])
    n = hh.shape[0]
    want = M.bank_rows(F, m, k, hh, ids)
    assert not want[1].any() and np.array_equal(want[0], want[F - 1]) and want[0, 0] & 1 and want[0, (m - 1) >> 3] >> ((m - 1) & 7) & 1
    seg = np.array([0, n // 2, n // 2, n], dtype=np.uint64)
    dh = _dev(hh)

    def table():
        return torch.zeros(F * rb // 4, dtype=torch.int32, device="cuda")

    def rows(t):
        return t.cpu().numpy().view(np.uint8).reshape(F, rb)

    t = table()
    c_add(N, t.data_ptr(), F, m, k, N.KEYS_HASHES, dh, n, k, _dev(ids.astype(np.uint32)))
    assert np.array_equal(rows(t), want)
    assert c_check(N, t.data_ptr(), F, m, k, N.KEYS_HASHES, dh, n, k, _dev(ids.astype(np.uint32))).all()
    assert not c_check(N, t.data_ptr(), F, m, k, N.KEYS_HASHES, dh, n, k, _dev(np.full(n, 1, dtype=np.uint32))).any()
    for route in (0, 1, 2):
        for split in (1, 2):
            t = table()
            rc = c_build(N, t.data_ptr(), F, m, k, N.KEYS_HASHES, dh, n, k, _dev(seg), None, split, route)
            if route == 1 and rb > 65536:
                assert rc == N.PSK_EINVAL and "LDS" in N.last_error()
                assert not t.any().item()
                continue
            assert rc == N.PSK_OK, N.last_error()
            assert np.array_equal(rows(t), want), (route, split)


def test_grid_cap_more_filters_than_workgroups(pa):
    rng = np.random.default_rng(9)
    F, n = 200_000, 400_000
    keys = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    ids = rng.integers(0, F, n)
    dkeys, dids = _dev(keys), torch.from_numpy(ids).cuda()
    new = lambda: pa.BloomFilterBank(F, 10, 0.05)  # noqa: E731
    banks = [new(), new(), new()]
    assert (banks[0].number_bits, banks[0].number_hashes, banks[0].row_bytes) == (63, 4, 16)
    want = M.bank_rows(F, 63, 4, M.hashes_fixed(keys, 4), ids)
    banks[0].add_many(dkeys, dids)
    banks[1]._add_policy = "grouped"
    banks[1].add_many(dkeys, dids)
    banks[2]._add_policy, banks[2]._route = "grouped", 1
    banks[2].add_many(dkeys, dids)
    for b in banks:
        assert np.array_equal(rows_of(b), want)
    assert np.array_equal(banks[0].elements_added, np.bincount(ids, minlength=F))


def test_row_addressing_beyond_4_gib(pa, N):
    """65 537 rows of 65 536 bytes: the last row starts at byte 2^32"""
    F, m, k, rb = 65537, 524288, 7, 65536
    free, _ = torch.cuda.mem_get_info()
    assert free > 6 * 2**30, "the device has no room for the 4 GiB bank"
    tab = torch.zeros(F * rb // 4, dtype=torch.int32, device="cuda")
    view = tab.view(F, rb // 4)
    rng = np.random.default_rng(10)
    targets = [0, 65535, 65536]
    n = 3000
    keys = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    ids = np.array(targets)[np.arange(n) % 3]
    order = np.argsort(ids, kind="stable")
    for mm, use_build in ((524288, False), (524287, True), (524288, True)):
        want = M.bank_rows(3, mm, k, M.hashes_fixed(keys, k), np.arange(n) % 3)
        if not use_build:
            c_add(N, tab.data_ptr(), F, mm, k, N.KEYS_FIXED, _dev(keys), n, 16, _dev(ids.astype(np.uint32)))
        else:
            cnt = np.bincount(ids, minlength=F)
            seg = np.zeros(F + 1, dtype=np.uint64)
            np.cumsum(cnt, out=seg[1:])
            N.check(c_build(N, tab.data_ptr(), F, mm, k, N.KEYS_FIXED, _dev(keys), n, 16, _dev(seg), _dev(order.astype(np.uint32)), 2, 1))
        for j, f in enumerate(targets):
            assert np.array_equal(view[f].cpu().numpy().view(np.uint8), want[j]), (mm, use_build, f)
        for f in (1, 2, 32768, 65534):
            assert not view[f].any().item()
        ans = c_check(N, tab.data_ptr(), F, mm, k, N.KEYS_FIXED, _dev(keys), n, 16, _dev(ids.astype(np.uint32)))
        assert ans.all()
        for f in targets:
            view[f].zero_()
    del view, tab
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ the class
def test_automatic_route(pa, monkeypatch):
    """host keys go direct; device keys with offsets go grouped; device keys with ids go grouped from BANK_GROUP_MIN_KEYS keys on where a
    filter's mean share of the batch is a segment that takes the LDS image -- and every choice leaves the same rows"""
    from pyprobables_amd import bank as B

    assert B.BANK_GROUP_MIN_KEYS == 1 << 21 and B.BANK_ROUTE_R == 16  # profiles/bank_bench.txt
    rng = np.random.default_rng(12)
    n = 3000
    keys = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    dkeys = _dev(keys)
    for F, est, fpr, want_path in ((4, 100, 0.01, "grouped"), (2000, 1000, 0.001, "direct")):  # 750 keys per filter / 1.5 keys per 452-word row
        ids = rng.integers(0, F, n)
        dids = torch.from_numpy(ids).cuda()
        bank = pa.BloomFilterBank(F, est, fpr)
        bank.add_many(dkeys, dids)
        assert bank._last_path == "direct"  # below BANK_GROUP_MIN_KEYS
        want = rows_of(bank)
        assert np.array_equal(want, M.bank_rows(F, bank.number_bits, bank.number_hashes, M.hashes_fixed(keys, bank.number_hashes), ids))
        monkeypatch.setattr(B, "BANK_GROUP_MIN_KEYS", 1024)
        bank = pa.BloomFilterBank(F, est, fpr)
        bank.add_many(dkeys, dids)
        assert bank._last_path == want_path and np.array_equal(rows_of(bank), want)
        bank.add_many(keys, ids)
        assert bank._last_path == "direct" and np.array_equal(rows_of(bank), want)
        order, offs = grouped(ids, F)
        bank.add_many(_dev(keys[order]), filter_offsets=offs)
        assert bank._last_path == "grouped" and np.array_equal(rows_of(bank), want)
        monkeypatch.setattr(B, "BANK_GROUP_MIN_KEYS", None)  # "never"
        bank.add_many(dkeys, dids)
        assert bank._last_path == "direct"
        monkeypatch.undo()


def test_empty_batches_launch_nothing(pa):
    bank = pa.BloomFilterBank(4, 100, 0.01)
    bank.add_many([], [])
    bank.add_many(torch.zeros((0, 16), dtype=torch.uint8, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda"))
    bank.add_many(torch.zeros((0, 16), dtype=torch.uint8, device="cuda"), filter_offsets=[0, 0, 0, 0, 0])
    got = bank.check_many([], [])
    assert isinstance(got, np.ndarray) and got.dtype == np.bool_ and got.size == 0
    got = bank.check_many(torch.zeros((0, 16), dtype=torch.uint8, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda"))
    assert got.is_cuda and got.numel() == 0
    assert not rows_of(bank).any() and bank.elements_added.tolist() == [0, 0, 0, 0]


def test_validation(pa):
    bank = pa.BloomFilterBank(4, 100, 0.01)
    keys = np.zeros((3, 16), dtype=np.uint8)
    dkeys = _dev(keys)
    for k_, bad in ((keys, [0, 1, 4]), (keys, [-1, 0, 0]), (dkeys, torch.tensor([0, 4, 1]).cuda()), (dkeys, torch.tensor([0, -1, 1]).cuda()), (dkeys, [0, 9, 1])):
        with pytest.raises(ValueError):
            bank.add_many(k_, bad)
        with pytest.raises(ValueError):
            bank.check_many(k_, bad)
    for offs in ([0, 1, 2, 3], [0, 2, 1, 3, 3], [1, 1, 2, 3, 3], [0, 1, 2, 3, 4]):
        with pytest.raises((ValueError, TypeError)):
            bank.add_many(dkeys, filter_offsets=offs)
        with pytest.raises((ValueError, TypeError)):
            bank.add_many(keys, filter_offsets=offs)
    with pytest.raises(ValueError):
        bank.add_many(dkeys, filter_offsets=torch.tensor([0, 2, 1, 3, 3]).cuda())
    with pytest.raises(ValueError):
        bank.add_many(keys, [0, 1])
    with pytest.raises(TypeError):
        bank.add_many(keys)
    with pytest.raises(TypeError):
        bank.add_many(keys, [0, 1, 2], filter_offsets=[0, 1, 2, 3, 3])
    with pytest.raises(TypeError):
        bank.add_many(keys, [0.0, 1.0, 2.0])
    assert not rows_of(bank).any() and bank.elements_added.tolist() == [0, 0, 0, 0]  # nothing was launched
    # validate=False: an id beyond the bank is skipped by the engine and by the counts
    bank.add_many(dkeys, torch.tensor([0, 4, 1]).cuda(), validate=False)
    assert bank.elements_added.tolist() == [1, 1, 0, 0] and rows_of(bank)[0].any() and rows_of(bank)[1].any() and not rows_of(bank)[2:].any()
    assert bank.check_many(dkeys, torch.tensor([0, 4, 1]).cuda(), validate=False).tolist() == [True, False, True]
    with pytest.raises(ValueError):
        pa.BloomFilterBank(0, 100, 0.01)
    with pytest.raises(pa.InitializationError):
        pa.BloomFilterBank(4, 0, 0.01)


def test_filter_and_set_filter_round_trip(pa):
    bank = pa.BloomFilterBank(6, 100, 0.01)
    words = [f"word-{i}" for i in range(120)]
    ids = [i % 5 for i in range(120)]
    bank.add_many(words + words[:10], ids + ids[:10])  # repeats are counted (bloom.py:239)
    assert bank.elements_added.tolist() == [26, 26, 26, 26, 26, 0]
    singles = []
    for f in range(6):
        blm = pa.BloomFilter(100, 0.01)
        mine = [w for w, i in zip(words + words[:10], ids + ids[:10]) if i == f]
        if mine:
            blm.add_many(mine)
        singles.append(blm)
        got = bank.filter(f)
        assert bytes(got) == bytes(blm) and got.elements_added == len(mine)
        assert got.export_hex() == blm.export_hex() and got.estimate_elements() == blm.estimate_elements()
    # a copy: changing it leaves the bank alone
    got = bank.filter(0)
    got.add_many(["something else"])
    assert bytes(bank.filter(0)) == bytes(singles[0])
    assert bytes(bank.filter(0).union(bank.filter(1))) == bytes(singles[0].union(singles[1]))
    # copy in: filter 5 becomes filter 2's union with filter 3
    u = singles[2].union(singles[3])
    bank.set_filter(5, u)
    assert bytes(bank.filter(5)) == bytes(u) and bank.elements_added[5] == u.elements_added
    assert bank.check_many(["word-2", "word-3", "word-4"], [5, 5, 5]).tolist()[:2] == [True, True]
    other = pa.BloomFilterBank(6, 100, 0.01)
    for f in range(6):
        other.set_filter(f, bank.filter(f))
    assert np.array_equal(rows_of(other), rows_of(bank)) and other.elements_added.tolist() == bank.elements_added.tolist()
    bank.clear(5)
    assert not rows_of(bank)[5].any() and bank.elements_added.tolist() == [26, 26, 26, 26, 26, 0] and rows_of(bank)[4].any()
    with pytest.raises(pa.SimilarityError):
        bank.set_filter(0, pa.BloomFilter(101, 0.01))
    with pytest.raises(pa.SimilarityError):
        bank.set_filter(0, pa.BloomFilter(100, 0.01, hash_function=pa.default_md5))
    with pytest.raises(TypeError):
        bank.set_filter(0, pa.CountingBloomFilter(100, 0.01))
    with pytest.raises(IndexError):
        bank.filter(6)
    bank.clear()
    assert not rows_of(bank).any() and not bank.elements_added.any()


def test_other_hash_functions_travel_as_hashes(pa):
    def mine(key, depth):
        return [(hash_seed * 0x9E3779B97F4A7C15 + sum(key.encode()) * 1000003) % 2**64 for hash_seed in range(1, depth + 1)]

    words = [f"w{i}" for i in range(200)]
    ids = [i % 3 for i in range(200)]
    for fn in (mine, pa.default_md5):
        bank = pa.BloomFilterBank(3, 100, 0.01, hash_function=fn)
        bank.add_many(words, ids)
        for f in range(3):
            blm = pa.BloomFilter(100, 0.01, hash_function=fn)
            blm.add_many([w for w, i in zip(words, ids) if i == f])
            assert bytes(bank.filter(f)) == bytes(blm)
        assert bank.check_many(words, ids).all()
