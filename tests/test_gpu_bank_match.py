"""BloomFilterBank.match_many on the GPU: "which filters may hold this key", read from the slice image (the bank transposed: psk_bank_slices)
by the row-AND kernel (psk_bank_match).  The answers are the reference's -- per probe, ``key in blm[f]`` of the REAL reference for all 70
filters of tests/golden/golden_bank_match.json -- and, where the reference has nothing to say (chosen tables, chosen hashes, wide rows, an
image beyond 4 GiB), the numpy model's (tests/bank_match_model.py, checked against that fixture in tests/test_bank_match_model.py).  Every
output buffer of a direct C ABI call has sentinel words behind it."""

import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import bank_match_model as MM  # noqa: E402
import bank_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

G = json.loads((ROOT / "tests" / "golden" / "golden_bank_match.json").read_text())
SENTINEL = 0x5A5AA5A5
GUARD = 8  # sentinel words behind every output


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


def guarded(words):
    """an int32 device buffer of `words` words, every word and GUARD words behind them the sentinel; 16-byte aligned"""
    return torch.full((words + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")


def guard_ok(t, words):
    return bool((t[words:] == SENTINEL).all().item())


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def as_bits(mask, filters):
    """any mask form (tensor or array, words) -> bool[n, filters]"""
    a = mask.cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
    return MM.mask_bits(np.ascontiguousarray(a).view(np.uint32), filters)


def c_slices(N, table, F, m, image, first=0, last=None):
    return N.lib().psk_bank_slices(table.data_ptr(), F, m, image.data_ptr(), first, F if last is None else last, 0, None)


def c_match(N, image, F, m, k, h):
    """psk_bank_match over PSK_KEYS_HASHES on the device, all three outputs, sentinels checked -> (mask bytes [n, srb], counts, offsets, ids)"""
    L = N.lib()
    h = np.ascontiguousarray(h, dtype=np.uint64)
    n, kk = h.shape
    words = MM.slice_row_bytes(F) // 4
    hd = _dev(h) if n else None
    keys = (N.KEYS_HASHES, hd.data_ptr() if n else None, None, n, kk)
    mask, count = guarded(n * words), guarded(n)
    N.check(L.psk_bank_match(image.data_ptr(), F, m, k, *keys, N.DEVICE, mask.data_ptr(), count.data_ptr(), None, None, 0, None))
    torch.cuda.synchronize()
    assert guard_ok(mask, n * words) and guard_ok(count, n)
    cnt = count[:n].cpu().numpy()
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(cnt, out=offs[1:])
    total = int(offs[-1])
    ids = guarded(total)
    od = _dev(offs[:-1].astype(np.uint64)) if n else guarded(0)
    N.check(L.psk_bank_match(image.data_ptr(), F, m, k, *keys, N.DEVICE, None, None, od.data_ptr(), ids.data_ptr(), 0, None))
    torch.cuda.synchronize()
    assert guard_ok(ids, total)
    return u32(mask[:n * words]).reshape(n, words).view(np.uint8), cnt, offs, ids[:total].cpu().numpy()


def agree(got, want_mask):
    """what c_match returned against the model's mask bytes"""
    mask, cnt, offs, ids = got
    assert np.array_equal(mask, want_mask)
    assert np.array_equal(cnt, MM.match_counts(want_mask))
    wo, wi = MM.match_ids(want_mask)
    assert np.array_equal(offs, wo) and np.array_equal(ids, wi)
    for i in range(len(cnt)):  # ascending per key (what match_ids gives, spelled out)
        assert (np.diff(ids[offs[i]:offs[i + 1]]) > 0).all()


# ------------------------------------------------------------------ the reference's answers
@pytest.mark.parametrize("ci", [0, 1])
def test_golden_every_form(pa, ci):
    c = G["cases"][ci]
    F, m, k = c["filters"], c["number_bits"], c["number_hashes"]
    pool = [dec(e) for e in c["pool"]]
    probes = pool + [dec(e) for e in c["absent"]]
    want = np.array([[(int.from_bytes(bytes.fromhex(h), "little") >> f) & 1 for f in range(F)] for h in c["masks"]], dtype=bool)
    bank = pa.BloomFilterBank(F, c["est"], c["fpr"])
    assert (bank.number_bits, bank.number_hashes, bank.slice_row_bytes) == (m, k, 16) and bank.slice_tensor is None
    bank.add_many([pool[i] for f in range(F) for i in c["sent"][f]], np.array([f for f in range(F) for _ in c["sent"][f]]))
    blob, offs = code_points(probes)
    for keys, on_dev in ((probes, False), ((_dev(blob), _dev(offs)), True)):
        mask = bank.match_many(keys)
        cnt = bank.match_many(keys, form="count")
        o, ids = bank.match_many(keys, form="ids")
        if on_dev:
            assert mask.is_cuda and mask.dtype == torch.int32 and cnt.is_cuda and cnt.dtype == torch.int32
            assert o.is_cuda and o.dtype == torch.int64 and ids.is_cuda and ids.dtype == torch.int32
            cnt, o, ids = cnt.cpu().numpy(), o.cpu().numpy(), ids.cpu().numpy()
        else:
            assert isinstance(mask, np.ndarray) and mask.dtype == np.uint32 and cnt.dtype == np.int32 and o.dtype == np.int64 and ids.dtype == np.int32
        assert tuple(mask.shape) == (len(probes), 4)
        assert np.array_equal(as_bits(mask, F), want)
        assert not as_bits(mask, 128)[:, F:].any()  # pad columns 70..127
        assert cnt.tolist() == want.sum(axis=1).tolist()
        assert o.tolist() == [0, *np.cumsum(want.sum(axis=1)).tolist()] and ids.tolist() == np.nonzero(want)[1].tolist()
    assert tuple(bank.slice_tensor.shape) == (m, 4)
    for i in (0, 1, 2, len(pool), len(probes) - 1, int(np.flatnonzero(want.sum(axis=1) == 0)[0]) if (want.sum(axis=1) == 0).any() else 3):
        assert bank.match(probes[i]) == np.flatnonzero(want[i]).tolist()
    assert bank.match(pool[0])[:1] == [0] and set(G["three"]) <= set(bank.match(pool[0]))


# ------------------------------------------------------------------ the transpose alone, through the C ABI
def chosen_rows(F, m, rng):
    """random fill plus chosen bits: bit 0 and bit m - 1 of filters 0, 31, 32, 63, 64 and F - 1 (set in some, cleared in others)"""
    rows = rng.integers(0, 256, (F, M.row_bytes(m)), dtype=np.uint8)
    nbytes = (m + 7) // 8
    if m % 8:
        rows[:, nbytes - 1] &= (1 << (m % 8)) - 1  # no pad bits
    rows[:, nbytes:] = 0
    for j, f in enumerate(f for f in (0, 31, 32, 63, 64, F - 1) if f < F):
        for p in (0, m - 1):
            if j % 2:
                rows[f, p >> 3] |= 1 << (p & 7)
            else:
                rows[f, p >> 3] &= ~(1 << (p & 7)) & 255
    return rows


@pytest.mark.parametrize("F", [1, 31, 32, 33, 64, 65, 127, 128, 129, 257, 1000])
def test_transpose_against_the_model(pa, N, F):
    rng = np.random.default_rng(F)
    srb = MM.slice_row_bytes(F)
    for m in (1, 63, 64, 127, 128, 959, 4097):
        rows = chosen_rows(F, m, rng)
        want = MM.slices_of(rows, F, m)
        assert not np.unpackbits(want, axis=1, bitorder="little")[:, F:].any()
        table = _dev(rows.view(np.uint32).reshape(-1))
        words = m * srb // 4
        image = guarded(words)
        assert c_slices(N, table, F, m, image) == N.PSK_OK, N.last_error()
        torch.cuda.synchronize()
        got = u32(image[:words]).view(np.uint8).reshape(m, srb)
        assert np.array_equal(got, want), (F, m)  # (pad columns included: `want` has them zero)
        assert guard_ok(image, words)


@pytest.mark.parametrize("F,m", [(257, 959), (70, 63), (1000, 127)])
def test_ranged_transpose_rewrites_exactly_its_word_columns(pa, N, F, m):
    rng = np.random.default_rng(F + m)
    srb = MM.slice_row_bytes(F)
    words, rw = m * srb // 4, srb // 4
    rows = chosen_rows(F, m, rng)
    want = MM.slices_of(rows, F, m).view(np.uint32).reshape(m, rw)
    table = _dev(rows.view(np.uint32).reshape(-1))
    last_word = (F - 1) >> 5
    spans = [(0, 32), (32, 64), (32 * last_word, F), (0, F)] + ([(64, 192), (128, 256)] if F > 256 else [])
    for first, last in spans:
        image = guarded(words)
        assert c_slices(N, table, F, m, image, first, last) == N.PSK_OK, N.last_error()
        torch.cuda.synchronize()
        got = u32(image[:words]).reshape(m, rw)
        hi = rw if last == F else last // 32  # the bank's end takes the row's pad words along
        assert np.array_equal(got[:, first // 32:hi], want[:, first // 32:hi]), (first, last)
        keep = np.ones(rw, dtype=bool)
        keep[first // 32:hi] = False
        assert (got[:, keep] == SENTINEL).all(), (first, last)
        assert guard_ok(image, words)
    image = guarded(words)
    for first, last in ((1, 32), (16, 64), (0, 33), (0, 48), (64, 32), (0, F + 32)):
        if last == F:
            continue
        assert c_slices(N, table, F, m, image, first, last) == N.PSK_EINVAL, (first, last)
    assert c_slices(N, table, F, m, image, 32, 32) == N.PSK_OK  # an empty range: nothing
    torch.cuda.synchronize()
    assert (u32(image) == SENTINEL).all()


# ------------------------------------------------------------------ the match kernel against the model, chosen and random hashes
def random_image(F, m, rng, density):
    """a slice image of the given bit density with pad columns zero; row 0 is all ones (over the filters), row m - 1 all zero when m > 2"""
    srb = MM.slice_row_bytes(F)
    bits = (rng.random((m, srb * 8)) < density).astype(np.uint8)
    bits[0] = 1
    if m > 2:
        bits[m - 1] = 0
    bits[:, F:] = 0
    return np.packbits(bits, axis=1, bitorder="little")


# filters -> slice rows of 16, 32, 48 (an idle lane in the group of 4), 64, 512, 1024, 1040 (one chunk + 16 bytes) and 2064 bytes
@pytest.mark.parametrize("F,srb", [(100, 16), (250, 32), (300, 48), (500, 64), (4000, 512), (8192, 1024), (8200, 1040), (16400, 2064)])
def test_match_against_the_model(pa, N, F, srb):
    assert MM.slice_row_bytes(F) == srb
    rng = np.random.default_rng(F)
    for m in (64, 77, 1):
        for k in (1, 7, 64):
            img = random_image(F, m, rng, 0.5 ** (1.0 / k) if m > 1 else 1.0)  # about half of the columns survive k rows
            image = _dev(img.view(np.uint32).reshape(-1))
            h = rng.integers(0, 2**63, (257, k + 1), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (257, k + 1), dtype=np.uint64)
            h[0, :] = np.uint64(m) * np.arange(1, k + 2, dtype=np.uint64)       # every position 0: the all-ones row -> every filter
            h[1, :] = h[0, :] + np.uint64(m - 1)                                 # every position m - 1: the zero row -> no filter (m > 2)
            h[63], h[64], h[256] = h[0], h[1], h[0]
            want = MM.match_mask(img, m, k, h)
            if m > 2:
                assert MM.match_counts(want)[[0, 1]].tolist() == [F, 0]
            for n in (0, 1, 63, 64, 65, 257):
                agree(c_match(N, image, F, m, k, h[:n]), want[:n])
    # "ids" with a total of 0: only keys that match nothing
    img = random_image(F, 77, rng, 0.5)
    none = np.full((65, 3), 76, dtype=np.uint64)
    got = c_match(N, _dev(img.view(np.uint32).reshape(-1)), F, 77, 3, none)
    assert got[3].size == 0 and not got[1].any() and not got[0].any() and got[2].tolist() == [0] * 66


def test_match_refuses_more_than_64_hashes(pa, N):
    image, out = guarded(64), guarded(64)
    h = _dev(np.zeros((1, 65), dtype=np.uint64))
    rc = N.lib().psk_bank_match(image.data_ptr(), 100, 1, 65, N.KEYS_HASHES, h.data_ptr(), None, 1, 65, N.DEVICE, out.data_ptr(), None, None, None, 0, None)
    assert rc == N.PSK_EINVAL and "at most 64" in N.last_error()
    torch.cuda.synchronize()
    assert (u32(out) == SENTINEL).all()
    bank = pa.BloomFilterBank(3, 10, 1e-21)  # a geometry of 70 hashes
    assert bank.number_hashes > 64
    with pytest.raises(pa.exceptions.NotSupportedError, match="check_many"):
        bank.match_many(["a"])


def test_image_beyond_4_gib(pa, N):
    """m = 2^22 + 1 rows of 1 KiB (8192 filters): the last row starts at byte 2^32; the image is set by hand, there is no bank table"""
    m, F = 2**22 + 1, 8192
    need = m * 1024
    if torch.cuda.mem_get_info()[0] < need + (1 << 30):
        pytest.skip("the device lacks the memory for a 4 GiB image")
    image = torch.zeros(m * 256, dtype=torch.int32, device="cuda")
    v = image.view(m, 256)
    sparse = {}

    def put(p, f):
        sparse.setdefault(p, set()).add(f)
    for f in (0, 5, 31, 32, 4095, 8191):
        put(0, f)
    for f in (5, 32, 100, 8191):
        put(2**22 - 1, f)
    for f in (5, 64, 100, 8191, 4095):
        put(2**22, f)
    for f in (0, 5):
        put(2**21, f)
    for p, fs in sparse.items():
        row = np.zeros(256, dtype=np.uint32)
        for f in fs:
            row[f >> 5] |= np.uint32(1 << (f & 31))
        v[p] = _dev(row)
    top, mid = 2**22, 2**21
    h = np.array([[0, top - 1, top], [top, top, top], [0, 0, 0], [top - 1, top, top - 1], [0, mid, top], [1, 0, top], [top, 0, m + top]], dtype=np.uint64)
    want = [sorted(set.intersection(*(sparse.get(int(x) % m, set()) for x in r))) for r in h]
    assert want[0] == [5, 8191] and want[1] == [5, 64, 100, 4095, 8191] and want[5] == [] and want[6] == [5, 4095, 8191]
    mask, cnt, offs, ids = c_match(N, image, F, m, 3, h)
    for i, w in enumerate(want):
        assert ids[offs[i]:offs[i + 1]].tolist() == w and cnt[i] == len(w)
        assert np.flatnonzero(MM.mask_bits(mask[i:i + 1], F)[0]).tolist() == w
    del v, image
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ every key layout, host and device
def _layout(name, rng, n):
    """-> (host form, device form, hashes of the model (n, k), alt)"""
    if name.startswith("fixed"):
        keys = rng.integers(0, 256, (n, int(name[5:])), dtype=np.uint8)
        return keys, _dev(keys), (lambda k: M.hashes_fixed(keys, k)), False
    if name == "ragged":
        keys = [bytes(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8)) for _ in range(n)]
        keys[5] = b""
        return keys, tuple(map(_dev, ragged_bytes(keys))), (lambda k: M.hashes_list(keys, k)), False
    if name == "codepoints":
        keys = ["".join(chr(int(x)) for x in rng.choice([65, 233, 955, 8364, 128512], int(rng.integers(0, 12)))) + str(i) for i in range(n)]
        return keys, tuple(map(_dev, code_points(keys))), (lambda k: M.hashes_list(keys, k)), False
    h = rng.integers(0, 2**63, (n, 12), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 12), dtype=np.uint64)
    return h, _dev(h), (lambda k: h[:, :k]), True


@pytest.mark.parametrize("layout", ["fixed8", "fixed16", "fixed32", "ragged", "codepoints", "hashes"])
def test_every_key_layout(pa, layout):
    rng = np.random.default_rng(23)
    F, n = 200, 700
    host, dev, hashes, alt = _layout(layout, rng, n)
    bank = pa.BloomFilterBank(F, 10, 0.05)  # 63 bits, 4 hashes: with ~10 keys a filter, false positives are common
    m, k = bank.number_bits, bank.number_hashes
    ids = rng.integers(0, F, n)
    ids[ids == 9] = 10  # an empty filter
    (bank.add_alt_many if alt else bank.add_many)(dev, torch.from_numpy(ids).cuda())
    rows = M.bank_rows(F, m, k, hashes(k), ids)
    want = MM.match_mask(MM.slices_of(rows, F, m), m, k, hashes(k))
    bits = MM.mask_bits(want, F)
    assert bits[np.arange(n), ids].all() and not bits[:, 9].any() and bits.sum() > n  # own filter; the empty one; some false positives
    match, check = (bank.match_alt_many, bank.check_alt_many) if alt else (bank.match_many, bank.check_many)
    for keys, on_dev in ((host, False), (dev, True)):
        mask = match(keys)
        assert (isinstance(mask, torch.Tensor) and mask.is_cuda) == on_dev
        assert np.array_equal(as_bits(mask, F), bits)
        cnt = match(keys, form="count")
        o, got_ids = match(keys, form="ids")
        cnt, o, got_ids = [x.cpu().numpy() if on_dev else x for x in (cnt, o, got_ids)]
        wo, wi = MM.match_ids(want)
        assert np.array_equal(cnt, MM.match_counts(want)) and np.array_equal(o, wo) and np.array_equal(got_ids, wi)
        for pid in ((ids + 1) % F, rng.integers(0, F, n)):  # sampled bits: the pairs answer of the existing lookup
            pairs = check(keys, torch.from_numpy(pid).cuda() if on_dev else pid)
            pairs = pairs.cpu().numpy() if on_dev else pairs
            assert np.array_equal(pairs, bits[np.arange(n), pid])


def test_other_hash_functions_travel_as_hashes(pa):
    def mine(key, depth):
        return [(hash_seed * 0x9E3779B97F4A7C15 + sum(key.encode()) * 1000003) % 2**64 for hash_seed in range(1, depth + 1)]

    F = 40
    words = [f"w{i}" for i in range(200)]
    ids = np.arange(200) % F
    for fn in (mine, pa.default_md5):
        bank = pa.BloomFilterBank(F, 10, 0.05, hash_function=fn)
        bank.add_many(words, ids)
        bits = as_bits(bank.match_many(words), F)
        pairs = bank.check_many([w for w in words for _ in range(F)], np.tile(np.arange(F), 200)).reshape(200, F)  # every (key, filter) pair
        assert np.array_equal(bits, pairs) and bits[np.arange(200), ids].all()
        assert bank.match(words[7]) == np.flatnonzero(pairs[7]).tolist()


# ------------------------------------------------------------------ the image follows the table
def test_staleness(pa):
    F = 100
    bank = pa.BloomFilterBank(F, 100, 0.01)
    a = [f"first-{i}" for i in range(50)]
    b = [f"second-{i}" for i in range(50)]
    fa, fb = np.arange(50) % F, (np.arange(50) + 37) % F
    assert bank.slice_tensor is None
    bank.add_many(a, fa)
    bits = as_bits(bank.match_many(a), F)
    assert bits[np.arange(50), fa].all() and bank._last_refresh == [(0, F)]
    assert not as_bits(bank.match_many(b), F)[np.arange(50), fb].all()
    for policy in ("direct", "grouped"):  # both add policies mark the image stale
        bank.clear()
        assert not as_bits(bank.match_many(a), F).any()
        bank._add_policy = policy
        bank.add_many(tuple(map(_dev, code_points(a))), torch.from_numpy(fa).cuda())
        assert bank._last_path == policy and bank._stale_all
        assert as_bits(bank.match_many(a), F)[np.arange(50), fa].all() and bank._last_refresh == [(0, F)]
        bank.add_many(tuple(map(_dev, code_points(b))), torch.from_numpy(fb).cuda())  # add more: the match sees the new keys
        assert as_bits(bank.match_many(b), F)[np.arange(50), fb].all()
    bank._add_policy = "auto"
    assert bank.match_many(a, form="count") is not None and bank._last_refresh == [(0, F)]  # (nothing stale: no new refresh)
    bank._last_refresh = None
    bank.match_many(a)
    assert bank._last_refresh is None
    # clear(f): column f is empty, its neighbours in the same word are kept; one ranged refresh
    before = as_bits(bank.match_many(a + b), F)
    bank.clear(37)
    after = as_bits(bank.match_many(a + b), F)
    assert bank._last_refresh == [(32, 64)]
    assert before[:, 37].any() and not after[:, 37].any()
    keep = np.arange(F) != 37
    assert np.array_equal(after[:, keep], before[:, keep])
    # set_filter: the match sees the new filter (the last column group: it ends at the bank's end)
    blm = pa.BloomFilter(100, 0.01)
    blm.add_many(["only-in-99", "also-in-99"])
    bank.set_filter(99, blm)
    assert bank.match("only-in-99") == [99] and bank._last_refresh == [(96, F)]
    assert as_bits(bank.match_many(a + b), F)[:, :99].tolist() == after[:, :99].tolist()
    # a write through table_tensor is seen after invalidate_slices()
    bank.table_tensor[5].copy_(bank.table_tensor[99])
    assert bank.match("only-in-99") == [99]
    bank.invalidate_slices()
    assert bank.match("only-in-99") == [5, 99] and bank._last_refresh == [(0, F)]
    # more stale groups than a handful: the whole bank
    big = pa.BloomFilterBank(32 * 12, 10, 0.05)
    big.add_many(["x"] * 12, np.arange(12) * 32)
    assert big.match("x") == (np.arange(12) * 32).tolist()
    for g in range(3):
        big.clear(32 * g)
    assert big.match("x") == (np.arange(3, 12) * 32).tolist() and big._last_refresh == [(0, 32), (32, 64), (64, 96)]
    for g in range(3, 12):
        big.clear(32 * g + 1)  # (an empty filter of each group)
    big.match("x")
    assert big._last_refresh == [(0, 32 * 12)]
    # drop_slices() frees the image, a match rebuilds it
    bank.drop_slices()
    assert bank.slice_tensor is None
    assert bank.match("only-in-99") == [5, 99] and tuple(bank.slice_tensor.shape) == (bank.number_bits, bank.slice_row_bytes // 4)
    bank.refresh_slices()
    assert bank._last_refresh == []
