"""BloomFilterBank.score_many on the GPU: whole queries against every filter (psk_bank_score: the row-AND of psk_bank_match added into
bit-plane counters, never a per-key mask) and the threshold form over the finished scores (psk_bank_score_select).  The answers are the
reference's -- the sums, over a query's keys, of ``key in blm[f]`` of the REAL reference for all 70 filters of
tests/golden/golden_bank_match.json -- and, where the reference has nothing to say (chosen tables, chosen hashes, wide rows, long queries,
an image beyond 4 GiB), the numpy models' (tests/bank_score_model.py over tests/bank_match_model.py, both checked against that fixture on
the CPU).  Every output buffer of a direct C ABI call is filled with a sentinel and has sentinel words behind it."""

import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import bank_match_model as MM  # noqa: E402
import bank_model as M  # noqa: E402
import bank_score_model as SM  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

G = json.loads((ROOT / "tests" / "golden" / "golden_bank_match.json").read_text())
SENTINEL = 0x5A5AA5A5  # (no score of these tests: they stay below 2^17, or are 2^31 - 1)
GUARD = 8  # sentinel words behind every output
GRID_CAP = 4096  # kBankGridCap


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


def guarded(words):
    """an int32 device buffer of `words` words, every word and GUARD words behind them the sentinel; 16-byte aligned"""
    return torch.full((words + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")


def guard_ok(t, words):
    return bool((t[words:] == SENTINEL).all().item())


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def c_score(N, image, F, m, k, h, offs, split=1):
    """psk_bank_score over PSK_KEYS_HASHES on the device into a sentinel-filled buffer -> int64[Q, F]; exactly Q * F words written"""
    h = np.ascontiguousarray(h, dtype=np.uint64)
    n, kk = h.shape
    Q = len(offs) - 1
    hd = _dev(h) if n else None
    od = _dev(np.asarray(offs, dtype=np.uint64))
    out = guarded(Q * F)
    N.check(N.lib().psk_bank_score(image.data_ptr(), F, m, k, N.KEYS_HASHES, hd.data_ptr() if n else None, None, n, kk, N.DEVICE, od.data_ptr(), Q, split,
                                   out.data_ptr(), 0, None))
    torch.cuda.synchronize()
    assert guard_ok(out, Q * F)
    got = u32(out[:Q * F]).reshape(Q, F)
    assert not (got == SENTINEL).any()  # every word of the matrix was written, zeros included
    return got.astype(np.int64)


def c_select(N, scores, thr):
    """psk_bank_score_select, both passes, sentinels checked -> (offsets, ids, scores)"""
    L = N.lib()
    Q, F = scores.shape
    sd, td = _dev(scores.astype(np.uint32).reshape(-1)), _dev(np.asarray(thr, dtype=np.uint32))
    count = guarded(Q)
    N.check(L.psk_bank_score_select(sd.data_ptr(), Q, F, td.data_ptr(), count.data_ptr(), None, None, None, 0, None))
    torch.cuda.synchronize()
    assert guard_ok(count, Q)
    offs = np.zeros(Q + 1, dtype=np.int64)
    np.cumsum(u32(count[:Q]), out=offs[1:])
    total = int(offs[-1])
    ids, hit, only = guarded(total), guarded(total), guarded(total)
    od = _dev(offs[:-1].astype(np.uint64))
    N.check(L.psk_bank_score_select(sd.data_ptr(), Q, F, td.data_ptr(), None, od.data_ptr(), ids.data_ptr(), hit.data_ptr(), 0, None))
    N.check(L.psk_bank_score_select(sd.data_ptr(), Q, F, td.data_ptr(), None, od.data_ptr(), only.data_ptr(), None, 0, None))  # ids without scores
    torch.cuda.synchronize()
    assert guard_ok(ids, total) and guard_ok(hit, total) and guard_ok(only, total) and torch.equal(ids, only)
    return offs, u32(ids[:total]).astype(np.int64), u32(hit[:total]).astype(np.int64)


def agree_select(got, scores, thr):
    o, ids, sc = got
    wo, wi, ws = SM.select(scores, thr)
    assert np.array_equal(o, wo) and np.array_equal(ids, wi) and np.array_equal(sc, ws.astype(np.int64))
    for q in range(scores.shape[0]):
        assert (np.diff(ids[o[q]:o[q + 1]]) > 0).all()  # ascending per query (what the model gives, spelled out)
        assert np.array_equal(sc[o[q]:o[q + 1]], scores[q, ids[o[q]:o[q + 1]]])  # scores beside their ids


def table_image(N, rows, F, m):
    """the slice image psk_bank_slices makes of table rows uint8[F, row_bytes(m)]"""
    table = _dev(rows.view(np.uint32).reshape(-1))
    image = torch.zeros(m * MM.slice_row_bytes(F) // 4, dtype=torch.int32, device="cuda")
    N.check(N.lib().psk_bank_slices(table.data_ptr(), F, m, image.data_ptr(), 0, F, 0, None))
    return image


# ------------------------------------------------------------------ the reference's answers
_GOLDEN = {}


def golden(pa, ci):
    """-> (case, bank built from `sent`, the queries' keys, their hashes, offsets, the reference's scores), once per case"""
    if ci not in _GOLDEN:
        c = G["cases"][ci]
        F = c["filters"]
        pool = [dec(e) for e in c["pool"]]
        probes = pool + [dec(e) for e in c["absent"]]
        want = np.array([[(int.from_bytes(bytes.fromhex(h), "little") >> f) & 1 for f in range(F)] for h in c["masks"]], dtype=bool)
        bank = pa.BloomFilterBank(F, c["est"], c["fpr"])
        assert (bank.number_bits, bank.number_hashes) == (c["number_bits"], c["number_hashes"])
        bank.add_many([pool[i] for f in range(F) for i in c["sent"][f]], np.array([f for f in range(F) for _ in c["sent"][f]]))
        idx, offs = SM.fixture_queries(c, extra=True)
        keys = [probes[i] for i in idx]
        S = SM.score_counts(want[idx], offs)
        S.setflags(write=False)
        _GOLDEN[ci] = (c, bank, keys, M.hashes_list(keys, c["number_hashes"]), offs, S)
    return _GOLDEN[ci]


@pytest.mark.parametrize("ci", [0, 1])
def test_golden_scores_every_layout(pa, N, ci):
    c, bank, keys, h, offs, S = golden(pa, ci)
    F, Q = c["filters"], len(offs) - 1
    assert Q == F + 4 and np.diff(offs)[-2:].tolist() == [4, 1] and S[-2].max() <= 4 and (S[-2] >= 2).any()  # the probe held twice counts twice
    blob, ko = code_points(keys)
    forms = [(bank.score_many, keys, offs, False), (bank.score_many, keys, _dev(offs), False), (bank.score_many, (blob, ko), offs.tolist(), False),
             (bank.score_many, (_dev(blob), _dev(ko)), _dev(offs), True), (bank.score_many, (_dev(blob), _dev(ko)), offs.astype(np.uint32), True),
             (bank.score_alt_many, h, offs, False), (bank.score_alt_many, _dev(h), _dev(offs.astype(np.int32)), True)]
    for call, k_, o_, on_dev in forms:
        got = call(k_, o_)
        if on_dev:
            assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.int32
        else:
            assert isinstance(got, np.ndarray) and got.dtype == np.int32
        assert tuple(got.shape) == (Q, F) and np.array_equal(host(got), S)
    assert not bank._stale_all and not bank._stale_groups  # scoring marks nothing stale
    assert np.array_equal(c_score(N, bank._slices, F, bank.number_bits, bank.number_hashes, h, offs), S)
    # one query made of all the keys
    one = bank.score(keys)
    assert isinstance(one, np.ndarray) and one.shape == (F,) and np.array_equal(one, S.sum(axis=0))
    ids, sc = bank.score(keys, threshold=int(one.max()))
    assert ids.tolist() == np.flatnonzero(one == one.max()).tolist() and (sc == one.max()).all()


@pytest.mark.parametrize("ci", [0, 1])
def test_golden_threshold_forms(pa, ci):
    c, bank, keys, h, offs, S = golden(pa, ci)
    F, Q, lens = c["filters"], len(offs) - 1, np.diff(offs)
    blob, ko = code_points(keys)
    dkeys = (_dev(blob), _dev(ko))

    def both(threshold, want_thr):
        want = SM.select(S, want_thr)
        for k_, o_, on_dev in ((keys, offs, False), (dkeys, _dev(offs), True)):
            got = bank.score_many(k_, o_, threshold=threshold)
            if on_dev:
                assert all(t.is_cuda for t in got) and [t.dtype for t in got] == [torch.int64, torch.int32, torch.int32]
            else:
                assert [t.dtype for t in got] == [np.int64, np.int32, np.int32]
            for g, w in zip(got, want):
                assert np.array_equal(host(g), w)
        return want

    # threshold 1: the union of match_many's ids over the query's keys
    o, ids, _ = both(1, np.ones(Q, dtype=np.int64))
    mo, mids = bank.match_many(keys, form="ids")
    for q in range(Q):
        assert ids[o[q]:o[q + 1]].tolist() == sorted(set(mids[mo[offs[q]]:mo[offs[q + 1]]].tolist()))
    # the query's length: the filters that may hold all of it (at least the filter the query was sent to)
    full = np.maximum(lens, 1)
    o, ids, sc = both(full, full)
    for f in range(F):
        assert (f in ids[o[f]:o[f + 1]].tolist()) == (lens[f] > 0)
    assert (sc == np.repeat(full, np.diff(o))).all()
    o, ids, _ = both(0.5, SM.thresholds(lens, 0.5))
    assert np.diff(o)[G["empty_filter"]] == 0 and 1 <= np.diff(o)[:F][lens[:F] > 0].min() < np.diff(o)[:F].max()
    per = (np.arange(Q) % 5) + 1
    both(per, per)
    both(_dev(per), per)


# ------------------------------------------------------------------ filter-count seams on chosen hashes
def windowed_hashes(rng, n, k, m):
    """key i takes its k positions from a window of three consecutive bits (so that rows of density 0.7 keep a third of the columns whatever k)"""
    start = rng.integers(0, m - 2, n, dtype=np.uint64)
    h = start[:, None] + rng.integers(0, 3, (n, k), dtype=np.uint64)
    return h + np.uint64(m) * rng.integers(0, 2**40, (n, k), dtype=np.uint64)


@pytest.mark.parametrize("F", [1, 31, 32, 33, 127, 128, 129, 8191, 8192, 8193, 16385])
def test_filter_count_seams(pa, N, F):
    m, rng = 40, np.random.default_rng(F)
    rows = np.zeros((F, M.row_bytes(m)), dtype=np.uint8)
    rows[:, :5] = np.packbits(rng.random((F, m)) < 0.7, axis=1, bitorder="little")
    rows[F - 1, :5] = 255  # the last filter holds everything: the last column counts every key
    image = table_image(N, rows, F, m)
    sl = MM.slices_of(rows, F, m)
    offs = np.cumsum([0, 0, 1, 70, 129, 0, 100])
    for k in (1, 64):
        h = windowed_hashes(rng, int(offs[-1]), k, m)
        want = SM.score_counts(MM.mask_bits(MM.match_mask(sl, m, k, h), F), offs)
        assert want[:, F - 1].tolist() == np.diff(offs).tolist() and (F < 31 or (want[3] > 0).sum() > F // 8)
        assert np.array_equal(c_score(N, image, F, m, k, h, offs), want)  # (c_score: exactly Q * F words written)
        assert np.array_equal(c_score(N, image, F, m, k, h, offs, split=3), want)
    assert np.array_equal(c_score(N, image, F, m, 1, np.zeros((0, 1), dtype=np.uint64), [0, 0, 0]), np.zeros((2, F)))  # no keys: zero rows
    out = guarded(4)
    N.check(N.lib().psk_bank_score(image.data_ptr(), F, m, 1, N.KEYS_HASHES, None, None, 0, 1, N.DEVICE, _dev(np.zeros(1, dtype=np.uint64)).data_ptr(), 0, 1,
                                   out.data_ptr(), 0, None))
    torch.cuda.synchronize()
    assert (u32(out) == SENTINEL).all()  # no queries: nothing


# ------------------------------------------------------------------ counter seams: every flush boundary of the bit-plane counters, and 2^16
def parity_bank(N):
    """k = 1, m = 2, three filters: one full, one empty, one holding position 0 only; key i of a query hashes to position i % 2"""
    rows = np.zeros((3, M.row_bytes(2)), dtype=np.uint8)
    rows[0, 0], rows[2, 0] = 3, 1
    return table_image(N, rows, 3, 2)


def parity_queries(lens):
    offs = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    h = np.concatenate([np.arange(n, dtype=np.uint64) % np.uint64(2) for n in lens] + [np.zeros(0, dtype=np.uint64)]).reshape(-1, 1)
    lens = np.asarray(lens, dtype=np.int64)
    return h, offs, np.stack([lens, np.zeros_like(lens), (lens + 1) // 2], axis=1)


SHORT = list(range(131))
LONG = [255, 256, 257, 1023, 65535, 65536, 65537, 70000]


@pytest.mark.parametrize("lens", [SHORT, LONG], ids=["0-130", "long"])
def test_counter_seams(pa, N, lens):
    image = parity_bank(N)
    h, offs, want = parity_queries(lens)
    assert np.array_equal(c_score(N, image, 3, 2, 1, h, offs), want)


# ------------------------------------------------------------------ split: the same scores whatever the number of parts
@pytest.mark.parametrize("split", [1, 2, 3, 7, 64])
def test_split_gives_identical_scores(pa, N, split):
    for ci in (0, 1):
        c, bank, keys, h, offs, S = golden(pa, ci)
        assert np.array_equal(c_score(N, bank._slices, c["filters"], bank.number_bits, bank.number_hashes, h, offs, split), S)
        bank._score_split = split
        try:
            assert bank.score_split_for(5) == split and np.array_equal(bank.score_many(keys, offs), S)
        finally:
            bank._score_split = None
    image = parity_bank(N)
    for lens in (SHORT, LONG):
        h, offs, want = parity_queries(lens)
        assert np.array_equal(c_score(N, image, 3, 2, 1, h, offs, split), want)


def test_more_queries_than_the_grid(pa, N):
    image = parity_bank(N)
    h, offs, want = parity_queries([q % 4 for q in range(GRID_CAP + 5)])
    for split in (1, 2):
        assert np.array_equal(c_score(N, image, 3, 2, 1, h, offs, split), want)


def test_automatic_split(pa):
    bank = pa.BloomFilterBank(8, 10, 0.05)
    cus = bank._cus
    assert bank.score_split_for(2 * cus) == 1 and bank.score_split_for(10**6) == 1 and bank.score_split_for(0) == 1
    assert bank.score_split_for(1) == 2 * cus and bank.score_split_for(2 * cus - 1) == 2 and bank.score_split_for(cus) == 2


# ------------------------------------------------------------------ the select kernel alone
# the wave-per-row form takes rows of up to 2048 columns, the workgroup-per-row form the rest; passes of 64 / 256 columns
@pytest.mark.parametrize("F", [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2047, 2048, 2049, 2304, 2305, 2561])
def test_select_against_the_model(pa, N, F):
    rng = np.random.default_rng(F)
    top = 2**31 - 1
    scores = rng.integers(0, 6, (9, F)).astype(np.int64)
    scores[1] = 0                    # a row of zeros
    scores[2] = 3                    # a row all at its threshold
    scores[3] = 2                    # ... and one all just below it
    scores[4, ::3] = top             # the highest score, threshold 2^31 - 1
    scores[5] = rng.integers(0, 2, F)
    scores[6, :] = 0
    scores[6, [0, F - 1]] = 7        # the first and the last column alone
    thr = np.array([2, 1, 3, 3, top, 1, 7, 5, 6], dtype=np.int64)
    agree_select(c_select(N, scores, thr), scores, thr)
    o, ids, sc = SM.select(scores, thr)
    assert np.diff(o)[1:5].tolist() == [0, F, 0, (F + 2) // 3] and np.diff(o)[6] == min(F, 2)


def test_select_more_rows_than_the_grid(pa, N):
    rng = np.random.default_rng(5)
    for Q, F in ((4 * GRID_CAP + 5, 5), (GRID_CAP + 5, 2049)):
        scores = rng.integers(0, 4, (Q, F)).astype(np.int64)
        thr = rng.integers(1, 5, Q)
        o, ids, sc = c_select(N, scores, thr)
        hit = scores >= thr[:, None]
        assert np.array_equal(np.diff(o), hit.sum(axis=1)) and np.array_equal(ids, np.nonzero(hit)[1]) and np.array_equal(sc, scores[hit])


# ------------------------------------------------------------------ the image follows updates
def test_scores_follow_updates(pa):
    F = 100
    bank = pa.BloomFilterBank(F, 100, 0.01)
    m, k = bank.number_bits, bank.number_hashes
    a = [f"first-{i}" for i in range(60)]
    b = [f"second-{i}" for i in range(60)]
    fa, fb = np.arange(60) % 7, (np.arange(60) % 5) + 37
    queries = a + b + ["only-in-99", "also-in-99"]
    offs = np.array([0, 60, 60, 120, 122, 122])
    hq = M.hashes_list(queries, k)
    held = []  # (hashes of a key, filter): the table the model builds

    def check(refresh="same"):
        rows = M.bank_rows(F, m, k, np.array([h for h, _ in held], dtype=np.uint64).reshape(-1, k), np.array([f for _, f in held], dtype=np.int64))
        want = SM.score_counts(MM.mask_bits(MM.match_mask(MM.slices_of(rows, F, m), m, k, hq), F), offs)
        assert np.array_equal(bank.score_many(queries, offs), want)
        assert np.array_equal(host(bank.score_many(tuple(map(_dev, code_points(queries))), _dev(offs))), want)
        if refresh != "same":
            assert bank._last_refresh == refresh
        return want

    def add(keys, ids):
        held.extend(zip(M.hashes_list(keys, k).tolist(), ids.tolist()))

    assert bank.slice_tensor is None
    check([(0, F)])  # an empty bank: the first score allocates and transposes
    assert tuple(bank.slice_tensor.shape) == (m, bank.slice_row_bytes // 4)
    for policy, keys, ids in (("direct", a, fa), ("grouped", b, fb)):
        bank._add_policy = policy
        bank.add_many(tuple(map(_dev, code_points(keys))), torch.from_numpy(ids).cuda())
        assert bank._last_path == policy and bank._stale_all
        add(keys, ids)
        want = check([(0, F)])
    bank._add_policy = "auto"
    assert want[0, :7].min() >= 8 and want[2, 37:42].min() >= 12 and not want[1].any()
    bank._last_refresh = None
    check(None)  # nothing stale: no refresh
    bank.clear(37)  # one ranged refresh
    held = [(h, f) for h, f in held if f != 37]
    assert check([(32, 64)])[2, 37] == 0
    blm = pa.BloomFilter(100, 0.01)
    blm.add_many(["only-in-99", "also-in-99"])
    bank.set_filter(99, blm)
    add(["only-in-99", "also-in-99"], np.array([99, 99]))
    assert check([(96, F)])[3].tolist() == [0] * 99 + [2]
    bank.table_tensor[5].copy_(bank.table_tensor[99])  # a write through the tensor is seen after invalidate_slices()
    assert bank.score(["only-in-99"]).tolist() == [0] * 99 + [1]
    bank.invalidate_slices()
    held = [(h, f) for h, f in held if f != 5] + [(h, 5) for h, f in held if f == 99]
    assert check([(0, F)])[3, [5, 99]].tolist() == [2, 2]
    bank.clear()
    held = []
    assert not check([(0, F)]).any()


# ------------------------------------------------------------------ 64-bit offsets into the slice image
def test_image_beyond_4_gib(pa, N):
    """m = 2^22 + 1 rows of 1 KiB (8192 filters): the last row starts at byte 2^32; the image is set by hand, there is no bank table"""
    m, F = 2**22 + 1, 8192
    need = m * 1024
    if torch.cuda.mem_get_info()[0] < need + (1 << 30):
        pytest.skip("the device lacks the memory for a 4 GiB image")
    image = torch.zeros(m * 256, dtype=torch.int32, device="cuda")
    v = image.view(m, 256)
    top, mid = 2**22, 2**21
    sparse = {0: {0, 5, 31, 32, 4095, 8191}, top - 1: {5, 32, 100, 8191}, top: {5, 64, 100, 8191, 4095}, mid: {0, 5}}
    for p, fs in sparse.items():
        row = np.zeros(256, dtype=np.uint32)
        for f in fs:
            row[f >> 5] |= np.uint32(1 << (f & 31))
        v[p] = _dev(row)
    h = np.array([[0, top - 1, top], [top, top, top], [0, 0, 0], [top - 1, top, top - 1], [0, mid, top], [1, 0, top], [top, 0, m + top]], dtype=np.uint64)
    offs = [0, 3, 3, 7]
    want = np.zeros((3, F), dtype=np.int64)
    for q in range(3):
        for r in h[offs[q]:offs[q + 1]]:
            for f in set.intersection(*(sparse.get(int(x) % m, set()) for x in r)):
                want[q, f] += 1
    assert want[0, 5] == 3 and want[0, 8191] == 3 and want[2, 5] == 3 and want[2, 0] == 0 and want[2, 4095] == 1
    for split in (1, 2):
        assert np.array_equal(c_score(N, image, F, m, 3, h, offs, split), want)
    del v, image
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ refusals: each returns before any launch
def test_c_abi_refusals_leave_the_outputs_alone(pa, N):
    L = N.lib()
    image, out, cnt = torch.zeros(64, dtype=torch.int32, device="cuda"), guarded(64), guarded(8)
    h = _dev(np.zeros((1, 65), dtype=np.uint64))
    qo = _dev(np.array([0, 1], dtype=np.uint64))
    thr = _dev(np.ones(1, dtype=np.uint32))

    def score(img=image.data_ptr(), k=1, offs=qo.data_ptr(), split=1, scores=out.data_ptr()):
        return L.psk_bank_score(img, 3, 2, k, N.KEYS_HASHES, h.data_ptr(), None, 1, 65, N.DEVICE, offs, 1, split, scores, 0, None)

    for kw, text in ((dict(img=None), "NULL"), (dict(offs=None), "NULL"), (dict(scores=None), "NULL"), (dict(k=65), "at most 64"), (dict(split=0), "split"),
                     (dict(img=image.data_ptr() + 4), "aligned")):
        assert score(**kw) == N.PSK_EINVAL and text in N.last_error(), kw

    def select(scores=out.data_ptr(), t=thr.data_ptr(), count=None, offs=None, ids=None, hit=None):
        return L.psk_bank_score_select(scores, 1, 3, t, count, offs, ids, hit, 0, None)

    for kw, text in ((dict(scores=None, count=cnt.data_ptr()), "NULL"), (dict(t=None, count=cnt.data_ptr()), "NULL"), (dict(), "no output"),
                     (dict(ids=cnt.data_ptr()), "go together"), (dict(offs=qo.data_ptr()), "go together"), (dict(hit=cnt.data_ptr()), "hit_scores_dev"),
                     (dict(count=cnt.data_ptr(), hit=cnt.data_ptr()), "hit_scores_dev")):
        assert select(**kw) == N.PSK_EINVAL and text in N.last_error(), kw
    torch.cuda.synchronize()
    assert (u32(out) == SENTINEL).all() and (u32(cnt) == SENTINEL).all()


def test_python_refusals(pa):
    wide = pa.BloomFilterBank(3, 10, 1e-21)  # a geometry of 70 hashes
    assert wide.number_hashes > 64
    with pytest.raises(pa.exceptions.NotSupportedError, match="check_many"):
        wide.score_many(["a"], [0, 1])
    bank = pa.BloomFilterBank(8, 10, 0.05)
    keys = ["a", "b", "c"]
    dkeys = tuple(map(_dev, code_points(keys)))
    for bad in ([0, 2, 1, 3], [1, 3], [0, 2], [0, 4]):  # decreasing; not from 0; not to n; beyond n
        with pytest.raises(ValueError, match="query_offsets"):
            bank.score_many(keys, bad)
        with pytest.raises(ValueError, match="query_offsets"):
            bank.score_many(dkeys, _dev(np.array(bad)))
        with pytest.raises(ValueError, match="query_offsets"):
            bank.score_many(keys, _dev(np.array(bad)))
    for bad in (np.array([0.0, 3.0]), torch.tensor([0.0, 3.0]).cuda(), np.array([[0, 3]]), np.zeros(0, dtype=np.int64), np.array([False, True]), "03"):
        with pytest.raises(TypeError, match="query_offsets"):
            bank.score_many(keys, bad)
    for bad in (0, -2, 1.5, 0.0, [1, 0], [1]):
        with pytest.raises(ValueError):
            bank.score_many(keys, [0, 1, 3], threshold=bad)
    for bad in (True, "1", [0.5, 0.5]):
        with pytest.raises(TypeError):
            bank.score_many(keys, [0, 1, 3], threshold=bad)
    assert bank.slice_tensor is None  # none of them got as far as the image
    assert not bank.score_many(keys, [0, 1, 3]).any() and bank.slice_tensor is not None
    assert bank.score_many(dkeys, _dev(np.array([0, 3])), validate=False).shape == (1, 8)
    assert bank.score_many([], [0]).shape == (0, 8) and bank.score_many([], [0, 0]).tolist() == [[0] * 8]
    o, ids, sc = bank.score_many([], [0, 0], threshold=1)
    assert o.tolist() == [0, 0] and ids.size == 0 and sc.size == 0
