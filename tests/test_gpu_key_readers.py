"""The key readers of psk_device.hpp -- KeysFixed16 / 8 / 32, KeysFixed<DWORDS>, KeysVarlen<uint8_t / uint32_t>, KeysInline64 and the
windowed walk under them (load_window16, first_window16, walk_key_bytes, walk_key_elems) -- pinned at their edges: every window class
at a 4 KiB page end (start alignment, overhang, shift, first / last window), every source of with_source / with_part_source at every
pointer alignment that selects it, every length class of pass 1's sort, and every length of the by-value key.

Every expected value comes from tests/key_reader_model.py (a plain numpy FNV-1a and a description of the window geometry) or from the
oracle; none from the engine.  tests/test_key_reader_model.py says on the CPU what the inputs used here reach.

Placement: every case puts its keys into ONE tensor of its own, with at least a 4 KiB page of that tensor in front of the first key and
behind the last one, and works from a page-aligned view -- so the model's addresses are the real ones, and no key and no window the
model says may be requested leaves the tensor: a wrong reader shows as a wrong hash, never as a fault.  Nothing is placed at the end of an
allocation on purpose.

Not covered: kKeyLenBig, a single key of 2^31 elements and more (the plain element-by-element walk): it would take minutes on one lane.
"""
import numpy as np
import pytest

import key_reader_model as M

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TABLES = [(400_000, 0.01), (28005615 // 16, 0.01)]  # a Barrett table (64-bit chains) / a power-of-two table: the 32-bit chains, hash32


@pytest.fixture(scope="module")
def pa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pyprobables_amd

    return pyprobables_amd


@pytest.fixture()
def part(request):
    """direct kernels / partitioned kernels"""
    from pyprobables_amd import _native as N

    names = ("partition", "partition_min_keys")
    old = [N.get_option(k) for k in names]
    N.set_option("partition", 1 if request.param else 0)
    N.set_option("partition_min_keys", 1)
    yield request.param
    for k, v in zip(names, old):
        N.set_option(k, v)


@pytest.fixture()
def option():
    """set engine options for one test; the old values come back afterwards"""
    from pyprobables_amd import _native as N

    old = {}

    def set_(name, value):
        old.setdefault(name, N.get_option(name))
        N.set_option(name, value)

    yield set_
    for name, value in old.items():
        N.set_option(name, value)


# ------------------------------------------------------------------------------------------------------------------------ placement
def _place(arr, lead=0):
    """`arr` (uint8 / int32, any shape) `lead` bytes behind a page boundary of a tensor of its own that has a page and more of random bytes
    in front of and behind it -> (the page-aligned uint8 view, the array's own flat view, in its dtype)"""
    raw = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
    size = lead + raw.size
    whole = torch.randint(0, 256, (size + 3 * M.PAGE,), dtype=torch.uint8, device="cuda")
    skip = M.PAGE + (-whole.data_ptr()) % M.PAGE
    view = whole[skip:skip + size]
    assert view.data_ptr() % M.PAGE == 0 and skip >= M.PAGE and whole.numel() - skip - size >= M.PAGE
    if raw.size:
        view[lead:].copy_(torch.from_numpy(raw))
    own = view[lead:]
    assert own.data_ptr() % M.PAGE == lead % M.PAGE
    return view, (own.view(torch.int32) if arr.dtype.itemsize == 4 else own)


def _inside(keys, view, elem_bytes=1):
    """no key and no window load of the (address, length) keys leaves the tensor `view` is cut from: a page on either side"""
    lo, hi = M.load_range(keys, elem_bytes)
    assert -M.PAGE <= lo and hi <= view.numel() + M.PAGE


# ------------------------------------------------------------------------------------------------------------- the C entry points
def _fnv(layout, data, offs, n, key_len, depth, host=False):
    from pyprobables_amd import _native as N

    if host:
        out = np.empty((n, depth), dtype=np.uint64)
        N.check(N.lib().psk_fnv1a_hash(layout, data, offs, n, key_len, depth, N.HOST, out.ctypes.data, 0, None))
        return out
    out = torch.empty((n, depth), dtype=torch.int64, device="cuda")
    N.check(N.lib().psk_fnv1a_hash(layout, data, offs, n, key_len, depth, N.DEVICE, out.data_ptr(), 0, None))
    return out.cpu().numpy().view(np.uint64)


def _qf(layout, data, offs, n, key_len, host=False):
    from pyprobables_amd import _native as N

    if host:
        out = np.empty(n, dtype=np.uint32)
        N.check(N.lib().psk_qf_hash(layout, data, offs, n, key_len, N.HOST, out.ctypes.data, 0, None))
        return out
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    N.check(N.lib().psk_qf_hash(layout, data, offs, n, key_len, N.DEVICE, out.data_ptr(), 0, None))
    return out.cpu().numpy().view(np.uint32)


def _triples(cap, bits, layout, data, offs, n, key_len):
    from pyprobables_amd import _native as N

    out = torch.empty((3, n), dtype=torch.int32, device="cuda")
    N.check(N.lib().psk_ck_triples(cap, bits, layout, data, offs, n, key_len, N.DEVICE, out.data_ptr(), 0, None))
    return out.cpu().numpy().view(np.uint32)


def _rows(got, want):
    """the first rows that differ, for the assertion's message"""
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))
    return f"{bad.size} rows differ, first {bad[:8].tolist()}"


@pytest.fixture(scope="module")
def seam_bytes_ref():
    blob, offs, pinned = M.seam_bytes()
    return M.hash_ragged(M.fnv64, blob, offs, range(17)), M.hash_ragged(M.fnv32, blob, offs)


@pytest.fixture(scope="module")
def seam_bytes_dev(pa):
    blob, offs, pinned = M.seam_bytes()
    view, dblob = _place(blob)
    _inside(M.keys_of(offs), view)
    return dblob, torch.from_numpy(offs).cuda()


# ------------------------------------------------------------------------------------------------------------ a. page seams, bytes
@pytest.mark.parametrize("depth", [1, 8, 9, 17])  # one hash<1> / one kGroup group / a group and the hash<1> tail / two groups and the tail
def test_byte_keys_at_every_page_seam_fnv(pa, seam_bytes_dev, seam_bytes_ref, depth):
    from pyprobables_amd import _native as N

    dblob, doffs = seam_bytes_dev
    n = doffs.numel() - 1
    got = _fnv(N.KEYS_VARLEN8, dblob.data_ptr(), doffs.data_ptr(), n, 0, depth)
    want = seam_bytes_ref[0][:, :depth]
    assert np.array_equal(got, want), _rows(got, want)


def test_byte_keys_at_every_page_seam_qf_hash(pa, seam_bytes_dev, seam_bytes_ref):
    from pyprobables_amd import _native as N

    dblob, doffs = seam_bytes_dev
    got = _qf(N.KEYS_VARLEN8, dblob.data_ptr(), doffs.data_ptr(), doffs.numel() - 1, 0)
    assert np.array_equal(got, seam_bytes_ref[1]), _rows(got, seam_bytes_ref[1])


def test_byte_keys_at_every_page_seam_from_the_host(pa, seam_bytes_ref):
    """the same pair handed over on the host: the engine stages it wherever it likes, the hashes are the same"""
    from pyprobables_amd import _native as N

    blob, offs, pinned = M.seam_bytes()
    n = offs.size - 1
    got = _fnv(N.KEYS_VARLEN8, blob.ctypes.data, offs.ctypes.data, n, 0, 9, host=True)
    assert np.array_equal(got, seam_bytes_ref[0][:, :9]), _rows(got, seam_bytes_ref[0][:, :9])
    got = _qf(N.KEYS_VARLEN8, blob.ctypes.data, offs.ctypes.data, n, 0, host=True)
    assert np.array_equal(got, seam_bytes_ref[1]), _rows(got, seam_bytes_ref[1])


# ------------------------------------------------------------------------------------------------------ b. page seams, code points
def test_code_point_keys_at_every_page_seam(pa):
    from pyprobables_amd import _native as N

    blob, offs, pinned = M.seam_code_points()
    assert blob.max() > 0xFFFF
    view, dblob = _place(blob)
    _inside(M.keys_of(offs, 4), view, 4)
    doffs = torch.from_numpy(offs).cuda()
    n = offs.size - 1
    want64, want32 = M.hash_ragged(M.fnv64, blob, offs, range(9)), M.hash_ragged(M.fnv32, blob, offs)
    for depth in (1, 9):
        got = _fnv(N.KEYS_VARLEN32, dblob.data_ptr(), doffs.data_ptr(), n, 0, depth)
        assert np.array_equal(got, want64[:, :depth]), (depth, _rows(got, want64[:, :depth]))
    got = _qf(N.KEYS_VARLEN32, dblob.data_ptr(), doffs.data_ptr(), n, 0)
    assert np.array_equal(got, want32), _rows(got, want32)
    got = _fnv(N.KEYS_VARLEN32, blob.ctypes.data, offs.ctypes.data, n, 0, 9, host=True)
    assert np.array_equal(got, want64), _rows(got, want64)
    got = _qf(N.KEYS_VARLEN32, blob.ctypes.data, offs.ctypes.data, n, 0, host=True)
    assert np.array_equal(got, want32), _rows(got, want32)


# ---------------------------------------------------------------------------------------------------------- c. fixed-length walk
@pytest.mark.parametrize("L,m,n", M.fixed_walk_cases())
def test_fixed_length_walk(pa, L, m, n):
    """keys that are no whole dwords, end to end (KeysFixed<false>): odd lengths take every start residue of the page"""
    from pyprobables_amd import _native as N

    keys = M.fixed_keys(L, m, n)
    view, flat = _place(keys, lead=m)
    _inside([(m + i * L, L) for i in range(n)], view)
    lens = np.full(n, L)
    got = _fnv(N.KEYS_FIXED, flat.data_ptr(), None, n, L, 9)
    want = M.fnv64(keys, lens, range(9))
    assert np.array_equal(got, want), _rows(got, want)
    got = _qf(N.KEYS_FIXED, flat.data_ptr(), None, n, L)
    assert np.array_equal(got, M.fnv32(keys, lens)), _rows(got, M.fnv32(keys, lens))


def test_fixed_length_zero_with_a_null_pointer(pa):
    from pyprobables_amd import _native as N

    none = np.zeros((5, 0), dtype=np.uint8)
    assert np.array_equal(_fnv(N.KEYS_FIXED, None, None, 5, 0, 9), M.fnv64(none, np.zeros(5, dtype=np.int64), range(9)))
    assert np.array_equal(_qf(N.KEYS_FIXED, None, None, 5, 0), M.fnv32(none, np.zeros(5, dtype=np.int64)))


# ------------------------------------------------------------------------------------------------------------- d. dispatch matrix
DISPATCH_LENGTHS = sorted({L for L, _ in M.DISPATCH_CELLS})
_dispatch_ref = {}


def _dispatch(L):
    """the keys of a length (the same at every misalignment) and the model's hashes of them, computed once"""
    if L not in _dispatch_ref:
        keys = M.dispatch_keys(L)
        lens = np.full(len(keys), L)
        _dispatch_ref[L] = (keys, M.fnv64(keys, lens, range(9)), M.fnv32(keys, lens))
    return _dispatch_ref[L]


def _cell(keys, m):
    """the key matrix at device pointer = page-aligned base + m -> the (n, L) tensor view"""
    n, L = keys.shape
    view, flat = _place(keys, lead=m)
    t = view[m:m + n * L].view(n, L)
    assert t.data_ptr() % 16 == m % 16 and t.data_ptr() == flat.data_ptr()
    if M.DISPATCH_EXPECTED[L, m] == "KeysFixed<false>":
        _inside([(m + i * L, L) for i in range(n)], view)
    return t


@pytest.mark.parametrize("L", DISPATCH_LENGTHS)
def test_dispatch_matrix_c_entry_points(pa, L):
    """every (key length, pointer misalignment) cell through psk_fnv1a_hash, psk_qf_hash and psk_ck_triples: the model's hashes, whatever
    source the pointer selects"""
    from pyprobables_amd import _native as N

    keys, want64, want32 = _dispatch(L)
    n = len(keys)
    cap, bits = 10007, 32
    want3 = M.cuckoo_triples(want64[:, 0], cap, bits)
    sources = set()
    for m in [m for l_, m in M.DISPATCH_CELLS if l_ == L]:
        t = _cell(keys, m)
        sources.add(M.fixed_source(L, t.data_ptr()))
        assert M.fixed_source(L, t.data_ptr()) == M.DISPATCH_EXPECTED[L, m]
        got = _fnv(N.KEYS_FIXED, t.data_ptr(), None, n, L, 9)
        assert np.array_equal(got, want64), (m, _rows(got, want64))
        got = _qf(N.KEYS_FIXED, t.data_ptr(), None, n, L)
        assert np.array_equal(got, want32), (m, _rows(got, want32))
        got = _triples(cap, bits, N.KEYS_FIXED, t.data_ptr(), None, n, L)
        assert np.array_equal(got, want3), (m, _rows(got.T, want3.T))
    assert len(sources) >= 2  # (equal across all m of one L: every m equals the same model rows)


@pytest.mark.parametrize("part", [False, True], indirect=True)
@pytest.mark.parametrize("est,fpr", TABLES)
@pytest.mark.parametrize("L", DISPATCH_LENGTHS)
def test_dispatch_matrix_bloom_filter(pa, oracle, part, est, fpr, L):
    keys, _, _ = _dispatch(L)
    n = len(keys)
    ref = None
    for m in [m for l_, m in M.DISPATCH_CELLS if l_ == L]:
        t = _cell(keys, m)
        blm = pa.BloomFilter(est_elements=est, false_positive_rate=fpr)
        if ref is None:
            ob = oracle.OracleBloom(blm.number_bits, blm.number_hashes)
            ob.add_keys(keys[: n // 2])
            ref = (ob.bloom.copy(), ob.check_keys(keys))
            assert ref[1][: n // 2].all() and not ref[1].all()  # (the lookups have both answers to give)
        blm.add_many(t[: n // 2])
        assert np.array_equal(np.frombuffer(bytes(blm.bloom), dtype=np.uint8), ref[0]), m
        assert blm.elements_added == n // 2
        assert np.array_equal(blm.check_many(t).cpu().numpy().astype(np.uint8), ref[1]), m


@pytest.mark.parametrize("part", [True], indirect=True)
@pytest.mark.parametrize("m", [4, 1])  # KeysFixed<true> / KeysFixed<false> under the counters' payloads
def test_dispatch_count_min_sketch_sixteen_byte_keys_off_alignment(pa, oracle, part, m):
    keys, _, _ = _dispatch(16)
    n = len(keys)
    w = (np.arange(n) % 8 + 1).astype(np.int32)
    t = _cell(keys, m)
    cms = pa.CountMinSketch(width=4096, depth=5)
    cms.add_many(t, torch.from_numpy(w).cuda())
    oc = oracle.OracleCMS(4096, 5)
    oc.add_keys(keys, w)
    assert np.array_equal(np.frombuffer(bytes(cms._bins), dtype=np.int32), oc.bins)
    assert cms.elements_added == oc.els_added
    assert np.array_equal(cms.check_many(t).cpu().numpy(), oc.check_keys(keys).astype(np.int32))


# ---------------------------------------------------------------------------------------------------- e. length classes of pass 1
_class_ref = {}


def _class_batch(name, cps):
    """(blob, offsets, keys as bytes or None, the model's 64-bit hashes for 7 seeds) of one batch of the length-class tests"""
    if (name, cps) not in _class_ref:
        blob, offs = M.ragged(M.class_batches()[name], 300 + sorted(M.class_batches()).index(name), cps)
        raw = blob.tobytes()
        keys = None if cps else [raw[offs[i]:offs[i + 1]] for i in range(offs.size - 1)]
        _class_ref[name, cps] = (blob, offs, keys, M.hash_ragged(M.fnv64, blob, offs, range(7)))
    return _class_ref[name, cps]


def _place_pair(blob, offs, cps):
    view, dblob = _place(blob)
    _inside(M.keys_of(offs, 4 if cps else 1), view, 4 if cps else 1)
    return dblob, torch.from_numpy(offs).cuda()


@pytest.mark.parametrize("part", [True], indirect=True)
@pytest.mark.parametrize("ragged_sort", [1, 0])
@pytest.mark.parametrize("est,fpr", TABLES)
@pytest.mark.parametrize("name,cps", [(k, False) for k in sorted(M.class_batches())] + [(k, True) for k in M.CODE_POINT_BATCHES])
def test_length_classes_of_pass_one(pa, oracle, part, option, ragged_sort, est, fpr, name, cps):
    """tiles that hold every length class, one class only, or the two extremes, through the partitioned path with and without the sort:
    add the first half, look all keys up"""
    option("ragged_sort", ragged_sort)
    blob, offs, keys, hashes = _class_batch(name, cps)
    n = offs.size - 1
    half = n // 2
    dblob, doffs = _place_pair(blob, offs, cps)
    blm = pa.BloomFilter(est_elements=est, false_positive_rate=fpr)
    assert blm.number_hashes == 7
    ob = oracle.OracleBloom(blm.number_bits, blm.number_hashes)
    if cps:
        ob.add_hashes(hashes[:half])
        want = ob.check_hashes(hashes)
    else:
        ob.add_varlen(keys[:half])
        want = ob.check_varlen(keys)
    blm.add_many((dblob, doffs[: half + 1]))
    assert np.array_equal(np.frombuffer(bytes(blm.bloom), dtype=np.uint8), ob.bloom)
    assert blm.elements_added == half == ob.els_added
    got = blm.check_many((dblob, doffs)).cpu().numpy().astype(np.uint8)
    assert np.array_equal(got, want), _rows(got, want)


@pytest.mark.parametrize("part", [True], indirect=True)
@pytest.mark.parametrize("ragged_sort", [1, 0])
def test_length_classes_under_the_counters(pa, oracle, part, option, ragged_sort):
    """the batch that holds every class, with weights 1 .. 8, into a CountMinSketch and a CountingBloomFilter"""
    option("ragged_sort", ragged_sort)
    blob, offs, keys, _ = _class_batch("all_classes", False)
    n = offs.size - 1
    w = (np.arange(n) % 8 + 1).astype(np.int32)
    dblob, doffs = _place_pair(blob, offs, False)
    dw = torch.from_numpy(w).cuda()

    cms = pa.CountMinSketch(width=4096, depth=5)
    oc = oracle.OracleCMS(4096, 5)
    h5 = M.hash_ragged(M.fnv64, blob, offs, range(5))
    for i in range(n):
        oc.add_alt(h5[i], int(w[i]))
    cms.add_many((dblob, doffs), dw)
    assert np.array_equal(np.frombuffer(bytes(cms._bins), dtype=np.int32), oc.bins)
    assert cms.elements_added == oc.els_added == int(w.sum())
    assert cms.check_many((dblob, doffs)).cpu().tolist() == [oc.check_alt(h5[i]) for i in range(n)]

    cbf = pa.CountingBloomFilter(est_elements=200_000, false_positive_rate=0.01)
    ocb = oracle.OracleCBF(cbf.number_bits, cbf.number_hashes)
    hk = M.hash_ragged(M.fnv64, blob, offs, range(cbf.number_hashes))
    for i in range(n):
        ocb.add_alt(hk[i], int(w[i]))
    cbf.add_many((dblob, doffs), dw)
    assert np.array_equal(np.frombuffer(bytes(cbf.bloom), dtype=np.uint32), ocb.bloom)
    assert cbf.elements_added == ocb.els_added
    got = cbf.check_many((dblob, doffs)).cpu().numpy().view(np.uint32)
    assert got.tolist() == [ocb.check_alt(hk[i]) for i in range(n)]


# ------------------------------------------------------------------------------------------------------------ f. the by-value key
@pytest.mark.parametrize("poll_us", [None, 0])  # the default: keys of <= 64 bytes ride in the kernel arguments (KeysInline64), 65 and 66 take
def test_single_keys_of_every_length(pa, oracle, option, poll_us):  # the staged page; 0: every length takes the staged page's fixed sources
    """`key in blm`, `cms.add(key)`, `cbf.remove(key)` ... for one key of every length 0 .. 66: every return value and the tables against
    the oracle, and the batch route's tables.  (KeysInline64's tail word is w[L / 4] for every length that has tail bytes -- at most
    w[15], for 61 .. 63 bytes; its index clamp only bites at 64 bytes, where no tail byte is read.  A tail word taken one too low at
    61 .. 63 bytes shows here as a wrong table at 61.)"""
    if poll_us is not None:
        option("host_poll_us", poll_us)
    rng = np.random.default_rng(64)
    keys = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in range(67)]
    for est, fpr in TABLES:
        blm = pa.BloomFilter(est_elements=est, false_positive_rate=fpr)
        ob = oracle.OracleBloom(blm.number_bits, blm.number_hashes)
        for key in keys:
            assert (key in blm) is bool(ob.check_varlen([key])[0]), len(key)
            blm.add(key)
            ob.add_varlen([key])
            assert (key in blm) is True, len(key)
            assert np.array_equal(np.frombuffer(bytes(blm.bloom), dtype=np.uint8), ob.bloom), len(key)
        assert blm.elements_added == len(keys)
        batch = pa.BloomFilter(est_elements=est, false_positive_rate=fpr)
        batch.add_many(keys)
        assert bytes(batch.bloom) == bytes(blm.bloom)

    cms, batch = pa.CountMinSketch(width=1000, depth=5), pa.CountMinSketch(width=1000, depth=5)
    oc = oracle.OracleCMS(1000, 5)
    for key in keys:
        h = oracle.default_fnv_1a(key, 5)
        assert cms.check(key) == oc.check_alt(h), len(key)
        assert cms.add(key, len(key) + 1) == oc.add_alt(h, len(key) + 1), len(key)
        assert cms.check(key) == oc.check_alt(h), len(key)
    assert np.array_equal(np.frombuffer(bytes(cms._bins), dtype=np.int32), oc.bins) and cms.elements_added == oc.els_added
    batch.add_many(keys, np.arange(1, len(keys) + 1, dtype=np.int32))
    assert bytes(batch._bins) == bytes(cms._bins)

    cbf, batch = (pa.CountingBloomFilter(est_elements=1000, false_positive_rate=0.01) for _ in range(2))
    ocb = oracle.OracleCBF(cbf.number_bits, cbf.number_hashes)
    for key in keys:
        h = oracle.default_fnv_1a(key, cbf.number_hashes)
        assert cbf.add(key, 3) == ocb.add_alt(h, 3), len(key)
        assert cbf.check(key) == ocb.check_alt(h), len(key)
        assert cbf.remove(key, 1) == ocb.remove_alt(h, 1), len(key)
    assert np.array_equal(np.frombuffer(bytes(cbf.bloom), dtype=np.uint32), ocb.bloom) and cbf.elements_added == ocb.els_added
    batch.add_many(keys, 3)
    batch.remove_many(keys)
    assert bytes(batch.bloom) == bytes(cbf.bloom) and batch.elements_added == cbf.elements_added
