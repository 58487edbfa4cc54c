"""The exact ordered CountMinSketch add (psk_cms_add_running, csrc/psk_running.hpp) where its kernels change behaviour: one to four radix
passes and the widths at which a digit is added, every tile and block size, chunks of deep sketches and the seams between them, the
uint32 segment sums at and beyond 2^32 with negative and at-rail bins underneath, ``elements_added`` at INT64_MAX, the wrap-free bound it
leaves for the unordered kernels, and negative weights of a device batch.

The bins are chosen (``E.lift`` + ``add_alt_many_ordered``) and the weights are never all equal, so two ops of one bin that change places
change a return value.  Everything is exact: every op's return value and its dtype, the WHOLE table (the reference's touched bins
scattered into zeros or into the preload, on the device), ``elements_added``, and that the parallel passes ran and the one-lane kernel did
not.  References: the Python-integer loop ``E.cms_running_counted`` for a few thousand ops, its numpy form ``E.cms_running_vec`` (tied to
the loop in tests/test_edge_hashes_host.py) beyond that, computed once per shape."""

import ctypes as C
import struct

import numpy as np
import pytest

import edge_hashes as E

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WHERE = ("host", "device")
QUERIES = ("min", "mean", "mean-min")
FOOTER = struct.Struct("IIq")  # width, depth, elements_added behind the bins of an exported sketch
I32_MAX, I32_MIN, I64_MAX = E.I32_MAX, -(2**31), E.I64_MAX
# csrc/psk_running.hpp: kRunChunk, kRunCells; csrc/psk_segscan.hpp: kRunSortTile, kRunSegBlock -- restated, so that a change there fails test_chunk_seams loudly
RUN_CHUNK, RUN_CELLS, RUN_SORT_TILE, RUN_SEG_BLOCK = 1 << 20, 1 << 23, 2048, 256


@pytest.fixture(scope="module")
def pa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pyprobables_amd

    return pyprobables_amd


@pytest.fixture()
def N():
    from pyprobables_amd import _native as N

    return N


def _dev(a):
    a = np.ascontiguousarray(a)  # (unsigned words travel as the signed tensors of the same bits)
    return torch.from_numpy(a.view({np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype))).cuda()


def _give(a, where):
    return a if where == "host" or a is None else _dev(a)


def _host(x):
    return x.cpu().numpy() if hasattr(x, "is_cuda") else np.asarray(x)


def _weights(n):
    return (1 + np.arange(n) % 5).astype(np.int32)


def _sketch(pa, width, depth, query, preload=None, els=0):
    """an empty sketch, or one loaded from an image: ``preload`` is the whole table (int32) or one value for every bin"""
    if preload is None and els == 0:
        cms = pa.CountMinSketch(width=width, depth=depth, device=0)
    else:
        bins = np.zeros(width * depth, dtype=np.int32) if preload is None else np.broadcast_to(np.asarray(preload, dtype=np.int32), (width * depth,))
        cms = pa.CountMinSketch.frombytes(bins.tobytes() + FOOTER.pack(width, depth, els), device=0)
    cms.query_type = query
    return cms


def _expect_table(cms, touched, preload=None):
    """the table tensor (padding included) with the reference's touched bins on top of zeros / the preload"""
    t = cms.table_tensor
    exp = torch.zeros_like(t)
    n = cms.width * cms.depth
    if preload is not None:
        exp[:n] = torch.from_numpy(np.broadcast_to(np.asarray(preload, dtype=np.int32), (n,)).copy()).to(t.device)
    if isinstance(touched, dict):
        idx = np.fromiter(touched.keys(), dtype=np.int64, count=len(touched))
        val = np.fromiter(touched.values(), dtype=np.int64, count=len(touched))
    else:  # the loop form's whole table
        idx = np.arange(n, dtype=np.int64)
        val = np.asarray(touched, dtype=np.int64)
    assert idx.size == 0 or (0 <= idx.min() and idx.max() < n and I32_MIN <= val.min() and val.max() <= I32_MAX)
    exp[torch.from_numpy(idx).to(t.device)] = torch.from_numpy(val.astype(np.int32)).to(t.device)
    return exp


def _ordered(N, cms, h, w, where, query, want, touched, els, preload=None, clamps=None):
    """one ordered batch of chosen hashes into `cms` and everything the file promises about it"""
    fast, seq = N.get_option("cms_running_fast"), N.get_option("cms_running_sequential")
    got = cms.add_alt_many_ordered(_give(h, where), _give(w, where))
    assert (N.get_option("cms_running_fast"), N.get_option("cms_running_sequential")) == (fast + 1, seq)
    assert isinstance(got, np.ndarray) if where == "host" else got.is_cuda
    assert _host(got).dtype == (np.int64 if query == "mean-min" else np.int32)
    got = _host(got).astype(np.int64)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (where, query, "first differing op", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]), "of", bad.size)
    assert torch.equal(cms.table_tensor, _expect_table(cms, touched, preload)), (where, query)
    assert cms.elements_added == els, (where, query)
    if clamps is not None:
        assert cms.batch_diagnostics()["saturated"] == clamps, (where, query)


# ------------------------------------------------------------------ a: radix passes and digit boundaries
PASS_WIDTHS = ((1, 2), (2, 2), (255, 2), (256, 2), (257, 2), (65536, 2), (65537, 2), (2**24, 2), (2**24 + 1, 2), (2**28 + 3, 1))
PASSES = {1: 1, 2: 1, 255: 1, 256: 1, 257: 2, 65536: 2, 65537: 3, 2**24: 3, 2**24 + 1: 4, 2**28 + 3: 4}  # ceil(lg width / 8), at least one
_pass_refs = {}


def _pass_case(width, depth):
    if width not in _pass_refs:
        n = 5000  # three sort tiles, the last one partial
        cols = np.stack([E.running_digit_columns(width, n, 10 + s) for s in range(depth)], axis=1)
        h, w = E.lift(cols, width, 2), _weights(n)
        queries = QUERIES if width >= 2 else QUERIES[:2]
        res, touched, els, _ = E.cms_running_vec(width, depth, h, w, queries)
        _pass_refs[width] = (h, w, dict(zip(queries, res)), touched, els)
    return _pass_refs[width]


@pytest.mark.parametrize("query", QUERIES)
@pytest.mark.parametrize("width,depth", PASS_WIDTHS, ids=[str(w) for w, _ in PASS_WIDTHS])
def test_radix_passes_and_digit_boundaries(pa, N, width, depth, query):
    """5000 ops whose columns sit on both sides of every 8-bit digit boundary the width has, and pairs of columns that differ in one digit
    only: 1, 2, 3 and 4 sort passes, and the widths at which a pass is added.  Width 1 has no mean-min (the C entry answers PSK_EINVAL):
    the call raises and leaves the sketch as it was."""
    assert max(1, ((width - 1).bit_length() + 7) // 8) == PASSES[width]
    h, w, res, touched, els = _pass_case(width, depth)
    for where in WHERE:
        if width == 1 and query == "mean-min":
            cms = _sketch(pa, width, depth, query, preload=np.array([5, -7], dtype=np.int32), els=11)
            before = cms.table_tensor.clone()
            fast, seq = N.get_option("cms_running_fast"), N.get_option("cms_running_sequential")
            with pytest.raises(ValueError):
                cms.add_alt_many_ordered(_give(h, where), _give(w, where))
            out, e = np.zeros(h.shape[0], dtype=np.int64), C.c_int64(0)
            rc = N.lib().psk_cms_add_running(cms._tab.handle, N.KEYS_HASHES, h.ctypes.data, None, h.shape[0], depth, w.ctypes.data, N.HOST, N.Q_MEANMIN, 11,
                                             out.ctypes.data, C.addressof(e), cms._tab.stream)
            assert rc == N.PSK_EINVAL and "width" in N.last_error()
            assert (N.get_option("cms_running_fast"), N.get_option("cms_running_sequential")) == (fast, seq)
            assert torch.equal(cms.table_tensor, before) and cms.elements_added == 11 and before[:2].tolist() == [5, -7]
            continue
        cms = _sketch(pa, width, depth, query)
        _ordered(N, cms, h, w, where, query, res[query], touched, els)
        del cms  # (2^28 + 3: one 1 GiB table at a time)


# ------------------------------------------------------------------ b: tile and block edges
TILE_NS = (1, 63, 64, 65, 255, 256, 257, 1023, 1025, 2047, 2048, 2049, 4095, 4097)
_tile_refs = {}


def _tile_case(n, query):
    width, depth = 777, 3
    if n not in _tile_refs:
        rng = np.random.default_rng(n)
        cols = rng.integers(0, width, size=(n, depth))
        hot = rng.random((n, depth)) < 0.5  # about half the ops of every row in ONE bin: a segment that runs through every block
        for s in range(depth):
            cols[hot[:, s], s] = (123, 0, width - 1)[s]
        _tile_refs[n] = (E.lift(cols, width, 3), _weights(n), {})
    h, w, refs = _tile_refs[n]
    if query not in refs:
        refs[query] = E.cms_running_counted(width, depth, h, w, query)
    return (h, w, *refs[query])


@pytest.mark.parametrize("query", QUERIES)
@pytest.mark.parametrize("n", TILE_NS)
def test_tile_and_block_edges(pa, N, n, query):
    """n one below, on and one above the wave (64), the segment block and weight tile (256), the single-workgroup scans (1024) and the
    sort tile (2048, and two of them)"""
    h, w, want, bins, els, _ = _tile_case(n, query)
    for where in WHERE:
        _ordered(N, _sketch(pa, 777, 3, query), h, w, where, query, want, bins, els)


# ------------------------------------------------------------------ c: deep sketches on the fast path, chunk seams
def _chunk(depth):
    """ops per chunk of a batch that is longer than one chunk (cms_running_arena in csrc/psk_running.hip)"""
    cap = min(RUN_CHUNK, RUN_CELLS // depth)
    return -(-cap // RUN_SORT_TILE) * RUN_SORT_TILE


DEEP = {9: 5000, 33: 256_000 + 1, 63: 135_168 + 257, 64: 2 * 131_072 + 2049}  # depth: n
_deep_refs = {}


def test_chunk_seams():
    """the shapes of test_deep_sketches_and_chunk_seams cross the seams they are named for"""
    assert [_chunk(d) for d in (1, 8, 9, 33, 63, 64)] == [1 << 20, 1 << 20, 933_888, 256_000, 135_168, 131_072]
    assert any(_chunk(d) & (_chunk(d) - 1) for d in DEEP), "a chunk size that is no power of two"
    assert DEEP[9] <= _chunk(9)                                                  # one chunk
    assert DEEP[33] == _chunk(33) + 1                                            # two chunks, the second holds one op
    assert DEEP[63] == _chunk(63) + RUN_SEG_BLOCK + 1                            # ... one op into its second segment block
    assert DEEP[64] == 2 * _chunk(64) + RUN_SORT_TILE + 1                        # three chunks, the last ends one op into its second sort tile


def _deep_case(depth):
    """(hashes, weights, {query: results}, touched bins, elements_added behind the batch, the start it was computed from)"""
    if depth not in _deep_refs:
        width, n = 4099, DEEP[depth]
        rng = np.random.default_rng(depth)
        cols = rng.integers(0, width, size=(n, depth))
        hot = rng.random((n, depth)) < 0.25  # one hot bin per row with ops in every chunk: each chunk starts from the table the last one left
        hot[-1] = True                       # (the last chunk may hold one op)
        for s in range(depth):
            cols[hot[:, s], s] = (s * 64 + 1) % width
            assert all(hot[lo:lo + _chunk(depth), s].any() for lo in range(0, n, _chunk(depth)))
        h, w = E.lift(cols, width, 4), _weights(n)
        # depth 64: elements_added reaches INT64_MAX inside the second chunk, in the middle of a tile; the third chunk starts clamped
        if depth == 64:
            w[-33_333:] += 2  # (weights that repeat evenly reach half their total at op n / 2, which opens a tile here)
        els0 = I64_MAX - int(w.sum()) // 2 if depth == 64 else 0
        if els0:
            at = int(np.searchsorted(np.cumsum(w.astype(np.int64)), I64_MAX - els0))  # the first op that ends at INT64_MAX
            assert _chunk(depth) < at < 2 * _chunk(depth) and 0 < at % 64 < 63 and 64 < at % RUN_SEG_BLOCK < RUN_SEG_BLOCK - 64
        res, touched, els, clamps = E.cms_running_vec(width, depth, h, w, ("min", "mean-min"), None, els0)
        assert clamps == 0 and els == (I64_MAX if els0 else int(w.sum()))
        _deep_refs[depth] = (h, w, dict(zip(("min", "mean-min"), res)), touched, els, els0)
    return _deep_refs[depth]


@pytest.mark.parametrize("query", ("min", "mean-min"))
@pytest.mark.parametrize("depth", sorted(DEEP))
def test_deep_sketches_and_chunk_seams(pa, N, depth, query):
    """depths 9 to 64 take the parallel passes in chunks of 2^23 / depth ops, rounded up to a sort tile: one chunk, a second chunk of one
    op, of 257 ops, and three chunks; mean-min sorts 63 and 64 values per op.  The min results do not depend on elements_added, so the
    depth-64 min case starts from an empty sketch and ends at the sum of the weights; its mean-min case starts from the footer."""
    h, w, res, touched, els, els0 = _deep_case(depth)
    if query == "min":
        els0, els = 0, int(w.sum())
    for where in WHERE:
        _ordered(N, _sketch(pa, 4099, depth, query, els=els0), h, w, where, query, res[query], touched, els, clamps=0)


# ------------------------------------------------------------------ d: saturation arithmetic
def _walk(t0):
    """weights that take a bin from t0 through 0 to INT32_MAX - 1, to exactly INT32_MAX (no clamp), one past it (a clamp), then a
    weight 0 at the rail (no clamp) and one more clamp"""
    targets = ([-5] if t0 < -5 else []) + [0, 3, I32_MAX - 1, I32_MAX]
    out, cur = [], t0
    for t in targets:
        out.append(t - cur)
        cur = t
    assert all(0 <= x <= I32_MAX for x in out)
    return out + [1, 0, 7]


def _sat_case(name):
    """(hashes, weights, preload or None)"""
    width, depth = 7, 3
    rng = np.random.default_rng(len(name))
    if name == "carry":  # 600 ops of INT32_MAX into bin 3 of every row, every fifth op: the sum passes 2^32 at its third element
        n = 3000
        cols = rng.integers(0, width - 1, size=(n, depth))
        cols[cols == 3] = width - 1
        w = _weights(n)
        cols[::5], w[::5] = 3, I32_MAX
        cols[2::35] = 3  # small weights into the same bin: their value is the stuck sum alone (INT32_MAX + w clamps whatever lies in front)
        assert w[2::35].max() < 6 and (E.indices(E.lift(cols, width, 5), width, depth) == 3).all(axis=1).sum() == 600 + 86
        return E.lift(cols, width, 5), w, None
    if name in ("from-int32-min", "from-minus-one"):  # the walk in bin 2 of every row, its ops 97 apart, small adds to the other bins between
        t0 = I32_MIN if name == "from-int32-min" else -1
        walk = _walk(t0)
        n = 97 * len(walk)
        cols = rng.integers(3, width, size=(n, depth))
        w = _weights(n)
        cols[50::97], w[50::97] = 2, walk
        assert t0 + sum(walk[:-3]) == I32_MAX and (t0 != I32_MIN or sum(walk[:-3]) == 2**32 - 1)
        return E.lift(cols, width, 6), w, t0
    n = 2000
    cols = rng.integers(0, width, size=(n, depth))
    w = _weights(n)
    if name == "zero-at-rail":  # every bin at INT32_MAX: weight 0 returns INT32_MAX and is no clamp, any other weight is one
        w[rng.random(n) < 0.6] = 0
        return E.lift(cols, width, 7), w, I32_MAX
    assert name == "zero-on-empty"  # 700 ops of weight 0 into an empty table (mean-min: 0), zeros among the weights after them
    w[:700] = 0
    w[700::3] = 0
    return E.lift(cols, width, 8), w, None


SAT_CASES = ("carry", "from-int32-min", "from-minus-one", "zero-at-rail", "zero-on-empty")


@pytest.mark.parametrize("query", QUERIES)
@pytest.mark.parametrize("name", SAT_CASES)
def test_saturation_arithmetic(pa, N, name, query):
    """uint32 segment sums at, on and beyond 2^32 - 1 carried over several blocks, with INT32_MIN, -1 and INT32_MAX underneath; weight 0
    at the rail and on an empty table; the clamp tally is the reference's"""
    width, depth = 7, 3
    h, w, t0 = _sat_case(name)
    pre = None if t0 is None else np.full(width * depth, t0, dtype=np.int32)
    want, bins, els, clamps = E.cms_running_counted(width, depth, h, w, query, pre)
    if name == "carry":
        assert clamps == 3 * (599 + 86) and (bins.reshape(depth, width)[:, 3] == I32_MAX).all()
    elif name.startswith("from-"):
        assert clamps == 3 * 2 and (bins.reshape(depth, width)[:, 2] == I32_MAX).all() and bins.min() < 0
    elif name == "zero-at-rail":
        assert clamps == 3 * int((w > 0).sum()) and (query != "min" or (want == I32_MAX).all())
    else:
        assert clamps == 0 and (want[:700] == 0).all() and want[700:].any()
    for where in WHERE:
        _ordered(N, _sketch(pa, width, depth, query, preload=pre), h, w, where, query, want, bins, els, preload=pre, clamps=clamps)


# ------------------------------------------------------------------ e: elements_added at INT64_MAX
@pytest.mark.parametrize("query", ("min", "mean-min"))
def test_elements_added_clamps_in_the_middle_of_a_tile_and_stays(pa, N, query):
    """3000 ops from INT64_MAX - 1000: the clamp falls inside the first weight tile; a second batch starts at INT64_MAX.  (Bins are
    non-negative: elements_added - bin stays inside int64, see DESIGN.md.)"""
    width, depth, n = 777, 3, 3000
    rng = np.random.default_rng(17)
    w = (1 + np.arange(n) % 7).astype(np.int32)
    at = int(np.searchsorted(np.cumsum(w), 1000))
    assert 0 < at % 64 < 63 and at < RUN_SEG_BLOCK
    h1, h2 = (E.lift(rng.integers(0, width, size=(n, depth)), width, 9 + i) for i in range(2))
    want1, bins1, els1, _ = E.cms_running_counted(width, depth, h1, w, query, None, I64_MAX - 1000)
    want2, bins2, els2, _ = E.cms_running_counted(width, depth, h2, w[::-1], query, bins1, els1)
    assert els1 == els2 == I64_MAX
    for where in WHERE:
        cms = _sketch(pa, width, depth, query, els=I64_MAX - 1000)
        _ordered(N, cms, h1, w, where, query, want1, bins1, I64_MAX)
        _ordered(N, cms, h2, np.ascontiguousarray(w[::-1]), where, query, want2, bins2, I64_MAX)


# ------------------------------------------------------------------ f: ordered and unordered batches taking turns
def _skewed_keys16(oracle, n, pool, salt):
    """n 16-byte keys drawn from `pool` distinct ones, cubed towards the first (integers only)"""
    i = np.arange(n, dtype=np.uint64) + np.uint64(salt * 1000003)
    with np.errstate(over="ignore"):
        z = i + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = (z ^ (z >> np.uint64(31))) % np.uint64(pool)
    idx = (x * x * x // np.uint64(pool * pool)).astype(np.int64)  # pool <= 2^20: x^3 < 2^60
    return oracle.gen_keys16(0, pool)[idx]


@pytest.mark.parametrize("where", WHERE)
def test_ordered_and_unordered_batches_take_turns_near_the_rail(pa, oracle, N, where):
    """add_many_ordered, unordered weighted add_many, remove_many, add_many_ordered on bins that start 500 under INT32_MAX.  The loaded
    table's wrap-free bound is INT32_MAX - 500 and the unordered add brings fewer than 500 in all: it may take its plain (wrapping) adds
    only if the bound did not count the ordered batch, whose hot keys stand at INT32_MAX by then"""
    width, depth, n = 1000, 4, 20_000
    cms = _sketch(pa, width, depth, "min", preload=I32_MAX - 500, els=2**40)
    oc = oracle.OracleCMS(width, depth)
    oc.bins[:] = I32_MAX - 500
    oc._els.value = 2**40

    def same(step):
        exp = torch.zeros_like(cms.table_tensor)
        exp[: width * depth] = torch.from_numpy(oc.bins).cuda()
        assert torch.equal(cms.table_tensor, exp), step
        assert cms.elements_added == oc.els_added, step

    keys = [_skewed_keys16(oracle, n, 5000, 40 + i) for i in range(4)]
    w1, w3, w4 = (oracle.gen_weights(20 + i, n) for i in range(3))
    w2 = np.zeros(n, dtype=np.int32)
    w2[::64] = 1 + np.arange(w2[::64].size) % 2
    assert w1.min() >= 0 and 0 < int(w2.sum()) < 500 and len({*w1.tolist()}) > 1
    fast, seq = N.get_option("cms_running_fast"), N.get_option("cms_running_sequential")
    got = cms.add_many_ordered(_give(keys[0], where), _give(w1, where))
    assert np.array_equal(_host(got).astype(np.int64), oc.add_keys(keys[0], w1, want_out=True)) and _host(got).dtype == np.int32
    same("ordered add")
    assert int((oc.bins == I32_MAX).sum()) > 0 and int((oc.bins < I32_MAX).sum()) > 0
    at_rail = oc.bins == I32_MAX
    cms.add_many(_give(keys[1], where), _give(w2, where))
    oc.add_keys(keys[1], w2)
    same("unordered add")
    assert (oc.bins[at_rail] == I32_MAX).all()
    cms.remove_many(_give(keys[2], where), _give(w3, where))
    oc.remove_keys(keys[2], w3)
    same("unordered remove")
    got = cms.add_many_ordered(_give(keys[3], where), _give(w4, where))
    assert np.array_equal(_host(got).astype(np.int64), oc.add_keys(keys[3], w4, want_out=True))
    same("second ordered add")
    assert (N.get_option("cms_running_fast"), N.get_option("cms_running_sequential")) == (fast + 2, seq)


# ------------------------------------------------------------------ g: negative weights of a device batch
@pytest.mark.parametrize("query", QUERIES)
def test_negative_device_weights_count_as_zero(pa, N, query):
    """the class refuses negative weights before anything runs, so this goes to psk_cms_add_running itself with a device batch: such a
    weight counts as 0 (csrc/psk_running.hpp, run_weight).  Results, table and elements_added equal the reference with those weights set
    to 0.  ``batch_diagnostics()`` of a CountMinSketch reports ``saturated`` only, so the violation tally is not asserted here."""
    width, depth, n = 777, 3, 3000
    rng = np.random.default_rng(23)
    cols = rng.integers(0, width, size=(n, depth))
    cols[::2, 1] = 400
    h, w = E.lift(cols, width, 11), _weights(n)
    w[::11] = -1 - (np.arange(w[::11].size) % 3)
    w[5], w[2047], w[2048] = I32_MIN, I32_MIN, -I32_MAX
    want, bins, els, _ = E.cms_running_counted(width, depth, h, np.maximum(w, 0), query, None, 100)
    cms = _sketch(pa, width, depth, query)
    assert set(cms.batch_diagnostics()) == {"saturated"}
    dh, dw = _dev(h), _dev(w)
    out = torch.full((n,), -77, dtype=torch.int64 if query == "mean-min" else torch.int32, device="cuda:0")
    e = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()  # (the sketch has a stream of its own: the tensors above are complete before it runs)
    fast, seq = N.get_option("cms_running_fast"), N.get_option("cms_running_sequential")
    rc = N.lib().psk_cms_add_running(cms._tab.handle, N.KEYS_HASHES, dh.data_ptr(), None, n, depth, dw.data_ptr(), N.DEVICE, QUERIES.index(query), 100,
                                     out.data_ptr(), e.data_ptr(), cms._tab.stream)
    assert rc == N.PSK_OK, N.last_error()
    cms.synchronize()
    assert (N.get_option("cms_running_fast"), N.get_option("cms_running_sequential")) == (fast + 1, seq)
    assert np.array_equal(out.cpu().numpy().astype(np.int64), want)
    assert torch.equal(cms.table_tensor, _expect_table(cms, bins)) and int(e.item()) == els
