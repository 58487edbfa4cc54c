"""CountMinSketchBank on the GPU: every route into the table (ids / direct atomics, ids / sort + grouped build, offsets / grouped build; the
build's routes 0 auto, 1 LDS image, 2 global atomics; host and device keys; every key layout; weighted and not) leaves the same rows, and the
rows are the reference's: byte for byte what the REAL reference exported per sketch (tests/golden/golden_cms_bank.json) and, at sizes the
reference is too slow for, what the numpy model (tests/cms_bank_model.py, checked against that fixture in tests/test_cms_bank_model.py)
computes.  The C ABI is driven directly where the Python layer would refuse the arguments or cannot express them (hostile seg / perm, a table
in the middle of a tensor)."""

import json
import struct
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import bank_model as BM  # noqa: E402  (the FNV chains of fixed / listed keys)
import cms_bank_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

G = json.loads((ROOT / "tests" / "golden" / "golden_cms_bank.json").read_text())
QUERIES = ("min", "mean", "mean-min")
I32_MAX, I32_MIN, I64_MAX = M.I32_MAX, M.I32_MIN, M.I64_MAX
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
    return bank.table_tensor.cpu().numpy()


def grouped(ids, S):
    """stable order by sketch and the offsets of the groups"""
    ids = np.asarray(ids)
    order = np.argsort(ids, kind="stable")
    offs = np.zeros(S + 1, dtype=np.int64)
    np.cumsum(np.bincount(ids, minlength=S), out=offs[1:])
    return order, offs


def blob_of(width, depth, bins, els):
    """an export: what CountMinSketch.frombytes takes"""
    return np.asarray(bins, dtype=np.int32).tobytes() + struct.pack("IIq", width, depth, els)


# every way into the table for DEVICE keys: (policy, ids or offsets, the build's route)
DEVICE_WAYS = [("direct", "ids", 0), ("direct", "offsets", 0)] + [("grouped", how, r) for how in ("ids", "offsets") for r in (0, 1, 2)]


def fill(bank, give, ids, w, policy, how, route, alt=False, split=None, dev_offs=False, dev_w=False):
    """send keys (give(index array) -> what add_many takes) with sketch `ids` and weights `w` (None: 1 each) into the bank along one way"""
    bank._add_policy, bank._route, bank._split = policy, route, split
    add = bank.add_alt_many if alt else bank.add_many
    wt = (lambda sel: None) if w is None else (lambda sel: torch.from_numpy(np.asarray(w)[sel].astype(np.int32)).cuda() if dev_w else np.asarray(w)[sel])
    if how == "ids":
        sel = np.arange(len(ids))
        add(give(sel), ids, num_els=wt(sel))
    else:
        order, offs = grouped(ids.cpu().numpy() if hasattr(ids, "is_cuda") else ids, bank.num_sketches)
        add(give(order), sketch_offsets=torch.from_numpy(offs).cuda() if dev_offs else offs, num_els=wt(order))
    bank._add_policy, bank._route, bank._split = "auto", 0, None


# ------------------------------------------------------------------ the golden streams
def want_rows(c):
    w, d = c["width"], c["depth"]
    want = np.zeros((c["sketches"], M.row_ints(w, d)), dtype=np.int32)
    for s, hx in enumerate(c["export_hex"]):
        want[s, : w * d] = np.frombuffer(bytes.fromhex(hx)[: 4 * w * d], dtype=np.int32)
    return want


@pytest.mark.parametrize("ci", range(5))
def test_golden_streams_every_route(pa, ci):
    c = G["cases"][ci]
    pool = [M.dec(e) for e in c["pool"]]
    idx = np.array([i for i, _, _ in c["stream"]])
    ids = np.array([s for _, s, _ in c["stream"]])
    wts = np.array([w for _, _, w in c["stream"]])
    S, want = c["sketches"], want_rows(c)

    def new():
        b = pa.CountMinSketchBank(S, c["width"], c["depth"])
        assert (b.width, b.depth, b.row_bytes, b.num_sketches) == (c["width"], c["depth"], 4 * want.shape[1], S)
        return b

    def giver(ix):
        def give_list(sel):
            return [pool[ix[j]] for j in sel]

        def give_dev(sel):
            blob, offs = code_points([pool[ix[j]] for j in sel])
            return (_dev(blob), _dev(offs))

        def give_alt(sel):
            return _dev(BM.hashes_list([pool[ix[j]] for j in sel], c["depth"]))
        return give_list, give_dev, give_alt

    rep = np.repeat(np.arange(len(idx)), wts)  # the same stream without weights: op (key, s, w) as w ops of weight 1
    banks = []
    for ix, sid, w in ((idx, ids, wts), (idx[rep], ids[rep], None)):
        give_list, give_dev, give_alt = giver(ix)
        for how in ("ids", "offsets"):  # host keys always go direct
            b = new()
            fill(b, give_list, sid, w, "auto", how, 0)
            assert b._last_path == "direct"
            banks.append(b)
        b = new()  # host keys, device ids
        b.add_many(give_list(np.arange(len(sid))), torch.from_numpy(sid).cuda(), num_els=w)
        banks.append(b)
        for policy, how, route in DEVICE_WAYS:
            for side in ("host", "device"):
                b = new()
                the_ids = torch.from_numpy(sid).cuda() if side == "device" and how == "ids" else sid
                fill(b, give_dev, the_ids, w, policy, how, route, split=None if route == 0 else 3, dev_offs=side == "device", dev_w=side == "device")
                assert b._last_path == policy
                banks.append(b)
        b = new()  # pre-computed hashes on the device, sorted and grouped
        fill(b, give_alt, torch.from_numpy(sid).cuda(), w, "grouped", "ids", 1, alt=True)
        banks.append(b)
    b = new()
    b.add_many(giver(idx)[0](np.arange(len(ids))), ids, num_els=wts)  # the automatic choice
    banks.append(b)
    for b in banks:
        assert np.array_equal(rows_of(b), want)
        assert b.elements_added.tolist() == c["elements_added"]
        assert b._bound.cpu().tolist() == c["elements_added"]  # (every op of a sketch could have met in one bin)
    b = banks[0]
    for s in range(S):  # the contract: the export of sketch s is the reference's, footer and all
        assert bytes(b.sketch(s)) == bytes.fromhex(c["export_hex"][s])
    # lookups: the reference's answers under the three queries, host and device
    pi, ps = np.array([i for i, _ in c["probes"]]), np.array([s for _, s in c["probes"]])
    absent = [M.dec(e) for e in c["absent"]]
    ai, as_ = np.array([i for i, _ in c["absent_probes"]]), np.array([s for _, s in c["absent_probes"]])
    for q in QUERIES:
        b.query_type = q
        assert b.query_type == q
        np_dt, t_dt = (np.int64, torch.int64) if q == "mean-min" else (np.int32, torch.int32)
        got = b.check_many([pool[i] for i in pi], ps)
        assert isinstance(got, np.ndarray) and got.dtype == np_dt and got.tolist() == c["answers_" + q]
        blob, offs = code_points([pool[i] for i in pi])
        got = b.check_many((_dev(blob), _dev(offs)), torch.from_numpy(ps).cuda())
        assert got.is_cuda and got.dtype == t_dt and got.cpu().tolist() == c["answers_" + q]
        assert b.check_many([absent[i] for i in ai], as_).tolist() == c["absent_answers_" + q]
        got = b.check_alt_many(BM.hashes_list([pool[i] for i in pi], c["depth"]), ps)
        assert got.tolist() == c["answers_" + q]
    b.query_type = "nonsense"
    assert b.query_type == "min"


@pytest.mark.parametrize("way", ["direct", "grouped0", "grouped1", "grouped2"])
def test_golden_rail_case(pa, way):
    """three adds of INT32_MAX to one key, then one add of 1: the bins stop at INT32_MAX, elements_added goes on"""
    r = G["rail"]
    b = pa.CountMinSketchBank(2, r["width"], r["depth"])
    b._add_policy = "direct" if way == "direct" else "grouped"
    b._route = 0 if way == "direct" else int(way[-1])
    key = torch.from_numpy(np.frombuffer(r["key"].encode(), dtype=np.uint8).reshape(1, -1).copy()).cuda()
    for step in r["steps"]:
        b.add_many(key, torch.tensor([1]).cuda(), num_els=torch.tensor([step["num_els"]], dtype=torch.int32).cuda())
        assert bytes(b.sketch(1)) == bytes.fromhex(step["export_hex"])
        assert b.elements_added.tolist() == [0, step["elements_added"]]
        for q in QUERIES:
            b.query_type = q
            assert b.check_many([r["key"], r["other"]], [1, 1]).tolist() == step["answers"][q]
        assert not rows_of(b)[0].any()
    assert b._bound.cpu().tolist() == [0, 3 * I32_MAX + 1] and b.batch_diagnostics()["saturated"] > 0


# ------------------------------------------------------------------ every key layout, against the model
def _layout(name, rng, n):
    """-> (host form, device form, (n, k)-hash function of the model, alt)"""
    if name.startswith("fixed"):
        L = int(name[5:])
        keys = rng.integers(0, 256, (n, L), dtype=np.uint8)
        return (lambda s: keys[s]), (lambda s: _dev(keys[s])), (lambda k: BM.hashes_fixed(keys, k)), False
    if name == "ragged":
        keys = [bytes(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8)) for _ in range(n)]
        keys[5] = b""

        def dev(s):
            blob, offs = ragged_bytes([keys[j] for j in s])
            return (_dev(blob), _dev(offs))
        return (lambda s: [keys[j] for j in s]), dev, (lambda k: BM.hashes_list(keys, k)), False
    if name == "codepoints":
        keys = ["".join(chr(int(x)) for x in rng.choice([65, 233, 955, 8364, 128512], int(rng.integers(0, 12)))) + str(i) for i in range(n)]

        def dev(s):
            blob, offs = code_points([keys[j] for j in s])
            return (_dev(blob), _dev(offs))
        return (lambda s: [keys[j] for j in s]), dev, (lambda k: BM.hashes_list(keys, k)), False
    h = rng.integers(0, 2**63, (n, 5), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 5), dtype=np.uint64)
    return (lambda s: h[s]), (lambda s: _dev(h[s])), (lambda k: h[:, :k]), True


@pytest.mark.parametrize("layout", ["fixed16", "fixed8", "fixed32", "fixed13", "fixed20", "ragged", "codepoints", "hashes"])
@pytest.mark.parametrize("weighted", [False, True])
def test_every_layout_every_route(pa, layout, weighted):
    rng = np.random.default_rng(11)
    S, n, width, depth = 37, 3000, (61 if weighted else 64), 5  # a non-power-of-two width next to a power of two
    host, dev, hashes, alt = _layout(layout, rng, n)
    ids = rng.integers(0, S, n)
    ids[ids == 9] = 10  # an empty sketch
    w = rng.choice([0, 1, 1, 3, 70000], n) if weighted else None
    new = lambda: pa.CountMinSketchBank(S, width, depth)  # noqa: E731
    want = M.bank_rows(S, width, depth, hashes(depth), ids, w)
    els = M.bank_els(S, ids, w)
    banks = []
    for how in ("ids", "offsets"):
        b = new()
        fill(b, host, ids, w, "auto", how, 0, alt)
        banks.append(b)
    for policy, how, route in DEVICE_WAYS:
        b = new()
        fill(b, dev, torch.from_numpy(ids).cuda() if how == "ids" else ids, w, policy, how, route, alt, split=2 if route == 1 else None, dev_offs=route == 2,
             dev_w=route != 0)
        banks.append(b)
    for b in banks:
        assert np.array_equal(rows_of(b), want)
        assert b.elements_added.tolist() == els and b._bound.cpu().tolist() == els
    # lookups along both sides; every key under its own id and under its neighbour's
    b = banks[-1]
    check = b.check_alt_many if alt else b.check_many
    for q in QUERIES:
        b.query_type = q
        for shift in (0, 1):
            pid = (ids + shift) % S
            model = M.bank_check(want, width, depth, hashes(depth), pid, q, els)
            assert np.array_equal(check(host(np.arange(n)), pid), model)
            assert np.array_equal(check(dev(np.arange(n)), torch.from_numpy(pid).cuda()).cpu().numpy(), model)
    assert (model == 0).any() and (model != 0).any()


def test_chunked_calls_and_the_automatic_choice(pa, monkeypatch):
    rng = np.random.default_rng(2)
    S, n, width, depth = 11, 2500, 100, 4
    keys = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    ids, w = rng.integers(0, S, n), rng.integers(0, 9, n)
    h = BM.hashes_fixed(keys, depth)
    want = M.bank_rows(S, width, depth, h, ids, w)
    for give in (lambda: keys, lambda: _dev(keys)):
        bank = pa.CountMinSketchBank(S, width, depth)
        bank._CHUNK = 1000  # three engine calls per batch
        bank._add_policy = "direct"
        bank.add_many(give(), ids, num_els=w)
        assert np.array_equal(rows_of(bank), want)
        got = bank.check_many(give(), (ids + 1) % S)
        got = got.cpu().numpy() if hasattr(got, "is_cuda") else got
        assert np.array_equal(got, M.bank_check(want, width, depth, h, (ids + 1) % S))
    from pyprobables_amd import cmsbank

    bank = pa.CountMinSketchBank(S, width, depth)
    bank.add_many(_dev(keys), _dev(ids))
    assert bank._last_path == "direct"  # below the threshold
    monkeypatch.setattr(cmsbank, "CMS_BANK_GROUP_MIN_KEYS", 1000)
    bank.add_many(_dev(keys), _dev(ids))
    assert bank._last_path == "grouped"
    assert np.array_equal(rows_of(bank), M.bank_rows(S, width, depth, np.concatenate([h, h]), np.concatenate([ids, ids])))
    wide = pa.CountMinSketchBank(2, 4097, 4)
    wide.add_many(_dev(keys), _dev(ids % 2))
    assert wide._last_path == "direct"  # rows over the image's cap never sort


# ------------------------------------------------------------------ geometry seams
def _keys16(rng, n):
    return rng.integers(0, 256, (n, 16), dtype=np.uint8)


def _all_ways(pa, S, width, depth, keys, ids, w, ways=DEVICE_WAYS, split=None):
    h = BM.hashes_fixed(keys, depth)
    want = M.bank_rows(S, width, depth, h, ids, w)
    for policy, how, route in ways:
        b = pa.CountMinSketchBank(S, width, depth)
        fill(b, lambda s: _dev(keys[s]), ids, w, policy, how, route, split=split, dev_offs=True, dev_w=w is not None)
        assert np.array_equal(rows_of(b), want), (policy, how, route)
    return b, h, want


def test_pad_ints_stay_zero(pa):
    """(7, 3): 21 ints in a row of 24"""
    rng = np.random.default_rng(3)
    S, n = 70, 5000
    keys, ids = _keys16(rng, n), rng.integers(0, S, n)
    b, _, want = _all_ways(pa, S, 7, 3, keys, ids, rng.integers(0, 5, n))
    assert b.row_bytes == 96 and not want[:, 21:].any() and want[:, :21].any()
    assert not rows_of(b)[:, 21:].any()


def test_the_image_cap(pa):
    """width * depth == 16384 takes the image (64 KiB of LDS); 4097 x 4 does not, and route 1 is refused there"""
    rng = np.random.default_rng(5)
    n = 6000
    keys, ids = _keys16(rng, n), rng.integers(0, 3, n)
    _all_ways(pa, 3, 4096, 4, keys, ids, None)
    _all_ways(pa, 3, 2048, 8, keys, ids, rng.integers(0, 3, n), ways=[("grouped", "offsets", 1), ("grouped", "ids", 0)])
    over = [wy for wy in DEVICE_WAYS if wy[2] != 1]
    _all_ways(pa, 3, 4097, 4, keys, ids, None, ways=over)
    b = pa.CountMinSketchBank(3, 4097, 4)
    b._add_policy, b._route = "grouped", 1
    with pytest.raises(ValueError, match="do not fit the LDS image"):
        b.add_many(_dev(keys), _dev(ids))
    assert not rows_of(b).any() and b.elements_added.tolist() == [0, 0, 0] and b._bound.cpu().tolist() == [0, 0, 0]


@pytest.mark.parametrize("width,depth", [(50, 1), (33, 64), (1, 3), (63, 2), (64, 2)])
def test_depths_and_widths(pa, width, depth):
    rng = np.random.default_rng(6)
    S, n = 9, 2000
    keys, ids, w = _keys16(rng, n), rng.integers(0, S, n), rng.integers(0, 4, n)
    b, h, want = _all_ways(pa, S, width, depth, keys, ids, w)
    els = M.bank_els(S, ids, w)
    for q in QUERIES:
        b.query_type = q
        if width == 1 and q == "mean-min":  # as CountMeanMinSketch of this package: the query divides by width - 1
            with pytest.raises(ValueError, match="width >= 2"):
                b.check_many(_dev(keys), _dev(ids))
            continue
        got = b.check_many(_dev(keys), _dev(ids)).cpu().numpy()
        assert np.array_equal(got, M.bank_check(want, width, depth, h, ids, q, els))


def test_depth_65_is_refused(pa):
    with pytest.raises(pa.NotSupportedError, match="at most 64 deep"):
        pa.CountMinSketchBank(3, 10, 65)


def test_more_sketches_than_the_grid(pa):
    rng = np.random.default_rng(7)
    S, n = 4096 + 37, 30000
    keys, ids = _keys16(rng, n), rng.integers(0, S, n)
    ids[:3] = [0, 4096, S - 1]
    b, _, want = _all_ways(pa, S, 8, 3, keys, ids, None, ways=[("grouped", "offsets", 1), ("grouped", "ids", 0), ("direct", "ids", 0)])
    assert want[4096:].any()
    r = b.reduce([[s] for s in range(S)])
    assert np.array_equal(rows_of(r), want)


def test_splits_empty_parts_and_empty_batches(pa):
    rng = np.random.default_rng(8)
    S, n = 5, 700
    keys = _keys16(rng, n)
    ids = np.sort(rng.choice([0, 1, 4], n))  # sketches 2 and 3 get nothing
    ids[:2] = 0
    ids[2:3] = 1  # sketch 1: one key -- fewer than any split
    ids[3:] = 4
    for split in (1, 2, 5, 64, 1000):  # 1000: more parts than the largest segment has keys
        for route in (0, 1, 2):
            _all_ways(pa, S, 40, 3, keys, ids, None, ways=[("grouped", "offsets", route)], split=split)
    b = pa.CountMinSketchBank(S, 40, 3)
    for policy in ("direct", "grouped"):
        b._add_policy = policy
        b.add_many(_dev(np.zeros((0, 16), dtype=np.uint8)), _dev(np.zeros(0, dtype=np.int64)))
        b.add_many(_dev(np.zeros((0, 16), dtype=np.uint8)), sketch_offsets=np.zeros(S + 1, dtype=np.int64))
        b.add_many([], [])
    assert b.check_many([], []).shape == (0,) and not rows_of(b).any() and b.elements_added.tolist() == [0] * S


def test_a_table_beyond_4_gib(pa):
    """rows of 64 KiB: row 65536 starts at byte 2^32"""
    width, depth, S = 4096, 4, 65538
    free, _ = torch.cuda.mem_get_info()
    assert free > 10 * 2**30, "the device has no room for the 4 GiB bank and the bank its reduce allocates"
    b = pa.CountMinSketchBank(S, width, depth)
    assert b.row_bytes == 65536
    rng = np.random.default_rng(9)
    n = 4000
    keys = _keys16(rng, n)
    targets = np.array([0, 65535, 65536, 65537])
    ids = targets[rng.integers(0, 4, n)]
    h = BM.hashes_fixed(keys, depth)
    small = M.bank_rows(4, width, depth, h, np.searchsorted(targets, ids))
    for policy, how, route in [("direct", "ids", 0), ("grouped", "ids", 1), ("grouped", "ids", 2)]:
        b.clear()
        fill(b, lambda s: _dev(keys[s]), _dev(ids), None, policy, how, route)
        assert np.array_equal(b.table_tensor[torch.from_numpy(targets).cuda()].cpu().numpy(), small)
        assert int(torch.count_nonzero(b._table)) == int(np.count_nonzero(small))
    got = b.check_many(_dev(keys), _dev(ids)).cpu().numpy()
    assert np.array_equal(got, M.bank_check(small, width, depth, h, np.searchsorted(targets, ids)))
    r = b.reduce([[65537, 65536], [0]])
    assert np.array_equal(rows_of(r)[0].astype(np.int64), small[3].astype(np.int64) + small[2]) and np.array_equal(rows_of(r)[1], small[0])


# ------------------------------------------------------------------ rails
@pytest.mark.parametrize("way", [("direct", "ids", 0), ("grouped", "ids", 0), ("grouped", "offsets", 1), ("grouped", "offsets", 2)])
def test_int32_max_weights_repeated(pa, way):
    rng = np.random.default_rng(12)
    S, n, width, depth = 3, 600, 16, 3
    keys, ids = _keys16(rng, n), rng.integers(0, S, n)
    w = rng.choice([I32_MAX, I32_MAX, 1, 0], n)
    b = pa.CountMinSketchBank(S, width, depth)
    h = BM.hashes_fixed(keys, depth)
    want, els = None, None
    for _ in range(2):
        fill(b, lambda s: _dev(keys[s]), ids, w, *way, dev_w=True)
        want, els = M.bank_rows(S, width, depth, h, ids, w, want), M.bank_els(S, ids, w, els)
        assert np.array_equal(rows_of(b), want) and b.elements_added.tolist() == els
    assert (want == I32_MAX).any() and want.max() == I32_MAX and want.min() >= 0


@pytest.mark.parametrize("start", [I32_MAX - 2, 0])
def test_the_image_swept_onto_loaded_bins(pa, start):
    """unweighted keys through the image onto bins that set_sketch loaded: at INT32_MAX - 2 the bound passes the rail and the sweep clamps,
    at 0 the sweep is the plain add"""
    rng = np.random.default_rng(13)
    width, depth, n = 8, 3, 40
    cms = pa.CountMinSketch.frombytes(blob_of(width, depth, np.full(width * depth, start), 5))
    b = pa.CountMinSketchBank(2, width, depth)
    b.set_sketch(1, cms)
    assert b._bound.cpu().tolist() == [0, start] and b.elements_added.tolist() == [0, 5]
    keys = _keys16(rng, n)
    b._add_policy, b._route, b._split = "grouped", 1, 1
    b.add_many(_dev(keys), sketch_offsets=_dev(np.array([0, 0, n])))
    hits = M.bank_rows(1, width, depth, BM.hashes_fixed(keys, depth), np.zeros(n, dtype=np.int64))[0].astype(np.int64)
    assert hits.max() >= 3
    want = np.minimum(start + hits, I32_MAX)
    assert np.array_equal(rows_of(b)[1], want) and not rows_of(b)[0].any()
    assert b._bound.cpu().tolist() == [0, start + n] and b.elements_added.tolist() == [0, 5 + n]
    assert (b.batch_diagnostics()["saturated"] > 0) == (start != 0)


def test_elements_added_clamps_at_int64_max(pa):
    width, depth = 8, 3
    cms = pa.CountMinSketch.frombytes(blob_of(width, depth, np.zeros(width * depth), I64_MAX - 5))
    b = pa.CountMinSketchBank(2, width, depth)
    b.set_sketch(0, cms)
    for policy in ("direct", "grouped"):
        b._add_policy = policy
        b.add_many(_dev(_keys16(np.random.default_rng(1), 4)), _dev(np.zeros(4, dtype=np.int64)), num_els=3)
        assert b.elements_added.tolist() == [I64_MAX, 0]
    assert bytes(b.sketch(0))[-8:] == struct.pack("q", I64_MAX)
    assert rows_of(b)[0].sum() == 2 * 4 * 3 * depth


def test_a_hot_key_in_one_part(pa):
    """100 000 copies of one key in one grouped part: every add meets the same `depth` LDS counters"""
    n, width, depth = 100_000, 2048, 5
    key = np.arange(16, dtype=np.uint8).reshape(1, 16)
    keys = _dev(np.repeat(key, n, axis=0))
    for route in (1, 0, 2):
        b = pa.CountMinSketchBank(1, width, depth)
        b._add_policy, b._route, b._split = "grouped", route, 1
        b.add_many(keys, sketch_offsets=[0, n])
        rows = rows_of(b)
        assert int(b.check_many(key, [0])[0]) == n
        assert rows.sum() == n * depth and np.count_nonzero(rows) == depth and b.elements_added.tolist() == [n]


# ------------------------------------------------------------------ hostile metadata
def test_unchecked_ids_beyond_the_bank_are_skipped(pa):
    rng = np.random.default_rng(14)
    S, n, width, depth = 6, 3000, 30, 4
    keys, ids, w = _keys16(rng, n), rng.integers(0, S + 3, n), rng.integers(-2, 5, n)
    h = BM.hashes_fixed(keys, depth)
    want, els = M.bank_rows(S, width, depth, h, ids, w), M.bank_els(S, ids, w)
    for policy in ("direct", "grouped"):
        b = pa.CountMinSketchBank(S, width, depth)
        b._add_policy = policy
        with pytest.raises(ValueError, match="sketch ids must lie in"):
            b.add_many(_dev(keys), _dev(ids), num_els=_dev(np.maximum(w, 0).astype(np.int32)))
        with pytest.raises(ValueError, match="num_els must be >= 0"):
            b.add_many(_dev(keys), _dev(ids % S), num_els=_dev(w.astype(np.int32)))
        with pytest.raises(ValueError, match="num_els must be >= 0"):
            b.add_many(keys, ids % S, num_els=w)
        assert not rows_of(b).any() and b.elements_added.tolist() == [0] * S and b._bound.cpu().tolist() == [0] * S
        b.add_many(_dev(keys), _dev(ids), num_els=_dev(w.astype(np.int32)), validate=False)  # ids beyond the bank: skipped; negative weights: 0
        assert np.array_equal(rows_of(b), want) and b.elements_added.tolist() == els and b._bound.cpu().tolist() == els
        b.query_type = "mean"
        got = b.check_many(_dev(keys), _dev(ids), validate=False).cpu().numpy()
        assert np.array_equal(got, M.bank_check(want, width, depth, h, ids, "mean"))


def c_build(N, tab, S, width, depth, keys, n, seg, perm, w, bound, split, route):
    return N.lib().psk_cms_bank_build(tab, S, width, depth, N.KEYS_FIXED, keys.data_ptr(), None, n, 16, seg.data_ptr(), perm.data_ptr() if perm is not None else None,
                                      w.data_ptr() if w is not None else None, bound.data_ptr() if bound is not None else None, None, split, route,
                                      torch.cuda.current_device(), None)


def test_hostile_seg_and_perm_read_and_write_nothing_outside(pa, N):
    """seg ending beyond n, perm entries beyond n, a table in the MIDDLE of a tensor: the table equals the model's for the valid part and the
    words around it stay"""
    rng = np.random.default_rng(15)
    S, n, width, depth, guard = 8, 2000, 7, 3, 8
    ri = M.row_ints(width, depth)
    keys = _keys16(rng, n)
    dkeys = _dev(keys)
    w = rng.integers(0, 6, n).astype(np.int32)
    perm = rng.permutation(n).astype(np.uint32)
    perm[::17] = n + np.arange(len(perm[::17]), dtype=np.uint32) * 1000  # entries at and beyond n: skipped
    perm[5] = 0xFFFFFFFF
    seg = np.linspace(0, n, S + 1).astype(np.uint64)
    seg[-1] = n + 5000  # ends beyond n: clamped
    seg[3] = seg[2]     # an empty segment
    pos_ids = np.searchsorted(seg[1:].astype(np.int64), np.arange(n), side="right")
    valid = perm < n
    h = BM.hashes_fixed(keys, depth)
    want = M.bank_rows(S, width, depth, h[perm[valid]], pos_ids[valid], w[perm[valid]])
    bound = _dev(np.full(S, 10**6, dtype=np.int64))
    for route in (0, 1, 2):
        for split in (1, 3):
            for bnd in (bound, None):
                big = torch.full((guard + S * ri + guard,), SENTINEL, dtype=torch.int32, device="cuda")
                big[guard:guard + S * ri] = 0
                N.check(c_build(N, big.data_ptr() + 4 * guard, S, width, depth, dkeys, n, _dev(seg), _dev(perm), _dev(w), bnd, split, route))
                got = big.cpu().numpy()
                assert (got[:guard] == SENTINEL).all() and (got[-guard:] == SENTINEL).all()
                assert np.array_equal(got[guard:-guard].reshape(S, ri), want), (route, split)
    seg[:] = n + 1  # nothing valid at all
    seg[0] = 2**40
    tab = torch.zeros(S * ri, dtype=torch.int32, device="cuda")
    N.check(c_build(N, tab.data_ptr(), S, width, depth, dkeys, n, _dev(seg), None, None, None, 2, 0))
    assert not tab.any()


# ------------------------------------------------------------------ reduce
def _loaded(pa, j):
    b = pa.CountMinSketchBank(len(j["members_hex"]), j["width"], j["depth"])
    m = M.BankModel(len(j["members_hex"]), j["width"], j["depth"])
    for s, hx in enumerate(j["members_hex"]):
        b.set_sketch(s, pa.CountMinSketch.frombytes(bytes.fromhex(hx)))
        m.load(s, bytes.fromhex(hx))
    return b, m


def test_reduce_the_golden_folds(pa):
    j = G["joins"]
    b, m = _loaded(pa, j)
    assert np.array_equal(rows_of(b)[:, : j["width"] * j["depth"]], m.bins) and b.elements_added.tolist() == m.els
    assert b._bound.cpu().tolist() == [max(0, int(r.max())) for r in m.bins]
    groups = [f["members"] for f in j["folds"]]
    for form in ("lists", "host", "device"):
        offs = np.zeros(len(groups) + 1, dtype=np.int64)
        np.cumsum([len(g) for g in groups], out=offs[1:])
        flat = np.concatenate(groups)
        r = b.reduce(groups if form == "lists" else (flat, offs) if form == "host" else (_dev(flat), _dev(offs)))
        assert r.num_sketches == len(groups) and (r.width, r.depth) == (b.width, b.depth)
        for g, f in enumerate(j["folds"]):
            assert bytes(r.sketch(g)) == bytes.fromhex(f["export_hex"])
        assert r.elements_added.tolist() == [f["elements_added"] for f in j["folds"]]
        assert r._bound.cpu().tolist() == [min(sum(max(0, int(m.bins[s].max())) for s in g), I64_MAX) for g in groups]
    # interop: the chained join of the single sketches agrees
    for g in (groups[3], groups[5]):
        acc = pa.CountMinSketch(width=b.width, depth=b.depth)
        for s in g:
            acc.join(b.sketch(s))
        assert bytes(acc) == bytes(b.reduce([g]).sketch(0))


def test_reduce_members_beyond_the_bank_and_empty_groups(pa):
    j = G["joins"]
    b, m = _loaded(pa, j)
    S = b.num_sketches
    groups = [[2, S + 4, 1], [], [S], [0]]
    with pytest.raises(ValueError, match="sketch ids must lie in"):
        b.reduce(groups)
    offs = np.array([0, 3, 3, 4, 5])
    flat = np.array([2, S + 4, 1, S, 0])
    want = m.reduce(groups)
    for members in (flat, _dev(flat)):
        r = b.reduce((members, _dev(offs)), validate=False)
        assert np.array_equal(rows_of(r)[:, : b.width * b.depth], want.bins) and r.elements_added.tolist() == want.els
        assert not rows_of(r)[1].any() and not rows_of(r)[2].any()
    with pytest.raises(ValueError, match="non-decreasing"):
        b.reduce((flat, np.array([0, 4, 3, 5])))


def test_reduce_beyond_the_grid_and_its_refusals(pa, N):
    """2100 groups x 2 row pieces (rows of 300 16-byte pieces) > the grid cap of 4096; bins on both rails in the sources"""
    rng = np.random.default_rng(16)
    S, width, depth, Gn = 40, 600, 2, 2100
    b = pa.CountMinSketchBank(S, width, depth)
    assert b.row_bytes == 4800
    bins = rng.integers(-50, 50, (S, width * depth)).astype(np.int64)
    bins[rng.random(bins.shape) < 0.02] = I32_MAX
    bins[rng.random(bins.shape) < 0.02] = I32_MIN
    bins[rng.random(bins.shape) < 0.05] = I32_MAX - 20
    bins[rng.random(bins.shape) < 0.05] = I32_MIN + 20
    b.table_tensor.copy_(_dev(bins.astype(np.int32)))
    els = rng.integers(-(2**62), 2**62, S)
    b._els.copy_(_dev(els))
    m = M.BankModel(S, width, depth)
    m.bins[:], m.els = bins, els.tolist()
    groups = [rng.integers(0, S, int(rng.integers(0, 6))).tolist() for _ in range(Gn)]
    r = b.reduce(groups)
    want = m.reduce(groups)
    assert np.array_equal(rows_of(r), want.bins) and r.elements_added.tolist() == want.els
    assert (want.bins == I32_MAX).any() and (want.bins == I32_MIN).any()
    seg, mem = _dev(np.array([0, 1], dtype=np.uint64)), _dev(np.array([0], dtype=np.uint32))
    dev = torch.cuda.current_device()
    tab = b._table.data_ptr()
    for dst in (tab, tab + b.row_bytes * (S - 1), tab - b.row_bytes + 16):
        rc = N.lib().psk_cms_bank_reduce(tab, None, S, width, depth, seg.data_ptr(), mem.data_ptr(), 1, dst, None, dev, None)
        assert rc == N.PSK_EINVAL and "dst overlaps src" in N.last_error()
    assert np.array_equal(rows_of(b), bins)


# ------------------------------------------------------------------ interop with the single sketch
def test_set_sketch_and_sketch_round_trip(pa):
    rng = np.random.default_rng(17)
    width, depth, n = 100, 4, 3000
    keys = _keys16(rng, n)
    cms = pa.CountMinSketch(width=width, depth=depth)
    cms.add_many(_dev(keys), rng.integers(1, 9, n).astype(np.int32))
    cms.remove_many(_dev(keys[:500]), 200)  # negative bins
    assert cms.table_tensor.min().item() < 0
    b = pa.CountMinSketchBank(3, width, depth)
    b.set_sketch(2, cms)
    assert bytes(b.sketch(2)) == bytes(cms) and b._bound.cpu().tolist() == [0, 0, int(cms.table_tensor.max().item())]
    for q in QUERIES:
        b.query_type = cms.query_type = q
        assert np.array_equal(b.check_many(_dev(keys), _dev(np.full(n, 2))).cpu().numpy(), cms.check_many(_dev(keys)).cpu().numpy())
        assert np.array_equal(b.check_many(keys[:50], np.full(50, 2)), cms.check_many(keys[:50]))
        assert not b.check_many(keys[:50], np.full(50, 1)).any()
        assert b.sketch(2).query_type == q
    b.add_many(_dev(keys[:10]), _dev(np.full(10, 2)), num_els=4)
    cms.add_many(_dev(keys[:10]), 4)
    assert bytes(b.sketch(2)) == bytes(cms)
    b.clear(2)
    assert not rows_of(b).any() and b.elements_added.tolist() == [0, 0, 0] and b._bound.cpu().tolist() == [0, 0, 0]
    b.set_sketch(0, cms)
    b.clear()
    assert not rows_of(b).any() and b.elements_added.tolist() == [0, 0, 0]
    with pytest.raises(pa.CountMinSketchError, match="mismatched"):
        b.set_sketch(0, pa.CountMinSketch(width=width, depth=depth + 1))
    with pytest.raises(pa.CountMinSketchError, match="mismatched"):
        b.set_sketch(0, pa.CountMinSketch(width=width, depth=depth, hash_function=lambda key, d: [7 + i for i in range(d)]))
    with pytest.raises(TypeError):
        b.set_sketch(0, "cms")
    with pytest.raises(IndexError, match="sketch 3 out of range"):
        b.sketch(3)


def test_a_host_hash_function_travels_as_hashes(pa):
    def hf(key, depth):
        base = sum(key.encode() if isinstance(key, str) else bytes(key))
        return [base * 2654435761 + 97 * i for i in range(depth)]

    keys = [f"k{i}" for i in range(200)]
    ids = np.arange(200) % 4
    b = pa.CountMinSketchBank(4, 50, 3, hash_function=hf)
    b.add_many(keys, ids, num_els=2)
    want = M.bank_rows(4, 50, 3, np.array([hf(k, 3) for k in keys], dtype=np.uint64), ids, np.full(200, 2))
    assert np.array_equal(rows_of(b), want)
    cms = pa.CountMinSketch(width=50, depth=3, hash_function=hf)
    cms.add_many([k for k, s in zip(keys, ids) if s == 1], 2)
    assert bytes(b.sketch(1)) == bytes(cms)


def test_unchecked_ids_beyond_32_bits_alias_no_sketch(pa):
    """an id of 2^32 + 1 under validate=False is an id beyond the bank: not sketch 1 of the engine's 32-bit words"""
    rng = np.random.default_rng(18)
    S, n, width, depth = 4, 500, 30, 3
    keys = _keys16(rng, n)
    ids = rng.integers(0, S, n)
    far = ids.copy()
    far[::3] += 2**32
    far[1::7] = -1 - ids[1::7]
    h = BM.hashes_fixed(keys, depth)
    want, els = M.bank_rows(S, width, depth, h, far), M.bank_els(S, far)
    for policy in ("direct", "grouped"):
        b = pa.CountMinSketchBank(S, width, depth)
        b._add_policy = policy
        b.add_many(_dev(keys), _dev(far), validate=False)
        assert np.array_equal(rows_of(b), want) and b.elements_added.tolist() == els and b._bound.cpu().tolist() == els
        assert np.array_equal(b.check_many(_dev(keys), _dev(far), validate=False).cpu().numpy(), M.bank_check(want, width, depth, h, far))


def test_device_weights_are_read_back_with_the_offsets(pa):
    rng = np.random.default_rng(19)
    S, n, width, depth = 4, 400, 30, 3
    keys = _dev(_keys16(rng, n))
    offs = _dev(np.array([0, 100, 100, 250, 400]))
    w = rng.integers(0, 5, n)
    neg, big = w.copy(), w.copy()
    neg[7], big[9] = -3, 2**31
    b = pa.CountMinSketchBank(S, width, depth)
    for bad, exc in ((_dev(neg.astype(np.int32)), ValueError), (_dev(neg), ValueError), (_dev(big), OverflowError)):
        with pytest.raises(exc, match="num_els"):
            b.add_many(keys, sketch_offsets=offs, num_els=bad)
        with pytest.raises(exc, match="num_els"):
            b.add_many(keys, torch.zeros(n, dtype=torch.int64, device="cuda"), num_els=bad)
    with pytest.raises(ValueError, match="sketch_offsets must be non-decreasing"):
        b.add_many(keys, sketch_offsets=_dev(np.array([0, 100, 50, 250, 400])), num_els=_dev(w))
    with pytest.raises(TypeError):
        b.add_many(keys, sketch_offsets=offs, num_els=torch.ones(n, device="cuda"))
    assert not rows_of(b).any() and b.elements_added.tolist() == [0] * S and b._bound.cpu().tolist() == [0] * S
    b.add_many(keys, sketch_offsets=offs, num_els=_dev(big), validate=False)  # unchecked: clamped into [0, INT32_MAX]
    ids = np.repeat(np.arange(S), [100, 0, 150, 150])
    h = BM.hashes_fixed(keys.cpu().numpy(), depth)
    assert np.array_equal(rows_of(b), M.bank_rows(S, width, depth, h, ids, np.minimum(big, I32_MAX)))
    assert b.elements_added.tolist() == M.bank_els(S, ids, np.minimum(big, I32_MAX))


def test_a_refused_launch_puts_the_bookkeeping_back(pa, monkeypatch):
    rng = np.random.default_rng(20)
    S, n, width, depth = 4, 300, 30, 3
    keys, ids = _dev(_keys16(rng, n)), _dev(rng.integers(0, S, n))
    b = pa.CountMinSketchBank(S, width, depth)
    b.add_many(keys, ids, num_els=2)
    rows, els, bound = rows_of(b), b.elements_added.tolist(), b._bound.cpu().tolist()
    b._add_policy, b._split = "grouped", 70000  # the engine refuses the split, after the bookkeeping has moved
    with pytest.raises(ValueError, match="split must be"):
        b.add_many(keys, ids)
    assert np.array_equal(rows_of(b), rows) and b.elements_added.tolist() == els and b._bound.cpu().tolist() == bound
    # rows of 2^32 ints or more: the build and the reduce kernels index a row with 32 bits (refusals of the C entries: test_cms_bank_model.py)
    from pyprobables_amd import cmsbank

    monkeypatch.setattr(cmsbank, "CMS_BANK_BUILD_MAX_INTS", 64)
    b._split = None
    with pytest.raises(ValueError, match="fewer than 2\\^32 ints"):
        b.add_many(keys, ids)
    with pytest.raises(pa.NotSupportedError, match="fewer than 2\\^32 ints"):
        b.reduce([[0, 1]])
    assert b.elements_added.tolist() == els
    b._add_policy = "auto"
    order, offs = grouped(ids.cpu().numpy(), S)
    b.add_many(keys[_dev(order)], sketch_offsets=_dev(offs))
    assert b._last_path == "direct" and b.elements_added.tolist() == [e + c for e, c in zip(els, np.diff(offs).tolist())]
