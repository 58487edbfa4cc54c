"""The exact ordered CountMinSketch batch with removes in it (psk_cms_update_running, the signed passes of csrc/psk_running.hpp) and the
methods on top: ``update_many_ordered`` / ``remove_many_ordered``, ``StreamThreshold.update_many`` / ``remove_many``.

Every op's return value, the table, elements_added and the PSK_CTR_SATURATED tally must be what the reference's loop of ``add`` /
``remove`` leaves (countminsketch.py:257-321): tests/golden/golden_signed_running.json is the real reference, tests/signed_running_model.py
its model (tied to the reference by tests/test_signed_running_model.py), ``update_ordered`` the sequential kernel on a twin sketch."""

import hashlib
import json
import struct
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import hitters_recipe as R  # noqa: E402
import signed_running_model as M  # noqa: E402

CASES = json.loads((ROOT / "tests" / "golden" / "golden_signed_running.json").read_text())["cases"]
I32_MIN, I32_MAX = M.I32
I64_MIN, I64_MAX = M.I64
FOOTER = struct.Struct("IIq")
CYCLE = (I32_MAX, I32_MAX, -I32_MAX, I32_MIN, I32_MIN, 0, 1, -1)  # (from any start: INT32_MAX by a clamp, 0, INT32_MIN exactly, INT32_MIN by a clamp)


def _SM(x):
    """hitters_recipe.sm over a uint64 array"""
    with np.errstate(over="ignore"):
        z = np.asarray(x, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


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
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(x):
    return x.cpu().numpy() if hasattr(x, "is_cuda") else np.asarray(x)


def _bins(cms):
    return cms.table_tensor.cpu().numpy()[: cms.width * cms.depth].astype(np.int64)


def _sat(cms, N):
    return cms._tab.counters()[N.CTR_SATURATED]


def rnd(n, salt):
    """n 64-bit numbers from integers alone"""
    return _SM(np.arange(n, dtype=np.uint64) + np.uint64(salt * 1000003)) if n else np.zeros(0, dtype=np.uint64)


def hashes_of(n, depth, pool, salt):
    """uint64[n][depth]: the hashes of n ops over `pool` distinct keys (a key's row is a function of the key alone)"""
    key = rnd(n, salt) % np.uint64(pool)
    with np.errstate(over="ignore"):
        return _SM((key[:, None] * np.uint64(131) + np.arange(depth, dtype=np.uint64)[None, :]).ravel()).reshape(n, depth)


def mixed_weights(n, salt):
    """signed int32 weights: a third from the rail cycle, a third anywhere in int32, a third small"""
    r = rnd(n, salt + 77)
    kind = (r >> np.uint64(40)) % np.uint64(3)
    cyc = np.array(CYCLE, dtype=np.int64)[(r % np.uint64(len(CYCLE))).astype(np.int64)]
    wide = (r % np.uint64(2**32)).astype(np.int64) - 2**31
    small = (r % np.uint64(11)).astype(np.int64) - 5
    return np.where(kind == 0, cyc, np.where(kind == 1, wide, small))


def near_rails(cells, below=3):
    return np.where(np.arange(cells) % 2 == 0, I32_MAX - below, I32_MIN + below).astype(np.int32)


def sketch(pa, width, depth, query="min", bins=None, els=0, cls="CountMinSketch", **kw):
    klass = getattr(pa, cls)
    if bins is None and els == 0:
        sk = klass(width=width, depth=depth, device=0, **kw)
    else:
        b = np.zeros(width * depth, dtype=np.int32) if bins is None else np.asarray(bins, dtype=np.int32)
        sk = klass.frombytes(b.tobytes() + FOOTER.pack(width, depth, els), device=0, **kw)
    sk.query_type = query
    return sk


def give(h, w, where):
    """the (hashes, weights) arguments of update_alt_many_ordered on either side"""
    w32 = None if w is None else np.asarray(w).astype(np.int32)
    if where == "device":
        return _dev(h.view(np.int64)), None if w32 is None else _dev(w32)
    return h, w32


def run_and_check(pa, N, width, depth, query, h, w, bins, els, where):
    """one call of update_alt_many_ordered against the model: results, table, elements_added, the saturation tally"""
    want, table, wels, clamps = M.signed_batch(width, depth, h, w, query, bins, els)
    sk = sketch(pa, width, depth, query, bins, els)
    sat0 = _sat(sk, N)
    got = sk.update_alt_many_ordered(*give(h, w, where))
    assert (got.is_cuda if where == "device" else isinstance(got, np.ndarray)) and got.dtype == (
        (torch.int64 if query == "mean-min" else torch.int32) if where == "device" else (np.int64 if query == "mean-min" else np.int32))
    assert np.array_equal(_host(got).astype(np.int64), np.asarray(want[query], dtype=np.int64))
    assert np.array_equal(_bins(sk), table)
    assert sk.elements_added == wels
    assert _sat(sk, N) - sat0 == clamps
    return sk, want[query], clamps


# ------------------------------------------------------------------ 1. fixture parity
def case_sketch(pa, case):
    name, _, _ = case["cls"].partition(":")
    kw = {"threshold": case["param"]} if name == "StreamThreshold" else {}
    p = case["preload"]
    return sketch(pa, case["width"], case["depth"], case["query"], M.preload_bins(case), p["elements_added"] if p else 0, name, **kw)


def case_keys(case, where):
    """str cases: the list of str (host) or its (n, 8) uint8 matrix on the device; key16 cases: the (n, 16) uint8 matrix on either side"""
    keys = R.stream_keys(case)
    if case["key_kind"] == "str" and where == "host":
        return keys
    mat = R.keys_matrix(keys)
    return _dev(mat) if where == "device" else mat


def check_case_end(case, sk, results, N, sat0):
    assert M.results_sha(_host(results)) == case["results_sha256"]
    assert sk.elements_added == case["elements_added"]
    assert hashlib.sha256(bytes(sk)).hexdigest() == case["export_sha256"]
    if case["bins"] is not None:
        assert _bins(sk).tolist() == case["bins"]
    assert _sat(sk, N) - sat0 == case["clamps"]
    if "tracked" in case:
        d = sk.meets_threshold
        if case["key_kind"] == "str":  # (array / tensor batches track bytes)
            d = {k.decode("latin-1") if isinstance(k, bytes) else k: v for k, v in d.items()}
        assert R.dict_pairs(case, d) == case["tracked"]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_one_batch(pa, N, case, where):
    sk = case_sketch(pa, case)
    w = M.stream_weights(case).astype(np.int32)
    fast0, sat0 = N.get_option("cms_update_running_fast"), _sat(sk, N)
    call = sk.update_many if "tracked" in case else sk.update_many_ordered
    res = call(case_keys(case, where), _dev(w) if where == "device" else w)
    assert (res.is_cuda if where == "device" else isinstance(res, np.ndarray)) and _host(res).dtype == (np.int64 if case["query"] == "mean-min" else np.int32)
    assert N.get_option("cms_update_running_fast") == fast0 + 1
    check_case_end(case, sk, res, N, sat0)


@pytest.mark.parametrize("case", [c for c in CASES if "tracked" in c], ids=[c["name"] for c in CASES if "tracked" in c])
def test_fixture_consecutive_batches(pa, N, case):
    """the dict carries over from batch to batch: a remove of a later batch pops what an earlier one stored"""
    keys, w, n = case_keys(case, "host"), M.stream_weights(case), case["n"]
    cuts = [0, 1, n // 7, n // 7 + 1, n // 2 + 5, n]
    sk = case_sketch(pa, case)
    sat0 = _sat(sk, N)
    parts = [sk.update_many(keys[lo:hi], w[lo:hi]) for lo, hi in zip(cuts, cuts[1:])]
    check_case_end(case, sk, np.concatenate(parts), N, sat0)


# ------------------------------------------------------------------ 10. StreamThreshold.remove_many next to add_many
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("case", [c for c in CASES if c["weights"] == "add_then_remove"], ids=[c["name"] for c in CASES if c["weights"] == "add_then_remove"])
def test_stream_threshold_add_many_then_remove_many(pa, N, case, where):
    keys, w, half = case_keys(case, where), M.stream_weights(case).astype(np.int32), case["n"] // 2
    sk = case_sketch(pa, case)
    sat0 = _sat(sk, N)
    wa, wr = w[:half], -w[half:]
    fast0, upd0 = N.get_option("cms_running_fast"), N.get_option("cms_update_running_fast")
    a = sk.add_many(keys[:half], _dev(wa) if where == "device" else wa)
    assert sk.meets_threshold
    r = sk.remove_many(keys[half:], _dev(wr) if where == "device" else wr)
    assert (N.get_option("cms_running_fast"), N.get_option("cms_update_running_fast")) == (fast0 + 1, upd0 + 1)
    assert r.is_cuda if where == "device" else isinstance(r, np.ndarray)
    check_case_end(case, sk, np.concatenate([_host(a), _host(r)]), N, sat0)


def test_remove_many_defaults_and_errors(pa):
    keys = ["a", "b", "a", "c", "a"]
    sk = sketch(pa, 100, 3, cls="StreamThreshold", threshold=2)
    assert sk.add_many(keys, 2).tolist() == [2, 2, 4, 2, 6] and sk.meets_threshold == {"a": 6, "b": 2, "c": 2}
    assert sk.remove_many(["a", "b"]).tolist() == [5, 1] and sk.meets_threshold == {"a": 5, "c": 2}  # num_els=None removes one
    assert sk.remove_many_ordered(["a", "a"], [1, 2]).tolist() == [4, 2] and sk.elements_added == 5
    before = bytes(sk)
    for call in (lambda: sk.remove_many_ordered(keys, -1), lambda: sk.remove_many(keys, [1, 1, -1, 1, 1]), lambda: sk.remove_many_ordered(keys, 2**31),
                 lambda: sk.update_many_ordered(keys, 2**31), lambda: sk.update_many(keys, [0, 0, -2**31 - 1, 0, 0]),
                 lambda: sk.update_many_ordered(_dev(R.keys_matrix(keys)), _dev(np.array([0, 0, 2**31, 0, 0], dtype=np.int64)))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="update_ordered"):
        sk.update_many_ordered(keys, 2**31)
    assert bytes(sk) == before and sk.meets_threshold == {"a": 5, "c": 2}
    assert sk.update_many_ordered(["a"], -2**31).tolist() == [I32_MIN + 2]  # 2^31 is reachable through the signed call alone
    hh = pa.HeavyHitters(num_hitters=3, width=100, depth=3, device=0)
    for call in (lambda: hh.update_many_ordered(keys, 1), lambda: hh.remove_many_ordered(keys)):
        with pytest.raises(pa.NotSupportedError):
            call()


# ------------------------------------------------------------------ 2. both rails inside one segment
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("t0", [I32_MAX - 3, I32_MIN + 3, 0])
def test_both_rails_inside_one_segment(pa, N, t0, where):
    """one key 600 times: one segment per row over three scan blocks, the weights swing the bin from rail to rail"""
    width, depth, n = 4, 2, 600
    h = np.tile(np.array([[5, 6]], dtype=np.uint64), (n, 1))
    w = np.array([CYCLE[i % len(CYCLE)] for i in range(n)], dtype=np.int64)
    bins = np.full(width * depth, t0, dtype=np.int32)
    _, want, clamps = run_and_check(pa, N, width, depth, "min", h, w, bins, 0, where)
    assert clamps > 0 and {I32_MIN, I32_MAX} <= set(want.tolist())
    # the fourth op removes 2^31 from 0 and lands exactly on INT32_MIN: not a clamp
    c3, c4 = (M.signed_batch(width, depth, h[:m], w[:m], "min", bins)[3] for m in (3, 4))
    assert want[1:4].tolist() == [I32_MAX, 0, I32_MIN] and c3 == c4 > 0
    sk = sketch(pa, width, depth, "min", bins)
    sat0 = _sat(sk, N)
    assert _host(sk.update_alt_many_ordered(*give(h[:4], w[:4], where))).tolist() == want[:4].tolist() and _sat(sk, N) - sat0 == c3


# ------------------------------------------------------------------ 3. tile edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049])
def test_tile_edges(pa, N, n):
    width, depth = 16, 3
    h, w, bins = hashes_of(n, depth, 40, n), mixed_weights(n, n), near_rails(width * depth)
    for query, where in (("min", "device"), ("mean", "host"), ("mean-min", "device")):
        run_and_check(pa, N, width, depth, query, h, w, bins, -7, where)


def test_more_scan_blocks_than_carry_threads(pa, N):
    """256 * 1025 unit ops of alternating sign into one row of 4 bins: 1025 scan blocks and 1025 tiles for single-workgroup carries of 1024
    threads, so a thread's stretch holds two items and half of the threads hold none (every other batch of this suite has fewer blocks per
    chunk than threads); the mean-min query shows elements_added in front of every tile"""
    n, width, depth = 256 * 1025, 4, 1
    w = np.where(np.arange(n) % 2 == 0, 1, -1)
    run_and_check(pa, N, width, depth, "mean-min", hashes_of(n, depth, 9, 21), w, near_rails(width * depth, 2), 5, "device")


# ------------------------------------------------------------------ 4. chunk seams
_seam_refs: dict = {}


def seam_stream(n):
    """depth 64, width 8 (chunks of 131 072 ops): small mixed weights, and around every seam one key alone: 10 ops that remove 2^31, 40
    that add INT32_MAX -- its bins stand at INT32_MAX from 20 ops in front of the seam to 20 behind it -- and 60 that remove 2^31 again
    (the signs the other way round at the second seam: INT32_MIN is held there).  elements_added, started 10 from either int64 rail,
    meets that rail in front of the first seam and behind it"""
    if n not in _seam_refs:
        width, depth = 8, 64
        h, w = hashes_of(n, depth, 50, 4), mixed_weights(n, 4)
        w = np.where(np.abs(w) > 5, w % 5, w)
        for seam in range(131072, n, 131072):
            lo, hi = seam - 30, min(seam + 80, n)
            sign = 1 if (seam // 131072) % 2 else -1
            h[lo:hi] = h[0]
            w[lo:hi] = (np.array([I32_MIN] * 10 + [I32_MAX] * 40 + [I32_MIN] * 60, dtype=np.int64) * sign).clip(I32_MIN, I32_MAX)[: hi - lo]
        bins = near_rails(width * depth, 100)
        want, table, _, clamps = M.signed_batch(width, depth, h, w, "min", bins, 0)
        _seam_refs[n] = (h, w, bins, want["min"], table, clamps)
    return _seam_refs[n]


def els_after(els, w):
    for x in np.asarray(w).tolist():
        els = min(I64_MAX, max(I64_MIN, els + x))
    return els


@pytest.mark.parametrize("els0", [I64_MAX - 10, I64_MIN + 10])
@pytest.mark.parametrize("n", [131073, 262149])
def test_chunk_seams(pa, N, n, els0):
    width, depth = 8, 64
    h, w, bins, want, table, clamps = seam_stream(n)
    wels = els_after(els0, w)
    assert clamps > 0 and wels != els0 + int(w.sum())  # elements_added met its rail
    for seam in range(131072, n, 131072):  # the key's bins stand at a rail on both sides of the seam
        assert len(set(want[seam - 15:min(seam + 15, n)].tolist())) == 1 and int(want[seam]) == (I32_MAX if seam == 131072 else I32_MIN)
    sk = sketch(pa, width, depth, "min", bins, els0)
    sat0, fast0 = _sat(sk, N), N.get_option("cms_update_running_fast")
    got = sk.update_alt_many_ordered(*give(h, w, "device"))
    assert N.get_option("cms_update_running_fast") == fast0 + 1
    assert np.array_equal(_host(got).astype(np.int64), want)
    assert np.array_equal(_bins(sk), table) and sk.elements_added == wels and _sat(sk, N) - sat0 == clamps


def test_mean_min_across_a_chunk_seam(pa, N):
    """elements_added after every op is carried from chunk to chunk (st[0]): only the mean-min query shows it per op"""
    n, width, depth = 131072 + 300, 8, 64
    h, w = hashes_of(n, depth, 50, 9), mixed_weights(n, 9)
    w = np.where(np.abs(w) > 5, w % 7 - 3, w)
    run_and_check(pa, N, width, depth, "mean-min", h, w, None, 1000, "device")


@pytest.mark.parametrize("els0", [I64_MAX - 10, I64_MIN + 10])
def test_every_cut_of_a_short_batch(pa, N, els0):
    """two consecutive calls leave what the uncut call leaves, wherever the cut lies"""
    n, width, depth = 40, 4, 3
    h, w, bins = hashes_of(n, depth, 6, 12), mixed_weights(n, 12), near_rails(width * depth)
    w[::5] = 9 if els0 > 0 else -9  # (elements_added meets its rail early and leaves it again)
    whole, want, clamps = run_and_check(pa, N, width, depth, "mean", h, w, bins, els0, "host")
    for cut in range(n + 1):
        sk = sketch(pa, width, depth, "mean", bins, els0)
        sat0 = _sat(sk, N)
        a = sk.update_alt_many_ordered(*give(h[:cut], w[:cut], "host"))
        b = sk.update_alt_many_ordered(*give(h[cut:], w[cut:], "device"))
        assert np.concatenate([a, _host(b)]).tolist() == want.tolist(), cut
        assert bytes(sk) == bytes(whole) and sk.elements_added == whole.elements_added and _sat(sk, N) - sat0 == clamps, cut


# ------------------------------------------------------------------ 5. mean-min with negative bins
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("depth", [4, 5])
def test_mean_min_negative_bins_and_a_prefix_that_turns(pa, N, depth, where):
    n, width = 3000, 50
    h = hashes_of(n, depth, 300, depth)
    w = (rnd(n, 31) % np.uint64(15)).astype(np.int64) - 7
    sk, want, _ = run_and_check(pa, N, width, depth, "mean-min", h, w, None, 3, where)
    els = 3 + np.cumsum(w)
    assert (_bins(sk) < 0).any() and (np.diff(els) > 0).any() and (np.diff(els) < 0).any() and (want < 0).any() and (want > 0).any()


# ------------------------------------------------------------------ 6. the sequential kernel on a twin
def test_twin_fed_through_update_ordered(pa, N):
    n, width, depth = 20_000, 64, 4
    h, w, bins = hashes_of(n, depth, 500, 6), mixed_weights(n, 6), near_rails(width * depth, 50)
    for query in M.QUERIES:
        a, b = sketch(pa, width, depth, query, bins, 17), sketch(pa, width, depth, query, bins, 17)
        opts0 = [N.get_option(o) for o in ("cms_update_running_fast", "cms_update_running_sequential", "cms_running_fast", "cms_running_sequential")]
        ca0, cb0 = a._tab.counters(), b._tab.counters()
        got = a.update_alt_many_ordered(*give(h, w, "host"))
        assert [N.get_option(o) for o in ("cms_update_running_fast", "cms_update_running_sequential", "cms_running_fast", "cms_running_sequential")] == \
            [opts0[0] + 1, opts0[1], opts0[2], opts0[3]]
        want = b._ordered(b._alt(h), w, N.OP_SIGNED)  # (update_ordered for pre-computed hashes)
        assert np.array_equal(got.astype(np.int64), want)
        assert bytes(a) == bytes(b) and a.elements_added == b.elements_added
        ca, cb = a._tab.counters(), b._tab.counters()
        for c in (N.CTR_SATURATED, N.CTR_ABS_BOUND):
            assert ca[c] - ca0[c] == cb[c] - cb0[c] > 0


# ------------------------------------------------------------------ 7. the one-lane kernel behind the same entry
def test_depth_65_takes_the_sequential_kernel(pa, N):
    n, width, depth = 500, 16, 65
    h, w, bins = hashes_of(n, depth, 30, 7), mixed_weights(n, 7), near_rails(width * depth)
    for query, where in (("min", "host"), ("mean-min", "device")):
        opts0 = [N.get_option(o) for o in ("cms_update_running_fast", "cms_update_running_sequential", "cms_running_sequential")]
        run_and_check(pa, N, width, depth, query, h, w, bins, 5, where)
        assert [N.get_option(o) for o in ("cms_update_running_fast", "cms_update_running_sequential", "cms_running_sequential")] == [opts0[0], opts0[1] + 1, opts0[2]]


# ------------------------------------------------------------------ 8. default weights, empty batches
@pytest.mark.parametrize("where", ["host", "device"])
def test_no_weights_is_add_many_ordered_and_empty_batches_change_nothing(pa, N, where):
    n, width, depth = 5000, 300, 5
    h = hashes_of(n, depth, 700, 8)
    hh = _dev(h.view(np.int64)) if where == "device" else h
    a, b = sketch(pa, width, depth, "mean-min"), sketch(pa, width, depth, "mean-min")
    ra, rb = a.update_alt_many_ordered(hh, None), b.add_alt_many_ordered(hh)
    assert np.array_equal(_host(ra), _host(rb)) and _host(ra).dtype == np.int64 and bytes(a) == bytes(b) and a.elements_added == n
    before, ctr0 = bytes(a), a._tab.counters()
    opts0 = [N.get_option(o) for o in ("cms_update_running_fast", "cms_update_running_sequential")]
    empty = a.update_alt_many_ordered(hh[:0], None)
    assert _host(empty).size == 0 and _host(empty).dtype == np.int64
    none = np.zeros((0, 16), dtype=np.uint8)
    assert _host(a.update_many_ordered(none, np.zeros(0, dtype=np.int32))).size == 0 and _host(a.remove_many_ordered(none)).size == 0
    assert bytes(a) == before and a.elements_added == n and a._tab.counters() == ctr0
    assert [N.get_option(o) for o in ("cms_update_running_fast", "cms_update_running_sequential")] == opts0


# ------------------------------------------------------------------ 9. the wrap-free bound after a signed batch
@pytest.mark.parametrize("up", [True, False])
def test_unordered_batches_after_a_signed_batch_keep_the_bound(pa, N, up):
    """a signed batch drives bins to within a few counts of a rail; the unordered add_many / remove_many that follows must saturate there
    (it chooses its kernel by PSK_CTR_ABS_BOUND, which the signed batch has to have raised), and check_many reads the model's table"""
    n, width, depth, sign = 4000, 32, 3, 1 if up else -1
    h = hashes_of(n, depth, 60, 10)
    w = np.where(rnd(n, 10) % np.uint64(4) == 0, -3, 2**26) * sign  # mostly towards the rail, some steps back
    sk, _, _ = run_and_check(pa, N, width, depth, "min", h, w, None, 0, "device")
    assert sk._tab.counters()[N.CTR_ABS_BOUND] >= int(np.abs(w).sum())
    _, table, els, _ = M.signed_batch(width, depth, h, w, "min")
    w2 = np.full(n, 2**20, dtype=np.int64) * sign
    _, table2, els2, clamps2 = M.signed_batch(width, depth, h, w2, "min", table, els)
    assert clamps2 > 0
    (sk.add_alt_many if up else sk.remove_alt_many)(_dev(h.view(np.int64)), _dev(np.abs(w2).astype(np.int32)))
    assert np.array_equal(_bins(sk), table2) and sk.elements_added == els2
    got = _host(sk.check_alt_many(_dev(h[:500].view(np.int64))))
    rows = np.arange(depth) * width
    assert got.tolist() == table2[(h[:500] % np.uint64(width)).astype(np.int64) + rows[None, :]].min(axis=1).tolist()


# ------------------------------------------------------------------ scratch
def test_signed_scratch_is_the_add_paths_plus_the_larger_aggregates(pa):
    """per (op, row) the signed passes hold what the add path holds (20 B); on top come 16 more bytes per 256-element block and row
    (a RunMap in place of a RunSeg) and 32 per 256-op tile, and psk_scratch_bytes reports them"""
    n, width, depth = 4096, 1024, 5
    h = _dev(hashes_of(n, depth, 500, 14).view(np.int64))
    a, b = sketch(pa, width, depth), sketch(pa, width, depth)
    a.add_alt_many_ordered(h)
    b.update_alt_many_ordered(h, None)
    a.synchronize(), b.synchronize()
    more = (n // 256) * (depth * 16 + 32)
    assert more <= b.scratch_bytes()["total"] - a.scratch_bytes()["total"] <= more + more // 4 + 16  # (buffers grow by a quarter more than asked)
    b.release_scratch()
    assert b.scratch_bytes()["total"] == 0 and _host(b.update_alt_many_ordered(h[:10], None)).size == 10  # regrows on demand
