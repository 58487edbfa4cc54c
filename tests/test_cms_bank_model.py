"""CountMinSketchBank without a GPU: the numpy model (tests/cms_bank_model.py) against the fixture recorded from the REAL reference
(tests/golden/golden_cms_bank.json: streams, the rail case, the join folds), and the host logic of pyprobables_amd/cmsbank.py that needs no
device -- weight refusals, the bound bookkeeping as pure functions, sizing, the C entry points' argument checks."""

import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import cms_bank_model as M  # noqa: E402

G = json.loads((ROOT / "tests" / "golden" / "golden_cms_bank.json").read_text())
QUERIES = ("min", "mean", "mean-min")


def test_fixture_shape():
    assert [(c["width"], c["depth"]) for c in G["cases"]] == [(8, 3), (7, 3), (64, 5), (100, 4), (16, 1)]
    for c in G["cases"]:
        assert c["sketches"] == 5 and c["elements_added"][3] == 0
        sent = {}
        for i, s, _ in c["stream"]:
            sent.setdefault(i, set()).add(s)
        assert sent[0] == {0, 1}  # one key goes to two sketches
        keys = [M.dec(e) for e in c["pool"]]
        assert "" in keys and any(isinstance(k, bytes) for k in keys) and any(isinstance(k, str) and max(map(ord, k), default=0) > 255 for k in keys)
    assert (ROOT / "tests" / "golden" / "golden_cms_bank.json").stat().st_size < 64 * 1024


@pytest.mark.parametrize("ci", range(5))
def test_model_streams_match_the_reference(ci):
    c = G["cases"][ci]
    pool = [M.dec(e) for e in c["pool"]]
    m = M.BankModel(c["sketches"], c["width"], c["depth"])
    for i, s, w in c["stream"]:
        m.add(pool[i], s, w)
    for s in range(c["sketches"]):
        assert m.export(s).hex() == c["export_hex"][s]
    assert m.els == c["elements_added"]
    absent = [M.dec(e) for e in c["absent"]]
    for q in QUERIES:
        assert [m.check(pool[i], s, q) for i, s in c["probes"]] == c["answers_" + q]
        assert [m.check(absent[i], s, q) for i, s in c["absent_probes"]] == c["absent_answers_" + q]


def test_model_rail_case():
    r = G["rail"]
    m = M.BankModel(1, r["width"], r["depth"])
    for step in r["steps"]:
        m.add(r["key"], 0, step["num_els"])
        assert m.export(0).hex() == step["export_hex"] and m.els[0] == step["elements_added"]
        for q in QUERIES:
            assert [m.check(r["key"], 0, q), m.check(r["other"], 0, q)] == step["answers"][q]
    assert max(m.bins[0]) == M.I32_MAX and m.els[0] == 3 * M.I32_MAX + 1


def test_model_join_folds():
    j = G["joins"]
    m = M.BankModel(len(j["members_hex"]), j["width"], j["depth"])
    for s, hx in enumerate(j["members_hex"]):
        m.load(s, bytes.fromhex(hx))
    assert m.bins.max() == M.I32_MAX and m.bins.min() == M.I32_MIN
    out = m.reduce([f["members"] for f in j["folds"]] + [[], [99, 2]])
    for g, f in enumerate(j["folds"]):
        assert out.export(g).hex() == f["export_hex"] and out.els[g] == f["elements_added"]
    n = len(j["folds"])
    assert not out.bins[n].any() and out.els[n] == 0
    assert out.export(n + 1) == m.export(2)  # a member beyond the bank is an empty sketch
    by = {tuple(f["members"]): f["export_hex"] for f in j["folds"]}
    assert by[(6, 8)] != by[(8, 6)] and by[(4, 9)] != by[(9, 4)]  # an accumulator on a rail stays frozen: the fold is not commutative


# ------------------------------------------------------------------ host logic of the package
def test_bound_bookkeeping_is_pure_and_never_wraps():
    from pyprobables_amd import cmsbank as B

    b = np.array([0, 5, 2**63 - 2, 2**63 - 1, -3], dtype=np.int64)
    w = np.array([7, 0, 9, 1, 2**63 - 1], dtype=np.int64)
    got = B.sat_add_i64(b, w)
    assert got.dtype == np.int64 and got.tolist() == [7, 5, 2**63 - 1, 2**63 - 1, 2**63 - 4]
    assert got[:4].tolist() == M.bound_after_add(b[:4], w[:4])
    torch = pytest.importorskip("torch")
    assert B.sat_add_i64(torch.from_numpy(b), torch.from_numpy(w)).tolist() == got.tolist()
    assert B.loaded_bound([-5, -1]) == 0 and B.loaded_bound([3, -9, 2**31 - 1]) == 2**31 - 1 and B.loaded_bound([]) == 0
    r = B.reduce_bounds([1, 2**63 - 1, 3, 10], [0, 2, 2, 5, 6], [0, 1, 2, 3, 99, -1])
    assert r.tolist() == [2**63 - 1, 0, 13, 0]


def test_host_weights_are_always_checked():
    from pyprobables_amd import cmsbank as B

    assert B.host_weights(None, 3) is None
    assert B.host_weights(4, 3).tolist() == [4, 4, 4]
    assert B.host_weights([0, 1, 2**31 - 1], 3).tolist() == [0, 1, 2**31 - 1]
    with pytest.raises(ValueError, match=">= 0"):
        B.host_weights([1, -1, 1], 3)
    with pytest.raises(ValueError, match=">= 0"):
        B.host_weights(-2, 3)
    with pytest.raises(OverflowError):
        B.host_weights([1, 2**31, 1], 3)
    with pytest.raises(ValueError, match="length"):
        B.host_weights([1, 2], 3)
    with pytest.raises(TypeError):
        B.host_weights([1.5, 2.0, 1.0], 3)


def test_sizing_and_refusals_before_any_device_is_touched():
    import pyprobables_amd as pa
    from pyprobables_amd.countminsketch import CountMinSketch

    assert CountMinSketch._geometry(None, None, 0.95, 0.01) == (200, 5, 0.95, 0.01)  # countminsketch.py:102-104: ceil(2 / 0.01), ceil(4.32)
    assert CountMinSketch._geometry(2048, 5, None, None) == (2048, 5, 1 - 1 / 32, 2 / 2048)
    with pytest.raises(pa.InitializationError, match="Must provide one of the following"):
        pa.CountMinSketchBank(4)
    with pytest.raises(pa.InitializationError, match="width and depth must be greater than 0"):
        pa.CountMinSketchBank(4, width=0, depth=3)
    with pytest.raises(pa.NotSupportedError, match="at most 64 deep"):
        pa.CountMinSketchBank(4, width=10, depth=65)
    with pytest.raises(ValueError, match="2\\^31 wide"):
        pa.CountMinSketchBank(4, width=2**31 + 1, depth=1)
    for bad in (0, -1, 2**31, 1.5):
        with pytest.raises(ValueError, match="num_sketches"):
            pa.CountMinSketchBank(bad, width=8, depth=3)


def test_c_entry_points_check_their_arguments_without_a_device():
    """argument refusals come before the device is touched: PSK_EINVAL and a message"""
    from pyprobables_amd import _native as N

    L = N.lib()
    tab = 1 << 20  # (a 16-byte aligned address that is never dereferenced)
    keys = (N.KEYS_FIXED, None, None, 0, 16)

    def einval(rc, text):
        assert rc == N.PSK_EINVAL and text in N.last_error(), N.last_error()

    einval(L.psk_cms_bank_add(tab, 4, 8, 65, *keys, N.DEVICE, None, None, None, None, 0, None), "1 .. 64 deep")
    einval(L.psk_cms_bank_add(tab, 4, 0, 3, *keys, N.DEVICE, None, None, None, None, 0, None), "1 .. 2^31 wide")
    einval(L.psk_cms_bank_add(tab, 4, 2**31 + 1, 3, *keys, N.DEVICE, None, None, None, None, 0, None), "1 .. 2^31 wide")
    einval(L.psk_cms_bank_add(tab, 0, 8, 3, *keys, N.DEVICE, None, None, None, None, 0, None), "sketches")
    einval(L.psk_cms_bank_add(tab + 4, 4, 8, 3, *keys, N.DEVICE, None, None, None, None, 0, None), "16-byte aligned")
    einval(L.psk_cms_bank_add(tab, 4, 8, 3, N.KEYS_FIXED, None, None, 2**32, 16, N.DEVICE, None, None, None, None, 0, None), "fewer than 2^32 keys")
    einval(L.psk_cms_bank_add(tab, 4, 8, 3, N.KEYS_HASHES, None, None, 0, 2, N.DEVICE, None, None, None, None, 0, None), "hashes per key")
    ids, w, data = np.zeros(3, dtype=np.uint32), np.array([1, -4, 2], dtype=np.int32), np.zeros(48, dtype=np.uint8)
    einval(L.psk_cms_bank_add(tab, 4, 8, 3, N.KEYS_FIXED, data.ctypes.data, None, 3, 16, N.HOST, ids.ctypes.data, w.ctypes.data, None, None, 0, None),
           "weight -4 of key 1 is negative")
    einval(L.psk_cms_bank_check(tab, 4, 8, 3, *keys, N.DEVICE, None, N.Q_MEANMIN, None, 0, None), "MIN and MEAN")
    einval(L.psk_cms_bank_check_meanmin(tab, 4, 1, 3, *keys, N.DEVICE, None, tab, None, 0, None), "width >= 2")
    einval(L.psk_cms_bank_build(tab, 4, 8, 3, *keys, None, None, None, None, None, 1, 0, 0, None), "seg_dev is NULL")
    einval(L.psk_cms_bank_build(tab, 4, 8, 3, *keys, tab, None, None, None, None, 0, 0, 0, None), "split must be")
    einval(L.psk_cms_bank_build(tab, 4, 8, 3, *keys, tab, None, None, None, None, 1, 3, 0, None), "route must be")
    einval(L.psk_cms_bank_build(tab, 4, 4097, 4, *keys, tab, None, None, None, None, 1, 1, 0, None), "do not fit the LDS image")
    einval(L.psk_cms_bank_reduce(tab, None, 4, 7, 3, tab, tab, 2, tab + 96, None, 0, None), "dst overlaps src")
    einval(L.psk_cms_bank_reduce(tab, None, 4, 7, 3, tab, tab, 2, None, None, 0, None), "dst_dev")


def test_rows_of_2_pow_32_ints_are_refused_by_build_and_reduce():
    """psk_cms_bank_build and psk_cms_bank_reduce index a row with 32 bits: width * depth (rounded up to 4) >= 2^32 is PSK_EINVAL before anything
    is enqueued, at the seam and beyond it; the row below the seam passes that check"""
    from pyprobables_amd import _native as N

    L = N.lib()
    tab = 1 << 20
    keys = (N.KEYS_FIXED, None, None, 0, 16)
    for width, depth in ((2**31, 2), (2**31 - 1, 2), (2**30, 4), (2**31, 64), (2**26, 64)):
        rc = L.psk_cms_bank_build(tab, 1, width, depth, *keys, tab, None, None, None, None, 1, 0, 0, None)
        assert rc == N.PSK_EINVAL and "fewer than 2^32 ints" in N.last_error(), (width, depth, N.last_error())
        rc = L.psk_cms_bank_reduce(tab, None, 1, width, depth, tab, tab, 1, tab, None, 0, None)
        assert rc == N.PSK_EINVAL and "fewer than 2^32 ints" in N.last_error(), (width, depth, N.last_error())
    for width, depth in ((2**31 - 2, 2), (2**30, 3)):  # 2^32 - 4 and 3 * 2^30 ints
        rc = L.psk_cms_bank_build(tab, 1, width, depth, *keys, tab, None, None, None, None, 1, 1, 0, None)  # (route 1: the next check in line)
        assert rc == N.PSK_EINVAL and "do not fit the LDS image" in N.last_error()
        rc = L.psk_cms_bank_reduce(tab, None, 1, width, depth, tab, tab, 1, tab, None, 0, None)
        assert rc == N.PSK_EINVAL and "dst overlaps src" in N.last_error()


def test_unchecked_ids_are_clipped_before_they_are_narrowed():
    from pyprobables_amd.cmsbank import CountMinSketchBank

    b = CountMinSketchBank.__new__(CountMinSketchBank)
    b._num_sketches = 5
    ids = np.array([0, 4, 5, -1, 2**32 + 1, 2**63 - 1], dtype=np.int64)
    assert b._clip_ids(ids).tolist() == [0, 4, 5, 5, 5, 5]
    assert b._ids_u32(b._clip_ids(ids)).tolist() == [0, 4, 5, 5, 5, 5]
    torch = pytest.importorskip("torch")
    assert b._clip_ids(torch.from_numpy(ids)).tolist() == [0, 4, 5, 5, 5, 5]
