"""BloomFilterBank.match_many without a GPU: the slice-row helper of the C ABI, the argument checks that run in front of any HIP call, and
the numpy model (tests/bank_match_model.py) against what the REAL reference answered for every (probe, filter) pair
(tests/golden/golden_bank_match.json, written by tests/golden/gen_golden_bank_match.py)."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import bank_match_model as MM  # noqa: E402
import bank_model as M  # noqa: E402

PATH = ROOT / "tests" / "golden" / "golden_bank_match.json"
G = json.loads(PATH.read_text())
REF = Path(os.environ.get("PYPROBABLES_REFERENCE", "/root/reference"))  # the checkout the generator scripts default to


def dec(e):
    return e[1] if e[0] == "s" else bytes.fromhex(e[1])


def case_model(c):
    """-> (rows, probes' hashes, expected bool[n, filters]) of one fixture case"""
    m, k, F = c["number_bits"], c["number_hashes"], c["filters"]
    pool = [dec(e) for e in c["pool"]]
    hp = M.hashes_list(pool, k)
    idx = np.array([i for f in range(F) for i in c["sent"][f]], dtype=np.int64)
    ids = np.array([f for f in range(F) for _ in c["sent"][f]], dtype=np.int64)
    rows = M.bank_rows(F, m, k, hp[idx], ids)
    probes = pool + [dec(e) for e in c["absent"]]
    want = np.array([[(int.from_bytes(bytes.fromhex(h), "little") >> f) & 1 for f in range(F)] for h in c["masks"]], dtype=bool)
    return rows, M.hashes_list(probes, k), want


def test_slice_row_bytes_of_the_c_abi():
    from pyprobables_amd import _native as N

    L = N.lib()
    assert [L.psk_bank_slice_row_bytes(f) for f in (1, 127, 128, 129, 4096, 8192, 2**32)] == [16, 16, 16, 32, 512, 1024, 2**29]
    assert all(L.psk_bank_slice_row_bytes(f) == MM.slice_row_bytes(f) for f in (1, 8, 70, 127, 128, 129, 255, 256, 257, 1000, 4097, 2**31 - 1))


def test_slice_and_match_calls_reject_bad_arguments_before_touching_a_device():
    from pyprobables_amd import _native as N

    L = N.lib()
    keys = np.zeros((1, 16), dtype=np.uint8)
    tab = img = 0x1000  # never dereferenced: every call below fails its checks
    assert L.psk_bank_slices(None, 64, 63, img, 0, 64, 0, None) == N.PSK_EINVAL and "NULL" in N.last_error()
    assert L.psk_bank_slices(tab, 64, 63, None, 0, 64, 0, None) == N.PSK_EINVAL
    assert L.psk_bank_slices(tab, 64, 63, img + 4, 0, 64, 0, None) == N.PSK_EINVAL and "aligned" in N.last_error()
    assert L.psk_bank_slices(tab, 0, 63, img, 0, 0, 0, None) == N.PSK_EINVAL
    assert L.psk_bank_slices(tab, 64, 0, img, 0, 64, 0, None) == N.PSK_EINVAL
    assert L.psk_bank_slices(tab, 64, 2**31 + 1, img, 0, 64, 0, None) == N.PSK_EINVAL
    for first, last in ((1, 64), (16, 64), (0, 33), (32, 48), (64, 32), (0, 96), (96, 96)):  # filters = 70 below
        assert L.psk_bank_slices(tab, 70, 63, img, first, last, 0, None) == N.PSK_EINVAL, (first, last)
    assert "multiple of 32" in N.last_error() or "range" in N.last_error()
    base = (N.KEYS_FIXED, keys.ctypes.data, None, 1, 16)
    out = 0x2000
    assert L.psk_bank_match(None, 70, 63, 4, *base, N.HOST, out, None, None, None, 0, None) == N.PSK_EINVAL and "NULL" in N.last_error()
    assert L.psk_bank_match(img, 70, 63, 4, *base, N.HOST, None, None, None, None, 0, None) == N.PSK_EINVAL and "no output" in N.last_error()
    assert L.psk_bank_match(img, 70, 63, 4, *base, N.HOST, None, None, out, None, 0, None) == N.PSK_EINVAL and "go together" in N.last_error()
    assert L.psk_bank_match(img, 70, 63, 4, *base, N.HOST, None, None, None, out, 0, None) == N.PSK_EINVAL and "go together" in N.last_error()
    assert L.psk_bank_match(img, 70, 63, 65, *base, N.HOST, out, None, None, None, 0, None) == N.PSK_EINVAL and "at most 64" in N.last_error()
    assert L.psk_bank_match(img, 70, 63, 0, *base, N.HOST, out, None, None, None, 0, None) == N.PSK_EINVAL
    assert L.psk_bank_match(img, 70, 63, 4, *base, N.HOST, out + 4, None, None, None, 0, None) == N.PSK_EINVAL and "aligned" in N.last_error()
    assert L.psk_bank_match(img, 70, 63, 4, N.KEYS_HASHES, keys.ctypes.data, None, 1, 3, N.HOST, out, None, None, None, 0, None) == N.PSK_EINVAL
    assert L.psk_bank_match(img, 70, 63, 4, N.KEYS_FIXED, keys.ctypes.data, None, 2**32, 16, N.HOST, out, None, None, None, 0, None) == N.PSK_EINVAL


def test_fixture_shape():
    assert PATH.stat().st_size < 100_000 and G["reference_version"] == "0.7.0"
    assert [(c["est"], c["fpr"], c["number_bits"], c["number_hashes"], c["filters"]) for c in G["cases"]] == [(10, 0.05, 63, 4, 70), (100, 0.01, 959, 7, 70)]
    assert sum(c["false_positives"] for c in G["cases"]) > 0
    assert sum(c["match_none"] for c in G["cases"]) > 0 and sum(c["match_three_or_more"] for c in G["cases"]) > 0
    for c in G["cases"]:
        pool = [dec(e) for e in c["pool"]]
        assert c["sent"][G["empty_filter"]] == [] and len(c["sent"]) == 70
        assert [f for f in range(70) if 0 in c["sent"][f]] == G["three"]
        assert any(isinstance(x, str) for x in pool) and any(isinstance(x, bytes) for x in pool) and "" in pool
        assert any(isinstance(x, str) and max(map(ord, x), default=0) > 255 for x in pool)
        assert len(c["absent"]) == 60 and len(c["masks"]) == len(pool) + 60


def test_model_equals_the_reference_on_every_probe_and_filter():
    for c in G["cases"]:
        m, k, F = c["number_bits"], c["number_hashes"], c["filters"]
        rows, hq, want = case_model(c)
        sl = MM.slices_of(rows, F, m)
        assert sl.shape == (m, MM.slice_row_bytes(F)) == (m, 16)
        mask = MM.match_mask(sl, m, k, hq)
        assert np.array_equal(MM.mask_bits(mask, F), want)
        assert not MM.mask_bits(mask, 128)[:, F:].any()                      # pad columns 70..127
        assert not MM.mask_bits(mask, F)[:, G["empty_filter"]].any()
        n = hq.shape[0]
        pairs = M.bank_check(rows, m, k, np.repeat(hq, F, axis=0), np.tile(np.arange(F), n)).reshape(n, F)  # every (probe, filter) pair
        assert np.array_equal(pairs, want)
        assert MM.match_counts(mask).tolist() == want.sum(axis=1).tolist()
        offs, ids = MM.match_ids(mask)
        assert offs.tolist() == [0, *np.cumsum(want.sum(axis=1)).tolist()]
        for i in range(n):
            assert ids[offs[i]:offs[i + 1]].tolist() == np.flatnonzero(want[i]).tolist()


@pytest.mark.parametrize("filters", [1, 127, 128, 129])
def test_model_helpers_at_the_row_seams(filters):
    m, k, n = 77, 3, 40
    rng = np.random.default_rng(filters)
    assert MM.slice_row_bytes(filters) == (16 if filters <= 128 else 32)
    rows = rng.integers(0, 256, (filters, M.row_bytes(m)), dtype=np.uint8)
    rows[:, m // 8] &= (1 << (m % 8)) - 1   # no pad bits
    rows[:, m // 8 + 1:] = 0
    rows[filters - 1, :] = 0
    rows[filters - 1, 0] = 1                # the last filter: bit 0 alone
    sl = MM.slices_of(rows, filters, m)
    assert sl.shape == (m, MM.slice_row_bytes(filters))
    for f in (0, filters // 2, filters - 1):
        for p in (0, 1, 31, 32, m - 1):
            assert (sl[p, f >> 3] >> (f & 7)) & 1 == (rows[f, p >> 3] >> (p & 7)) & 1
    assert not np.unpackbits(sl, axis=1, bitorder="little")[:, filters:].any()
    h = rng.integers(0, 2**63, (n, k), dtype=np.uint64)
    h[0] = 0                                # bit 0 three times: matches the last filter
    mask = MM.match_mask(sl, m, k, h)
    want = M.bank_check(rows, m, k, np.repeat(h, filters, axis=0), np.tile(np.arange(filters), n)).reshape(n, filters)
    assert want[0, filters - 1]
    assert np.array_equal(MM.mask_bits(mask, filters), want)
    assert np.array_equal(MM.match_counts(mask), want.sum(axis=1))
    offs, ids = MM.match_ids(mask)
    assert offs[-1] == want.sum() and ids.tolist() == np.nonzero(want)[1].tolist()
    assert MM.match_ids(mask.view(np.uint32))[1].tolist() == ids.tolist()  # word view, little endian


def test_regenerating_the_fixture_gives_the_committed_bytes(tmp_path):
    if not (REF / "probables").is_dir():
        pytest.skip("the reference checkout is not on this machine")
    out = tmp_path / "golden_bank_match.json"
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, str(ROOT / "tests" / "golden" / "gen_golden_bank_match.py"), str(REF), str(out)], check=True, env=env, capture_output=True)
    assert out.read_bytes() == PATH.read_bytes()
