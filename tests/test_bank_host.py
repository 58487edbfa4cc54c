"""BloomFilterBank without a GPU: the row-size helper of the C ABI, the pure grouping helper, the numpy model (tests/bank_model.py) against
what the REAL reference exported per filter (tests/golden/golden_bank.json, written by tests/golden/gen_golden_bank.py), and -- where the
reference is at hand -- that the generator still writes the committed bytes."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import bank_model as M  # noqa: E402

PATH = ROOT / "tests" / "golden" / "golden_bank.json"
G = json.loads(PATH.read_text())
REF = Path(os.environ.get("PYPROBABLES_REFERENCE", "/root/reference"))  # the checkout the generator scripts default to
FOOTER = 20  # bytes of the QQf footer behind the table


def dec(e):
    return e[1] if e[0] == "s" else bytes.fromhex(e[1])


def test_row_bytes_of_the_c_abi():
    from pyprobables_amd import _native as N

    L = N.lib()
    assert L.psk_bank_row_bytes(63) == 16
    assert L.psk_bank_row_bytes(959) == 128
    assert L.psk_bank_row_bytes(524303) == 65552
    assert L.psk_bank_row_bytes(524288) == 65536 and L.psk_bank_row_bytes(524287) == 65536
    assert all(L.psk_bank_row_bytes(m) == M.row_bytes(m) == L.psk_bloom_table_bytes(m) for m in (1, 8, 127, 128, 129, 14378, 95851))


def test_bank_calls_reject_bad_arguments_before_touching_a_device():
    """the argument checks run in front of any HIP call: they answer on a machine without a GPU"""
    from pyprobables_amd import _native as N

    L = N.lib()
    keys = np.zeros((1, 16), dtype=np.uint8)
    ids = np.zeros(1, dtype=np.uint32)
    tab = 0x1000  # never dereferenced: every call below fails its checks
    base = (N.KEYS_FIXED, keys.ctypes.data, None, 1, 16)
    assert L.psk_bank_add(None, 4, 63, 4, *base, N.HOST, ids.ctypes.data, 0, None) == N.PSK_EINVAL and "NULL table" in N.last_error()
    assert L.psk_bank_add(tab, 0, 63, 4, *base, N.HOST, ids.ctypes.data, 0, None) == N.PSK_EINVAL
    assert L.psk_bank_add(tab, 4, 0, 4, *base, N.HOST, ids.ctypes.data, 0, None) == N.PSK_EINVAL
    assert L.psk_bank_add(tab, 4, 2**31 + 1, 4, *base, N.HOST, ids.ctypes.data, 0, None) == N.PSK_EINVAL
    assert L.psk_bank_add(tab, 4, 63, 0, *base, N.HOST, ids.ctypes.data, 0, None) == N.PSK_EINVAL
    assert L.psk_bank_add(tab, 4, 63, 4, *base, N.HOST, None, 0, None) == N.PSK_EINVAL and "ids" in N.last_error()
    assert L.psk_bank_add(tab, 4, 63, 4, N.KEYS_HASHES, keys.ctypes.data, None, 1, 3, N.HOST, ids.ctypes.data, 0, None) == N.PSK_EINVAL
    assert L.psk_bank_check(tab, 4, 63, 4, *base, N.HOST, ids.ctypes.data, None, 0, None) == N.PSK_EINVAL
    assert L.psk_bank_build(tab, 4, 63, 4, *base, None, None, 1, 0, 0, None) == N.PSK_EINVAL and "seg_dev" in N.last_error()
    assert L.psk_bank_build(tab, 4, 63, 4, *base, tab, None, 0, 0, 0, None) == N.PSK_EINVAL and "split" in N.last_error()
    assert L.psk_bank_build(tab, 4, 63, 4, *base, tab, None, 1, 3, 0, None) == N.PSK_EINVAL and "route" in N.last_error()
    # a row over the LDS cap: route 1 is refused (m = 524303 is (54700, 0.01): 65552 bytes)
    assert L.psk_bank_build(tab, 4, 524303, 7, *base, tab, None, 1, 1, 0, None) == N.PSK_EINVAL and "LDS" in N.last_error()


def test_group_ids():
    from pyprobables_amd.bank import group_ids

    perm, seg = group_ids([2, 0, 2, 5, 0, 2], 7)
    assert perm.dtype == np.uint32 and seg.dtype == np.uint64
    assert perm.tolist() == [1, 4, 0, 2, 5, 3]            # stable: the keys of a filter in their order of arrival
    assert seg.tolist() == [0, 2, 2, 5, 5, 5, 6, 6]       # filters 1, 3, 4 and 6 are empty
    perm, seg = group_ids(np.full(5, 3, dtype=np.uint32), 4)  # all keys in one filter (the last)
    assert perm.tolist() == [0, 1, 2, 3, 4] and seg.tolist() == [0, 0, 0, 0, 5]
    perm, seg = group_ids(np.zeros(0, dtype=np.int64), 3)
    assert perm.size == 0 and seg.tolist() == [0, 0, 0, 0]
    for bad in ([0, 3], [-1, 0], [2**32]):
        with pytest.raises(ValueError):
            group_ids(bad, 3)
    with pytest.raises(TypeError):
        group_ids([0.5], 3)
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 50, 1000)
    perm, seg = group_ids(ids, 50)
    for f in range(50):
        assert perm[int(seg[f]):int(seg[f + 1])].tolist() == np.flatnonzero(ids == f).tolist()


def test_fixture_shape():
    assert PATH.stat().st_size < 100_000 and G["reference_version"] == "0.7.0"
    assert [(c["est"], c["fpr"], c["number_bits"], c["number_hashes"]) for c in G["cases"]] == [(10, 0.05, 63, 4), (100, 0.01, 959, 7), (1000, 0.001, 14378, 10)]
    assert [M.row_bytes(c["number_bits"]) for c in G["cases"]] == [16, 128, 1808]
    k = G["known_spam_eggs"]
    assert len(k) == 56 and k.startswith("20008000200074010a00") and k.endswith("cdcc4c3d")
    assert G["cases"][0]["false_positives"] > 0 and G["cases"][1]["false_positives"] > 0
    for c in G["cases"]:
        pool = [dec(e) for e in c["pool"]]
        assert c["filters"] == 5 and c["elements_added"][3] == 0
        assert any(isinstance(x, str) for x in pool) and any(isinstance(x, bytes) for x in pool) and "" in pool
        assert any(isinstance(x, str) and max(map(ord, x), default=0) > 255 for x in pool)
        assert {f for i, f in c["stream"] if i == 0} == {0, 1}  # one key in two filters


def test_model_equals_the_reference_per_filter():
    known = M.bank_rows(1, 63, 4, M.hashes_list(["spam", b"eggs"], 4), [0, 0])
    assert known[0, :8].tobytes().hex() == G["known_spam_eggs"][:16]
    for c in G["cases"]:
        m, k, F = c["number_bits"], c["number_hashes"], c["filters"]
        pool = [dec(e) for e in c["pool"]]
        hp = M.hashes_list(pool, k)
        idx = np.array([i for i, _ in c["stream"]])
        ids = np.array([f for _, f in c["stream"]])
        rows = M.bank_rows(F, m, k, hp[idx], ids)
        nbytes = (m + 7) // 8
        for f in range(F):
            raw = bytes.fromhex(c["export_hex"][f])
            assert len(raw) == nbytes + FOOTER
            assert rows[f, :nbytes].tobytes() == raw[:nbytes], (m, f)
            assert not rows[f, nbytes:].any()
        assert np.bincount(ids, minlength=F).tolist() == c["elements_added"]
        pi = np.array([i for i, _ in c["probes"]])
        pf = np.array([f for _, f in c["probes"]])
        assert M.bank_check(rows, m, k, hp[pi], pf).astype(int).tolist() == c["answers"]
        ha = M.hashes_list([dec(e) for e in c["absent"]], k)
        ai = np.array([i for i, _ in c["absent_probes"]])
        af = np.array([f for _, f in c["absent_probes"]])
        assert M.bank_check(rows, m, k, ha[ai], af).astype(int).tolist() == c["absent_answers"]
        assert M.bank_check(rows, m, k, hp[pi], np.full(pi.size, F)).sum() == 0  # an id beyond the bank answers False


def test_vectorised_hashes_equal_the_per_key_chain():
    rng = np.random.default_rng(5)
    for L in (0, 1, 7, 16, 33):
        keys = rng.integers(0, 256, (20, L), dtype=np.uint8)
        assert np.array_equal(M.hashes_fixed(keys, 10), M.hashes_list([bytes(r) for r in keys], 10))


def test_regenerating_the_fixture_gives_the_committed_bytes(tmp_path):
    if not (REF / "probables").is_dir():
        pytest.skip("the reference checkout is not on this machine")
    out = tmp_path / "golden_bank.json"
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, str(ROOT / "tests" / "golden" / "gen_golden_bank.py"), str(REF), str(out)], check=True, env=env, capture_output=True)
    assert out.read_bytes() == PATH.read_bytes()
