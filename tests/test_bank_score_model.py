"""BloomFilterBank.score_many without a GPU: the numpy model (tests/bank_score_model.py) on what the REAL reference answered for every
(probe, filter) pair of tests/golden/golden_bank_match.json, the facts about that fixture the GPU tests lean on, the pure threshold helper of
the package against the model's restatement, and the C ABI's declarations and argument checks that run in front of any HIP call."""

import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import bank_match_model as MM  # noqa: E402
import bank_model as M  # noqa: E402
import bank_score_model as SM  # noqa: E402

G = json.loads((ROOT / "tests" / "golden" / "golden_bank_match.json").read_text())
# per case: the longest sent[f], the highest score of a query sent[f] in a filter other than f, and the highest number of filters that half
# of such a query selects -- read off the fixture; the score of the whole probe list peaks at 54 / 134
FACTS = [dict(full=15, other=9, half=8, whole=54), dict(full=121, other=64, half=6, whole=134)]


def dec(e):
    return e[1] if e[0] == "s" else bytes.fromhex(e[1])


def reference_bits(c):
    return np.array([[(int.from_bytes(bytes.fromhex(h), "little") >> f) & 1 for f in range(c["filters"])] for h in c["masks"]], dtype=bool)


@pytest.mark.parametrize("ci", [0, 1])
def test_model_on_the_reference_answers(ci):
    c, facts = G["cases"][ci], FACTS[ci]
    F, m, k = c["filters"], c["number_bits"], c["number_hashes"]
    want = reference_bits(c)
    idx, offs = SM.fixture_queries(c)
    S = SM.score_counts(want[idx], offs)
    assert S.shape == (F + 2, F) and S.dtype == np.int32
    for q in range(F + 2):  # the definition, spelled out: a sum of the reference's answers over the query's keys
        assert S[q].tolist() == [sum(int(want[i, f]) for i in idx[offs[q]:offs[q + 1]]) for f in range(F)]
    # the model's own row-AND gives the same bits as the reference, so the GPU tests may score chosen tables with it
    pool = [dec(e) for e in c["pool"]]
    probes = pool + [dec(e) for e in c["absent"]]
    rows = M.bank_rows(F, m, k, M.hashes_list(pool, k)[np.array([i for f in range(F) for i in c["sent"][f]])], np.array([f for f in range(F) for _ in c["sent"][f]]))
    mine = MM.mask_bits(MM.match_mask(MM.slices_of(rows, F, m), m, k, M.hashes_list(probes, k)), F)
    assert np.array_equal(SM.score_counts(mine[idx], offs), S)
    # the facts about the fixture
    lens = np.diff(offs)
    empty = G["empty_filter"]
    assert empty == 41 and lens[empty] == 0 and not S[empty].any() and lens[:F].max() == facts["full"]
    own = S[np.arange(F), np.arange(F)]
    assert own.tolist() == lens[:F].tolist()  # no false negatives: a filter holds all it was sent
    others = S[:F].copy()
    others[np.arange(F), np.arange(F)] = -1
    assert others.max() == facts["other"] < facts["full"]
    assert all((S[q] == 0).any() for q in range(F))
    t = SM.thresholds(lens, 0.5)
    o, ids, sc = SM.select(S, t)
    per = np.diff(o)
    assert per[empty] == 0
    held = per[:F][lens[:F] > 0]
    assert held.min() == 1 and held.max() == facts["half"] and (held == 1).sum() >= 10  # the threshold separates: often the own filter alone
    for q in range(F):
        if lens[q]:
            assert q in ids[o[q]:o[q + 1]].tolist()
    assert S[F][empty] == 0 and S[F].max() == facts["whole"] and lens[F] == len(probes)
    assert lens[F + 1] == 60 and S[F + 1].max() < S[F].max()


def test_select_of_the_model():
    counts = np.array([[0, 3, 2, 3], [0, 0, 0, 0], [5, 5, 5, 5], [1, 2**31 - 1, 7, 0]], dtype=np.int64)
    o, ids, sc = SM.select(counts, [3, 1, 5, 2**31 - 1])
    assert o.tolist() == [0, 2, 2, 6, 7] and ids.tolist() == [1, 3, 0, 1, 2, 3, 1] and sc.tolist() == [3, 3, 5, 5, 5, 5, 2**31 - 1]
    assert ids.dtype == np.int32 and sc.dtype == np.int32 and o.dtype == np.int64
    o, ids, sc = SM.select(np.zeros((0, 4), dtype=np.int32), [])
    assert o.tolist() == [0] and ids.size == 0 and sc.size == 0


def test_score_thresholds_against_the_model():
    from pyprobables_amd.bank import score_thresholds

    lens = np.array([0, 1, 2, 3, 4, 10, 15, 120, 121, 1000, 2**20], dtype=np.int64)
    for t in (1, 2, 7, 2**31 - 1, np.int64(5)):
        got = score_thresholds(lens, t)
        assert got.dtype == np.uint32 and got.tolist() == SM.thresholds(lens, int(t)).tolist() == [int(t)] * lens.size
    arr = np.arange(1, lens.size + 1)
    for a in (arr, arr.astype(np.uint32), list(arr)):
        assert score_thresholds(lens, a).tolist() == SM.thresholds(lens, arr).tolist() == arr.tolist()
    # fractions: lengths 0 and 1, and products that are exact integers (0.5 * 2, 0.25 * 4, 0.1 * 10 -- 0.1 is above one tenth, so 0.1 * 1000
    # is 100.00000000000001 in exact arithmetic but exactly 100.0 after the one rounding both sides do)
    for f in (0.5, 0.25, 0.75, 1.0, 0.1, 0.3, 1e-9, np.float64(0.5), np.float32(0.2)):
        got = score_thresholds(lens, f)
        assert got.dtype == np.uint32 and got.tolist() == SM.thresholds(lens, float(f)).tolist(), f
        assert got[0] == 1 and got[1] == 1 and (got >= 1).all() and (got <= np.maximum(lens, 1)).all()
    assert score_thresholds(lens, 0.5).tolist() == [1, 1, 1, 2, 2, 5, 8, 60, 61, 500, 2**19]
    assert score_thresholds(lens, 1.0).tolist() == np.maximum(lens, 1).tolist()
    assert score_thresholds(np.zeros(0, dtype=np.int64), 3).size == 0 and score_thresholds(np.zeros(0, dtype=np.int64), []).size == 0
    for bad in (0, -1, 2**32, 0.0, -0.5, 1.5, float("nan"), float("inf"), [0] * lens.size, [-1] * lens.size, [1, 2], np.array([[1] * lens.size])):
        with pytest.raises((ValueError, TypeError)):
            score_thresholds(lens, bad)
    for bad in (0, 1.5, 0.0, [0] * lens.size, [1, 2]):
        with pytest.raises(ValueError):
            score_thresholds(lens, bad)
    for bad in (True, "1", None, [0.5] * lens.size, 1 + 0j):
        with pytest.raises(TypeError):
            score_thresholds(lens, bad)
    with pytest.raises(TypeError):
        score_thresholds(lens.astype(np.float64), 1)


def test_header_declares_both_entries_and_the_prototypes_carry_them():
    from pyprobables_amd import _native as N

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "psk.h").read_text(), flags=re.S)
    for name, args in (("psk_bank_score", 16), ("psk_bank_score_select", 10)):
        decl = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", text)
        assert decl, f"{name} is not declared in include/psk.h"
        assert decl.group(1).count(",") + 1 == args == len(N.PROTOTYPES[name][1])
        assert hasattr(N.lib(), name)


def test_score_calls_reject_bad_arguments_before_touching_a_device():
    from pyprobables_amd import _native as N

    L = N.lib()
    keys = np.zeros((1, 16), dtype=np.uint8)
    img, qo, out = 0x1000, 0x2000, 0x3000  # never dereferenced: every call below fails its checks
    base = (N.KEYS_FIXED, keys.ctypes.data, None, 1, 16)

    def score(image=img, F=70, m=63, k=4, keys=base, offs=qo, queries=1, split=1, scores=out):
        return L.psk_bank_score(image, F, m, k, *keys, N.HOST, offs, queries, split, scores, 0, None)

    assert score(image=None) == N.PSK_EINVAL and "NULL" in N.last_error()
    assert score(offs=None) == N.PSK_EINVAL and "NULL" in N.last_error()
    assert score(scores=None) == N.PSK_EINVAL and "NULL" in N.last_error()
    assert score(k=65) == N.PSK_EINVAL and "at most 64" in N.last_error()
    assert score(k=0) == N.PSK_EINVAL
    assert score(split=0) == N.PSK_EINVAL and "split" in N.last_error()
    assert score(split=65536) == N.PSK_EINVAL and "split" in N.last_error()
    assert score(image=img + 4) == N.PSK_EINVAL and "aligned" in N.last_error()
    assert score(F=0) == N.PSK_EINVAL and score(m=0) == N.PSK_EINVAL and score(m=2**31 + 1) == N.PSK_EINVAL
    assert score(keys=(N.KEYS_HASHES, keys.ctypes.data, None, 1, 3)) == N.PSK_EINVAL
    assert score(keys=(N.KEYS_FIXED, keys.ctypes.data, None, 2**32, 16)) == N.PSK_EINVAL and "2^32" in N.last_error()

    def select(scores=out, queries=1, F=70, thr=qo, count=None, offs=None, ids=None, hit=None):
        return L.psk_bank_score_select(scores, queries, F, thr, count, offs, ids, hit, 0, None)

    assert select(scores=None, count=img) == N.PSK_EINVAL and "NULL" in N.last_error()
    assert select(thr=None, count=img) == N.PSK_EINVAL and "NULL" in N.last_error()
    assert select() == N.PSK_EINVAL and "no output" in N.last_error()
    assert select(ids=img) == N.PSK_EINVAL and "go together" in N.last_error()
    assert select(offs=img) == N.PSK_EINVAL and "go together" in N.last_error()
    assert select(offs=img, hit=img) == N.PSK_EINVAL and "go together" in N.last_error()
    assert select(hit=img) == N.PSK_EINVAL and "hit_scores_dev" in N.last_error()
    assert select(count=img, hit=img) == N.PSK_EINVAL and "hit_scores_dev" in N.last_error()
    assert select(F=0, count=img) == N.PSK_EINVAL
