"""tests/bank_stats_model.py against every record of tests/golden/golden_bank_stats.json (the REAL reference's answers): the rows are built
with bank_model's restatement of the reference's hash, then bit counts, estimates, rates, the full intersection matrix, the recorded jaccards
and the folded rows must all be the reference's.  No GPU, no engine."""

import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import bank_model as M  # noqa: E402
import bank_stats_model as S  # noqa: E402

G = json.loads((ROOT / "tests" / "golden" / "golden_bank_stats.json").read_text())


sent_indices, fixture_keys = S.sent_indices, S.fixture_keys


def model_table(c):
    keys, ids = fixture_keys(c)
    m, k = c["number_bits"], c["number_hashes"]
    return S.as_words(M.bank_rows(c["filters"], m, k, M.hashes_list(keys, k), ids))


@pytest.fixture(scope="module", params=[0, 1])
def case(request):
    c = G["cases"][request.param]
    return c, model_table(c)


def test_the_fixture_holds_its_edge_cases():
    for c in G["cases"]:
        m = c["number_bits"]
        assert c["bits"][G["full"]] == m and c["estimate"][G["full"]] == -1 and c["bits"][G["empty"]] == 0 and c["estimate"][G["empty"]] == 0
        a, b = G["same"]
        assert c["sent"][a] == c["sent"][b] and c["intersections"][a][b] == c["bits"][a] > 0
        a, b = G["disjoint"]
        assert c["intersections"][a][b] == 0 and c["bits"][a] > 0 and c["bits"][b] > 0
        assert len(c["jaccard_hex"]) >= 200 and len(c["groups"]) >= 10
        assert c["elements_added"] == [len(sent_indices(s)) for s in c["sent"]]


def test_counts_estimates_and_rates(case):
    c, table = case
    m, k = c["number_bits"], c["number_hashes"]
    assert table.shape == (c["filters"], M.row_bytes(m) // 4)
    assert S.popcount(table).tolist() == c["bits"]
    assert S.estimates(table, m, k).tolist() == c["estimate"]
    assert [S.false_positive_rate(e, m, k).hex() for e in c["elements_added"]] == c["fpr_hex"]
    ids = [69, 0, 5, 5, 41, 70, 1000]  # any order, repeats, beyond the table
    assert S.popcount(table, ids).tolist() == [c["bits"][f] if f < 70 else 0 for f in ids]


def test_overlap_and_jaccard(case):
    c, table = case
    want = np.array(c["intersections"], dtype=np.int64)
    got = S.overlap(table)
    assert np.array_equal(got, want) and np.array_equal(got, got.T) and np.array_equal(np.diag(got), c["bits"])
    a, b = [3, 3, 69, 41, 200], [5, 0, 70, 7, 8, 7]
    sub = S.overlap(table, a, None, b)
    for i, fa in enumerate(a):
        for j, fb in enumerate(b):
            assert sub[i, j] == (want[fa, fb] if fa < 70 and fb < 70 else 0)
    bits = np.array(c["bits"], dtype=np.int64)
    jac = S.jaccard(got, bits, bits)
    for i, j, h in c["jaccard_hex"]:
        assert float(jac[i, j]).hex() == h, (i, j)
    assert jac[G["empty"], G["empty"]] == 1.0 and jac[G["empty"], 0] == 0.0 and jac[G["same"][0], G["same"][1]] == 1.0


def test_folds(case):
    c, table = case
    m, k = c["number_bits"], c["number_hashes"]
    groups = [g["members"] for g in c["groups"]]
    nbytes = (m + 7) // 8
    for op, name in (("or", "union"), ("and", "intersection")):
        rows = S.reduce_rows(table, groups, op)
        est = S.estimates(rows, m, k)
        for g, rec in enumerate(c["groups"]):
            raw = rows[g].view(np.uint8)
            assert bytes(raw[:nbytes]).hex() == rec[name]["row_hex"] and not raw[nbytes:].any(), (op, g)
            assert int(est[g]) == rec[name]["elements_added"], (op, g)
    assert not S.reduce_rows(table, [[], [3]], "and")[0].any() and not S.reduce_rows(table, [[]], "or").any()
    assert not S.reduce_rows(table, [[3, 70]], "and").any()  # a member beyond the table is an empty row
    assert np.array_equal(S.reduce_rows(table, [[3, 70]], "or")[0], table[3])
