"""tests/edge_hashes.py checked on the host: the chosen hashes hit the cells they were built for (Python integers), and the numpy references
agree with the sequential oracle on pre-hashed streams -- keys whose hashes all name one cell and hash rows with k + 3 columns included."""

import numpy as np
import pytest

import edge_hashes as E

U64 = 1 << 64
BLOOM_M = [E.bloom_bits(*g) for g in (E.BLOOM_DIRECT, E.BLOOM_2P28, E.BLOOM_NP2, E.BLOOM_2P31)]
CBF_M = [E.bloom_bits(*g) for g in (E.CBF_DIRECT, E.CBF_SLICES32, E.CBF_NIBBLE, E.CBF_WINDOW)]
ALL_M = sorted({*BLOOM_M, *CBF_M, *(w for w, _ in E.CMS_SHAPES)})


def test_the_geometries_are_the_ones_the_gpu_tests_count_on(oracle):
    assert [oracle.bloom_params(*g)[2] for g in (E.BLOOM_DIRECT, E.BLOOM_2P28, E.BLOOM_NP2, E.BLOOM_2P31)] == BLOOM_M
    assert BLOOM_M[1] == 2**28 and not E.is_pow2(BLOOM_M[2])
    assert 2**31 - 2**24 < BLOOM_M[3] < 2**31          # reduce_small's r = h - q * m reaches towards 2 m ~ 2^32
    assert CBF_M[1] < 2**25 and 2**23 < CBF_M[2] < 2**24 < CBF_M[3]


@pytest.mark.parametrize("m", ALL_M)
def test_edge_cells(m):
    cells = E.edge_cells(m)
    got = set(cells.tolist())
    assert cells.tolist() == sorted(got) and cells[0] == 0 and cells[-1] == m - 1 and {1, m - 2} <= got
    for s in range(10, 21):
        last = (m - 1) >> s << s
        assert last in got, "first cell of the final (partial) block"
        if last:
            assert {last - 1, 1 << s, (1 << s) - 1} <= got
    assert cells.size <= 4 + 11 * 2 * 130


@pytest.mark.parametrize("m", ALL_M)
def test_hashes_for_hits_the_cells(m):
    cells = E.edge_cells(m)
    for how in ("low", "high", "mid"):
        hs = [int(h) for h in E.hashes_for(cells, m, how)]
        assert [h % m for h in hs] == cells.tolist(), how
        if how == "low":
            assert hs == cells.tolist()
        if how == "high":
            assert all(h + m >= U64 for h in hs)
            if E.is_pow2(m):
                assert all(h >> 32 == 0xFFFFFFFF for h in hs)
    if E.is_pow2(m):
        with pytest.raises(AssertionError):
            E.hashes_for([0], m, "short")
        return
    magic = U64 // m
    lo, hi = E.short_cells(m)
    assert lo == 0 and lo < hi < m
    for seed in (None, 3):
        hs = [int(h) for h in E.hashes_for([lo, hi], m, "short", seed)]
        assert [h % m for h in hs] == [lo, hi]
        assert all((h * magic) >> 64 == h // m - 1 for h in hs), "the truncated quotient is one short: the correction runs"
    assert int(E.hashes_for([hi], m, "short", None)[0]) > U64 - 2 * m  # (the largest such hash of the class)
    # one past the largest remainder no hash qualifies, and a multiple of m always does
    if hi + 1 < m:
        with pytest.raises(AssertionError):
            E.hashes_for([hi + 1], m, "short")
    assert (m * magic) >> 64 == 0


def _stream(m, k, n, seed, cols):
    """n hash rows of `cols` >= k columns: boundary cells through every route, ordinary rows, rows whose k hashes name ONE cell and rows with
    k - 1 on one cell; the columns beyond k hold noise that must not count"""
    rng = np.random.default_rng(seed)
    h = rng.integers(0, 2**63, size=(n, cols), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    cells = E.edge_cells(m)
    edge = E.any_how(rng.choice(cells, size=(n // 4) * k), m, seed).reshape(-1, k)
    h[: n // 4, :k] = edge
    one = E.any_how(np.repeat(rng.choice(cells, size=n // 8), k), m, seed + 1).reshape(-1, k)
    h[n // 4: n // 4 + n // 8, :k] = one
    if k > 1:
        h[n // 4: n // 4 + n // 16, k - 1] = h[: n // 16, 0]  # k - 1 on one cell, the last elsewhere
    return h


@pytest.mark.parametrize("m,k", [(9586, 7), (1 << 12, 5), (1021, 3), (64, 20)])
def test_bloom_reference_agrees_with_the_oracle(oracle, m, k):
    h = _stream(m, k, 2000, 1, k + 3)
    ob = oracle.OracleBloom(m, k)
    ob.add_hashes(h[:1000])
    idx = E.indices(h, m, k)
    table = E.bloom_table(m, idx[:1000])
    assert np.array_equal(table, ob.bloom)
    want = ob.check_hashes(h)
    assert 0 < int(want.sum()) and (m == 64 or int(want.sum()) < 2000)
    assert np.array_equal(E.bloom_check(table, idx).astype(np.uint8), want)
    assert m % 8 == 0 or table[-1] >> (m % 8) == 0, "bits beyond m stay clear"


@pytest.mark.parametrize("m,k", [(9586, 7), (1 << 12, 5), (1021, 3)])
def test_cbf_reference_agrees_with_the_oracle(oracle, m, k):
    h = _stream(m, k, 2000, 2, k + 3)
    w = np.random.default_rng(5).choice([1, 7, 3000], size=2000)
    oc = oracle.OracleCBF(m, k)
    ref = E.cbf_counters(m)
    for row, wi in zip(h, w):
        oc.add_alt(row, int(wi))
    idx = E.indices(h, m, k)
    ref.add(idx, w)
    assert np.array_equal(ref.table(np.uint32), oc.bloom) and ref.els == oc.els_added
    # all k hashes on one cell put k * w into it
    one = slice(500 + 125, 750)
    assert (ref.exact[idx[one, 0]] >= k * w[one]).all() and (idx[one] == idx[one, :1]).all()
    # check: the first k columns, and check_alt's min over ALL supplied columns
    assert np.array_equal(ref.values(idx).min(axis=1), [oc.check_alt(r[:k]) for r in h])
    assert np.array_equal(ref.values(E.indices(h, m, k + 3)).min(axis=1), [oc.check_alt(r) for r in h])
    # removes of what was added (every counter stays >= 0 and below the rail)
    back = np.arange(0, 2000, 3)
    for i in back:
        oc.remove_alt(h[i], int(w[i]))
    ref.remove(idx[back], w[back])
    assert np.array_equal(ref.table(np.uint32), oc.bloom) and ref.els == oc.els_added
    # the rail: adds that carry a counter to 2^32 - 2, to 2^32 - 1 and past it (k distinct cells: next to the rail the reference's
    # repeated-index add overflows its array and raises)
    top_cells = E.edge_cells(m)[-k:]
    top = E.hashes_for(top_cells, m, "high").reshape(1, k)
    for wi in (2**32 - 2 - int(ref.exact[top_cells].max()), 1, 5):
        oc.add_alt(top[0], wi)
        ref.add(E.indices(top, m, k), wi)
        assert np.array_equal(ref.table(np.uint32), oc.bloom) and ref.els == oc.els_added
    assert ref.table(np.uint32)[top_cells].max() == 2**32 - 1 and ref.exact[top_cells].max() == 2**32 + 4


@pytest.mark.parametrize("width,depth", [(7, 3), (1021, 4), (1 << 10, 5), (997, 8)])
def test_cms_reference_agrees_with_the_oracle(oracle, width, depth):
    rng = np.random.default_rng(9)
    h = rng.integers(0, 2**63, size=(2000, depth), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    cells = E.edge_cells(width)
    h[:600] = E.any_how(rng.choice(cells, size=600 * depth), width, 4).reshape(600, depth)
    h[600:900, 0] = h[600, 0]  # keys that collide in ONE row only
    w = rng.choice([0, 1, 15, 16, 4000], size=2000)
    idx = E.cms_indices(h, width, depth)
    for query in ("min", "mean", "mean-min"):
        oc = oracle.OracleCMS(width, depth, query)
        want = np.array([oc.add_alt(row, int(wi)) for row, wi in zip(h, w)], dtype=np.int64)
        got, bins, els = E.cms_running(width, depth, h, w, query)
        assert np.array_equal(got, want), query
        ref = E.cms_counters(width, depth)
        ref.add(idx, w)
        assert np.array_equal(ref.table(np.int32), oc.bins) and np.array_equal(bins, oc.bins) and ref.els == els == oc.els_added
        assert np.array_equal(E.cms_query(ref.values(idx), query, width, ref.els), [oc.check_alt(r) for r in h]), query
        back = np.arange(0, 2000, 5)
        for i in back:
            oc.remove_alt(h[i], int(w[i]))
        ref.remove(idx[back], w[back])
        assert np.array_equal(ref.table(np.int32), oc.bins) and ref.els == oc.els_added
        assert np.array_equal(E.cms_query(ref.values(idx), query, width, ref.els), [oc.check_alt(r) for r in h]), query
    # the rail at 2^31 - 1
    oc = oracle.OracleCMS(width, depth)
    ref = E.cms_counters(width, depth)
    for wi in (2**31 - 2, 1, 9):
        oc.add_alt(h[0], wi)
        ref.add(idx[:1], wi)
        assert np.array_equal(ref.table(np.int32), oc.bins) and ref.els == oc.els_added
