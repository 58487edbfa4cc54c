"""tests/edge_hashes.py checked on the host: the chosen hashes hit the cells they were built for (Python integers), and the numpy references
agree with the sequential oracle on pre-hashed streams -- keys whose hashes all name one cell and hash rows with k + 3 columns included.
The cuckoo filter's triples: ``ck_triples`` is the model's and the reference's rule, its chosen inputs reach both branches of the index
arithmetic, and each way that arithmetic could be subtly wrong, restated here, gives another answer on them."""

import os
import sys
from pathlib import Path

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


@pytest.mark.parametrize("query", ("min", "mean", "mean-min"))
@pytest.mark.parametrize("width,depth", [(7, 3), (3, 4), (777, 5), (300, 8)])
def test_vectorised_running_reference_is_the_loop(width, depth, query):
    """results, touched bins (and nothing else changed), elements_added and clamp count of ``cms_running_vec`` against the Python-integer
    loop: preloaded negative and at-rail bins, weights of 0 and of INT32_MAX, elements_added starting 10 under INT64_MAX"""
    rng = np.random.default_rng(width + depth)
    n = 1500
    cols = rng.integers(0, width, size=(n, depth))
    cols[::2, 0] = width - 1  # one long segment
    h = E.lift(cols, width, 3)
    pre = rng.integers(0, 50, size=width * depth).astype(np.int32)
    pre[0::5], pre[1::5], pre[2::5] = E.I32_MAX, -(2**31), E.I32_MAX - 20
    pre[3::5] = -7
    weights = {
        "small": rng.choice([0, 1, 2, 9], size=n),
        "rail": rng.choice([0, 1, E.I32_MAX, E.I32_MAX - 1, 12345], size=n),
        "ones": None,
    }
    # (elements_added - bin must stay inside int64 for mean-min: the high start goes with an empty or non-negative table)
    pos = np.where(pre < 0, 3, pre)
    starts = [(None, 0), (pre, 5), (pos, E.I64_MAX - 10), (None, E.I64_MAX - 10), (pos, E.I64_MAX)]
    if query != "mean-min":
        starts.append((pre, E.I64_MAX - 10))
    for name, w in weights.items():
        for bins, els in starts:
            want, wbins, wels, wclamps = E.cms_running_counted(width, depth, h, w, query, bins, els)
            got, touched, gels, gclamps = E.cms_running_vec(width, depth, h, w, query, bins, els)
            assert np.array_equal(got, want) and got.dtype == np.int64, (name, els)
            after = np.zeros(width * depth, dtype=np.int64) if bins is None else bins.astype(np.int64)
            assert set(touched) == set(np.unique(E.cms_indices(h, width, depth)).tolist())
            after[list(touched)] = list(touched.values())
            assert np.array_equal(after, wbins), (name, els)
            assert (gels, gclamps) == (wels, wclamps), (name, els)
            assert E.cms_running(width, depth, h, w, query, bins, els)[2] == wels  # (the three-value form is unchanged)
    assert E.cms_running_counted(width, depth, h, weights["rail"], query, pre, 5)[3] > 0
    # a uniform preload given as one integer, and the empty batch
    want = E.cms_running_counted(width, depth, h, weights["small"], query, np.full(width * depth, E.I32_MAX - 500, dtype=np.int32), 9)
    got = E.cms_running_vec(width, depth, h, weights["small"], query, E.I32_MAX - 500, 9)
    assert np.array_equal(got[0], want[0]) and got[2:] == want[2:] and all(want[1][k] == v for k, v in got[1].items())
    assert E.cms_running_vec(width, depth, h[:0], None, query, None, 77)[1:] == ({}, 77, 0)
    # several queries in one walk of the rows
    both = E.cms_running_vec(width, depth, h, weights["small"], ("min", query), pre, 5)
    one = E.cms_running_vec(width, depth, h, weights["small"], query, pre, 5)
    assert isinstance(both[0], tuple) and np.array_equal(both[0][1], one[0]) and both[1:] == one[1:]
    assert np.array_equal(both[0][0], E.cms_running(width, depth, h, weights["small"], "min", pre, 5)[0])


@pytest.mark.parametrize("width", (1, 2, 255, 256, 257, 65536, 65537, 2**24, 2**24 + 1, 2**28 + 3))
def test_running_digit_columns(width):
    n = 5000
    cols = E.running_digit_columns(width, n, 1)
    assert cols.shape == (n,) and cols.dtype == np.int64 and 0 <= cols.min() and cols.max() < width
    got = set(cols.tolist())
    assert {c for c in (*E.RUN_DIGIT_EDGES, width - 1) if c < width} <= got
    ndigits = max(1, ((width - 1).bit_length() + 7) // 8)
    assert ndigits == {1: 1, 2: 1, 255: 1, 256: 1, 257: 2, 65536: 2, 65537: 3, 2**24: 3, 2**24 + 1: 4, 2**28 + 3: 4}[width]
    if width > 1:
        u = np.array(sorted(got), dtype=np.int64)
        x = u[:, None] ^ u[None, :] if u.size <= 600 else None
        for d in range(ndigits):  # a pair of columns that differ in digit d alone
            if x is not None:
                assert ((x != 0) & ((x & ~(0xFF << (8 * d))) == 0)).any(), d
            else:
                rest = u & ~np.int64(0xFF << (8 * d))
                assert (np.unique(rest, return_counts=True)[1] > 1).any(), d
    # interleaved: a chosen column's ops are spread over the three sort tiles of the batch
    if width > 600:
        where = np.flatnonzero(cols == width - 1)
        assert where.size >= 2 and np.unique(cols).size > 1000


# ------------------------------------------------------------------ cuckoo filter
CK_FPS = E.ck_edge_fingerprints(0)
CK_CORRECTED = (3, 37, 1_000_003, 1_610_612_737, 2_146_483_645)
CK_REF = Path(os.environ.get("PYPROBABLES_REFERENCE", "/root/reference"))


def test_ck_edge_fingerprints_hold_what_they_promise():
    got = set(CK_FPS)
    assert {0, 1, 2**31 - 1, 2**31, 2**32 - 1} <= got and all({10**k - 1, 10**k} <= got for k in range(1, 10))
    assert all(sum(fp.bit_length() == n for fp in CK_FPS) >= 8 for n in range(1, 33))
    assert CK_FPS == E.ck_edge_fingerprints(0) != E.ck_edge_fingerprints(1)
    assert E.CK_CAPACITIES == (1, 2, 3, 37, 4096, 1_000_003, 2**30, 1_610_612_737, 2_146_483_645, 2**31 - 1)
    assert E.fnv_1a("") == E.FNV_BASIS and E.fnv_1a(b"a") == E.fnv_1a("a") == 0xAF63DC4C8601EC8C  # (the published test vector)


@pytest.mark.parametrize("bits", [1, 4, 8, 13, 21, 29, 32])
@pytest.mark.parametrize("cap", [1, 3, 37, 4096, 1_000_003, 2_146_483_645, 2**31 - 1])
def test_ck_triples_equal_the_model(cap, bits):
    import cuckoo_model as M

    m = M.CuckooModel.__new__(M.CuckooModel)  # (no table of `cap` rows: only the two functions of capacity and width)
    m.capacity, m.finger_bits = cap, bits
    hashes = [fp | (i * 0x9E3779B97F4A7C15 % U64 & ~0xFFFFFFFF) for i, fp in enumerate(CK_FPS[:600])]  # noise above the fingerprint
    assert E.ck_triples(hashes, cap, bits) == [(fp := h & ((1 << bits) - 1), *m.indices(fp)) for h in hashes]
    keys = [f"k{i}" for i in range(50)] + ["é€", b"\x00\xff", ""]
    assert E.ck_triples([E.fnv_1a(k) for k in keys], cap, bits) == [(m.fingerprint(k), *m.indices(m.fingerprint(k))) for k in keys]
    assert [E.fnv_1a(k) for k in keys] == [M.fnv_1a(k) for k in keys]


def test_ck_triples_equal_the_live_reference():
    if not (CK_REF / "probables").is_dir():
        pytest.skip("the reference checkout is not on this machine")
    sys.path.insert(0, str(CK_REF))
    try:
        from probables import CuckooFilter
    finally:
        sys.path.remove(str(CK_REF))
    keys = [f"k{i}" for i in range(200)] + ["é€", ""]
    for rate, B, bits in ((0.5, 4, 4), (0.01, 4, 10), (0.001, 5, 14), (1e-5, 7, 21), (1e-6, 16, 25), (1e-7, 16, 29), (1e-8, 16, 32)):
        for cap in (3, 37, 1_000_003, 2_146_483_645, 2**31 - 1):
            ref = CuckooFilter.init_error_rate(rate, capacity=5, bucket_size=B)
            assert ref.fingerprint_size_bits == bits
            ref._cuckoo_capacity = cap  # (the two functions under test read nothing else; a table of 2^31 rows is not built)
            assert [ref._generate_fingerprint_info(k) for k in keys] == [(i1, i2, fp) for fp, i1, i2 in E.ck_triples(map(E.fnv_1a, keys), cap, bits)]
            some = [fp for fp in CK_FPS[:300] if fp < 1 << bits]
            assert [ref._indicies_from_fingerprint(fp) for fp in some] == [t[1:] for t in E.ck_triples(some, cap, 32)]


@pytest.mark.parametrize("cap", CK_CORRECTED)
def test_ck_fingerprints_reach_both_branches_of_the_correction(cap):
    short = sum(E.ck_short(E.fnv_1a(str(fp)), cap) for fp in CK_FPS)
    print(cap, short, len(CK_FPS) - short)
    assert short >= 100 and len(CK_FPS) - short >= 100
    # (2^31 - 1 leaves 2^64 mod c = 4: next to no hash is short there, which is why the two capacities above stand next to it)
    assert sum(E.ck_short(E.fnv_1a(str(fp)), 2**31 - 1) for fp in CK_FPS) < 100


def _decimal_hash(fp, places=10, keep_last_zero=True):
    """fnv_1a(str(fp)) as a digit loop from the most significant of `places` places, leading zeros suppressed"""
    h, started, p = E.FNV_BASIS, False, 10 ** (places - 1)
    for k in range(places):
        digit = fp // p
        fp -= digit * p
        started = started or digit != 0 or (keep_last_zero and k == places - 1)
        if started:
            h = ((h ^ (0x30 + digit)) * E.FNV_PRIME) % U64
        p //= 10
    return h


def test_ck_inputs_tell_the_wrong_variants_apart():
    """each way the triples could be subtly wrong, restated here: on the chosen inputs its output differs from ck_triples"""
    assert [_decimal_hash(fp) for fp in CK_FPS] == [E.fnv_1a(str(fp)) for fp in CK_FPS]  # (the loop written right IS str())
    for cap in CK_CORRECTED:
        want = [t[2] for t in E.ck_triples(CK_FPS, cap, 32)]
        magic = U64 // cap
        uncorrected = [(h := E.fnv_1a(str(fp))) - ((h * magic) >> 64) * cap for fp in CK_FPS]
        wrong = [fp for fp, a, b in zip(CK_FPS, uncorrected, want) if a != b]
        assert len(wrong) >= 100 and all(E.ck_short(E.fnv_1a(str(fp)), cap) for fp in wrong), "the estimate without its correction"
    for cap in E.CK_CAPACITIES[1:]:
        want = {fp: t[2] for fp, t in zip(CK_FPS, E.ck_triples(CK_FPS, cap, 32))}
        if cap >= 37:  # (modulo 2 and 3 the empty string and "0" happen to agree)
            assert _decimal_hash(0, keep_last_zero=False) % cap != want[0], "fp == 0 hashed as the empty string"
        big = [fp for fp in CK_FPS if fp >= 10**9]
        assert len(big) > 1000 and 10**9 in big and 2**32 - 1 in big
        assert sum(_decimal_hash(fp, places=9) % cap != want[fp] for fp in big) >= 1000, "a digit loop of 9 places"
    # the mask: bits rounded up to whole bytes, and idx_2 from the hash before the mask
    rng = np.random.default_rng(8)
    hashes = [int(h) for h in rng.integers(0, 2**64, size=200, dtype=np.uint64)] + [U64 - 1, 1 << 63]
    for bits in range(1, 33):
        want = E.ck_triples(hashes, 1_000_003, bits)
        if bits % 8:
            assert E.ck_triples(hashes, 1_000_003, (bits + 7) // 8 * 8) != want and want[-2][0] == (1 << bits) - 1, "a byte mask for a bit mask"
        if bits < 32:
            unmasked = [(fp, i1, E.fnv_1a(str(h & 0xFFFFFFFF)) % 1_000_003) for h, (fp, i1, _) in zip(hashes, want)]
            assert sum(a != b for a, b in zip(unmasked, want)) >= 100, "idx_2 from the unmasked hash"
        assert want[-1] == (0, 0, E.fnv_1a("0") % 1_000_003)  # 2^63: nothing of it is left
