"""The filters of a BloomFilterBank as sets, on the GPU: bit counts and estimates (psk_bank_popcount), all-pairs overlap and jaccard
(psk_bank_overlap) and the union / intersection of groups of filters (psk_bank_reduce).  The answers are the reference's -- every record of
tests/golden/golden_bank_stats.json, written by the REAL reference -- and, where the reference has nothing to say (chosen tables at the
kernel's tile, chunk and grid seams, tables beyond 4 GiB, rows of 2^31 bits), the numpy model's (tests/bank_stats_model.py, checked against
that fixture in tests/test_bank_stats_model.py).  Every output buffer of a direct C ABI call has sentinel words behind it."""

import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import bank_match_model as MM  # noqa: E402
import bank_model as M  # noqa: E402
import bank_stats_model as S  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

G = json.loads((ROOT / "tests" / "golden" / "golden_bank_stats.json").read_text())
SENTINEL = 0x5A5AA5A5
GUARD = 8  # sentinel words behind every output


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


@pytest.fixture(scope="module")
def B(pa):
    from pyprobables_amd import bank

    return bank


def _dev(a):
    a = np.ascontiguousarray(a)  # (unsigned words travel as the signed tensors of the same bits)
    return torch.from_numpy(a.view({np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype))).cuda()


def guarded(words):
    """an int32 device buffer of `words` words, every word and GUARD words behind them the sentinel; 16-byte aligned"""
    return torch.full((words + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")


def guard_ok(t, words):
    return bool((t[words:] == SENTINEL).all().item())


def ptr(t):
    return None if t is None else t.data_ptr()


def ids_dev(ids):
    return None if ids is None else _dev(np.asarray(ids, dtype=np.uint32))


def c_popcount(N, table, F, m, ids, n):
    """psk_bank_popcount -> int64[n], sentinels checked"""
    out = guarded(2 * n)
    idt = ids_dev(ids)
    N.check(N.lib().psk_bank_popcount(table.data_ptr(), F, m, ptr(idt), n, out.data_ptr(), 0, None))
    torch.cuda.synchronize()
    assert guard_ok(out, 2 * n)
    return out[:2 * n].cpu().numpy().view(np.int64)


def c_overlap(N, ta, Fa, a, na, tb, Fb, b, nb, m, same_list=False):
    """psk_bank_overlap -> uint32[na, nb] as int64, sentinels checked; same_list: b is THE pointer of a (the symmetric case with a list)"""
    out = guarded(na * nb)
    ad = ids_dev(a)
    bd = ad if same_list else ids_dev(b)
    N.check(N.lib().psk_bank_overlap(ta.data_ptr(), Fa, ptr(ad), na, tb.data_ptr(), Fb, ptr(bd), nb, m, out.data_ptr(), 0, None))
    torch.cuda.synchronize()
    assert guard_ok(out, na * nb)
    return out[:na * nb].cpu().numpy().view(np.uint32).astype(np.int64).reshape(na, nb)


def c_reduce(N, src, F, m, groups, op, want_bits=True):
    """psk_bank_reduce -> (uint32[G, W], int64[G] or None), sentinels checked"""
    W = M.row_bytes(m) // 4
    Gn = len(groups)
    seg = np.zeros(Gn + 1, dtype=np.uint64)
    np.cumsum([len(g) for g in groups], out=seg[1:])
    members = np.array([f for g in groups for f in g] or [0], dtype=np.uint32)
    dst, bits = guarded(Gn * W), guarded(2 * Gn) if want_bits else None
    sd, md = _dev(seg), _dev(members)  # (held until the kernel has run)
    N.check(N.lib().psk_bank_reduce(src.data_ptr(), F, m, sd.data_ptr(), md.data_ptr(), Gn, op, dst.data_ptr(), ptr(bits), 0, None))
    torch.cuda.synchronize()
    assert guard_ok(dst, Gn * W) and (bits is None or guard_ok(bits, 2 * Gn))
    return dst[:Gn * W].cpu().numpy().view(np.uint32).reshape(Gn, W), None if bits is None else bits[:2 * Gn].cpu().numpy().view(np.int64)


def random_table(F, W, rng, density=0.5):
    """uint32[F, W]: random words of the given bit density; row 0 all ones, the last row all zeros (F > 2)"""
    bits = (rng.random((F, W * 32)) < density).astype(np.uint8)
    t = np.packbits(bits, axis=1, bitorder="little").view(np.uint32).reshape(F, W)
    t[0] = 0xFFFFFFFF
    if F > 2:
        t[F - 1] = 0
    return t


# ------------------------------------------------------------------ the reference's answers
@pytest.fixture(scope="module", params=[0, 1])
def golden(pa, request):
    c = G["cases"][request.param]
    bank = pa.BloomFilterBank(c["filters"], c["est"], c["fpr"])
    keys, ids = S.fixture_keys(c)
    bank.add_many(keys, ids)
    return c, bank


def test_golden_counts_estimates_and_rates(golden):
    c, bank = golden
    assert (bank.number_bits, bank.number_hashes) == (c["number_bits"], c["number_hashes"])
    assert bank.elements_added.tolist() == c["elements_added"]
    bits = bank.bits_set()
    assert bits.is_cuda and bits.dtype == torch.int64 and bits.tolist() == c["bits"]
    est = bank.estimate_elements()
    assert isinstance(est, np.ndarray) and est.dtype == np.int64 and est.tolist() == c["estimate"]
    assert est[G["full"]] == -1 and est[G["empty"]] == 0
    fpr = bank.current_false_positive_rate()
    assert fpr.dtype == np.float64 and [float(x).hex() for x in fpr] == c["fpr_hex"]
    ids = [69, 0, 5, 5, 41]  # any order, repeats; host lists and device tensors
    for form in (ids, np.array(ids), torch.tensor(ids, device="cuda")):
        assert bank.bits_set(form).tolist() == [c["bits"][f] for f in ids]
        assert bank.estimate_elements(form).tolist() == [c["estimate"][f] for f in ids]
    assert bank.bits_set([]).tolist() == [] and bank.estimate_elements(np.zeros(0, dtype=np.int64)).tolist() == []
    for f in (5, 7, 41):
        assert bank.filter(f).estimate_elements() == c["estimate"][f]


def test_golden_overlap_and_jaccard(golden):
    c, bank = golden
    want = np.array(c["intersections"], dtype=np.int64)
    ov = bank.overlap()
    assert ov.is_cuda and ov.dtype == torch.int32 and tuple(ov.shape) == (70, 70)
    assert np.array_equal(ov.cpu().numpy(), want)
    assert torch.equal(ov.T, ov) and torch.equal(torch.diagonal(ov).to(torch.int64), bank.bits_set())
    jac = bank.jaccard()
    assert jac.is_cuda and jac.dtype == torch.float64
    jac = jac.cpu().numpy()
    for i, j, h in c["jaccard_hex"]:
        assert float(jac[i, j]).hex() == h, (i, j)
    bits = c["bits"]
    for i in range(70):  # every other pair against Python's own quotient
        for j in range(70):
            union = bits[i] + bits[j] - int(want[i, j])
            assert jac[i, j] == (1.0 if union == 0 else int(want[i, j]) / union), (i, j)
    a, b = [3, 3, 69, 41, 5], torch.tensor([5, 0, 7, 8, 7, 41, 20], device="cuda")
    sub = bank.overlap(a=a, b=b)
    assert tuple(sub.shape) == (5, 7) and np.array_equal(sub.cpu().numpy(), want[np.ix_(a, b.tolist())])
    assert np.array_equal(bank.jaccard(a=a, b=b).cpu().numpy(), jac[np.ix_(a, b.tolist())])
    assert np.array_equal(bank.overlap(a=a).cpu().numpy(), want[a]) and np.array_equal(bank.overlap(b=a).cpu().numpy(), want[:, a])
    assert tuple(bank.overlap(a=[], b=[1]).shape) == (0, 1)
    # another bank of the same geometry: its filters 0..9 hold what this bank's 60..69 hold
    other = type(bank)(10, c["est"], c["fpr"])
    for f in range(10):
        other.set_filter(f, bank.filter(60 + f))
    assert np.array_equal(bank.overlap(other).cpu().numpy(), want[:, 60:])
    assert np.array_equal(other.overlap(bank, a=[9, 0]).cpu().numpy(), want[[69, 60]])
    assert np.array_equal(bank.jaccard(other, b=[1]).cpu().numpy(), jac[:, 61:62])


def test_golden_folds(golden):
    c, bank = golden
    m = c["number_bits"]
    nbytes = (m + 7) // 8
    groups = [g["members"] for g in c["groups"]]
    offs = np.zeros(len(groups) + 1, dtype=np.int64)
    np.cumsum([len(g) for g in groups], out=offs[1:])
    members = np.array([f for g in groups for f in g], dtype=np.int64)
    forms = (groups, (offs, members), (torch.from_numpy(offs).cuda(), torch.from_numpy(members).cuda()))
    for op, name in (("or", "union"), ("and", "intersection")):
        for form in forms:
            red = bank.reduce(form, op=op)
            assert isinstance(red, type(bank)) and red.num_filters == len(groups) and red.number_bits == m and red.device == bank.device
            rows = red.table_tensor.cpu().numpy().view(np.uint8)
            for g, rec in enumerate(c["groups"]):
                assert bytes(rows[g, :nbytes]).hex() == rec[name]["row_hex"] and not rows[g, nbytes:].any(), (op, g)
            assert red.elements_added.tolist() == [rec[name]["elements_added"] for rec in c["groups"]]
            assert red.elements_added.tolist() == red.estimate_elements().tolist()
    red = bank.reduce([[], [3]])  # an empty group under "or": an empty filter with count 0
    assert not red.table_tensor[0].any().item() and red.elements_added.tolist() == [0, c["estimate"][3]]
    o, mem = torch.tensor([0, 0, 1], device="cuda"), torch.tensor([3], device="cuda")
    red = bank.reduce((o, mem), op="and", validate=False)  # unchecked device data: the zero row
    assert not red.table_tensor[0].any().item() and torch.equal(red.table_tensor[1], bank.table_tensor[3])


# ------------------------------------------------------------------ tile and chunk seams, through the C ABI on raw tables
def test_constants_mirror_the_kernel(B):
    assert (B.BANK_OVERLAP_T, B.BANK_OVERLAP_C, B.BANK_GRID_CAP) == (64, 32, 4096)


@pytest.mark.parametrize("which", ["1", "T-1", "T", "T+1", "2T+1"])
def test_tile_and_chunk_seams(pa, N, B, which):
    T, C = B.BANK_OVERLAP_T, B.BANK_OVERLAP_C
    F = {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1}[which]
    rng = np.random.default_rng(F)
    for W in (4, C - 4, C, C + 4, 2 * C + 4):
        m = 32 * W
        ta, tb = random_table(F, W, rng), random_table(F + 3, W, rng, 0.3)
        da, db = _dev(ta.reshape(-1)), _dev(tb.reshape(-1))
        full = S.overlap(ta)
        assert np.array_equal(c_popcount(N, da, F, m, None, F), S.popcount(ta))
        # symmetric: NULL lists, and one list passed on both sides
        assert np.array_equal(c_overlap(N, da, F, None, F, da, F, None, F, m), full), (F, W)
        perm = rng.permutation(F)
        assert np.array_equal(c_overlap(N, da, F, perm, F, da, F, None, F, m, same_list=True), full[np.ix_(perm, perm)]), (F, W)
        # rectangular, NULL lists: the first na rows against the first nb
        na, nb = max(1, F - 2), max(1, (F + 1) // 2)
        assert np.array_equal(c_overlap(N, da, F, None, na, da, F, None, nb, m), full[:na, :nb]), (F, W)
        # rectangular, lists that are unsorted, repeat, and na != nb
        a, b = rng.integers(0, F, F + 5), rng.integers(0, F, max(1, F // 3) + 2)
        assert np.array_equal(c_overlap(N, da, F, a, a.size, da, F, b, b.size, m), full[np.ix_(a, b)]), (F, W)
        # two tables
        cross = S.overlap(ta, None, tb, None)
        assert np.array_equal(c_overlap(N, da, F, None, F, db, F + 3, None, F + 3, m), cross), (F, W)
        b2 = rng.integers(0, F + 3, 7)
        assert np.array_equal(c_overlap(N, da, F, a, a.size, db, F + 3, b2, 7, m), cross[np.ix_(a, b2)]), (F, W)
        assert np.array_equal(c_popcount(N, da, F, m, a, a.size), S.popcount(ta, a))
        groups = [list(rng.integers(0, F, int(s))) for s in (1, 2, 3, 4, 5, 9, 0)] + [list(range(F))]
        for op, name in ((0, "or"), (1, "and")):
            rows, bits = c_reduce(N, da, F, m, groups, op)
            want = S.reduce_rows(ta, groups, name)
            assert np.array_equal(rows, want) and np.array_equal(bits, S.popcount(want)), (F, W, name)


# rows of 4096 bytes (a wave per row at its widest; one piece of a fold; an overlap in 2 parts of 16 chunks), 4112 (a workgroup per row; two
# pieces; parts of 17 and 16 chunks, the last chunk 4 words) and 12304 (four pieces; six parts)
@pytest.mark.parametrize("W", [1024, 1028, 3076])
def test_row_size_classes(pa, N, W):
    rng = np.random.default_rng(W)
    F, m = 6, 32 * W - 3
    t = random_table(F, W, rng)
    t[:, -1] &= np.uint32((1 << 29) - 1)  # no pad bits
    d = _dev(t.reshape(-1))
    assert np.array_equal(c_popcount(N, d, F, m, None, F), S.popcount(t))
    ids = [5, 0, 0, 3, 9]
    assert np.array_equal(c_popcount(N, d, F, m, ids, 5), S.popcount(t, ids))
    assert np.array_equal(c_overlap(N, d, F, None, F, d, F, None, F, m), S.overlap(t))  # (rows this long are cut into parts that meet through atomics)
    a, b = [4, 1, 1, 7, 0], [0, 5, 2]
    assert np.array_equal(c_overlap(N, d, F, a, 5, d, F, b, 3, m), S.overlap(t, a, None, b))
    groups = [[1, 2], [0, 4, 3, 2, 1], [], [5], [0]]
    for op, name in ((0, "or"), (1, "and")):
        rows, bits = c_reduce(N, d, F, m, groups, op)
        want = S.reduce_rows(t, groups, name)
        assert np.array_equal(rows, want) and np.array_equal(bits, S.popcount(want))
        assert c_reduce(N, d, F, m, groups, op, want_bits=False)[1] is None


def test_ids_beyond_the_table_are_empty_rows(pa, N):
    rng = np.random.default_rng(3)
    F, W = 70, 8
    m = 32 * W
    t = random_table(F, W, rng)
    d = _dev(t.reshape(-1))
    a, b = [0, 70, 5, 2**32 - 1, 69], [71, 1, 1000, 0]
    got = c_overlap(N, d, F, a, 5, d, F, b, 4, m)
    assert np.array_equal(got, S.overlap(t, a, None, b)) and not got[[1, 3]].any() and not got[:, [0, 2]].any() and got[0, 3] == m
    assert c_popcount(N, d, F, m, a, 5).tolist() == [m, 0, int(S.popcount(t)[5]), 0, 0]
    for op, name in ((0, "or"), (1, "and")):
        rows, bits = c_reduce(N, d, F, m, [[3, 70], [70], [3]], op)
        assert np.array_equal(rows, S.reduce_rows(t, [[3, 70], [70], [3]], name)) and np.array_equal(bits, S.popcount(rows))
    L = N.lib()
    out = guarded(16)
    assert L.psk_bank_popcount(d.data_ptr(), F, m, None, F - 1, out.data_ptr(), 0, None) == N.PSK_EINVAL  # NULL ids: n == filters
    assert L.psk_bank_overlap(d.data_ptr(), F, None, F + 1, d.data_ptr(), F, None, 1, m, out.data_ptr(), 0, None) == N.PSK_EINVAL
    assert L.psk_bank_overlap(d.data_ptr(), F, None, 1, d.data_ptr(), F, None, F + 1, m, out.data_ptr(), 0, None) == N.PSK_EINVAL
    assert L.psk_bank_popcount(d.data_ptr(), F, m, out.data_ptr(), 0, out.data_ptr(), 0, None) == N.PSK_OK  # n == 0 launches nothing
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == SENTINEL).all()


def test_grid_cap(pa, N, B):
    """more rows, tiles and row pieces than the grid holds, 16-byte rows: popcount (four rows a workgroup), overlap rectangular and symmetric,
    reduce"""
    cap, T = B.BANK_GRID_CAP, B.BANK_OVERLAP_T
    rng = np.random.default_rng(5)
    F = T * (cap + 1)  # cap + 1 row tiles; more than 4 * cap rows
    t = rng.integers(0, 2**32, (F, 4), dtype=np.uint32)
    t[cap * T] = 0xFFFFFFFF
    d = _dev(t.reshape(-1))
    want = S.popcount(t)
    assert np.array_equal(c_popcount(N, d, F, 128, None, F), want)
    ids = rng.integers(0, F, 4 * cap + 7)
    assert np.array_equal(c_popcount(N, d, F, 128, ids, ids.size), want[ids])
    b = [cap * T, 1, F - 1]
    assert np.array_equal(c_overlap(N, d, F, None, F, d, F, b, 3, 128), S.overlap(t, None, None, b))  # (cap + 1) x 1 tiles
    assert np.array_equal(c_overlap(N, d, F, b, 3, d, F, None, F, 128), S.overlap(t, b, None, None))  # 1 x (cap + 1) tiles
    ntiles = 1
    while ntiles * (ntiles + 1) // 2 <= cap:
        ntiles += 1
    n = (ntiles - 1) * T + 1  # ntiles (ntiles + 1) / 2 > cap tiles on or above the diagonal, the last one a single row wide
    sym = c_overlap(N, d, F, None, n, d, F, None, n, 128)
    assert np.array_equal(sym, S.overlap(t[:n]))
    groups = [[int(x), int(y)] for x, y in rng.integers(0, F, (cap + 5, 2))]
    for op, name in ((0, "or"), (1, "and")):
        rows, bits = c_reduce(N, d, F, 128, groups, op)
        assert np.array_equal(rows, S.reduce_rows(t, groups, name)) and np.array_equal(bits, S.popcount(rows))


def test_addressing_beyond_4_gib(pa, N):
    """65 537 rows of 65 536 bytes: the last row starts at byte 2^32.  A few words are set in rows 0, 65535 and 65536; popcount, overlap and reduce
    are asked about just those rows through id lists.  An overlap whose na * nb passes 2^32 needs an output of 16 GiB beside the table and is
    left out: the output index is computed in 64 bits from the same (row, column) as the ones checked here."""
    F, m, W = 65537, 524288, 16384
    if torch.cuda.mem_get_info()[0] < 6 * 2**30:
        pytest.skip("the device lacks the memory for a 4 GiB bank")
    tab = torch.zeros(F * W, dtype=torch.int32, device="cuda")
    view = tab.view(F, W)
    targets = [0, 65535, 65536]
    small = np.zeros((3, W), dtype=np.uint32)
    small[0, [0, 5, W - 1]] = [0xFFFFFFFF, 0x0F0F0F0F, 0x80000001]
    small[1, [0, 5, 7000]] = [0x0000FFFF, 0xFFFFFFFF, 0x3]
    small[2, [0, 7000, W - 1]] = [0xFF00FF00, 0x1, 0xFFFFFFFF]
    for j, f in enumerate(targets):
        view[f] = _dev(small[j])
    assert c_popcount(N, tab, F, m, targets, 3).tolist() == S.popcount(small).tolist()
    ids = [65536, 0, 65535, 65536, 1]
    want = S.overlap(small, [2, 0, 1, 2, 3], None, [2, 1, 0])
    assert np.array_equal(c_overlap(N, tab, F, ids, 5, tab, F, [65536, 65535, 0], 3, m), want) and want[0, 0] == S.popcount(small)[2]
    groups = [[0, 65536], [65535, 65536], [65536], [0, 65535, 65536]]
    local = [[0, 2], [1, 2], [2], [0, 1, 2]]
    for op, name in ((0, "or"), (1, "and")):
        rows, bits = c_reduce(N, tab, F, m, groups, op)
        assert np.array_equal(rows, S.reduce_rows(small, local, name)) and np.array_equal(bits, S.popcount(rows))
    del view, tab
    torch.cuda.empty_cache()


def test_rows_of_2_to_the_31_bits(pa, N):
    """two rows with every bit set: the overlap of 2^31 fits the unsigned word of the C entry; the Python method refuses such a bank"""
    m = 2**31
    if torch.cuda.mem_get_info()[0] < 2**30:
        pytest.skip("the device lacks the memory for two rows of 256 MiB")
    tab = torch.full((2 * (m // 32),), -1, dtype=torch.int32, device="cuda")
    assert c_overlap(N, tab, 2, None, 2, tab, 2, None, 2, m).tolist() == [[m, m], [m, m]]
    del tab
    torch.cuda.empty_cache()
    bank = pa.BloomFilterBank(2, 10, 0.05)
    bank._num_bits = m  # (a bank of this geometry would hold 256 MiB a row: the refusal comes before anything is read)
    with pytest.raises(pa.exceptions.NotSupportedError, match="int32"):
        bank.overlap()
    with pytest.raises(pa.exceptions.NotSupportedError):
        bank.jaccard()


# ------------------------------------------------------------------ refusals
def test_refusals(pa, N):
    bank = pa.BloomFilterBank(8, 100, 0.01)
    bank.add_many(["a", "b", "c"], [0, 1, 2])
    with pytest.raises(pa.exceptions.SimilarityError):
        bank.overlap(pa.BloomFilterBank(8, 100, 0.02))
    with pytest.raises(pa.exceptions.SimilarityError):
        bank.jaccard(pa.BloomFilterBank(8, 100, 0.01, hash_function=pa.default_md5))
    with pytest.raises(TypeError):
        bank.overlap(pa.BloomFilter(100, 0.01))
    with pytest.raises(ValueError, match="op must be"):
        bank.reduce([[0, 1]], op="xor")
    with pytest.raises(ValueError, match="empty group"):
        bank.reduce([[0], []], op="and")
    with pytest.raises(ValueError, match="empty group"):
        bank.reduce((np.array([0, 1, 1]), np.array([0])), op="and")
    with pytest.raises(ValueError, match="empty group"):
        bank.reduce((torch.tensor([0, 1, 1], device="cuda"), torch.tensor([0], device="cuda")), op="and")
    with pytest.raises(ValueError, match="non-decreasing"):
        bank.reduce((np.array([0, 2, 1]), np.array([0, 1])))
    for bad in ([8], [-1], np.array([0, 8]), torch.tensor([0, 8], device="cuda"), torch.tensor([-1], device="cuda")):
        with pytest.raises(ValueError, match="filter ids"):
            bank.bits_set(bad)
        with pytest.raises(ValueError, match="filter ids"):
            bank.estimate_elements(bad)
        with pytest.raises(ValueError, match="filter ids"):
            bank.overlap(a=bad)
        with pytest.raises(ValueError, match="filter ids"):
            bank.jaccard(b=bad)
        with pytest.raises(ValueError, match="filter ids"):
            bank.reduce([bad if isinstance(bad, list) else bad.tolist()])
    assert bank.bits_set(torch.tensor([0, 8], device="cuda"), validate=False).tolist() == [int(bank.bits_set([0])[0]), 0]  # unchecked: an empty row
    with pytest.raises(TypeError):
        bank.bits_set([0.5])
    # the C entry: dst inside src, any other op
    L, W = N.lib(), bank.row_bytes // 4
    t = bank.table_tensor
    seg, mem = _dev(np.array([0, 2], dtype=np.uint64)), _dev(np.array([0, 1], dtype=np.uint32))
    before = t.clone()
    for dst in (t[0], t[7], t[3]):
        assert L.psk_bank_reduce(t.data_ptr(), 8, bank.number_bits, seg.data_ptr(), mem.data_ptr(), 1, 0, dst.data_ptr(), None, 0, None) == N.PSK_EINVAL
        assert "overlaps" in N.last_error()
    dst = guarded(W)
    assert L.psk_bank_reduce(t.data_ptr(), 8, bank.number_bits, seg.data_ptr(), mem.data_ptr(), 1, 2, dst.data_ptr(), None, 0, None) == N.PSK_EINVAL
    assert L.psk_bank_reduce(t.data_ptr(), 8, bank.number_bits, seg.data_ptr(), mem.data_ptr(), 1, -1, dst.data_ptr(), None, 0, None) == N.PSK_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(t, before) and (dst.cpu().numpy().view(np.uint32) == SENTINEL).all()


def test_another_devices_bank_is_refused(pa):
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    bank, far = pa.BloomFilterBank(4, 100, 0.01, device=0), pa.BloomFilterBank(4, 100, 0.01, device=1)
    with pytest.raises(ValueError, match="cuda:1"):
        bank.overlap(far)
    with pytest.raises(ValueError, match="cuda:1"):
        bank.jaccard(far)


# ------------------------------------------------------------------ the slice image is neither used nor invalidated
def test_slice_image_is_left_alone(pa):
    F = 40
    bank = pa.BloomFilterBank(F, 100, 0.01)
    m, k = bank.number_bits, bank.number_hashes
    words = [f"w{i}" for i in range(200)]
    ids = np.arange(200) % F
    bank.add_many(words, ids)
    before = bank.match_many(words)
    assert bank._last_refresh == [(0, F)]
    bank._last_refresh = None
    bank.overlap(), bank.jaccard(a=[1, 2]), bank.bits_set(), bank.estimate_elements()
    groups = [[0, 1, 2], [5], list(range(F)), [7, 8]]
    red = bank.reduce(groups)
    both = bank.reduce(groups, op="and")
    assert np.array_equal(bank.match_many(words), before) and bank._last_refresh is None and not bank._stale_all
    rows = M.bank_rows(F, m, k, M.hashes_list(words, k), ids)
    h = M.hashes_list(words, k)
    for r, name in ((red, "or"), (both, "and")):
        folded = S.reduce_rows(S.as_words(rows), groups, name)
        want = MM.match_mask(MM.slices_of(folded.view(np.uint8).reshape(len(groups), -1), len(groups), m), m, k, h)
        assert r.slice_tensor is None
        got = r.match_many(words)
        assert np.array_equal(MM.mask_bits(got, len(groups)), MM.mask_bits(want, len(groups))), name
    assert MM.mask_bits(red.match_many(words), 4)[:, 2].all()  # the union of all filters holds every word
