"""The table algebra at its rails, tails and grid caps: k_table_binop, k_or_reduce, k_table_count, k_add_sat_i32, k_add_u32, k_cbf_intersect
and k_cbf_jaccard (psk_device.hpp, entered through psk_table_ops.hip), called directly on bare device tensors and through
CountMinSketch.join and CountingBloomFilter.union / intersection / jaccard_index.  Every comparison is exact: against
tests/table_algebra_model.py, which tests/test_table_algebra_model.py holds against the real reference, and against the cases recorded
from the reference itself (tests/golden/golden_table_algebra.json).

Sizes: the elementwise entries at every n around a wave and a 256-thread block and one size past each grid cap with an odd tail (4096
blocks for add_sat_i32 / add_u32, 2048 for cbf_intersect, 1024 for cbf_jaccard_counts and the counts); the uint4 entries at word counts
around a block and past their caps.  Values: every branch of the join and of the unsigned sum (frozen rails, sums exactly on a rail and
one past it, counters with the top bit set) many times per wave and in the tail block.  Then the state the algebra leaves behind: adds
and removes onto its result saturate as the reference's do."""

import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import table_algebra_model as M  # noqa: E402

G = json.loads((ROOT / "tests" / "golden" / "golden_table_algebra.json").read_text())
JOIN_BRANCHES = [(b["name"], b["self"], b["second"]) for b in G["join_branches"]]
CBF_BRANCHES = [(b["name"], b["a"], b["b"]) for b in G["cbf_branches"]]                       # some of these pass 2^32 - 1

AROUND = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025]
BLOCK = 256
# one size past each cap: two full strides of cap * 256 threads and a tail of one block and one element
PAST_CAP = {"add_sat_i32": 2 * 2**20 + 257, "add_u32": 2 * 2**20 + 257, "cbf_intersect": 2 * 2**19 + 257, "cbf_jaccard_counts": 2 * 2**18 + 257}
CAP_BLOCKS = {"add_sat_i32": 4096, "add_u32": 4096, "cbf_intersect": 2048, "cbf_jaccard_counts": 1024}
VEC_WORDS = [4, 8, 252, 256, 260, 1024 + 4]
BINOP_PAST_CAP_WORDS = 4 * (2**20 + 65)     # nvec = 2^20 + 65 > 4096 blocks * 256 threads: a 16 MiB table
COUNT_PAST_CAP_WORDS = 4 * (2 * 2**18 + 65)  # nvec = 2 * 2^18 + 65 > 1024 blocks * 256 threads, twice over


def size_id(entry, n):
    return f"n{n}_past_the_{CAP_BLOCKS[entry]}_block_cap" if n == PAST_CAP[entry] else f"n{n}"


@pytest.fixture(scope="module")
def pa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pyprobables_amd

    return pyprobables_amd


@pytest.fixture(scope="module")
def N(pa):
    from pyprobables_amd import _native

    _native.lib()
    return _native


def stream():
    return torch.cuda.current_stream().cuda_stream or None


def bits(a):
    """int64 values -> their 32-bit patterns as an int32 host array (two's complement for the signed tables, the low word for unsigned ones)"""
    return (M._i64(a) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def unsigned(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def signed(t) -> np.ndarray:
    return t.cpu().numpy().astype(np.int64)


class Guarded:
    """n 32-bit elements on the device with a guard element on each side; `off` = 0: the elements start on a 16-byte boundary,
    `off` = 1: one element (4 bytes) behind one, as a view one element into a tensor does"""

    GUARD = 0x5A5AA5A5

    def __init__(self, values, off: int):
        n = len(values)
        lead = 4 + off                                       # the left guard is element lead - 1
        host = np.full(lead + n + 1, self.GUARD, dtype=np.int64)
        host[lead:lead + n] = values
        self.whole = torch.from_numpy(bits(host)).cuda()
        self.view = self.whole[lead:lead + n]
        self.lead, self.n = lead, n
        assert self.whole.data_ptr() % 16 == 0 and self.ptr % 16 == 4 * off

    @property
    def ptr(self) -> int:
        return self.whole.data_ptr() + 4 * self.lead         # (a view of 0 elements has no pointer of its own to ask for)

    def guards_untouched(self) -> bool:
        w = unsigned(self.whole)
        return bool((w[: self.lead] == self.GUARD).all() and w[self.lead + self.n] == self.GUARD)


def tiled(branches, n, shift=0):
    """branch i of the table is branches[(i + shift) % len]: 33 / 24 branches against waves of 64 lanes -- every branch lands on every lane,
    several times per wave, and in the tail block"""
    idx = (np.arange(n) + shift) % len(branches)
    a = np.array([b[1] for b in branches], dtype=np.int64)[idx]
    b = np.array([b[2] for b in branches], dtype=np.int64)[idx]
    return a, b


# ====================================================================== direct entry calls: the elementwise entries
def run_add_sat_i32(N, a, b, off):
    dst, src = Guarded(a, off), Guarded(b, off)
    assert N.lib().psk_table_add_sat_i32(dst.ptr, src.ptr, len(a), 0, stream()) == N.PSK_OK
    assert dst.guards_untouched() and src.guards_untouched()
    assert np.array_equal(signed(src.view), M._i64(b))
    return signed(dst.view)


def run_add_u32(N, a, b, off, want_tally=True):
    dst, src = Guarded(a, off), Guarded(b, off)
    ov = C.c_uint64(0xDEAD)
    assert N.lib().psk_table_add_u32(dst.ptr, src.ptr, len(a), C.byref(ov) if want_tally else None, 0, stream()) == N.PSK_OK
    assert dst.guards_untouched() and src.guards_untouched()
    assert np.array_equal(unsigned(src.view), M._i64(b))
    return unsigned(dst.view), (ov.value if want_tally else None)


def run_cbf_intersect(N, a, b, off, want_tally=True):
    dst, x, y = Guarded(np.full(len(a), 0x77777777, dtype=np.int64), off), Guarded(a, off), Guarded(b, off)
    ov = C.c_uint64(0xDEAD)
    assert N.lib().psk_cbf_intersect(dst.ptr, x.ptr, y.ptr, len(a), C.byref(ov) if want_tally else None, 0, stream()) == N.PSK_OK
    assert dst.guards_untouched() and x.guards_untouched() and y.guards_untouched()
    assert np.array_equal(unsigned(x.view), M._i64(a)) and np.array_equal(unsigned(y.view), M._i64(b))
    return unsigned(dst.view), (ov.value if want_tally else None)


def run_jaccard_counts(N, a, b, off):
    x, y = Guarded(a, off), Guarded(b, off)
    out = (C.c_uint64 * 2)(0xDEAD, 0xDEAD)
    assert N.lib().psk_cbf_jaccard_counts(x.ptr, y.ptr, len(a), out, 0, stream()) == N.PSK_OK
    return int(out[0]), int(out[1])


ALIGN = [pytest.param(0, id="aligned16"), pytest.param(1, id="four_bytes_off")]


@pytest.mark.parametrize("off", ALIGN)
@pytest.mark.parametrize("n", [pytest.param(n, id=size_id("add_sat_i32", n)) for n in AROUND + [PAST_CAP["add_sat_i32"]]])
def test_add_sat_i32_sizes(N, n, off):
    a, b = tiled(JOIN_BRANCHES, n, shift=n % 7)
    got = run_add_sat_i32(N, a, b, off)
    assert np.array_equal(got, M.join(a, b))


@pytest.mark.parametrize("off", ALIGN)
@pytest.mark.parametrize("n", [pytest.param(n, id=size_id("add_u32", n)) for n in AROUND + [PAST_CAP["add_u32"]]])
def test_add_u32_sizes(N, n, off):
    a, b = tiled(CBF_BRANCHES, n, shift=n % 7)
    want, overflowed = M.add_u32(a, b)
    got, tally = run_add_u32(N, a, b, off)
    assert np.array_equal(got, want) and tally == overflowed
    assert overflowed > 0 or n < len(CBF_BRANCHES)


@pytest.mark.parametrize("off", ALIGN)
@pytest.mark.parametrize("n", [pytest.param(n, id=size_id("cbf_intersect", n)) for n in AROUND + [PAST_CAP["cbf_intersect"]]])
def test_cbf_intersect_sizes(N, n, off):
    a, b = tiled(CBF_BRANCHES, n, shift=n % 7)
    want, overflowed = M.intersect(a, b)
    got, tally = run_cbf_intersect(N, a, b, off)
    assert np.array_equal(got, want) and tally == overflowed


@pytest.mark.parametrize("off", ALIGN)
@pytest.mark.parametrize("n", [pytest.param(n, id=size_id("cbf_jaccard_counts", n)) for n in AROUND + [PAST_CAP["cbf_jaccard_counts"]]])
def test_cbf_jaccard_counts_sizes(N, n, off):
    a, b = tiled(CBF_BRANCHES, n, shift=n % 7)
    assert run_jaccard_counts(N, a, b, off) == M.jaccard_counts(a, b)
    assert run_jaccard_counts(N, b, a, off) == M.jaccard_counts(b, a)


# ---------------------------------------------------------------------- every branch by name: a table that holds nothing else
BRANCH_N = 5 * BLOCK + 65                      # six blocks, the last one wave and one lane


def recorded(case, name, field, names="branches"):
    return case[field][case[names].index(name)]


@pytest.mark.parametrize("name,x,y", [pytest.param(*b, id=b[0]) for b in JOIN_BRANCHES])
def test_join_branch(N, name, x, y):
    """the whole table is this one branch; the value is the one the reference recorded for it, after one join and after two"""
    case = G["join"][0]
    a, b = np.full(BRANCH_N, x, dtype=np.int64), np.full(BRANCH_N, y, dtype=np.int64)
    once = run_add_sat_i32(N, a, b, 0)
    assert np.array_equal(once, M.join(a, b)) and set(once.tolist()) == {recorded(case, name, "joined_bins")}
    twice = run_add_sat_i32(N, once, b, 1)
    assert np.array_equal(twice, M.join(once, b)) and set(twice.tolist()) == {recorded(case, name, "joined_twice_bins")}


@pytest.mark.parametrize("name,x,y", [pytest.param(*b, id=b[0]) for b in CBF_BRANCHES])
def test_unsigned_sum_intersect_and_jaccard_branch(N, name, x, y):
    """one branch in every element: the sum and the intersection the reference recorded (or, past 2^32 - 1, the rail and a tally of
    every element), and the two counts -- an unsigned `> 0` on counters with the top bit set"""
    a, b = np.full(BRANCH_N, x, dtype=np.int64), np.full(BRANCH_N, y, dtype=np.int64)
    fits = x + y <= M.U32_MAX
    case = G["cbf"][0]
    got, tally = run_add_u32(N, a, b, 0)
    assert np.array_equal(got, M.add_u32(a, b)[0]) and tally == M.add_u32(a, b)[1] == (0 if fits else BRANCH_N)
    assert set(got.tolist()) == {recorded(case, name, "union_table") if fits else M.U32_MAX}
    got, tally = run_cbf_intersect(N, a, b, 1)
    assert np.array_equal(got, M.intersect(a, b)[0]) and tally == M.intersect(a, b)[1] == (0 if fits else BRANCH_N)
    assert set(got.tolist()) == {recorded(case, name, "intersection_table") if fits else M.U32_MAX}
    assert run_jaccard_counts(N, a, b, 0) == M.jaccard_counts(a, b) == (BRANCH_N * bool(x or y), BRANCH_N * bool(x and y))


OVERFLOW_N = 37 * BLOCK + 65


def overflow_pattern(kind):
    a, b = np.full(OVERFLOW_N, 3, dtype=np.int64), np.full(OVERFLOW_N, 4, dtype=np.int64)
    if kind == "in_one_wave":                   # 64 overflows, all in the third wave of block 5
        a[5 * BLOCK + 128:5 * BLOCK + 192] = M.U32_MAX
    elif kind == "in_one_lane":
        a[9 * BLOCK + 77] = M.U32_MAX
    elif kind == "spread_over_blocks":          # one or two per block, moving through the lanes, the tail block too
        a[np.arange(0, OVERFLOW_N, 131)] = 2**31
        b[np.arange(0, OVERFLOW_N, 131)] = 2**31
        a[OVERFLOW_N - 1] = M.U32_MAX
    elif kind == "every_element":
        a[:] = M.U32_MAX - 2
    return a, b


@pytest.mark.parametrize("kind", ["in_one_wave", "in_one_lane", "spread_over_blocks", "every_element", "none"])
def test_overflow_tally(N, kind):
    a, b = overflow_pattern(kind)
    want = {"in_one_wave": 64, "in_one_lane": 1, "spread_over_blocks": len(range(0, OVERFLOW_N, 131)) + 1, "every_element": OVERFLOW_N, "none": 0}
    for model, run in ((M.add_u32, run_add_u32), (M.intersect, run_cbf_intersect)):
        tab, overflowed = model(a, b)
        assert overflowed == want[kind]
        got, tally = run(N, a, b, 1)
        assert np.array_equal(got, tab) and tally == overflowed
        got, tally = run(N, a, b, 0, want_tally=False)          # overflowed_host = NULL is accepted; the table is clamped all the same
        assert np.array_equal(got, tab) and tally is None


# ====================================================================== direct entry calls: the uint4 entries
WORD_KINDS = ["only_top_bit", "only_low_bit", "all_ones", "mixed"]


def words(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "mixed":
        w = rng.integers(0, 2**32, size=n, dtype=np.int64)
        w[rng.random(n) < 0.3] = 0
        special = rng.random(n)
        w[special < 0.1] = 0x80000000
        w[(special >= 0.1) & (special < 0.2)] = 1
        w[(special >= 0.2) & (special < 0.3)] = 0xFFFFFFFF
        return w
    value = {"only_top_bit": 0x80000000, "only_low_bit": 1, "all_ones": 0xFFFFFFFF}[kind]
    return np.where(rng.random(n) < 0.6, value, 0).astype(np.int64)


def dev(a):
    t = torch.from_numpy(bits(a)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def vec_id(nwords, cap_words, cap):
    return f"words{nwords}_past_the_{cap}_block_cap" if nwords == cap_words else f"words{nwords}"


@pytest.mark.parametrize("nwords", [pytest.param(w, id=vec_id(w, BINOP_PAST_CAP_WORDS, 4096)) for w in VEC_WORDS + [BINOP_PAST_CAP_WORDS]])
def test_table_or_and_sizes(N, nwords):
    a, b = words("mixed", nwords, 1), words("mixed", nwords, 2)
    for fn, model in ((N.lib().psk_table_or, M.table_or), (N.lib().psk_table_and, M.table_and)):
        dst, src = dev(a), dev(b)
        assert fn(dst.data_ptr(), src.data_ptr(), nwords, 0, stream()) == N.PSK_OK
        assert np.array_equal(unsigned(dst), model(a, b)) and np.array_equal(unsigned(src), b)
    for kind in WORD_KINDS[:3]:                   # 0x80000000 | 1, & 0xFFFFFFFF ...: no bit of a word leaks into its neighbour
        x, y = words(kind, nwords, 3), words("all_ones", nwords, 4)
        dst, src = dev(x), dev(y)
        assert N.lib().psk_table_or(dst.data_ptr(), src.data_ptr(), nwords, 0, stream()) == N.PSK_OK
        assert np.array_equal(unsigned(dst), M.table_or(x, y))
        dst = dev(x)
        assert N.lib().psk_table_and(dst.data_ptr(), src.data_ptr(), nwords, 0, stream()) == N.PSK_OK
        assert np.array_equal(unsigned(dst), M.table_and(x, y))


@pytest.mark.parametrize("kind", WORD_KINDS)
@pytest.mark.parametrize("nwords", [pytest.param(w, id=vec_id(w, COUNT_PAST_CAP_WORDS, 1024)) for w in VEC_WORDS + [COUNT_PAST_CAP_WORDS]])
def test_popcount_and_nonzero_sizes(N, nwords, kind):
    w = words(kind, nwords, 5)
    tab = dev(w)
    for fn, model in ((N.lib().psk_table_popcount, M.popcount), (N.lib().psk_table_nonzero_u32, M.nonzero)):
        first, second = C.c_uint64(0xDEAD), C.c_uint64(7)
        assert fn(tab.data_ptr(), nwords, C.byref(first), 0, stream()) == N.PSK_OK
        assert fn(tab.data_ptr(), nwords, C.byref(second), 0, stream()) == N.PSK_OK          # the tally is zeroed per call
        assert first.value == second.value == model(w)
    assert np.array_equal(unsigned(tab), w)
    if kind != "mixed":                           # one bit per set word -- or 32: popcount and non-zero part ways by exactly that factor
        assert M.popcount(w) == M.nonzero(w) * (32 if kind == "all_ones" else 1) > 0


@pytest.mark.parametrize("right", WORD_KINDS[:3])
@pytest.mark.parametrize("left", WORD_KINDS[:3])
@pytest.mark.parametrize("n", [pytest.param(3 * BLOCK + 65, id="n833"), pytest.param(PAST_CAP["cbf_jaccard_counts"], id=size_id("cbf_jaccard_counts", PAST_CAP["cbf_jaccard_counts"]))])
def test_cbf_jaccard_counts_on_single_bit_words(N, n, left, right):
    """counters that are only 0x80000000, only 1 or 0xFFFFFFFF against each other, zeros in between: `> 0` is an unsigned compare"""
    a, b = words(left, n, 41), words(right, n, 42)
    assert run_jaccard_counts(N, a, b, 1) == M.jaccard_counts(a, b) == (int(((a != 0) | (b != 0)).sum()), int(((a != 0) & (b != 0)).sum()))


@pytest.mark.parametrize("nslices", [1, 2, 3, 8])
@pytest.mark.parametrize("nwords", [pytest.param(w, id=f"words{w}") for w in VEC_WORDS])
def test_or_reduce_slices_sizes(N, nwords, nslices):
    src_host = words("mixed", nwords * nslices, 6 + nslices)
    src, dst = dev(src_host), dev(np.full(nwords, 0x77777777, dtype=np.int64))
    assert N.lib().psk_or_reduce_slices(dst.data_ptr(), src.data_ptr(), nslices, nwords, 0, stream()) == N.PSK_OK
    assert np.array_equal(unsigned(dst), M.or_slices(src_host, nslices)) and np.array_equal(unsigned(src), src_host)


@pytest.mark.parametrize("nslices", [1, 2])
def test_or_reduce_slices_past_the_4096_block_cap(N, nslices):
    nwords = BINOP_PAST_CAP_WORDS
    src_host = np.concatenate([words(kind, nwords, 20 + i) for i, kind in enumerate(["only_top_bit", "only_low_bit"][:nslices])])
    src, dst = dev(src_host), dev(np.full(nwords, 0x77777777, dtype=np.int64))
    assert N.lib().psk_or_reduce_slices(dst.data_ptr(), src.data_ptr(), nslices, nwords, 0, stream()) == N.PSK_OK
    assert np.array_equal(unsigned(dst), M.or_slices(src_host, nslices))


def test_or_reduce_in_place_on_the_first_slice(N):
    """the merge reduces into slice 0 of its own receive buffer (psk_merge.hip): dst == src"""
    nwords, nslices = 260, 3
    src_host = words("mixed", nwords * nslices, 31)
    src = dev(src_host)
    assert N.lib().psk_or_reduce_slices(src.data_ptr(), src.data_ptr(), nslices, nwords, 0, stream()) == N.PSK_OK
    got = unsigned(src)
    assert np.array_equal(got[:nwords], M.or_slices(src_host, nslices)) and np.array_equal(got[nwords:], src_host[nwords:])


# ====================================================================== refusals: the host-side argument check, before any launch
def refusals():
    """(id, call(L, dst, src, out) -> status): dst and src are 32-word tables; every pointer handed over lies inside them"""
    cases = []
    for name in ("psk_table_or", "psk_table_and"):
        cases += [
            (f"{name}-words_not_a_multiple_of_4", lambda L, d, s, o, name=name: getattr(L, name)(d, s, 6, 0, stream())),
            (f"{name}-dst_four_bytes_off", lambda L, d, s, o, name=name: getattr(L, name)(d + 4, s, 8, 0, stream())),
            (f"{name}-src_four_bytes_off", lambda L, d, s, o, name=name: getattr(L, name)(d, s + 4, 8, 0, stream())),
            (f"{name}-dst_eight_bytes_off", lambda L, d, s, o, name=name: getattr(L, name)(d + 8, s, 8, 0, stream())),
            (f"{name}-dst_null", lambda L, d, s, o, name=name: getattr(L, name)(None, s, 8, 0, stream())),
            (f"{name}-src_null", lambda L, d, s, o, name=name: getattr(L, name)(d, None, 8, 0, stream())),
        ]
    for name in ("psk_table_popcount", "psk_table_nonzero_u32"):
        cases += [
            (f"{name}-words_not_a_multiple_of_4", lambda L, d, s, o, name=name: getattr(L, name)(d, 7, o, 0, stream())),
            (f"{name}-table_four_bytes_off", lambda L, d, s, o, name=name: getattr(L, name)(d + 4, 8, o, 0, stream())),
            (f"{name}-table_null", lambda L, d, s, o, name=name: getattr(L, name)(None, 8, o, 0, stream())),
            (f"{name}-out_null", lambda L, d, s, o, name=name: getattr(L, name)(d, 8, None, 0, stream())),
        ]
    cases += [
        ("psk_or_reduce_slices-no_slices", lambda L, d, s, o: L.psk_or_reduce_slices(d, s, 0, 8, 0, stream())),
        ("psk_or_reduce_slices-words_not_a_multiple_of_4", lambda L, d, s, o: L.psk_or_reduce_slices(d, s, 2, 6, 0, stream())),
        ("psk_or_reduce_slices-dst_four_bytes_off", lambda L, d, s, o: L.psk_or_reduce_slices(d + 4, s, 2, 8, 0, stream())),
        ("psk_or_reduce_slices-src_four_bytes_off", lambda L, d, s, o: L.psk_or_reduce_slices(d, s + 4, 2, 8, 0, stream())),
        ("psk_or_reduce_slices-dst_null", lambda L, d, s, o: L.psk_or_reduce_slices(None, s, 2, 8, 0, stream())),
        ("psk_or_reduce_slices-src_null", lambda L, d, s, o: L.psk_or_reduce_slices(d, None, 2, 8, 0, stream())),
        ("psk_table_add_sat_i32-dst_null", lambda L, d, s, o: L.psk_table_add_sat_i32(None, s, 8, 0, stream())),
        ("psk_table_add_sat_i32-src_null", lambda L, d, s, o: L.psk_table_add_sat_i32(d, None, 8, 0, stream())),
        ("psk_table_add_u32-dst_null", lambda L, d, s, o: L.psk_table_add_u32(None, s, 8, o, 0, stream())),
        ("psk_table_add_u32-src_null", lambda L, d, s, o: L.psk_table_add_u32(d, None, 8, o, 0, stream())),
        ("psk_cbf_intersect-dst_null", lambda L, d, s, o: L.psk_cbf_intersect(None, s, s, 8, o, 0, stream())),
        ("psk_cbf_intersect-a_null", lambda L, d, s, o: L.psk_cbf_intersect(d, None, s, 8, o, 0, stream())),
        ("psk_cbf_intersect-b_null", lambda L, d, s, o: L.psk_cbf_intersect(d, s, None, 8, o, 0, stream())),
        ("psk_cbf_jaccard_counts-a_null", lambda L, d, s, o: L.psk_cbf_jaccard_counts(None, s, 8, o, 0, stream())),
        ("psk_cbf_jaccard_counts-b_null", lambda L, d, s, o: L.psk_cbf_jaccard_counts(d, None, 8, o, 0, stream())),
        ("psk_cbf_jaccard_counts-out_null", lambda L, d, s, o: L.psk_cbf_jaccard_counts(d, s, 8, None, 0, stream())),
    ]
    return [pytest.param(call, id=name) for name, call in cases]


@pytest.mark.parametrize("call", refusals())
def test_refused_before_any_launch(N, call):
    """PSK_EINVAL out of the argument check: both tables and the result words are as they were -- a launch would have changed dst (the
    tables are chosen so that OR, AND, the sums and the reduce all differ from dst) or the result words (a tally starts from 0)"""
    a = np.arange(1, 33, dtype=np.int64) * 0x01010101 % 2**31
    b = (np.arange(1, 33, dtype=np.int64) * 0x00F0F0F1 + 5) % 2**31
    assert not np.array_equal(M.table_or(a, b)[:8], a[:8]) and not np.array_equal(M.table_and(a, b)[:8], a[:8])
    dst, src = dev(a), dev(b)
    out = (C.c_uint64 * 2)(0xDEAD, 0xBEEF)
    torch.cuda.synchronize()
    assert call(N.lib(), dst.data_ptr(), src.data_ptr(), out) == N.PSK_EINVAL
    assert N.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(unsigned(dst), a) and np.array_equal(unsigned(src), b)
    assert (out[0], out[1]) == (0xDEAD, 0xBEEF)


def test_empty_tables_are_accepted(N):
    """n = 0 / no words: PSK_OK, nothing written, the tallies 0"""
    L = N.lib()
    dst, src = dev(np.arange(8, dtype=np.int64) + 1), dev(np.arange(8, dtype=np.int64) + 11)
    d, s = dst.data_ptr(), src.data_ptr()
    out = (C.c_uint64 * 2)(0xDEAD, 0xBEEF)
    assert L.psk_table_or(d, s, 0, 0, stream()) == L.psk_table_and(d, s, 0, 0, stream()) == L.psk_or_reduce_slices(d, s, 3, 0, 0, stream()) == 0
    assert L.psk_table_popcount(d, 0, out, 0, stream()) == 0 and out[0] == 0
    out[0] = 0xDEAD
    assert L.psk_table_nonzero_u32(d, 0, out, 0, stream()) == 0 and out[0] == 0
    assert unsigned(dst).tolist() == list(range(1, 9)) and unsigned(src).tolist() == list(range(11, 19))


# ====================================================================== through the classes: the recorded cases
def by_name(cases):
    return [pytest.param(c, id=c["name"]) for c in cases]


def cms_with(pa, bins, els, width, depth):
    c = pa.CountMinSketch(width=width, depth=depth)
    c._tab.write(np.array(bins, dtype=np.int32))
    c._els_added = els
    return c


def cbf_with(pa, table, els=0, est=None, fpr=None):
    f = pa.CountingBloomFilter(est_elements=est or G["cbf"][0]["est_elements"], false_positive_rate=fpr or G["cbf"][0]["fpr"])
    assert f.number_bits == len(table)
    f._tab.write(np.array(table, dtype=np.uint32))
    f.elements_added = els
    return f


@pytest.mark.parametrize("case", by_name(G["join"]))
def test_join_as_the_reference_recorded_it(pa, case):
    a = cms_with(pa, case["a_bins"], case["a_elements_added"], case["width"], case["depth"])
    b = cms_with(pa, case["b_bins"], case["b_elements_added"], case["width"], case["depth"])
    a.join(b)
    assert (list(a._bins), a.elements_added) == (case["joined_bins"], case["joined_elements_added"])
    a.join(b)                                     # bins that reached a rail in the first join stay frozen
    assert (list(a._bins), a.elements_added) == (case["joined_twice_bins"], case["joined_twice_elements_added"])
    assert (list(b._bins), b.elements_added) == (case["b_bins_after"], case["b_elements_added_after"])


@pytest.mark.parametrize("case", by_name(G["cbf"]))
def test_union_intersection_jaccard_as_the_reference_recorded_them(pa, case):
    a, b = cbf_with(pa, case["a_table"], case["a_elements_added"]), cbf_with(pa, case["b_table"], case["b_elements_added"])
    assert (a.number_bits, a.number_hashes) == (case["m"], case["k"])
    assert (a._cnt_number_bits_set(), b._cnt_number_bits_set()) == (case["a_bits_set"], case["b_bits_set"])
    assert (a.jaccard_index(b), b.jaccard_index(a), a.jaccard_index(a)) == (case["jaccard"], case["jaccard_ba"], case["jaccard_self"])
    for op in ("union", "intersection"):
        for tag, (x, y) in (("", (a, b)), ("_ba", (b, a))):
            err = case[f"{op}{tag}_error"]
            if err is not None:                   # a sum passes 2^32 - 1: the reference's exception, type and text
                assert err["type"] == "OverflowError"
                with pytest.raises(OverflowError) as info:
                    getattr(x, op)(y)
                assert str(info.value) == err["message"]
            else:
                res = getattr(x, op)(y)
                assert list(res.bloom) == case[f"{op}{tag}_table"]
                assert res.elements_added == case[f"{op}{tag}_elements_added"] == res.estimate_elements()
            # the operands are as they were, whatever became of the result
            assert (list(a.bloom), a.elements_added) == (case["a_table_after"], case["a_elements_added"])
            assert (list(b.bloom), b.elements_added) == (case["b_table_after"], case["b_elements_added"])


# ====================================================================== the state the algebra leaves behind
FOLLOW_EST, FOLLOW_FPR = G["cbf_follow_on"][0]["est_elements"], G["cbf_follow_on"][0]["fpr"]


def reaches_the_rail(case) -> bool:
    return "small" not in case["name"]


@pytest.mark.parametrize("how", ["one_key_at_a_time", "one_key_batches"])
@pytest.mark.parametrize("case", by_name(G["cbf_follow_on"]))
def test_adds_onto_a_union_or_intersection_as_the_reference_recorded_them(pa, case, how):
    """`add` (the ordered kernel) gives the reference's return values; `add_many`, one key per batch, is the same stream through the
    unordered kernels, whose path -- wrapping atomicAdd or saturating CAS -- follows the bound the algebra left on the result"""
    a, b = cbf_with(pa, case["a_table"], 0, FOLLOW_EST, FOLLOW_FPR), cbf_with(pa, case["b_table"], 0, FOLLOW_EST, FOLLOW_FPR)
    res = getattr(a, case["op"])(b)
    assert (list(res.bloom), res.elements_added) == (case["result_table"], case["result_elements_added"])
    for op in case["ops"]:
        if how == "one_key_at_a_time":
            assert res.add(op["key"], op["count"]) == op["returned"]
        else:
            res.add_many([op["key"]], op["count"])
        assert res.elements_added == op["elements_added"]
    assert (list(res.bloom), res.elements_added) == (case["final_table"], case["final_elements_added"])
    keys = [op["key"] for op in case["ops"]]
    assert [res.check(k) for k in keys] == case["final_checks"] == res.check_many(keys).tolist()
    if how == "one_key_batches":
        assert (res.batch_diagnostics()["saturated"] > 0) == reaches_the_rail(case)
    assert (list(a.bloom), list(b.bloom)) == (case["a_table"], case["b_table"])


@pytest.mark.parametrize("how", ["one_key_at_a_time", "one_key_batches"])
@pytest.mark.parametrize("case", by_name(G["cms_follow_on"]))
def test_adds_and_removes_onto_a_join_as_the_reference_recorded_them(pa, case, how):
    a = cms_with(pa, case["a_bins"], case["a_elements_added"], case["width"], case["depth"])
    b = cms_with(pa, case["b_bins"], case["b_elements_added"], case["width"], case["depth"])
    a.join(b)
    assert (list(a._bins), a.elements_added) == (case["joined_bins"], case["joined_elements_added"])
    for op in case["ops"]:
        if how == "one_key_at_a_time":
            assert getattr(a, op["op"])(op["key"], op["count"]) == op["returned"]
        else:
            getattr(a, op["op"] + "_many")([op["key"]], op["count"])
        assert a.elements_added == op["elements_added"]
    assert (list(a._bins), a.elements_added) == (case["final_bins"], case["final_elements_added"])
    keys = [op["key"] for op in case["ops"]]
    assert [a.check(k) for k in keys] == case["final_checks"] == a.check_many(keys).tolist()
    if how == "one_key_batches":
        assert a.batch_diagnostics()["saturated"] > 0


# ---------------------------------------------------------------------- ... and at a size where whole batches meet the rail
BIG_EST, BIG_FPR = 20_000, 0.01               # 191 702 counters, 7 hashes
N_DIRECT, N_PARTITIONED = 5_000, 300_000      # a batch for the direct atomic kernels, one for the partitioned path


@pytest.fixture(scope="module")
def big_batches(oracle):
    """n -> (keys, weights 1..7) for both batch sizes; generated once"""
    out = {}
    for n in (N_DIRECT, N_PARTITIONED):
        keys, w = oracle.gen_keys16(1000, n), oracle.gen_weights(1000, n)
        assert 1 <= w.min() and w.max() <= 7
        out[n] = (keys, w)
    return out


def cbf_delta(oracle, m, k, keys, w):
    oc = oracle.OracleCBF(m, k)
    oc.update_keys(keys, w.astype(np.int64))
    return oc.bloom.astype(np.int64)


def cbf_min_per_key(oracle, m, k, table, keys):
    oc = oracle.OracleCBF(m, k)
    oc.bloom[:] = M.as_u32(table)
    return oc.check_keys(keys).astype(np.int64)


@pytest.mark.parametrize("where", ["host_keys", "device_keys"])
@pytest.mark.parametrize("n", [pytest.param(N_DIRECT, id="direct_kernels"), pytest.param(N_PARTITIONED, id="partitioned_path")])
@pytest.mark.parametrize("op", ["union", "intersection"])
def test_add_many_onto_a_union_or_intersection_three_under_the_rail(pa, oracle, big_batches, op, n, where):
    """both operands hold 2^31 - 2 in every counter: the result holds 2^32 - 4, so every key of the batch lands on counters three counts
    under the rail.  The reference saturates there (countingbloom.py:149-151); a wrapping add would leave small numbers."""
    a = pa.CountingBloomFilter(est_elements=BIG_EST, false_positive_rate=BIG_FPR)
    m, k = a.number_bits, a.number_hashes
    a._tab.write(np.full(m, 2**31 - 2, dtype=np.uint32))
    b = pa.CountingBloomFilter(est_elements=BIG_EST, false_positive_rate=BIG_FPR)
    b._tab.write(np.full(m, 2**31 - 2, dtype=np.uint32))
    res = getattr(a, op)(b)
    base = np.full(m, 2**32 - 4, dtype=np.int64)
    assert np.array_equal(np.frombuffer(bytes(res.bloom), dtype=np.uint32), base) and res.elements_added == -1   # bloom.py:348-349: full
    keys, w = big_batches[n]
    if where == "device_keys":
        res.add_many(torch.from_numpy(keys).cuda(), torch.from_numpy(w.astype(np.int32)).cuda())
    else:
        res.add_many(keys, w.astype(np.uint32))
    want = M.cbf_add_delta(base, cbf_delta(oracle, m, k, keys, w))
    got = np.frombuffer(bytes(res.bloom), dtype=np.uint32).astype(np.int64)
    print(f"counters on the rail: {int((got == M.U32_MAX).sum())} (model {int((want == M.U32_MAX).sum())}), below 2^31: {int((got < 2**31).sum())}")
    assert np.array_equal(got, want)
    assert int((want == M.U32_MAX).sum()) > 1000
    diag = res.batch_diagnostics()
    assert diag["violations"] == 0 and diag["saturated"] > 0
    assert res.elements_added == -1 + int(w.sum())
    probe = keys[:4096]
    checks = res.check_many(torch.from_numpy(probe).cuda()).cpu().numpy().view(np.uint32) if where == "device_keys" else res.check_many(probe)
    assert np.array_equal(checks.astype(np.int64), cbf_min_per_key(oracle, m, k, want, probe))
    assert int((checks == M.U32_MAX).sum()) > 100


@pytest.mark.parametrize("op", ["union", "intersection"])
def test_add_many_onto_a_union_or_intersection_of_small_counters_stays_unsaturated(pa, oracle, big_batches, op):
    a = pa.CountingBloomFilter(est_elements=BIG_EST, false_positive_rate=BIG_FPR)
    m, k = a.number_bits, a.number_hashes
    a._tab.write(np.full(m, 5, dtype=np.uint32))
    b = pa.CountingBloomFilter(est_elements=BIG_EST, false_positive_rate=BIG_FPR)
    b._tab.write(np.full(m, 6, dtype=np.uint32))
    res = getattr(a, op)(b)
    total = np.full(m, 11, dtype=np.int64)
    for n in (N_DIRECT, N_PARTITIONED):
        keys, w = big_batches[n]
        res.add_many(torch.from_numpy(keys).cuda(), torch.from_numpy(w.astype(np.int32)).cuda())
        total = total + cbf_delta(oracle, m, k, keys, w)           # the plain sum
    assert int(total.max()) < 2**31
    assert np.array_equal(np.frombuffer(bytes(res.bloom), dtype=np.uint32).astype(np.int64), total)
    assert res.batch_diagnostics() == {"violations": 0, "saturated": 0}


def cms_delta(oracle, width, depth, keys, w):
    oc = oracle.OracleCMS(width, depth)
    oc.add_keys(keys, w.astype(np.int32))
    return oc.bins.astype(np.int64)


@pytest.mark.parametrize("where", ["host_keys", "device_keys"])
@pytest.mark.parametrize("n", [pytest.param(N_DIRECT, id="direct_kernels"), pytest.param(N_PARTITIONED, id="partitioned_path")])
@pytest.mark.parametrize("rail", ["toward_int32_max", "toward_int32_min"])
def test_add_many_and_remove_many_onto_a_join_three_from_the_rail(pa, oracle, big_batches, rail, n, where):
    """every bin of the join stands three counts from one rail; add_many (remove_many toward INT32_MIN) saturates there as
    countminsketch.py:280-284 / :312-316 do"""
    width, depth = 4099, 5
    up = rail == "toward_int32_max"
    a, b = pa.CountMinSketch(width=width, depth=depth), pa.CountMinSketch(width=width, depth=depth)
    a._tab.write(np.full(width * depth, 2**30 if up else -(2**30), dtype=np.int32))
    b._tab.write(np.full(width * depth, 2**30 - 4 if up else -(2**30) + 3, dtype=np.int32))
    a.join(b)
    base = np.full(width * depth, M.I32_MAX - 3 if up else M.I32_MIN + 3, dtype=np.int64)
    assert np.array_equal(np.frombuffer(bytes(a._bins), dtype=np.int32), base)
    keys, w = big_batches[n]
    args = (torch.from_numpy(keys).cuda(), torch.from_numpy(w.astype(np.int32)).cuda()) if where == "device_keys" else (keys, w.astype(np.int32))
    (a.add_many if up else a.remove_many)(*args)
    delta = cms_delta(oracle, width, depth, keys, w)
    want = M.cms_add_delta(base, delta) if up else M.cms_remove_delta(base, delta)
    got = np.frombuffer(bytes(a._bins), dtype=np.int32).astype(np.int64)
    edge = M.I32_MAX if up else M.I32_MIN
    print(f"bins on the rail: {int((got == edge).sum())} (model {int((want == edge).sum())})")
    assert np.array_equal(got, want) and int((want == edge).sum()) > 1000
    assert a.batch_diagnostics()["saturated"] > 0
    assert a.elements_added == (int(w.sum()) if up else -int(w.sum()))
    oc = oracle.OracleCMS(width, depth)
    oc.bins[:] = M.as_i32(want)
    probe = keys[:4096]
    checks = a.check_many(torch.from_numpy(probe).cuda()).cpu().numpy() if where == "device_keys" else a.check_many(probe)
    assert np.array_equal(np.asarray(checks).astype(np.int64), oc.check_keys(probe))
    assert int((np.asarray(checks) == edge).sum()) > 100
