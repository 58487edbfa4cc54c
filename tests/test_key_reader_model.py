"""tests/key_reader_model.py on the CPU: its hash reference against the package's own per-key functions and the reference's golden
vectors, and the ADEQUACY of the inputs it hands to tests/test_gpu_key_readers.py -- which window classes, length classes and key
sources those inputs reach.  These are conditions on the inputs, not measurements: the generators are chosen so that they hold."""
import numpy as np

import key_reader_model as M
from _util import as_key
from pyprobables_amd import hashes as H


def _elements(keys):
    arrs = [np.array([ord(c) for c in k], dtype=np.uint32) if isinstance(k, str) else np.frombuffer(bytes(k), dtype=np.uint8).astype(np.uint32)
            for k in keys]
    el = np.zeros((len(keys), max([a.size for a in arrs] + [1])), dtype=np.uint32)
    for i, a in enumerate(arrs):
        el[i, : a.size] = a
    return el, np.array([a.size for a in arrs])


# ---------------------------------------------------------------------------------------------------------------- reference check
def test_vectorised_hashes_equal_the_golden_vectors(golden):
    cases = golden["hashes"]
    assert {c["type"] for c in cases} == {"str", "bytes"}
    keys = [as_key(c) for c in cases]
    depth = max(c["depth"] for c in cases)
    el, lens = _elements(keys)
    h64, h32 = M.fnv64(el, lens, range(depth)), M.fnv32(el, lens, range(3))
    for i, c in enumerate(cases):
        assert [int(v) for v in h64[i, : c["depth"]]] == c["hashes"], c["key"][:40]
        assert [int(v) for v in h32[i]] == [H.fnv_1a_32(keys[i], s) for s in range(3)]
    assert np.array_equal(M.fnv64(el, lens), h64[:, 0]) and np.array_equal(M.fnv32(el, lens, 2), h32[:, 2])


def test_vectorised_hashes_equal_the_per_key_functions_on_random_keys():
    rng = np.random.default_rng(5)
    lens = np.concatenate([np.arange(301), rng.integers(0, 301, size=99)])
    byte_keys = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in lens]
    str_keys = ["".join(map(chr, np.where((c := rng.integers(0, M.MAX_CODE_POINT + 1, size=n)) // 0x800 == 0x1B, 0x20AC, c))) for n in lens]  # (no surrogates)
    assert max(map(ord, "".join(str_keys))) > 0xFFFF
    for keys in (byte_keys, str_keys):
        el, got_lens = _elements(keys)
        assert np.array_equal(got_lens, lens)
        h64, h32 = M.fnv64(el, lens, (0, 1, 16)), M.fnv32(el, lens)
        assert [[int(v) for v in row] for row in h64] == [[H.fnv_1a(k, s) for s in (0, 1, 16)] for k in keys]
        assert [int(v) for v in h32] == [H.fnv_1a_32(k) for k in keys]
    # the ragged front end: the same keys as one (blob, offsets) pair, short and long keys padded apart
    blob = np.frombuffer(b"".join(byte_keys), dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum(lens)])
    assert np.array_equal(M.hash_ragged(M.fnv64, blob, offs, (0, 1, 16)), M.fnv64(*_elements(byte_keys), (0, 1, 16)))
    assert np.array_equal(M.hash_ragged(M.fnv32, blob, offs), M.fnv32(*_elements(byte_keys)))
    el, n = M.pad(blob, offs)
    assert np.array_equal(n, lens) and np.array_equal(M.fnv64(el, n), M.hash_ragged(M.fnv64, blob, offs))


def test_cuckoo_triples_of_the_model():
    keys = [b"", b"a", b"this is a test", bytes(range(40))]
    h0 = np.array([H.fnv_1a(k) for k in keys], dtype=np.uint64)
    for cap, bits in ((10000, 32), (977, 12)):
        fp = [int(h) & ((1 << bits) - 1) for h in h0]
        want = [fp, [f % cap for f in fp], [H.fnv_1a(str(f)) % cap for f in fp]]
        assert M.cuckoo_triples(h0, cap, bits).tolist() == want


# ---------------------------------------------------------------------------------------------------------------- window geometry
def test_windows_of_hand_worked_keys():
    end = 3 * M.PAGE
    # 20 bytes from 6 bytes in front of a page end: a = 2, span = 22 -> two windows; the first overhangs by 8 and NEEDS the next page
    # (sh = 0); the last one starts in the next page.  The last window is requested twice.
    w = M.windows(end - 6, 20)
    assert [(x.index, x.first, x.last, x.over, x.sh, x.need) for x in w] == [(0, True, False, 8, 0, 22), (1, False, True, 0, 0, 6), (1, False, True, 0, 0, 6)]
    assert {x.a for x in w} == {2} and w[0].addr == end - 8
    # 5 bytes that end 3 bytes in front of the page end: the window overhangs by 8, needs nothing there and moves down two dwords
    (w0, w1) = M.windows(end - 8, 5)
    assert w0 == w1 and (w0.a, w0.over, w0.sh, w0.first, w0.last, w0.addr - 4 * w0.sh) == (0, 8, 2, True, True, end - 16)
    # the last byte of the page: overhang 12, moved down three dwords
    assert M.windows(end - 1, 1)[0][:6] == (3, 0, True, True, 12, 3)
    assert M.windows(end - 1, 2)[0][:6] == (3, 0, True, True, 12, 0)  # ... unless the key goes on behind the page end
    assert M.windows(100, 0) == [] and M.windows(100, 0, 4) == []
    # code points: five elements whose last one is the page's last dword: window 1 holds ONE element and moves down three dwords
    w = M.windows(end - 20, 5, 4)
    assert [(x.index, x.over, x.sh, x.need) for x in w] == [(0, 0, 0, 16), (1, 12, 3, 4), (1, 12, 3, 4)]
    assert M.windows(end - 8, 4, 4)[0][4:6] == (8, 0)  # four elements across the page end: the window stays
    assert M.load_range([(end - 1, 1)]) == (end - 16, end) and M.load_range([(end - 20, 5, )], 4) == (end - 20, end)


def test_reachable_classes():
    r1, r4 = M.reachable(1), M.reachable(4)
    # 4 alignments x 7 (overhang, shift) pairs x first / last = 112; a window that is not the key's last one needs the bytes behind it
    # and never moves: 2 x 4 x 3 classes cannot occur
    assert len(r1) == 88 and all(sh == 0 or last for _, _, sh, _, last in r1)
    assert {(over, sh) for _, over, sh, _, _ in r1} == {(0, 0), (4, 0), (4, 1), (8, 0), (8, 2), (12, 0), (12, 3)}
    assert len(r4) == 22 and {a for a, *_ in r4} == {0} and r4 == {c for c in r1 if c[0] == 0}


def test_seam_batches_reach_every_class_and_stay_inside_their_pages():
    """the inputs of the page-seam tests: byte keys (through psk_fnv1a_hash and psk_qf_hash alike: one pair serves both) and code points"""
    for entry_points, (blob, offs, pinned), eb in ((("psk_fnv1a_hash", "psk_qf_hash"), M.seam_bytes(), 1), (("psk_fnv1a_hash", "psk_qf_hash"), M.seam_code_points(), 4)):
        keys = M.keys_of(offs, eb)
        assert offs[0] == 0 and offs[-1] == blob.size and blob.nbytes % M.PAGE == 0
        assert M.classes_of([keys[i] for i in pinned], eb) == M.reachable(eb), entry_points
        reached, lo, hi = M.survey(keys, eb)
        assert reached == M.reachable(eb)
        assert 0 <= lo and hi <= blob.nbytes  # no window leaves the blob itself, let alone the pages around it
        rest = np.setdiff1d(np.arange(len(keys)), pinned)
        # the stretches between: one per page, a page less the pinned keys on both sides (bytes: 96 before and up to 15 + 96 behind a
        # page end; code points: up to 273 + 4 elements before and 3 + 273 behind)
        assert len(rest) == blob.nbytes // M.PAGE and np.diff(offs)[rest].min() >= (M.PAGE - 96 - 111 if eb == 1 else 1024 - 277 - 276)
    blob, offs, pinned = M.seam_bytes()
    ends = np.arange(1, blob.size // M.PAGE) * M.PAGE
    at = {(int(s - ends[np.argmin(np.abs(ends - s))]), int(n)) for s, n in zip(offs[pinned], np.diff(offs)[pinned])}
    assert at == {(s, n) for s in range(-96, 16) for n in range(97)}  # every (start, length) is pinned, once
    assert len(pinned) == 112 * 97
    blob, offs, pinned = M.seam_code_points()
    lens = np.diff(offs)[pinned]
    assert set(lens.tolist()) == set(M.SEAM_CODE_POINT_LENGTHS) and blob.max() > 0xFFFF and blob.min() >= 0
    for n in M.SEAM_CODE_POINT_LENGTHS:  # every start from which the key or the window behind it touches the page end
        starts = offs[pinned][lens == n]
        assert sorted(int(s - round(s / 1024) * 1024) for s in starts) == list(range(-(n + 4), 4)), n


def test_fixed_walk_cases_take_every_start_residue_and_stay_inside():
    for L, m, n in M.fixed_walk_cases():
        keys = [(m + i * L, L) for i in range(n)]
        if L % 2:
            assert {a % M.PAGE for a, _ in keys} == set(range(M.PAGE))  # gcd(L, 4096) = 1
        assert M.fixed_source(L, m) == "KeysFixed<false>"
        lo, hi = M.load_range(keys)
        assert lo >= 0 and hi <= m + n * L + 16
    odd = M.classes_of([(i * L, L) for L in M.FIXED_WALK_ODD for i in range(M.FIXED_WALK_N)])
    assert {c[:3] for c in odd} == {c[:3] for c in M.reachable(1)}  # every (alignment, overhang, shift) also on the fixed-length walk
    assert {m for L, m, _ in M.fixed_walk_cases() if L in M.FIXED_WALK_EVEN} == {0, 1, 2, 3}


# ---------------------------------------------------------------------------------------------------------------- dispatch matrix
def test_dispatch_matrix_maps_to_the_expected_sources():
    assert set(M.DISPATCH_CELLS) == set(M.DISPATCH_EXPECTED) and len(M.DISPATCH_CELLS) == 3 * 7 + 6 * 3
    base = 5 * M.PAGE
    for L, m in M.DISPATCH_CELLS:
        assert M.fixed_source(L, base + m) == M.DISPATCH_EXPECTED[L, m], (L, m)
    assert {M.DISPATCH_EXPECTED[c] for c in M.DISPATCH_CELLS} == set(M.SOURCES) and len(M.SOURCES) == 5
    # what no test handed over before: 16-byte keys at a 4- / 8-aligned pointer, whole-dword lengths at an odd one
    assert M.DISPATCH_EXPECTED[16, 4] == M.DISPATCH_EXPECTED[16, 8] == "KeysFixed<true>"
    assert all(M.DISPATCH_EXPECTED[L, 1] == "KeysFixed<false>" for L in (8, 16, 32))
    assert M.DISPATCH_N > 2 * M.TILE and M.DISPATCH_N % M.TILE
    for L, m in M.DISPATCH_CELLS:  # the windows of the misaligned cells stay inside the matrix's pages
        if M.DISPATCH_EXPECTED[L, m] == "KeysFixed<false>":
            lo, hi = M.load_range([(m + i * L, L) for i in range(M.DISPATCH_N)])
            assert lo >= 0 and hi <= m + M.DISPATCH_N * L + 16


# ----------------------------------------------------------------------------------------------------------------- length classes
def test_len_class_boundaries():
    assert [M.len_class(n) for n in (0, 47, 48, 63, 64, 255, 256, 271, 272, 273, 1000, 2**31 - 1)] == [0, 47, 48, 48, 49, 60, 61, 61, 62, 62, 62, 62]
    assert {M.len_class(n) for n in range(2000)} == set(range(63))


def test_class_batches_hold_what_their_names_say():
    b = M.class_batches()
    lens = b["all_classes"]
    assert lens.size == 2 * M.TILE + 777
    full = lens.size // M.TILE
    for t in range(full):  # every one of the 63 classes in every full tile -- and in every stretch of 80 keys, whatever tile the engine cuts
        assert {M.len_class(int(n)) for n in lens[t * M.TILE:(t + 1) * M.TILE]} == set(range(63))
    assert all({M.len_class(int(n)) for n in lens[s:s + 80]} == set(range(63)) for s in range(0, lens.size - 80, 37))
    assert {272, 273, 400, 1000, 48, 63, 256, 271} <= set(lens.tolist())
    assert {M.len_class(int(n)) for n in b["one_class_300"]} == {62} and b["one_class_300"].size == M.TILE + 1
    assert {M.len_class(int(n)) for n in b["one_class_48_63"]} == {48} and set(b["one_class_48_63"].tolist()) == set(range(48, 64))
    for name in ("extremes_alternating", "extremes_blocks_of_64"):
        assert b[name].size == 2 * M.TILE + 1 and set(b[name].tolist()) == {0, 1000}
    assert b["extremes_alternating"][:4].tolist() == [0, 1000, 0, 1000]
    blocks = b["extremes_blocks_of_64"]
    assert not blocks[:64].any() and (blocks[64:128] == 1000).all() and not blocks[128:192].any()
    assert set(M.CODE_POINT_BATCHES) <= set(b)
    for name, lens in b.items():  # ragged(): the keys' elements end to end, nothing else
        for cps in (False, True):
            blob, offs = M.ragged(lens[:200], 1, cps)
            assert np.array_equal(np.diff(offs), lens[:200]) and blob.size == offs[-1] and blob.dtype == (np.int32 if cps else np.uint8)
