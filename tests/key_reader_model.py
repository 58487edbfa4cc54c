"""The key readers of psk_device.hpp, restated for the tests: what they must compute, which 16-byte windows they ask for, which
source a fixed-length batch must take -- and the inputs of tests/test_gpu_key_readers.py, so that tests/test_key_reader_model.py can
say on the CPU what those inputs reach.  Plain Python / numpy; nothing here imports the engine.

* ``fnv64`` / ``fnv32``: FNV-1a of a whole batch at once (the constants of pyprobables_amd/hashes.py: basis + 31 * seed, the WHOLE
  element XORed in, so a code point above 255 goes in whole).
* ``windows``: the window requests of ``first_window16`` + ``walk_key_bytes`` (byte keys) and of ``KeysVarlen::first`` +
  ``walk_key_elems`` (4-byte elements) for a key at a byte address, each with what ``load_window16`` makes of it.  A description of the
  geometry, written from the comments and the code of those functions; no hashing in it.
* ``fixed_source``: the source ``with_source`` (psk_stage.hpp) and ``with_part_source`` (psk_host.hpp) must choose.
* ``len_class``: ``KeysVarlen::len_class``, the 63 classes of pass 1's length sort.
* the generators: ``seam_bytes``, ``seam_code_points``, ``fixed_walk_cases``, ``DISPATCH_CELLS``, ``class_batches``.

Addresses are byte offsets from a page-aligned base: only an address's position inside its 4 KiB page matters to the readers.
"""

from collections import namedtuple

import numpy as np

PAGE = 4096
FNV64_BASIS, FNV64_PRIME = 0xCBF29CE484222325, 0x100000001B3
FNV32_BASIS, FNV32_PRIME = 0x811C9DC5, 0x01000193


# ------------------------------------------------------------------------------------------------------------------ hash reference
def _fnv(elements, lengths, seed, basis, prime, dtype):
    el = np.asarray(elements)
    lengths = np.asarray(lengths, dtype=np.int64)
    n = lengths.size
    assert el.ndim == 2 and el.shape[0] == n and (n == 0 or int(lengths.max(initial=0)) <= el.shape[1])
    seeds = [int(seed)] if np.ndim(seed) == 0 else [int(s) for s in seed]
    mask = (1 << (8 * np.dtype(dtype).itemsize)) - 1
    h = np.empty((n, len(seeds)), dtype=dtype)
    h[:] = np.array([(basis + 31 * s) & mask for s in seeds], dtype=dtype)
    if n:
        # the keys longest first: the keys still running at column c are then the first live[c] rows -- the mask of the step is a prefix
        order = np.argsort(-lengths, kind="stable")
        maxlen = int(lengths.max())
        cols = np.ascontiguousarray(el[order, :maxlen].T)
        live = n - np.cumsum(np.bincount(lengths, minlength=maxlen + 1))[:maxlen]
        hs = h[order]
        p = dtype(prime)
        for c in range(maxlen):
            k = int(live[c])
            hv = hs[:k]
            np.bitwise_xor(hv, cols[c, :k, None].astype(dtype), out=hv)  # hval ^= element (whole)
            np.multiply(hv, p, out=hv)                                   # hval *= prime, mod 2^64 / 2^32
        h[order] = hs
    return h[:, 0] if np.ndim(seed) == 0 else h


def fnv64(elements, lengths, seed=0):
    """64-bit FNV-1a of key i = elements[i, :lengths[i]] -> uint64[n] for one seed, uint64[n, len(seed)] for a sequence of seeds"""
    return _fnv(elements, lengths, seed, FNV64_BASIS, FNV64_PRIME, np.uint64)


def fnv32(elements, lengths, seed=0):
    """32-bit FNV-1a (the QuotientFilter's hash), as fnv64"""
    return _fnv(elements, lengths, seed, FNV32_BASIS, FNV32_PRIME, np.uint32)


def pad(blob, offsets):
    """a ragged (blob, offsets) pair -> (elements[n, longest key], lengths[n])"""
    offsets = np.asarray(offsets, dtype=np.int64)
    lengths = np.diff(offsets)
    out = np.zeros((lengths.size, int(lengths.max(initial=0))), dtype=blob.dtype)
    for i in range(lengths.size):
        out[i, : lengths[i]] = blob[offsets[i]:offsets[i + 1]]
    return out, lengths


def hash_ragged(fn, blob, offsets, seed=0, split=128):
    """fn (fnv64 / fnv32) over a ragged pair; the keys of up to `split` elements and the longer ones are padded apart, so that a few
    long keys do not pad thousands of short ones"""
    offsets = np.asarray(offsets, dtype=np.int64)
    lengths = np.diff(offsets)
    width = 1 if np.ndim(seed) == 0 else len(seed)
    out = np.empty((lengths.size, width), dtype=np.uint64 if fn is fnv64 else np.uint32)
    for rows in (np.flatnonzero(lengths <= split), np.flatnonzero(lengths > split)):
        if rows.size:
            sub = np.zeros((rows.size, int(lengths[rows].max())), dtype=blob.dtype)
            for r, i in enumerate(rows):
                sub[r, : lengths[i]] = blob[offsets[i]:offsets[i + 1]]
            out[rows] = fn(sub, lengths[rows], seed).reshape(rows.size, width)
    return out[:, 0] if np.ndim(seed) == 0 else out


def cuckoo_triples(h0, capacity, fp_bits):
    """(fp, idx_1, idx_2)[n] of psk_ck_triples from the keys' fnv_1a(key, 0): fp = h & (2^bits - 1), idx_1 = fp % capacity,
    idx_2 = fnv_1a(str(fp)) % capacity"""
    fp = np.asarray(h0, dtype=np.uint64) & np.uint64((1 << fp_bits) - 1)
    digits = [np.frombuffer(str(int(v)).encode(), dtype=np.uint8) for v in fp]
    el = np.zeros((fp.size, 20), dtype=np.uint8)
    for i, d in enumerate(digits):
        el[i, : d.size] = d
    h2 = fnv64(el, [d.size for d in digits])
    return np.stack([fp, fp % np.uint64(capacity), h2 % np.uint64(capacity)]).astype(np.uint32)


# --------------------------------------------------------------------------------------------------------------- window geometry
# a: the key's start alignment (address & 3; 0 for 4-byte elements).  index: window number, window t covers [w + 16 t, w + 16 t + 16)
# with w = address - a.  first / last: window 0 / the key's last window.  over: bytes of the window beyond its 4 KiB page (0, 4, 8, 12).
# sh: dwords the load is moved down (then it ends at the page end).  addr: the window's own address; the load reads
# [addr - 4 sh, addr - 4 sh + 16).  need: the bytes of the window the caller says it uses.
Window = namedtuple("Window", "a index first last over sh addr need")


def _window(a, index, nwin, addr, need):
    in_page = addr & (PAGE - 1)
    over = in_page - (PAGE - 16) if in_page > PAGE - 16 else 0
    sh = over >> 2 if need + over <= 16 else 0  # need beyond the page end: the next page holds key bytes, the window stays where it is
    return Window(a, index, index == 0, index == nwin - 1, over, sh, addr, need)


def windows(addr, length, elem_bytes=1):
    """the windows the walk of ONE key of `length` elements at byte address `addr` requests, in request order: the first window, then in
    front of the hashing of window t the window min(t + 1, last) -- so the last window is requested twice.  An empty key requests no
    window of its own (KeysVarlen::first takes one at the blob's first element, and nobody looks at it)."""
    if elem_bytes == 1:
        a = addr & 3
        w = addr - a
        span = a + length
        nwin = (span + 15) >> 4 if length else 0
        need = lambda t: span - 16 * t                         # noqa: E731  (everything from the window's start to the key's end)
    else:
        assert elem_bytes == 4 and addr % 4 == 0
        a, w = 0, addr
        nwin = (length + 3) >> 2
        need = lambda t: 4 * min(length - 4 * t, 4)            # noqa: E731  (the key's elements inside the window)
    if nwin == 0:
        return []
    order = [0] + [min(t + 1, nwin - 1) for t in range(nwin)]
    return [_window(a, t, nwin, w + 16 * t, need(t)) for t in order]


def window_class(w):
    return (w.a, w.over, w.sh, w.first, w.last)


def survey(keys, elem_bytes=1):
    """a list of (address, length) keys in ONE pass -> (the window classes they reach, lo, hi) with [lo, hi) the bytes their window
    loads touch, the keys' own bytes included"""
    classes, lo, hi = set(), None, None
    for addr, length in keys:
        spans = [(addr, addr + length * elem_bytes)]
        for w in windows(addr, length, elem_bytes):
            classes.add(window_class(w))
            spans.append((w.addr - 4 * w.sh, w.addr - 4 * w.sh + 16))
        lo = min([s for s, _ in spans] + ([] if lo is None else [lo]))
        hi = max([e for _, e in spans] + ([] if hi is None else [hi]))
    return classes, lo, hi


def classes_of(keys, elem_bytes=1):
    """the window classes a list of (address, length) keys reaches"""
    return survey(keys, elem_bytes)[0]


def reachable(elem_bytes=1):
    """every window class there is, by brute force: all starts in [page end - 96, page end + 16) and all lengths 0 .. 96"""
    end = 4 * PAGE
    return classes_of([(s, n) for s in range(end - 96, end + 16, elem_bytes) for n in range(97)], elem_bytes)


def load_range(keys, elem_bytes=1):
    """[lo, hi): the bytes the window loads of a list of (address, length) keys touch, the keys' own bytes included"""
    return survey(keys, elem_bytes)[1:]


# ----------------------------------------------------------------------------------------------------------------- source chooser
SOURCES = ("KeysFixed16", "KeysFixed8", "KeysFixed32", "KeysFixed<true>", "KeysFixed<false>")


def fixed_source(key_len, addr):
    """the source a PSK_KEYS_FIXED batch of `key_len`-byte keys at `addr` must take"""
    if key_len == 16 and addr % 16 == 0:
        return "KeysFixed16"
    if key_len == 8 and addr % 8 == 0:
        return "KeysFixed8"
    if key_len == 32 and addr % 16 == 0:
        return "KeysFixed32"
    if key_len % 4 == 0 and addr % 4 == 0:
        return "KeysFixed<true>"
    return "KeysFixed<false>"


# (key length, misalignment of the device pointer) cells of the dispatch matrix, and the source each must take -- written out by hand
DISPATCH_CELLS = [(L, m) for L in (8, 16, 32) for m in (0, 1, 2, 3, 4, 8, 12)] + [(L, m) for L in (4, 12, 20, 24, 64, 68) for m in (0, 1, 4)]
DISPATCH_EXPECTED = {
    **{(8, m): s for m, s in zip((0, 1, 2, 3, 4, 8, 12), ("KeysFixed8", "KeysFixed<false>", "KeysFixed<false>", "KeysFixed<false>",
                                                          "KeysFixed<true>", "KeysFixed8", "KeysFixed<true>"))},
    **{(16, m): s for m, s in zip((0, 1, 2, 3, 4, 8, 12), ("KeysFixed16", "KeysFixed<false>", "KeysFixed<false>", "KeysFixed<false>",
                                                           "KeysFixed<true>", "KeysFixed<true>", "KeysFixed<true>"))},
    **{(32, m): s for m, s in zip((0, 1, 2, 3, 4, 8, 12), ("KeysFixed32", "KeysFixed<false>", "KeysFixed<false>", "KeysFixed<false>",
                                                           "KeysFixed<true>", "KeysFixed<true>", "KeysFixed<true>"))},
    **{(L, m): ("KeysFixed<false>" if m == 1 else "KeysFixed<true>") for L in (4, 12, 20, 24, 64, 68) for m in (0, 1, 4)},
}
DISPATCH_N = 5000  # keys per cell: two 2048-key tiles and a tail


def dispatch_keys(L):
    """the keys of every cell of one key length (the same keys at every misalignment)"""
    return np.random.default_rng(1000 + L).integers(0, 256, size=(DISPATCH_N, L), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------ pass 1's length sort
TILE = 2048  # keys of a full pass-1 tile


def len_class(length):
    """KeysVarlen::len_class: the exact length below 48 elements, steps of 16 up to 271, one class for the rest -- 0 .. 62"""
    return length if length < 48 else (48 + ((length - 48) >> 4) if length < 48 + 14 * 16 else 62)


def all_class_lengths(n=2 * TILE + 777):
    """lengths that cycle through every class: 0 .. 47, both ends of every 16-step class (48, 63, 64, 79, ... 256, 271), then 272, 273,
    400 and 1000 -- 80 lengths, so that every stretch of 80 keys, and with it every full tile, holds every class"""
    cycle = list(range(48)) + [v for c in range(14) for v in (48 + 16 * c, 63 + 16 * c)] + [272, 273, 400, 1000]
    return np.array([cycle[i % len(cycle)] for i in range(n)], dtype=np.int64)


def class_batches():
    """name -> lengths (in elements) of the batches of the length-class tests"""
    blocks = np.where((np.arange(2 * TILE + 1) // 64) % 2 == 0, 0, 1000)
    return {
        "all_classes": all_class_lengths(),
        "one_class_300": np.full(TILE + 1, 300, dtype=np.int64),
        "one_class_48_63": 48 + (np.arange(TILE + 1) * 7) % 16,
        "extremes_alternating": np.where(np.arange(2 * TILE + 1) % 2 == 0, 0, 1000),
        "extremes_blocks_of_64": blocks,
    }


CODE_POINT_BATCHES = ("all_classes", "extremes_alternating", "extremes_blocks_of_64")
MAX_CODE_POINT = 0x2FFFF


def ragged(lengths, seed, code_points=False):
    """(blob, offsets) of random keys of the given lengths: uint8 bytes, or int32 code points up to 0x2FFFF"""
    lengths = np.asarray(lengths, dtype=np.int64)
    offs = np.zeros(lengths.size + 1, dtype=np.int64)
    np.cumsum(lengths, out=offs[1:])
    rng = np.random.default_rng(seed)
    if code_points:
        return rng.integers(0, MAX_CODE_POINT + 1, size=int(offs[-1]), dtype=np.int32), offs
    return rng.integers(0, 256, size=int(offs[-1]), dtype=np.uint8), offs


# ------------------------------------------------------------------------------------------------------------------ seam batches
def _chains(combos):
    """(start, length) pairs, starts relative to a page end, -> chains of pairs that lie end to end (the next key starts where the last
    one ended), every pair in exactly one chain.  A chain goes on for as long as some unused pair starts where it stands."""
    left = {}
    for s, n in combos:
        left.setdefault(s, []).append(n)
    for v in left.values():
        v.sort(reverse=True)  # (shortest last)
    chains = []
    for s0 in sorted(left):
        while left[s0]:
            s, chain = s0, []
            while left.get(s):
                ls = left[s]
                # the shortest unused length that leads to a start with unused pairs (0 stays here); none: the longest ends the chain
                pick = next((j for j in range(len(ls) - 1, -1, -1) if ls[j] == 0 or left.get(s + ls[j])), 0)
                n = ls.pop(pick)
                chain.append((s, n))
                s += n
            chains.append(chain)
    return chains


def _lay_out(chains, page_elems):
    """chain j around page end j + 1, the stretches between the chains as keys of their own -> (offsets, indices of the pinned keys)"""
    offs, pinned, pos = [0], [], 0
    for j, chain in enumerate(chains):
        end = (j + 1) * page_elems
        assert end + chain[0][0] > pos
        pos = end + chain[0][0]
        offs.append(pos)  # the stretch up to the chain
        for s, n in chain:
            assert pos == end + s
            pinned.append(len(offs) - 1)
            pos += n
            offs.append(pos)
    total = (len(chains) + 1) * page_elems
    assert pos < total
    offs.append(total)
    return np.array(offs, dtype=np.int64), np.array(pinned, dtype=np.int64)


_cache = {}


def seam_bytes():
    """byte keys pinned at every (start, length) with the start in [page end - 96, page end + 16) and the length in 0 .. 96, several
    around each page end, the ~3.9 KiB between two page ends' keys as a key of its own (hundreds of windows each) ->
    (blob uint8, offsets int64, indices of the pinned keys).  The blob starts on a page boundary and ends on one."""
    if "bytes" not in _cache:
        offs, pinned = _lay_out(_chains([(s, n) for s in range(-96, 16) for n in range(97)]), PAGE)
        blob = np.random.default_rng(4096).integers(0, 256, size=int(offs[-1]), dtype=np.uint8)
        _cache["bytes"] = (blob, offs, pinned)
    return _cache["bytes"]


SEAM_CODE_POINT_LENGTHS = tuple(range(41)) + (47, 48, 49, 271, 272, 273)


def seam_code_points():
    """code-point keys of the lengths 0 .. 40, 47 .. 49 and 271 .. 273 at every start from which the key, or the window behind its last
    element, touches the page end: element positions [-(length + 4), 4) around it -> (blob int32, offsets int64 in elements, pinned)"""
    if "cps" not in _cache:
        offs, pinned = _lay_out(_chains([(s, n) for n in SEAM_CODE_POINT_LENGTHS for s in range(-(n + 4), 4)]), PAGE // 4)
        blob = np.random.default_rng(4097).integers(0, MAX_CODE_POINT + 1, size=int(offs[-1]), dtype=np.int32)
        _cache["cps"] = (blob, offs, pinned)
    return _cache["cps"]


def keys_of(offsets, elem_bytes=1):
    """(byte address, length) of every key of a pair whose blob starts on a page boundary"""
    offsets = np.asarray(offsets, dtype=np.int64)
    return [(int(o) * elem_bytes, int(n)) for o, n in zip(offsets[:-1], np.diff(offsets))]


# -------------------------------------------------------------------------------------------------------------- fixed-length walk
FIXED_WALK_ODD = (1, 3, 5, 7, 13, 17, 31, 33, 63, 65)   # 4096 keys end to end from a page boundary: gcd(L, 4096) = 1, every residue
FIXED_WALK_EVEN = (6, 10, 18)                           # from base misalignments 0 .. 3
FIXED_WALK_N = 4096


def fixed_walk_cases():
    """(key length, misalignment of the base, keys) of the fixed-length walk"""
    return [(L, 0, FIXED_WALK_N) for L in FIXED_WALK_ODD] + [(L, m, FIXED_WALK_N) for L in FIXED_WALK_EVEN for m in range(4)]


def fixed_keys(L, m, n):
    return np.random.default_rng(7000 + 16 * L + m).integers(0, 256, size=(n, L), dtype=np.uint8)
