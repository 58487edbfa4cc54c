"""Canonical layout of a quotient filter: a pure numpy model (test infrastructure, no GPU, no reference needed).

The reference's ``QuotientFilter`` (probables/quotientfilter/quotientfilter.py) drops duplicates, keeps every run sorted by remainder and
the runs of a cluster in quotient order, so its four arrays depend only on the SET of 32-bit hashes it was fed.  For the sorted distinct
hashes h_0 < h_1 < ... with q_i = h_i >> r, r = 32 - q:

    pos_i = max(q_i, pos_{i-1} + 1)  =  i + max_{j <= i} (q_j - j)                     (a prefix-max scan)

and when pos_{n-1} >= size the tail wraps into the head: the same scan with carry-in pos_{-1} = pos_{n-1} - size, i.e.
pos_i = i + max(c + 1, max_{j <= i} (q_j - j)).  One repeat suffices for n <= size (the carry cannot grow: c + 1 + n - 1 <= pos_{n-1}).
Element i is stored at pos_i mod size.

tests/test_quotient_model.py ties this model to the live reference and to tests/golden/golden_quotient.json; the GPU tests use it for
shapes the fixtures are too small for.
"""

from __future__ import annotations

import numpy as np


def remainder_dtype(q: int):
    """the reference's three width classes (array type codes B / I / L by r)"""
    r = 32 - q
    return np.uint8 if r <= 8 else (np.uint16 if r <= 16 else np.uint32)


def positions(hs: np.ndarray, q: int) -> np.ndarray:
    """slot (before the final `mod size`) of each of the sorted distinct hashes `hs`"""
    r, size = 32 - q, 1 << q
    n = hs.size
    if n > size:
        raise ValueError("more distinct hashes than slots")
    idx = np.arange(n, dtype=np.int64)
    m = np.maximum.accumulate((hs.astype(np.int64) >> r) - idx) if n else idx
    pos = idx + m
    if n and pos[-1] >= size:
        pos = idx + np.maximum(m, pos[-1] - size + 1)
    return pos


def canonical(hashes, q: int):
    """-> (filter, occupied, continuation, shifted) as the reference holds them after any stream with this set of hashes;
    the three metadata arrays as uint8[size] of 0 / 1"""
    r, size = 32 - q, 1 << q
    hs = np.unique(np.asarray(list(hashes) if not isinstance(hashes, np.ndarray) else hashes, dtype=np.uint64)).astype(np.int64)
    qs, rs = hs >> r, hs & ((1 << r) - 1)
    p = positions(hs, q) % size
    filt = np.zeros(size, dtype=remainder_dtype(q))
    occ, cont, sh = (np.zeros(size, dtype=np.uint8) for _ in range(3))
    filt[p] = rs
    occ[qs] = 1
    cont[p[1:]] = qs[1:] == qs[:-1]
    sh[p] = p != qs
    return filt, occ, cont, sh


def sorted_hashes(hashes) -> list[int]:
    return sorted({int(h) for h in hashes})


def reference_order(hashes, q: int) -> list[int]:
    """the order of the reference's ``get_hashes()``: slot order starting at the first empty slot -- the sorted list rotated to the
    first hash whose quotient lies behind that slot.  (A full table has no empty slot; the reference's walk runs off the table there.)"""
    size, r = 1 << q, 32 - q
    hs = sorted_hashes(hashes)
    filt, occ, cont, sh = canonical(hs, q)
    empty = np.flatnonzero((occ | cont | sh) == 0)
    if empty.size == 0:
        raise ValueError("full table: the reference cannot list it")
    e = int(empty[0])
    k = int(np.searchsorted(np.asarray(hs, dtype=np.int64), (e + 1) << r))
    return hs[k:] + hs[:k]


def contains(hashes, probes) -> list[bool]:
    s = {int(h) for h in hashes}
    return [int(p) in s for p in probes]


def final_quotient(stream, q: int, max_load: float = 0.85) -> int:
    """the quotient an auto-expanding reference filter ends with: ``add_alt`` tests ``load_factor >= max_load_factor`` at the START of
    every call (duplicates included), so the table doubles only when another call follows the one that reached the threshold"""
    seen = set()
    for h in stream:
        while len(seen) / (1 << q) >= max_load:
            q += 1
        seen.add(int(h))
    return q
