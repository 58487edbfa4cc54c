"""BloomFilterBank in numpy: row f of the bank is the reference's BloomFilter table after add() of the keys sent to f.

``hashes_of`` restates the reference's ``default_fnv_1a`` on Python integers (one key: str by code point, bytes by byte);
``hashes_fixed`` is the same chain vectorised over an (n, L) uint8 matrix.  ``bank_rows`` sets the bits, ``bank_check`` answers
lookups; rows are ``row_bytes(m)`` wide (ceil(m / 8) rounded up to 16), bits LSB first.  Nothing here imports the engine or the reference.
"""

from __future__ import annotations

import numpy as np

U64 = 1 << 64
FNV_BASIS, FNV_PRIME = 14695981039346656037, 1099511628211


def row_bytes(m: int) -> int:
    return ((m + 7) // 8 + 15) & ~15


def hashes_of(key, k: int) -> list:
    out = []
    elems = list(map(ord, key)) if isinstance(key, str) else list(bytes(key))
    for seed in range(k):
        h = (FNV_BASIS + 31 * seed) % U64
        for e in elems:
            h = ((h ^ e) * FNV_PRIME) % U64
        out.append(h)
    return out


def hashes_fixed(keys: np.ndarray, k: int) -> np.ndarray:
    """(n, L) uint8 -> (n, k) uint64"""
    keys = np.ascontiguousarray(keys, dtype=np.uint8)
    out = np.empty((keys.shape[0], k), dtype=np.uint64)
    prime = np.uint64(FNV_PRIME)
    with np.errstate(over="ignore"):
        for seed in range(k):
            h = np.full(keys.shape[0], (FNV_BASIS + 31 * seed) % U64, dtype=np.uint64)
            for j in range(keys.shape[1]):
                h = (h ^ keys[:, j].astype(np.uint64)) * prime
            out[:, seed] = h
    return out


def hashes_list(keys, k: int) -> np.ndarray:
    return np.array([hashes_of(key, k) for key in keys], dtype=np.uint64).reshape(len(keys), k)


def bank_rows(filters: int, m: int, k: int, hashes: np.ndarray, ids, rows: np.ndarray | None = None) -> np.ndarray:
    """uint8[filters, row_bytes(m)] after the keys with (n, >= k) ``hashes`` went to filters ``ids``; ids >= filters are skipped"""
    rows = np.zeros((filters, row_bytes(m)), dtype=np.uint8) if rows is None else rows.copy()
    ids = np.asarray(ids, dtype=np.int64)
    keep = (ids >= 0) & (ids < filters)
    bit = np.asarray(hashes, dtype=np.uint64)[keep][:, :k] % np.uint64(m)
    f = np.repeat(ids[keep], k)
    bit = bit.reshape(-1).astype(np.int64)
    np.bitwise_or.at(rows, (f, bit >> 3), (1 << (bit & 7)).astype(np.uint8))
    return rows


def bank_check(rows: np.ndarray, m: int, k: int, hashes: np.ndarray, ids) -> np.ndarray:
    """bool[n]: all k bits of key i set in row ids[i]; False for ids >= filters"""
    ids = np.asarray(ids, dtype=np.int64)
    ok = (ids >= 0) & (ids < rows.shape[0])
    safe = np.where(ok, ids, 0)
    bit = (np.asarray(hashes, dtype=np.uint64)[:, :k] % np.uint64(m)).astype(np.int64)
    got = (rows[safe[:, None], bit >> 3] >> (bit & 7).astype(np.uint8)) & 1
    return ok & got.all(axis=1)
