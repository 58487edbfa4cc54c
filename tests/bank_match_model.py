"""BloomFilterBank.match_many in numpy: the slice image (the bank transposed) and "which filters may hold this key".

``slices_of`` transposes the rows of ``bank_model.bank_rows``: slice row p holds bit p of every filter, ``slice_row_bytes(filters)`` wide
(ceil(filters / 8) rounded up to 16), bits LSB first, columns at and beyond ``filters`` zero.  ``match_mask`` is the AND of a key's k slice
rows; ``match_counts`` and ``match_ids`` restate it as counts and as (offsets, ascending ids).  Nothing here imports the engine or the reference.
"""

from __future__ import annotations

import numpy as np

from bank_model import row_bytes  # noqa: F401  (re-exported: the two layouts side by side)


def slice_row_bytes(filters: int) -> int:
    return ((filters + 7) // 8 + 15) & ~15


def slices_of(rows: np.ndarray, filters: int, m: int) -> np.ndarray:
    """uint8[filters, row_bytes(m)] -> uint8[m, slice_row_bytes(filters)]"""
    bits = np.unpackbits(np.ascontiguousarray(rows[:filters], dtype=np.uint8), axis=1, bitorder="little")[:, :m]  # [filters, m]
    out = np.zeros((m, slice_row_bytes(filters) * 8), dtype=np.uint8)
    out[:, :filters] = bits.T
    return np.packbits(out, axis=1, bitorder="little")


def match_mask(slices: np.ndarray, m: int, k: int, hashes: np.ndarray) -> np.ndarray:
    """uint8[n, slice_row_bytes]: bit f of row i is set when all k bits of key i are set in filter f"""
    bit = (np.asarray(hashes, dtype=np.uint64)[:, :k] % np.uint64(m)).astype(np.int64)  # hashes: (n, >= k)
    out = np.full((bit.shape[0], slices.shape[1]), 255, dtype=np.uint8)
    for j in range(k):
        out &= slices[bit[:, j]]
    return out


def _bytes(mask: np.ndarray) -> np.ndarray:
    """[n, w] words of any width, little endian -> uint8[n, w * itemsize] (n = 0 included)"""
    mask = np.ascontiguousarray(mask)
    return mask.view(np.uint8).reshape(mask.shape[0], mask.shape[1] * mask.itemsize)


def mask_bits(mask: np.ndarray, filters: int) -> np.ndarray:
    """uint8[n, bytes] (or uint32 words, little endian) -> bool[n, filters]"""
    raw = _bytes(mask)
    return np.unpackbits(raw, axis=1, bitorder="little")[:, :filters].astype(bool)


def match_counts(mask: np.ndarray) -> np.ndarray:
    raw = _bytes(mask)
    return np.unpackbits(raw, axis=1).sum(axis=1).astype(np.int32)


def match_ids(mask: np.ndarray):
    """-> (offsets int64[n + 1], ids int32[total]): the set columns of row i, ascending, are ids[offsets[i]:offsets[i + 1]]"""
    raw = _bytes(mask)
    bits = np.unpackbits(raw, axis=1, bitorder="little")
    offsets = np.zeros(mask.shape[0] + 1, dtype=np.int64)
    np.cumsum(bits.sum(axis=1), out=offsets[1:])
    return offsets, np.nonzero(bits)[1].astype(np.int32)
