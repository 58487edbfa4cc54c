"""The filters of a BloomFilterBank as sets, in numpy, over a ``uint32[F][W]`` table (W = row_bytes(m) / 4 words; pad bits zero):
bit counts, ``estimate_elements``, the all-pairs intersection counts, ``jaccard_index`` and the OR / AND of groups of rows.

``estimate`` and ``false_positive_rate`` restate bloom.py:340-352 and 361-369 on Python numbers; ``jaccard`` is Python's ``I / U`` of
bloom.py:448-460.  An id at or beyond the table counts as an empty row, as the engine reads it.  Nothing here imports the engine or the reference.
"""

from __future__ import annotations

import math

import numpy as np

from bank_model import row_bytes  # noqa: F401  (re-exported)


def as_words(rows: np.ndarray) -> np.ndarray:
    """uint8[F, row_bytes] (or words already) -> uint32[F, W]"""
    rows = np.ascontiguousarray(rows)
    return rows if rows.dtype == np.uint32 else rows.view(np.uint32).reshape(rows.shape[0], -1)


def _bits(table: np.ndarray) -> np.ndarray:
    """uint32[n, W] -> uint8[n, 32 W] of 0 / 1"""
    return np.unpackbits(np.ascontiguousarray(table).view(np.uint8).reshape(table.shape[0], -1), axis=1, bitorder="little")


def take(table: np.ndarray, ids=None) -> np.ndarray:
    """the rows ``ids`` of the table (None: all); an id >= F gives a zero row"""
    if ids is None:
        return table
    ids = np.asarray(ids, dtype=np.int64)
    ok = (ids >= 0) & (ids < table.shape[0])
    out = table[np.where(ok, ids, 0)].copy()
    out[~ok] = 0
    return out


def popcount(table: np.ndarray, ids=None) -> np.ndarray:
    """int64[n]: the set bits of each row"""
    return _bits(take(table, ids)).sum(axis=1, dtype=np.int64)


def estimate(bits: int, m: int, k: int) -> int:
    """bloom.py:340-352"""
    if bits >= m:
        return -1
    log_n = math.log(1 - (float(bits) / float(m)))
    tmp = float(m) / float(k)
    return int(-1 * tmp * log_n)


def estimates(table: np.ndarray, m: int, k: int, ids=None) -> np.ndarray:
    return np.array([estimate(int(c), m, k) for c in popcount(table, ids)], dtype=np.int64)


def false_positive_rate(elements_added: int, m: int, k: int) -> float:
    """bloom.py:361-369"""
    num = k * -1 * elements_added
    dbl = num / m
    exp = math.exp(dbl)
    return math.pow((1 - exp), k)


def overlap(table_a: np.ndarray, a=None, table_b: np.ndarray | None = None, b=None) -> np.ndarray:
    """int64[na, nb]: popcount(row a_i AND row b_j) -- AND of 0 / 1 bits is their product, so the matrix is one matmul (exact in float32 up to 2^24
    bits a row, in float64 beyond)"""
    ba, bb = _bits(take(table_a, a)), _bits(take(table_a if table_b is None else table_b, b))
    t = np.float32 if ba.shape[1] < 2**24 else np.float64
    return np.rint(ba.astype(t) @ bb.astype(t).T).astype(np.int64)


def jaccard(inter: np.ndarray, ca: np.ndarray, cb: np.ndarray) -> np.ndarray:
    """float64[na, nb]: bloom.py:448-460 from the counts, each entry Python's own quotient of two ints"""
    out = np.empty(inter.shape, dtype=np.float64)
    for i in range(inter.shape[0]):
        for j in range(inter.shape[1]):
            union = int(ca[i]) + int(cb[j]) - int(inter[i, j])
            out[i, j] = 1.0 if union == 0 else int(inter[i, j]) / union
    return out


def reduce_rows(table: np.ndarray, groups, op: str) -> np.ndarray:
    """uint32[G, W]: row g = the OR / AND of the rows groups[g]; an empty group gives zeros under either op"""
    out = np.zeros((len(groups), table.shape[1]), dtype=np.uint32)
    for g, members in enumerate(groups):
        rows = take(table, members)
        if len(members):
            out[g] = np.bitwise_or.reduce(rows, axis=0) if op == "or" else np.bitwise_and.reduce(rows, axis=0)
    return out


def sent_indices(s):
    """a "sent" entry of tests/golden/golden_bank_stats.json -> pool indices in the order of their add()"""
    return list(range(s[1], s[2])) if s and s[0] == "range" else list(s)


def fixture_keys(c):
    """-> (keys, ids): every key of the fixture with the filter it goes to"""
    keys, ids = [], []
    for f, s in enumerate(c["sent"]):
        for i in sent_indices(s):
            keys.append(c["key_prefix"] + str(i))
            ids.append(f)
    return keys, np.array(ids, dtype=np.int64)
