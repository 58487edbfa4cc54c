"""The table algebra stated plainly, on int64 numpy arrays and Python ints: what the kernels behind CountMinSketch.join (countminsketch.py:380-399),
CountingBloomFilter.union / intersection / jaccard_index (countingbloom.py:210-300), BloomFilter.union / intersection and the slice reduce of the
multi-GPU merge have to give.  tests/test_table_algebra_model.py holds every function against cases recorded from the real reference
(tests/golden/golden_table_algebra.json); the GPU tests use them at sizes the reference is too slow for."""

import numpy as np

I32_MIN, I32_MAX = -(2**31), 2**31 - 1
U32_MAX = 2**32 - 1
I64_MIN, I64_MAX = -(2**63), 2**63 - 1
U64_MAX = 2**64 - 1


def _i64(a):
    return np.asarray(a, dtype=np.int64)


def join(dst, src):
    """countminsketch.py:381-391: a bin of `dst` that stands on a rail stays as it is, every other bin takes the clamped sum"""
    d, s = _i64(dst), _i64(src)
    frozen = (d == I32_MIN) | (d == I32_MAX)
    return np.where(frozen, d, np.clip(d + s, I32_MIN, I32_MAX))


def join_elements(a: int, b: int) -> int:
    """countminsketch.py:394-399"""
    return max(min(int(a) + int(b), I64_MAX), I64_MIN)


def add_u32(dst, src):
    """-> (clamped sum, number of elements whose sum passes 2^32 - 1); the reference's array('I') store raises when that number is not 0"""
    t = _i64(dst) + _i64(src)
    return np.minimum(t, U32_MAX), int((t > U32_MAX).sum())


def intersect(a, b):
    """countingbloom.py:235-238: (a > 0 and b > 0) ? a + b : 0, clamped and counted like add_u32"""
    a, b = _i64(a), _i64(b)
    t = np.where((a > 0) & (b > 0), a + b, 0)
    return np.minimum(t, U32_MAX), int((t > U32_MAX).sum())


def jaccard_counts(a, b):
    """countingbloom.py:260-266 -> (#(a > 0 or b > 0), #(a > 0 and b > 0))"""
    x, y = _i64(a) > 0, _i64(b) > 0
    return int((x | y).sum()), int((x & y).sum())


def jaccard(a, b) -> float:
    """countingbloom.py:267-269"""
    cu, ci = jaccard_counts(a, b)
    return 1.0 if cu == 0 else ci / cu


def nonzero(words) -> int:
    """countingbloom.py:302-304"""
    return int((_i64(words) != 0).sum())


def popcount(words) -> int:
    """bloom.py:552-557 on 32-bit words"""
    w = _i64(words).astype(np.uint32)
    return int(np.unpackbits(w.view(np.uint8)).sum())


def or_slices(src, nslices: int):
    """dst[w] = OR over j of src[j * slice + w]"""
    s = _i64(src).reshape(nslices, -1)
    return np.bitwise_or.reduce(s, axis=0)


def table_or(a, b):
    return _i64(a) | _i64(b)


def table_and(a, b):
    return _i64(a) & _i64(b)


# ---- what an update does to a table that came out of the algebra (the reference's add / remove, per counter)
def cbf_add_delta(table, delta):
    """countingbloom.py:146-153: adds saturate at 2^32 - 1.  `delta[i]` is the sum of the counts a batch adds to counter i (all counts
    are positive, so the saturating adds commute: the end value is min(sum, rail) in any order)."""
    return np.minimum(_i64(table) + _i64(delta), U32_MAX)


def cms_add_delta(bins, delta):
    """countminsketch.py:276-284 with num_els >= 0 throughout: min(sum, INT32_MAX) in any order"""
    return np.minimum(_i64(bins) + _i64(delta), I32_MAX)


def cms_remove_delta(bins, delta):
    """countminsketch.py:309-316 with num_els >= 0 throughout: max(difference, INT32_MIN) in any order"""
    return np.maximum(_i64(bins) - _i64(delta), I32_MIN)


def as_u32(a) -> np.ndarray:
    return _i64(a).astype(np.uint32)


def as_i32(a) -> np.ndarray:
    return _i64(a).astype(np.int32)
