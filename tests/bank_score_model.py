"""BloomFilterBank.score_many in numpy: whole queries against every filter.

A query is a run of keys, ``offsets[q]:offsets[q + 1]``; its score in filter f is the number of its keys that f may hold, a repeated key counted
each time: the column sums of the per-key answers (``bank_match_model.mask_bits`` of ``match_mask``, or the reference's own ``key in blm[f]``).
``select`` keeps, per query, the filters whose score reaches the query's threshold, ascending; ``thresholds`` restates
``pyprobables_amd.bank.score_thresholds``.  Nothing here imports the engine or the reference.
"""

from __future__ import annotations

import math

import numpy as np


def score_counts(bits: np.ndarray, offsets) -> np.ndarray:
    """bool[n, F] (key i may be in filter f), offsets[Q + 1] -> int32[Q, F]"""
    bits = np.asarray(bits, dtype=bool)
    offsets = np.asarray(offsets, dtype=np.int64)
    out = np.zeros((offsets.size - 1, bits.shape[1]), dtype=np.int32)
    for q in range(offsets.size - 1):
        out[q] = bits[offsets[q]:offsets[q + 1]].sum(axis=0)
    return out


def select(counts: np.ndarray, thresholds):
    """-> (offsets int64[Q + 1], ids int32[total], scores int32[total]): the filters of query q with counts[q, f] >= thresholds[q], ascending"""
    counts = np.asarray(counts)
    thresholds = np.asarray(thresholds, dtype=np.int64)
    ids, scores, offsets = [], [], [0]
    for q in range(counts.shape[0]):
        f = np.flatnonzero(counts[q].astype(np.int64) >= thresholds[q])
        ids.append(f)
        scores.append(counts[q, f])
        offsets.append(offsets[-1] + f.size)
    cat = (lambda parts: np.concatenate(parts).astype(np.int32)) if ids else (lambda parts: np.zeros(0, dtype=np.int32))
    return np.array(offsets, dtype=np.int64), cat(ids), cat(scores)


def fixture_queries(case: dict, extra: bool = False):
    """the queries both test files put to a case of golden_bank_match.json, as (probe indices int64[n], offsets int64[Q + 1]): ``sent[f]`` for
    every filter f (one of them empty), the whole probe list (pool + absent), the absent keys alone; ``extra``: a query holding one probe twice
    among others, and a single-key query"""
    n_pool, n = len(case["pool"]), len(case["pool"]) + len(case["absent"])
    qs = [list(s) for s in case["sent"]] + [list(range(n)), list(range(n_pool, n))]
    if extra:
        qs += [[3, 7, 3, n_pool + 1], [0]]
    offsets = np.zeros(len(qs) + 1, dtype=np.int64)
    np.cumsum([len(q) for q in qs], out=offsets[1:])
    return np.array([i for q in qs for i in q], dtype=np.int64), offsets


def thresholds(lengths, threshold) -> np.ndarray:
    """uint32[Q]: an int for every query, one int per query, or a fraction in (0, 1] of each query's length, at least 1 (exact: Python's
    float product and math.ceil, one query at a time)"""
    lengths = [int(x) for x in lengths]
    if isinstance(threshold, float):
        return np.array([max(1, math.ceil(threshold * n)) for n in lengths], dtype=np.uint32)
    if isinstance(threshold, int):
        return np.full(len(lengths), threshold, dtype=np.uint32)
    t = [int(x) for x in threshold]
    assert len(t) == len(lengths)
    return np.array(t, dtype=np.uint32)
