"""Chosen tables for the in-place removal (``psk_qf_remove_alt``): one case table, ``name -> (q, held, gone)``, that the host model
(tests/test_quotient_remove_model.py) and the GPU (tests/test_gpu_quotient_remove_edges.py) both run, and what a test needs to say why a case
is in it: where ``qf_model.canonical`` puts every hash, and which cluster it belongs to.  numpy only, no GPU.

    q = 8    cluster seams, word seams, the table's end, the occupied scan over a zero word, three-word clusters, the ring with one empty slot
    q = 10   words full of dirty clusters: only lanes that run together can go wrong here
    widths   q = 23 (r = 9, the first uint16 width), q = 16 (r = 16, the last), q = 15 (r = 17, the first uint32 width)
"""

from __future__ import annotations

import random

import numpy as np

import qf_model as M


def m(q: int, quot: int, rem: int) -> int:
    return (quot << (32 - q)) | rem


def layout(held, q: int):
    """-> (hs, slot, start): the sorted distinct hashes, the slot ``canonical`` stores each in and the start of its cluster (a cluster: a slot
    in use with shifted = 0 and the shifted slots behind it, round the table's end)"""
    size, r = 1 << q, 32 - q
    hs = np.unique(np.asarray(list(held) if not isinstance(held, np.ndarray) else held, dtype=np.uint64)).astype(np.int64)
    slot = M.positions(hs, q) % size
    head = slot == (hs >> r)
    if not hs.size:
        return hs, slot, slot
    assert head.any(), "a table without a cluster start is full and then some"
    idx = np.flatnonzero(head)
    k = np.cumsum(head) - 1  # the head in front of each element; -1: the cluster that came over the table's end
    return hs, slot, slot[idx[k]]


def facts(q: int, held, gone) -> dict:
    """what the property checks read: per dirty cluster its start, its slots in ring order and which of them die"""
    size = 1 << q
    hs, slot, start = layout(held, q)
    hit = np.isin(hs, np.asarray(sorted(set(gone)), dtype=np.int64))
    clusters = {}
    for b in np.unique(start[hit]).tolist():
        mine = start == b
        off = (slot[mine] - b) % size
        order = np.argsort(off)
        clusters[b] = {"length": int(mine.sum()), "slots": slot[mine][order].tolist(), "dead": sorted(((slot[mine & hit] - b) % size).tolist()),
                       "words": sorted({s >> 5 for s in slot[mine].tolist()}), "wraps": bool(b + int(mine.sum()) > size)}
    return {"hits": int(hit.sum()), "empty": size - int(hs.size), "clusters": clusters, "all_starts": sorted(set(start.tolist())),
            "slot": dict(zip(hs.tolist(), slot.tolist()))}


def most_dirty_starts_in_one_word(f: dict) -> int:
    words = [b >> 5 for b in f["clusters"]]
    return max((words.count(w) for w in set(words)), default=0)


Q8, Q10 = 8, 10


def m8(quot, *rems):
    return [m(Q8, quot, r) for r in rems]


THREE_WORDS = [m(Q8, 28 + i // 2, 1 + i % 2) for i in range(76)]  # one cluster, slots 28 .. 103
LONG_RUN = m8(10, *range(1, 81))  # one run, slots 10 .. 89
RMAX8 = (1 << 24) - 1

CASES = {
    "dead_head_run_survives": (Q8, m8(10, 1, 2) + m8(11, 1), m8(10, 1)),
    "head_run_dies_next_run_falls_home": (Q8, m8(10, 1, 2) + m8(11, 1, 2), m8(10, 1, 2)),
    "gap_splits_cluster_in_three": (Q8, m8(10, 1, 2) + m8(11, 1) + m8(13, 1, 2) + m8(15, 1), m8(10, 2) + m8(13, 1)),
    "whole_cluster": (Q8, m8(10, 1, 2) + m8(11, 1) + m8(20, 1), m8(10, 1, 2) + m8(11, 1)),
    "seam_31_32_dead_each_side": (Q8, m8(29, 1, 2) + m8(30, 1, 2) + m8(31, 1, 2) + m8(32, 1), m8(29, 2) + m8(31, 2)),
    "three_words_shift_by_one": (Q8, THREE_WORDS, m8(28, 1)),
    "three_words_last_only": (Q8, THREE_WORDS, m8(65, 2)),
    "two_clusters_one_word": (Q8, m8(3, 1, 2) + m8(4, 1) + m8(20, 1, 2) + m8(21, 1), m8(3, 2) + m8(20, 1)),
    "three_clusters_middle_untouched": (Q8, m8(3, 1, 2) + m8(10, 1, 2) + m8(20, 1, 2), m8(3, 1) + m8(20, 2)),
    "over_the_end_dead_each_side": (Q8, m8(254, 1, 2) + m8(255, 1, 2) + m8(0, 1) + m8(1, 1), m8(254, 2) + m8(0, 1)),
    "over_the_end_head_dies": (Q8, m8(254, 1) + m8(255, 1, 2) + m8(0, 1, 2), m8(254, 1)),
    "over_the_end_shifted_head_dies": (Q8, m8(254, 1, 2) + m8(255, 1, 2) + m8(0, 1), m8(254, 1)),
    "over_the_end_occupied_scan_wraps": (Q8, m8(254, 1, 2, 3) + m8(0, 1, 2), m8(254, 2)),
    "over_the_end_only_wrapped_part": (Q8, m8(254, 1, 2) + m8(255, 1, 2) + m8(0, 1, 2), m8(0, 1, 2)),
    "next_occupied_two_words_on": (Q8, LONG_RUN + m8(85, 1, 2), m8(10, 80) + m8(85, 1)),
    "long_run_first_middle_last": (Q8, LONG_RUN, m8(10, 1, 40, 80)),
    "absent_only": (Q8, m8(10, 2, 4) + m8(11, 1) + m8(13, 1), m8(10, 1, 3, 9) + m8(12, 1) + m8(14, 1) + m8(200, 0) + [0, 0xFFFFFFFF]),
    "remainder_zero_and_max": (Q8, m8(10, 0, RMAX8) + m8(11, 0) + m8(12, RMAX8), m8(10, 0) + m8(11, 0)),
    "one_empty_slot_ring": (Q8, [m(Q8, i, 1) for i in range(256) if i != 100], m8(101, 1) + m8(99, 1) + m8(255, 1) + m8(0, 1)),
    "one_empty_slot_shifted_ring": (Q8, m8(5, *range(1, 256)), m8(5, 1, 128, 255)),
}

# ---- q = 10: every metadata word shared by the lanes of many dirty clusters
DOMINO = [m(Q10, 3 * c, r) for c in range(341) for r in (1, 2)]  # 341 clusters of two slots, one empty slot between neighbours; 3 against 32: a cluster on every seam
QUADS = [m(Q10, 5 * c + d, r) for c in range(204) for d in (0, 1) for r in (1, 2)]  # 204 clusters of four slots (two runs of two), period 5
SHARED_WORD_CASES = ("domino_heads", "domino_seconds", "domino_alternate", "quads_middle_two")
CASES.update({
    "domino_heads": (Q10, DOMINO, [m(Q10, 3 * c, 1) for c in range(341)]),
    "domino_seconds": (Q10, DOMINO, [m(Q10, 3 * c, 2) for c in range(341)]),
    "domino_alternate": (Q10, DOMINO, [m(Q10, 3 * c, 1 + c % 2) for c in range(341)]),
    "quads_middle_two": (Q10, QUADS, [h for c in range(204) for h in (m(Q10, 5 * c, 2), m(Q10, 5 * c + 1, 1))]),
})


# ---- the remainder widths: a few hundred hashes round the table's end, one run of 40 over it, remainders 0 and 2^r - 1 on both sides of a dead slot
def width_case(q: int):
    size, r = 1 << q, 32 - q
    rmax = (1 << r) - 1
    rng = random.Random(q)
    held = {m(q, (size - 300 + rng.randrange(400)) % size, rng.choice((0, rmax, rng.randrange(1 << r), rng.randrange(16)))) for _ in range(300)}
    run = [m(q, size - 20, x) for x in [0, *range(100, 138), rmax]]  # slots size - 20 .. size + 19 at the least
    triples = [m(q, quot, x) for quot in (size - 1, 0, size - 150, 60) for x in (0, 1, rmax)]  # 0 | dead | 2^r - 1 in one run
    held |= set(run) | set(triples)
    pool = sorted(held - set(run) - set(triples))
    gone = rng.sample(pool, len(pool) // 3) + run[1:38:3] + [run[0]] + triples[1::3]
    gone += [h ^ 1 for h in rng.sample(pool, 20) if h ^ 1 not in held]  # and some that are not there
    return q, sorted(held), gone


WIDTH_CASES = {"width_q23_r9": 23, "width_q16_r16": 16, "width_q15_r17": 15}
CASES.update({name: width_case(q) for name, q in WIDTH_CASES.items()})

NAMES = list(CASES)
