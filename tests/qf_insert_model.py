"""Insertion in place into a quotient filter's table: a plain-Python step model of the three launches behind ``psk_qf_add_alt``
(pyprobables_amd/csrc/psk_quotient.hip; DESIGN.md "Quotient filter: insertion in place").  Test infrastructure, no GPU.

The model works on the four arrays slot by slot, as the kernels do, and never computes the canonical table of the union:
tests/test_quotient_insert_model.py holds it against ``qf_model.canonical``.

    starts   per batch hash: b = the start of the cluster that holds the hash's quotient slot (the slot itself when it is empty).
             Hashes with equal b are a group; its leader is the hash that comes first in ring order from b.
    spans    per leader: the walk from b as if no carry arrived there.  The walk merges the old elements (slot order) with the batch
             hashes (ring order from the leader) by (quotient, remainder) and gives every item the next free slot; it stops in front of
             the first item whose own quotient's slot is not behind the write frontier.  A batch hash the walk takes in that belongs to
             another group marks that group as covered.  A walk whose frontier comes round to b is a table that does not fit.
    write    per leader that nobody covered (the head of a region): the same walk again -- exact now -- then the region is written from
             its end backward: from the first new hash's slot on it is contiguous, so the items in descending order take descending slots.
"""

from __future__ import annotations

import numpy as np


class Table:
    """the four arrays of one table (numpy, one entry per slot) and its quotient"""

    def __init__(self, filt, occ, cont, sh, q):
        self.filt, self.occ, self.cont, self.sh, self.q = filt, occ, cont, sh, q
        self.size, self.r = 1 << q, 32 - q

    def copy(self):
        return Table(self.filt.copy(), self.occ.copy(), self.cont.copy(), self.sh.copy(), self.q)

    def arrays(self):
        return self.filt, self.occ, self.cont, self.sh

    def in_use(self, s):
        return bool(self.occ[s] | self.sh[s])


def group_start(t: Table, quot: int) -> int:
    if not t.in_use(quot):
        return quot
    s = quot
    for _ in range(t.size):
        if not t.sh[s]:
            break
        s = (s - 1) % t.size
    return s


def is_leader(t: Table, hs, bs, i) -> bool:
    n = len(hs)
    if n == 1:
        return True
    p = (i - 1) % n
    if bs[p] != bs[i]:
        return True
    return (hs[p] - (bs[p] << t.r)) % 2**32 > (hs[i] - (bs[i] << t.r)) % 2**32


def _next_occ(t: Table, oc):
    for _ in range(t.size):
        oc = (oc + 1) % t.size
        if t.occ[oc]:
            break
    return oc


def _prev_occ(t: Table, oc):
    for _ in range(t.size):
        oc = (oc - 1) % t.size
        if t.occ[oc]:
            break
    return oc


class Walk:
    __slots__ = ("b", "end", "rend", "p0", "used", "added", "oc_last", "pq", "over")


def walk(t: Table, hs, bs, i0, covered=None) -> Walk:
    """the read-only forward walk of the group led by batch hash i0"""
    size, r, n = t.size, t.r, len(hs)
    rmask = (1 << r) - 1
    w = Walk()
    b = w.b = bs[i0]
    ro = nxt = used = added = 0  # offsets from b: the old slot being read, the write frontier; batch hashes taken in, of them new
    oc, oc_at = b, -1  # the quotient of the old element at offset `oc_at`
    w.p0, w.pq, w.oc_last, w.rend, w.over = 0, None, b, 0, False
    for _ in range(2 * size + n + 4):
        if nxt >= size:
            w.over = True
            break
        s = (b + ro) % size
        have_old = t.in_use(s)
        if not have_old and ro < nxt:  # an empty slot under the frontier takes one unit of carry
            ro += 1
            continue
        if have_old and oc_at != ro:
            if not t.cont[s]:
                oc = s if not t.sh[s] else _next_occ(t, oc)
            oc_at = ro
        have_new = used < n
        own = False
        if have_new:
            j = (i0 + used) % n
            nq, nr = ((hs[j] >> r) - b) % size, hs[j] & rmask
            own = bs[j] == b
        if not have_old and not have_new:
            break
        qo = (oc - b) % size
        take_old, same = have_old, False
        if have_old and have_new:
            ko, kn = (qo, int(t.filt[s])), (nq, nr)
            take_old, same = ko < kn, ko == kn
        cq = qo if take_old or same else nq
        if cq >= nxt and not own:
            break
        if have_new and not take_old and covered is not None and not own:
            covered.add(bs[j])
        if same:  # the hash is in the table already
            used += 1
            continue
        if take_old:
            if not added:
                w.pq = qo
            w.oc_last = oc
            ro += 1
            nxt += 1
            w.rend = ro
        else:
            if not added:
                w.p0 = nxt
            added += 1
            used += 1
            nxt += 1
    else:
        w.over = True
    w.end, w.used, w.added = nxt, used, added
    return w


def write_region(t: Table, hs, i0, w: Walk) -> None:
    """the backward write of one region whose forward walk gave `w`"""
    size, r, n, b = t.size, t.r, len(hs), w.b
    rmask = (1 << r) - 1
    k, ro, oc, step = w.used, w.rend, w.oc_last, False
    prev = None  # the item of the slot above: (offset, quotient offset, remainder)

    def emit(item, c):
        p, qoff, rem = item
        s = (b + p) % size
        t.filt[s], t.cont[s], t.sh[s] = rem, int(c), int(p != qoff)

    for wp in range(w.end - 1, w.p0 - 1, -1):
        while True:
            while ro > 0 and not t.in_use((b + ro - 1) % size):
                ro -= 1
            have_old, have_new = ro > 0, k > 0
            if have_old:
                s = (b + ro - 1) % size
                if step:
                    oc, step = _prev_occ(t, oc), False
                ko = ((oc - b) % size, int(t.filt[s]))
            if have_new:
                h = hs[(i0 + k - 1) % n]
                kn = (((h >> r) - b) % size, h & rmask)
            if have_old and have_new and ko == kn:
                k -= 1
                continue
            break
        assert have_old or have_new
        if have_old and (not have_new or ko > kn):
            item = (wp, *ko)
            step = not t.cont[s]  # a run start: the element below belongs to the occupied quotient before this one
            ro -= 1
        else:
            item = (wp, *kn)
            k -= 1
        if prev is not None:
            emit(prev, prev[1] == item[1])
        prev = item
    emit(prev, w.pq is not None and w.pq == prev[1])
    for x in range(w.used):
        t.occ[hs[(i0 + x) % n] >> r] = 1


def add_in_place(t: Table, batch, order=None):
    """the table `t` after ``add_alt`` of every hash of `batch` (sorted, distinct) -> (added, status); status != 0: nothing was written.
    `order` permutes the head lanes of the write launch (regions are independent of each other)."""
    hs = [int(h) for h in batch]
    n = len(hs)
    if n == 0:
        return 0, 0
    bs = [group_start(t, h >> t.r) for h in hs]
    leaders = [i for i in range(n) if is_leader(t, hs, bs, i)]
    covered, status = set(), 0
    for i in leaders:
        if walk(t, hs, bs, i, covered).over:
            status = 1
    if status:
        return 0, status
    heads = [i for i in leaders if bs[i] not in covered]
    if order is not None:
        heads = [heads[x % len(heads)] for x in order(len(heads))] if heads else heads
    snapshot = t.copy()  # every head reads the table as the other heads find it: a head's walk looks at its own region and the stop slot only
    added = 0
    for i in heads:
        w = walk(snapshot, hs, bs, i)
        assert not w.over
        if w.added:
            write_region_from(snapshot, t, hs, i, w)
            added += w.added
    return added, 0


def write_region_from(src: Table, dst: Table, hs, i0, w: Walk) -> None:
    """one head lane: reads its region from the table as it was (`src`; in place that is the same memory, no other lane writes the region) and
    writes it into `dst`"""
    region = Table(dst.filt, dst.occ, dst.cont, dst.sh, dst.q)
    # the lane's own reads and writes go to the same memory: replay on `dst`, whose region is still the old one
    size = src.size
    for off in range(w.end):
        s = (w.b + off) % size
        assert (dst.filt[s], dst.cont[s], dst.sh[s]) == (src.filt[s], src.cont[s], src.sh[s]), "two regions overlap"
    write_region(region, hs, i0, w)


def table_of(arrays, q) -> Table:
    filt, occ, cont, sh = (np.array(a) for a in arrays)
    return Table(filt, occ, cont, sh, q)
