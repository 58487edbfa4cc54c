"""The ordered CountingBloomFilter batch (psk_cbf_add_running / psk_cbf_update_running, DESIGN.md "Ordered CountingBloomFilter batches")
as a model: the (a, p) maps and their composition law as code, the literal loop, the optimistic scan of one chunk with its verification
rule, and the chunked executor on top of the two.

An op acts on ONE counter as a map on its value x, MAX = 2^32 - 1 sticky:
    add w                 x -> min(x + w, MAX)                        = (w, w)
    FULL remove of w      x -> MAX if x == MAX else x - w             = (-w, -inf)
    (a, p)(x) = MAX if x == MAX or x + p >= MAX else x + a            a: the signed sum, p: the largest prefix sum that ends in an add
    (a1, p1) then (a2, p2) = (a1 + a2, max(p1, a1 + p2))
The rail is a parameter everywhere: the brute-force tests run on toy rails, the filter on uint32."""

import numpy as np

MAX = 2**32 - 1
NONE = float("-inf")


# ------------------------------------------------------------------ the law (Python integers)
def add_map(w):
    return (w, w)


def remove_map(w):
    return (-w, NONE)


IDENTITY = (0, NONE)


def combine(f, g):
    """f, then g"""
    a1, p1 = f
    a2, p2 = g
    return (a1 + a2, max(p1, a1 + p2))


def apply(f, x, rail=MAX):
    a, p = f
    return rail if x == rail or x + p >= rail else x + a


def op_map(w, c=1):
    """the map of an op of signed weight w that probes the counter c times (c > 1: for the ops the verification lets through)"""
    return add_map(w * c) if w >= 0 else remove_map(-w * c)


# ------------------------------------------------------------------ the literal loop (countingbloom.py:135-208 as k_cbf_ordered runs it)
def new_tally():
    return {"added": 0, "removed": 0, "saturated": 0, "abs": 0}


def serial(table, bins, weights, tally=None):
    """ops one after the other on `table` (a list / array of Python-int-like counters, changed in place): w >= 0 adds w, w < 0 removes
    -w.  bins: n rows of k counter indices.  Where the reference's array('I') store would raise OverflowError the counter wraps, as in
    the kernel.  -> the n return values"""
    tally = new_tally() if tally is None else tally
    out = []
    for idx, w in zip(bins, weights):
        idx, w = [int(i) for i in idx], int(w)
        tally["abs"] += abs(w)
        if w >= 0:
            vals = [int(table[i]) + w for i in idx]  # :146 the pre-read
            for s, i in enumerate(idx):
                if vals[s] > MAX:
                    table[i] = MAX
                    vals[s] = MAX
                    tally["saturated"] += 1
                else:
                    table[i] = (int(table[i]) + w) & MAX
            tally["added"] += w
            out.append(min(vals))
        else:
            w = -w
            mn = min(int(table[i]) for i in idx)
            if mn == MAX:
                out.append(MAX)
            elif mn == 0:
                out.append(0)
            else:
                tr = min(mn, w)
                for i in idx:
                    if int(table[i]) < MAX:
                        table[i] = (int(table[i]) - tr) & MAX
                tally["removed"] += tr
                out.append(mn - tr)
    return out


# ------------------------------------------------------------------ one chunk, optimistically: the scan of maps, op by op (Python)
def scan_chunk_maps(table, bins, weights):
    """the passes of psk_cbf_running.hpp in the small: probes sorted by (counter, arrival), an exclusive scan of maps per counter, the
    per-op pass with the verification rule.  -> (results, {counter: final value}, flagged, tally).  The table is NOT changed."""
    n = len(bins)
    k = len(bins[0]) if n else 0
    probes = sorted((int(bins[i][s]), i * k + s) for i in range(n) for s in range(k))  # stable: arrival order inside a counter
    before = [0] * (n * k)
    final = {}
    flagged = False
    j = 0
    while j < len(probes):
        c, f = probes[j][0], IDENTITY
        t0 = int(table[c])
        while j < len(probes) and probes[j][0] == c:
            op = probes[j][1] // k
            grp = j
            while grp < len(probes) and probes[grp][0] == c and probes[grp][1] // k == op:
                grp += 1
            cnt, w = grp - j, int(weights[op])
            b = apply(f, t0)
            for t in range(j, grp):
                before[probes[t][1]] = b  # the value in front of the OP, for every probe of the group
            if cnt > 1:
                if w < 0:
                    flagged |= b != MAX and b < cnt * -w
                else:
                    flagged |= b + w <= MAX < b + cnt * w
            f = combine(f, op_map(w, cnt))
            j = grp
        final[c] = apply(f, t0)
    out, tally = [], new_tally()
    for i in range(n):
        w, b = int(weights[i]), before[i * k:(i + 1) * k]
        tally["abs"] += abs(w)
        if w >= 0:
            out.append(min(min(x + w, MAX) for x in b))
            tally["saturated"] += sum(x + w > MAX for x in b)
            tally["added"] += w
        else:
            mn = min(b)
            if mn == MAX:
                out.append(MAX)
            else:
                flagged |= mn < -w  # absent (mn == 0 < w) or partial
                out.append((mn + w) & MAX)
                tally["removed"] += -w
    return out, final, flagged, tally


# ------------------------------------------------------------------ one chunk, optimistically, in numpy (the same values; large streams)
def scan_chunk(table, bins, weights):
    """scan_chunk_maps with every counter's ops stepped in numpy, position j of every counter's list in one step.  bins: int64[n][k],
    weights: int64[n], table: uint32 / int64 array.  -> (results int64[n], counters int64[], their final values int64[], flagged, tally)"""
    bins = np.asarray(bins, dtype=np.int64)
    n, k = bins.shape
    w = np.asarray(weights, dtype=np.int64)
    flat = bins.ravel()
    order = np.argsort(flat, kind="stable")
    sb, sop = flat[order], order // k
    first = np.ones(n * k, dtype=bool)  # first probe of its (counter, op) group
    first[1:] = (sb[1:] != sb[:-1]) | (sop[1:] != sop[:-1])
    g = np.nonzero(first)[0]
    gcnt = np.diff(np.append(g, n * k))
    gb, gw = sb[g], w[sop[g]]
    head = np.ones(g.size, dtype=bool)
    head[1:] = gb[1:] != gb[:-1]
    starts = np.nonzero(head)[0]
    lens = np.diff(np.append(starts, g.size))
    by_len = np.argsort(-lens, kind="stable")
    starts, lens = starts[by_len], lens[by_len]
    tab = np.asarray(table).astype(np.int64)
    val = tab[gb[starts]]
    gbefore = np.empty(g.size, dtype=np.int64)
    flagged = False
    alive = np.searchsorted(-lens, -np.arange(int(lens[0]) if lens.size else 0), side="left")
    for j in range(int(lens[0]) if lens.size else 0):
        m = int(alive[j])
        at = starts[:m] + j
        v, ww, cc = val[:m], gw[at], gcnt[at]
        gbefore[at] = v
        dup = cc > 1
        if dup.any():
            flagged |= bool((dup & (ww < 0) & (v != MAX) & (v < cc * -ww)).any())
            flagged |= bool((dup & (ww >= 0) & (v + ww <= MAX) & (v + cc * ww > MAX)).any())
        nv = np.where(ww >= 0, np.minimum(v + cc * ww, MAX), np.where(v == MAX, MAX, v + cc * ww))
        val[:m] = nv
    before = np.empty(n * k, dtype=np.int64)
    before[order] = np.repeat(gbefore, gcnt)
    before = before.reshape(n, k)
    isadd = w >= 0
    mn = before.min(axis=1)
    out = np.where(isadd, np.minimum(mn + w, MAX), np.where(mn == MAX, MAX, (mn + w) & MAX))
    live = ~isadd & (mn != MAX)
    flagged |= bool((live & (mn < -w)).any())
    tally = {"added": int(w[isadd].sum()), "removed": int(-w[live].sum()), "abs": int(np.abs(w).sum()),
             "saturated": int(((before + w[:, None] > MAX) & isadd[:, None]).sum())}
    return out, gb[starts], val, flagged, tally


# ------------------------------------------------------------------ the batch: chunk after chunk, a flagged chunk replayed by the loop
def execute(table, bins, weights, cap, vectorised=False):
    """-> (results, tally, fast chunks, replayed chunks); `table` (numpy, uint32 or int64) is changed in place"""
    n = len(bins)
    out, tally, fast, replayed = [], new_tally(), 0, 0
    for base in range(0, n, cap):
        b, w = bins[base:base + cap], weights[base:base + cap]
        if vectorised:
            res, cs, vals, flagged, t = scan_chunk(table, b, w)
            final = None
        else:
            res, final, flagged, t = scan_chunk_maps(table, b, w)
        if flagged:
            replayed += 1
            res = serial(table, b, w, tally)
        else:
            fast += 1
            if final is None:
                table[cs] = vals
            else:
                for c, v in final.items():
                    table[c] = v
            for key in tally:
                tally[key] += t[key]
        out.extend(int(x) for x in res)
    return out, tally, fast, replayed


def sm(x):
    """splitmix64 of a Python integer"""
    z = (x + 0x9E3779B97F4A7C15) & (2**64 - 1)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
    return z ^ (z >> 31)
