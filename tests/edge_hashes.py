"""Chosen 64-bit hashes for the pre-hashed batch entries (``*_alt_many``), and exact numpy references of what they must do.

FNV spreads real keys evenly, so parity tests on real keys sample the middle of the index arithmetic.  The helpers here build hashes that
land on a table's boundary cells through every route of ``h % m`` (a small value, the top of the 64-bit range, a random multiple, a
value whose truncated quotient estimate is one short), and restate the three sketches' rules on plain integer arrays:

* Bloom            bit ``h % m`` of a little-endian bit array, byte ``c // 8`` bit ``c % 8``;
* CountingBloom    counter ``h % m`` per hash (a repeated index counts twice), saturating at 2^32 - 1;
* CountMinSketch   bin ``h_i % width + i * width`` per row, saturating at 2^31 - 1; min / mean / mean-min queries.

The last section does the same for the cuckoo filter's triples: fingerprints at which the decimal digits of ``str(fp)`` or the 32-bit word
turn over, capacities up to 2^31 - 1 at which the second index needs (or never needs) the correction of its quotient estimate, and the rule
itself in Python integers.

Only numpy and Python integers: nothing here imports the engine, the oracle or the cuckoo model, so it can check all three.
"""

from __future__ import annotations

import numpy as np

U64 = 1 << 64
U32_MAX = 2**32 - 1
I32_MAX = 2**31 - 1
I64_MAX, I64_MIN = 2**63 - 1, -(2**63)
HOWS = ("low", "high", "mid", "short")

# the smallest geometries at which each engine path still exists (tests/test_gpu_edge_hashes.py); (est_elements, false_positive_rate)
BLOOM_DIRECT, BLOOM_2P28, BLOOM_NP2, BLOOM_2P31 = (1000, 0.01), (28005615, 0.01), (10_000_000, 0.01), (223_000_000, 0.01)
CBF_DIRECT, CBF_SLICES32, CBF_NIBBLE, CBF_WINDOW = (1000, 0.01), (2_000_000, 0.01), (1_000_000, 0.01), (3_600_000, 0.01)
CMS_SHAPES = ((7, 3), (100_003, 4), (2**20, 5), (1_000_003, 5))  # (width, depth)


def bloom_bits(est: int, fpr: float) -> int:
    """number_bits of the reference's sizing rule (fpr rounded through a C float, ln(2)^2 as the literal the reference uses)"""
    import math
    import struct

    p32 = struct.unpack("f", struct.pack("f", float(fpr)))[0]
    return math.ceil((-est * math.log(p32)) / 0.4804530139182)


def is_pow2(m: int) -> bool:
    return m & (m - 1) == 0


# ------------------------------------------------------------------ cells
def edge_cells(m: int) -> np.ndarray:
    """sorted unique cells of a table of ``m`` cells at which a slice of 2^s cells (s = 10 .. 20) begins or ends: whatever the engine's
    slice shift is, its first / last cell-in-slice, its last (partial) slice and the table's own ends are among them"""
    m = int(m)
    cells = {0, 1, m - 2, m - 1}
    for s in range(10, 21):
        nb = (m - 1) >> s  # boundaries j << s, 1 <= j <= nb, lie below m
        js = range(1, nb + 1) if nb <= 128 else [*range(1, 65), *range(nb - 63, nb + 1)]
        for j in js:
            cells.update((j << s, (j << s) - 1))
        cells.update((nb << s, m - 1))  # the final (partial) block: its first and last cell
    return np.array(sorted(c for c in cells if 0 <= c < m), dtype=np.int64)


def _short_q_range(m: int, r: int):
    """the quotients q for which h = q * m + r has floor(h * floor(2^64 / m) / 2^64) == q - 1, as (q_lo, q_hi) or None.
    With 2^64 = magic * m + e:  h * magic = q * 2^64 + (r * magic - q * e), and r * magic < 2^64, so the estimate is one short exactly when
    q * e > r * magic."""
    magic, e = divmod(U64, m)
    q_hi = (U64 - 1 - r) // m
    q_lo = r * magic // e + 1
    return (q_lo, q_hi) if q_lo <= q_hi else None


def short_cells(m: int) -> list[int]:
    """the smallest and the largest remainder ``h % m`` that a hash with a one-short quotient estimate can have (non-power-of-two m)"""
    m = int(m)
    assert m > 1 and not is_pow2(m), "a power-of-two modulus is a mask: no quotient estimate"
    lo = next(r for r in range(m) if _short_q_range(m, r))
    hi = next(r for r in range(min(m - 1, U64 % m), -1, -1) if _short_q_range(m, r))  # (q <= magic: nothing above e = 2^64 mod m qualifies)
    assert hi == m - 1 or _short_q_range(m, hi + 1) is None
    return [lo, hi]


def hashes_for(cells, m: int, how: str, seed: int | None = 0) -> np.ndarray:
    """uint64 hashes ``h`` with ``h % m == cell`` for every cell.

    ``low``: h = cell.  ``high``: the largest h < 2^64 of the residue class (a power-of-two m: high word all ones).  ``mid``: a seeded
    random multiple of m on top of the cell.  ``short`` (non-power-of-two m, cells within ``short_cells(m)``): h whose truncated quotient
    ``(h * (2**64 // m)) >> 64`` is ``h // m - 1`` -- the largest such h per cell (``seed=None``) or a seeded random one."""
    m = int(m)
    cells = [int(c) for c in np.asarray(cells).reshape(-1)]
    assert how in HOWS and all(0 <= c < m for c in cells)
    rng = np.random.default_rng(seed)
    out = []
    for c in cells:
        q_top = (U64 - 1 - c) // m
        if how == "low":
            h = c
        elif how == "high":
            h = c + q_top * m
        elif how == "mid":
            h = c + m * int(rng.integers(1, q_top + 1, dtype=np.uint64))
        else:
            assert not is_pow2(m), "short: non-power-of-two m only"
            qr = _short_q_range(m, c)
            assert qr is not None, f"no hash of remainder {c} mod {m} has a short quotient estimate"
            q = qr[1] if seed is None else int(rng.integers(qr[0], qr[1] + 1, dtype=np.uint64))
            h = c + q * m
        out.append(h)
    # postcondition, in Python integers
    for c, h in zip(cells, out):
        assert 0 <= h < U64 and h % m == c
        if how == "high":
            assert h + m >= U64 and (not is_pow2(m) or m > 1 << 32 or h >> 32 == 0xFFFFFFFF)
        if how == "short":
            assert (h * (U64 // m)) >> 64 == h // m - 1
    return np.array(out, dtype=np.uint64)


def any_how(cells, m: int, seed: int = 0) -> np.ndarray:
    """one hash per cell, each through a seeded random choice of ``low`` / ``high`` / ``mid``"""
    cells = np.asarray(cells).reshape(-1)
    pick = np.random.default_rng(seed).integers(0, 3, size=cells.size)
    per_how = [hashes_for(cells, m, how, seed) for how in HOWS[:3]]
    return np.choose(pick, per_how).astype(np.uint64) if cells.size else np.zeros(0, dtype=np.uint64)


def lift(cells, m: int, seed: int = 0) -> np.ndarray:
    """``mid`` for large batches: cell + a seeded random multiple of m, vectorised (same shape as ``cells``)"""
    m = int(m)
    c = np.asarray(cells, dtype=np.uint64)
    assert c.size == 0 or int(c.max()) < m
    q = np.random.default_rng(seed).integers(0, (U64 - m) // m, size=c.shape, dtype=np.uint64)  # c + q * m <= 2^64 - 1
    h = c + q * np.uint64(m)
    assert np.array_equal(h % np.uint64(m), c)
    return h


# ------------------------------------------------------------------ indices
def indices(hashes, m: int, k: int) -> np.ndarray:
    """int64[n][k]: ``h % m`` of the first k columns (exact: numpy's uint64 remainder)"""
    h = np.asarray(hashes, dtype=np.uint64)
    assert h.ndim == 2 and h.shape[1] >= k
    return (h[:, :k] % np.uint64(m)).astype(np.int64)


def cms_indices(hashes, width: int, depth: int) -> np.ndarray:
    """int64[n][depth]: ``h_i % width + i * width``"""
    return indices(hashes, width, depth) + np.arange(depth, dtype=np.int64) * int(width)


# ------------------------------------------------------------------ Bloom
def bloom_table(m: int, idx, table=None) -> np.ndarray:
    """uint8[ceil(m / 8)] with bit ``c % 8`` of byte ``c // 8`` set for every index (ORed into ``table`` when given)"""
    t = np.zeros((int(m) + 7) // 8, dtype=np.uint8) if table is None else table
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    np.bitwise_or.at(t, idx >> 3, (1 << (idx & 7)).astype(np.uint8))
    return t


def bloom_check(table, idx) -> np.ndarray:
    """bool[n]: every one of the key's bits is set"""
    idx = np.asarray(idx, dtype=np.int64)
    return ((table[idx >> 3] >> (idx & 7).astype(np.uint8)) & 1).all(axis=1)


def bloom_member(set_cells, idx) -> np.ndarray:
    """``bloom_check`` without the table: every index of a key is among the cells that were set (tables too large to keep on the host)"""
    return np.isin(np.asarray(idx, dtype=np.int64), np.asarray(set_cells, dtype=np.int64)).all(axis=1)


# ------------------------------------------------------------------ counters
class Counters:
    """exact counters of a CountingBloom (``rail`` 2^32 - 1) or CountMinSketch (2^31 - 1) table, kept unclipped in int64.

    Adds: the reference stores min(counter + w, rail) per index, and a counter on the rail stays there under adds, so clipping the exact sum
    once at the end is the reference's table for any add-only stream.  Removes are accepted only where plain subtraction IS the reference's
    result: no touched counter on the rail before, none below zero after (the reference raises or clamps there: out of scope)."""

    def __init__(self, cells: int, rail: int):
        self.exact = np.zeros(int(cells), dtype=np.int64)
        self.rail = int(rail)
        self.els = 0

    def add(self, idx, w=1):
        idx = np.asarray(idx, dtype=np.int64)
        w = np.broadcast_to(np.asarray(w, dtype=np.int64).reshape(-1, 1), idx.shape)
        assert (w >= 0).all()
        np.add.at(self.exact, idx, w)  # a repeated index counts every time
        self.els += int(w[:, 0].sum())

    def remove(self, idx, w=1):
        idx = np.asarray(idx, dtype=np.int64)
        w = np.broadcast_to(np.asarray(w, dtype=np.int64).reshape(-1, 1), idx.shape)
        assert (self.exact[idx] < self.rail).all(), "remove next to a saturated counter: out of scope"
        np.subtract.at(self.exact, idx, w)
        assert (self.exact >= 0).all(), "remove below zero: out of scope"
        self.els -= int(w[:, 0].sum())

    def table(self, dtype) -> np.ndarray:
        return np.minimum(self.exact, self.rail).astype(dtype)

    def values(self, idx) -> np.ndarray:
        """int64[n][cols]: the stored (clipped) counters"""
        return np.minimum(self.exact[np.asarray(idx, dtype=np.int64)], self.rail)


def cbf_counters(m: int) -> Counters:
    return Counters(m, U32_MAX)


def cms_counters(width: int, depth: int) -> Counters:
    return Counters(int(width) * int(depth), I32_MAX)


def cms_query(vals, query: str, width: int, els_added: int) -> np.ndarray:
    """int64[n]: the min / mean / mean-min estimate from each key's ``depth`` bins (Python's floor division throughout)"""
    v = np.sort(np.asarray(vals, dtype=np.int64), axis=1)
    depth = v.shape[1]
    if query == "min":
        return v[:, 0].copy()
    if query == "mean":
        return v.sum(axis=1) // depth
    assert query == "mean-min"
    calc = np.sort(v - (int(els_added) - v) // (int(width) - 1), axis=1)
    res = calc[:, depth // 2] if depth % 2 else (calc[:, depth // 2] + calc[:, depth // 2 - 1]) // 2
    return np.where((v[:, 0] == 0) & (v[:, -1] == 0), 0, res)


def cms_running(width: int, depth: int, hashes, weights, query: str, bins=None, els: int = 0):
    """the ordered add as a sequential loop in Python integers: (int64 results[n], int32 bins, elements_added)"""
    return cms_running_counted(width, depth, hashes, weights, query, bins, els)[:3]


def cms_running_counted(width: int, depth: int, hashes, weights, query: str, bins=None, els: int = 0):
    """``cms_running`` and, as a fourth value, its clamp count: the (op, row) pairs with ``bin + w > INT32_MAX``"""
    width, depth = int(width), int(depth)
    clamps = 0
    idx = cms_indices(hashes, width, depth).tolist()
    bins = np.zeros(width * depth, dtype=np.int64) if bins is None else np.asarray(bins).astype(np.int64)
    n = len(idx)
    w = np.broadcast_to(np.asarray(1 if weights is None else weights, dtype=np.int64), (n,)).tolist()
    out = np.empty(n, dtype=np.int64)
    for i, row in enumerate(idx):
        vals = []
        for x in row:  # (an index cannot repeat inside one key: the rows are disjoint)
            v = int(bins[x]) + w[i]
            if v > I32_MAX:
                v, clamps = I32_MAX, clamps + 1
            bins[x] = v
            vals.append(v)
        els = min(els + w[i], I64_MAX)
        vals.sort()
        if query == "min":
            res = vals[0]
        elif query == "mean":
            res = sum(vals) // depth
        elif vals[0] == 0 and vals[-1] == 0:
            res = 0
        else:
            assert query == "mean-min"
            calc = sorted(v - (els - v) // (width - 1) for v in vals)
            res = calc[depth // 2] if depth % 2 else (calc[depth // 2] + calc[depth // 2 - 1]) // 2
        out[i] = res
    return out, bins.astype(np.int32), els, clamps


def cms_running_vec(width: int, depth: int, hashes, weights, query, bins=None, els: int = 0):
    """the same rule in numpy, for batches the loop is too slow for: (int64 results[n], {bin index: value} of the touched bins,
    elements_added, clamp count).  ``query``: one name, or a tuple of names (the results are a tuple then: the rows are walked once).
    ``bins``: None (an empty table), one int (every bin holds it) or the whole table (read at the touched bins only); nothing of the
    table's size is allocated here.

    Weights are >= 0, so a bin never decreases and clamping at every step equals clamping the exact running sum once: per row a stable
    argsort of the bins, the cumulative sum of the weights inside each run of equal bins (int64: n * INT32_MAX < 2^63), the bin's start
    value on top, the clamp, and back to op order.  An op clamps when the (clamped) value in front of it plus its weight passes INT32_MAX."""
    width, depth, els = int(width), int(depth), int(els)
    h = np.asarray(hashes, dtype=np.uint64)
    n = h.shape[0]
    assert h.ndim == 2 and h.shape[1] >= depth and n * I32_MAX < I64_MAX
    w = np.ascontiguousarray(np.broadcast_to(np.asarray(1 if weights is None else weights, dtype=np.int64), (n,)))
    assert n == 0 or (0 <= int(w.min()) and int(w.max()) <= I32_MAX)
    vals = np.empty((depth, n), dtype=np.int64)
    touched, clamps = {}, 0
    at = np.arange(n, dtype=np.int64)
    for s in range(depth):
        col = h[:, s] % np.uint64(width)
        order = np.argsort(col.astype(np.uint16 if width <= 1 << 16 else np.int64), kind="stable")  # (16-bit keys: numpy's radix sort)
        sc, sw = col.astype(np.int64)[order], w[order]
        head = np.ones(n, dtype=bool)
        head[1:] = sc[1:] != sc[:-1]
        cs = np.cumsum(sw)
        first = np.maximum.accumulate(np.where(head, at, 0))  # where this element's run begins
        seg = cs - (cs - sw)[first]                            # inclusive sum inside the run
        if bins is None or isinstance(bins, (int, np.integer)):
            t0 = np.full(n, 0 if bins is None else int(bins), dtype=np.int64)
        else:
            t0 = np.asarray(bins)[sc + s * width].astype(np.int64)
        after = np.minimum(t0 + seg, I32_MAX)
        clamps += int((np.minimum(t0 + seg - sw, I32_MAX) + sw > I32_MAX).sum())
        vals[s, order] = after
        last = np.ones(n, dtype=bool)
        last[:-1] = head[1:]
        touched.update(zip((sc[last] + s * width).tolist(), after[last].tolist()))
    cw = np.cumsum(w)
    room = I64_MAX - els  # what elements_added can still take (els <= INT64_MAX, so room >= 0; beyond int64 for a negative start: no clamp)
    els_after = els + np.minimum(cw, min(room, I64_MAX))
    names = (query,) if isinstance(query, str) else tuple(query)
    assert all(q in ("min", "mean", "mean-min") for q in names)
    outs = [np.empty(n, dtype=np.int64) for _ in names]
    for lo in range(0, n, 1 << 15):  # (the sort of depth values per op, a slab of ops at a time)
        v = np.sort(vals[:, lo:lo + (1 << 15)].T, axis=1)
        for q, out in zip(names, outs):
            if q == "min":
                res = v[:, 0]
            elif q == "mean":
                res = v.sum(axis=1) // depth
            else:
                e = els_after[lo:lo + (1 << 15), None]
                assert int(e.max()) - int(v.min()) <= I64_MAX, "elements_added - bin leaves int64: outside what the sketch claims"
                calc = np.sort(v - (e - v) // (width - 1), axis=1)
                res = calc[:, depth // 2] if depth % 2 else (calc[:, depth // 2] + calc[:, depth // 2 - 1]) // 2
                res = np.where((v[:, 0] == 0) & (v[:, -1] == 0), 0, res)
            out[lo:lo + (1 << 15)] = res
    return outs[0] if isinstance(query, str) else tuple(outs), touched, (int(els_after[-1]) if n else els), clamps


RUN_DIGIT_EDGES = (0, 1, 255, 256, 257, 65535, 65536, 2**24 - 1, 2**24)


def running_digit_columns(width: int, n: int, seed: int = 0) -> np.ndarray:
    """int64[n] columns of a table ``width`` wide for the ordered add's 8-bit radix sort, interleaved in arrival order: the members of
    ``RUN_DIGIT_EDGES`` and ``width - 1`` that lie below the width, for every digit position the width has several pairs of columns that
    differ in exactly that digit (both orders of arrival), and seeded random columns for the rest; every chosen column comes several times,
    so that its bin is a segment of ops from all over the batch"""
    width = int(width)
    rng = np.random.default_rng(seed)
    chosen = [c for c in (*RUN_DIGIT_EDGES, width - 1) if 0 <= c < width]
    ndigits = max(1, ((width - 1).bit_length() + 7) // 8)
    for d in range(ndigits):
        for _ in range(8):
            a = int(rng.integers(0, width))
            b = a ^ (int(rng.integers(1, 256)) << (8 * d))
            if b < width:  # (the top digit of a narrow table has few values: such a pair may not exist)
                chosen += [a, b] if rng.integers(0, 2) else [b, a]
    cols = rng.integers(0, width, size=n, dtype=np.int64)
    reps = max(1, min(6, (n // 2) // len(chosen)))
    spots = rng.permutation(n)[: reps * len(chosen)]
    cols[spots] = np.resize(np.array(chosen, dtype=np.int64), spots.size)
    return cols


# ------------------------------------------------------------------ cuckoo filter
# A key of a cuckoo filter becomes (fp, idx_1, idx_2): fp = h & (2^bits - 1), idx_1 = fp % capacity, idx_2 = fnv_1a(str(fp)) % capacity.
# The capacities: the smallest ones, a prime, a power of two, and four near 2^31 -- two of them (1_610_612_737 and 2_146_483_645) chosen
# because a quarter of all 64-bit hashes have a one-short quotient estimate there, which 2^31 - 1 (2^64 mod c = 4) practically never has.
CK_CAPACITIES = (1, 2, 3, 37, 4096, 1_000_003, 2**30, 1_610_612_737, 2_146_483_645, 2**31 - 1)
FNV_BASIS, FNV_PRIME = 14695981039346656037, 1099511628211


def fnv_1a(data) -> int:
    """64-bit FNV-1a, seed 0: a str goes in code point by code point, bytes byte by byte"""
    h = FNV_BASIS
    for e in (map(ord, data) if isinstance(data, str) else data):
        h = ((h ^ e) * FNV_PRIME) % U64
    return h


def ck_triples(hashes, capacity: int, bits: int) -> list:
    """[(fp, idx_1, idx_2)] per 64-bit hash, in Python integers"""
    capacity, bits = int(capacity), int(bits)
    assert capacity >= 1 and 1 <= bits <= 32
    out = []
    for h in hashes:
        fp = int(h) & ((1 << bits) - 1)
        out.append((fp, fp % capacity, fnv_1a(str(fp)) % capacity))
    return out


def ck_edge_fingerprints(seed: int = 0) -> list:
    """fingerprints at which the decimal digits or the 32-bit word turn over, and seeded random ones of every bit length (4375 in all)"""
    fps = [0, 1]
    for k in range(1, 10):
        fps += [10**k - 1, 10**k]
    fps += [2**31 - 1, 2**31, 2**32 - 1]
    rng = np.random.default_rng(seed)
    for length in range(1, 33):
        fps += [int(x) for x in rng.integers(1 << (length - 1), 1 << length, size=8, dtype=np.uint64)]
    fps += [int(x) for x in rng.integers(0, 1 << 32, size=4096, dtype=np.uint64)]
    assert len(fps) == 4375 and all(0 <= fp < 2**32 for fp in fps)
    return fps


def ck_short(h: int, capacity: int) -> bool:
    """the truncated quotient estimate of ``h // capacity`` is one short: a reduction by that estimate needs its correction step"""
    h, capacity = int(h), int(capacity)
    return (h * (U64 // capacity)) >> 64 == h // capacity - 1
