"""The signed ordered CountMinSketch batch (psk_cms_update_running, DESIGN.md 3.9 "signed batches") as a model: the composition law
of clamp-add maps as code, and the whole batch in numpy.

An op of weight w on a bin is the map x -> clamp(x + w, LO, HI): an add clamps above only, a remove below only
(countminsketch.py:280-284, :312-316), and the value in front of the op lies inside the rails, so the full clamp describes both.
A map is a triple (a, lo, hi): x -> min(hi, max(lo, x + a)), lo <= hi.  The rails are parameters everywhere: the brute-force tests run
on toy rails, the sketch on int32 (bins) and int64 (elements_added)."""

import hashlib

import numpy as np

I32 = (-(2**31), 2**31 - 1)
I64 = (-(2**63), 2**63 - 1)
M64 = 2**64 - 1
QUERIES = ("min", "mean", "mean-min")


# ------------------------------------------------------------------ the law (Python integers)
def clamp(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


def op_map(w, rails):
    return (w, rails[0], rails[1])


def identity(rails):
    """the identity on every value inside the rails"""
    return (0, rails[0], rails[1])


def combine(f, g):
    """f, then g"""
    a1, lo1, hi1 = f
    a2, lo2, hi2 = g
    return (a1 + a2, clamp(lo1 + a2, lo2, hi2), clamp(hi1 + a2, lo2, hi2))


def apply(f, x):
    a, lo, hi = f
    return min(hi, max(lo, x + a))


def sequential(x, weights, rails):
    """the clamp loop: (value after every op, number of ops whose unclamped value lies strictly outside the rails)"""
    out, clamps = [], 0
    for w in weights:
        v = x + w
        clamps += v < rails[0] or v > rails[1]
        x = clamp(v, *rails)
        out.append(x)
    return out, clamps


def scanned(x, weights, rails):
    """the same from an inclusive scan of maps: op i's value is clamp(F_exclusive(x) + w_i), F_exclusive the identity at the head"""
    out, clamps = [], 0
    f = identity(rails)
    for w in weights:
        prev = apply(f, x)
        v = prev + w
        clamps += v < rails[0] or v > rails[1]
        out.append(clamp(v, *rails))
        f = combine(f, op_map(w, rails))
    return out, clamps


# ------------------------------------------------------------------ the whole batch (numpy)
def fnv_matrix(keys, depth):
    """default_fnv_1a (hashes.py:71-103) of every key -> uint64[n][depth]; keys: str (by code point <= 255) or bytes objects, or (n, L) uint8"""
    if isinstance(keys, np.ndarray):
        raw = [bytes(r) for r in keys]
    else:
        raw = [k.encode("latin-1") if isinstance(k, str) else bytes(k) for k in keys]
    uniq = {}
    for k in raw:
        if k not in uniq:
            row = []
            for s in range(depth):
                h = (14695981039346656037 + 31 * s) & M64
                for c in k:
                    h = ((h ^ c) * 1099511628211) & M64
                row.append(h)
            uniq[k] = row
    return np.array([uniq[k] for k in raw], dtype=np.uint64).reshape(len(raw), depth)


def _segments(seg_id, w, start, rails):
    """seg_id sorted, arrival order inside equal ids; w: int64 weights in that order; start: the value every element's segment begins
    with.  -> (value after every element, clamp count).  Position j of every segment in one numpy step, the longest segments first."""
    n = seg_id.size
    after = np.empty(n, dtype=np.int64)
    if n == 0:
        return after, 0
    head = np.ones(n, dtype=bool)
    head[1:] = seg_id[1:] != seg_id[:-1]
    starts = np.nonzero(head)[0]
    lens = np.diff(np.append(starts, n))
    by_len = np.argsort(-lens, kind="stable")
    starts, lens = starts[by_len], lens[by_len]
    val = start[starts].astype(np.int64)
    alive = np.searchsorted(-lens, -np.arange(int(lens[0])), side="left")  # segments longer than j
    clamps = 0
    lo, hi = rails
    for j in range(int(lens[0])):
        k = int(alive[j])
        at = starts[:k] + j
        v = val[:k] + w[at]
        clamps += int(((v < lo) | (v > hi)).sum())
        v = np.clip(v, lo, hi)
        val[:k] = v
        after[at] = v
    return after, clamps


def query_values(vals, els_after, width, query):
    """vals: int64[n][depth] values of the rows after every op; els_after: elements_added after every op (Python integers, object
    array) -> int64[n], an object array for 'mean-min' (countminsketch.py:429-453)"""
    n, depth = vals.shape
    v = np.sort(vals, axis=1)
    if query == "min":
        return v[:, 0].copy()
    if query == "mean":
        return v.sum(axis=1) // depth
    assert query == "mean-min"
    if n and max(abs(int(min(els_after))), abs(int(max(els_after)))) < 2**62:  # (elements_added - bin stays inside int64: plain numpy)
        e = np.asarray(els_after, dtype=np.int64)[:, None]
        calc = np.sort(v - (e - v) // (width - 1), axis=1)
        res = calc[:, depth // 2] if depth % 2 else (calc[:, depth // 2] + calc[:, depth // 2 - 1]) // 2
        return np.where((v[:, 0] == 0) & (v[:, -1] == 0), 0, res)
    vo = v.astype(object)
    calc = np.sort(vo - (np.asarray(els_after, dtype=object)[:, None] - vo) // (width - 1), axis=1)
    res = calc[:, depth // 2] if depth % 2 else (calc[:, depth // 2] + calc[:, depth // 2 - 1]) // 2
    res = np.where((v[:, 0] == 0) & (v[:, -1] == 0), 0, res)
    return res  # (Python integers: elements_added - bin may leave int64 next to the int64 rails)


def signed_batch(width, depth, hashes, weights, queries, bins=None, els=0, rails=I32, els_rails=I64):
    """the ordered signed batch: ({query: int64 results[n]}, final table int64[depth * width], elements_added, clamp count).
    hashes: uint64[n][>= depth]; weights: None (+1) or integers, w >= 0 adds w, w < 0 removes -w; bins: None or the table in front."""
    width, depth, els = int(width), int(depth), int(els)
    h = np.asarray(hashes, dtype=np.uint64)
    h = h if h.ndim == 2 else h.reshape(0, depth)
    n = h.shape[0]
    w = np.ascontiguousarray(np.broadcast_to(np.asarray(1 if weights is None else weights, dtype=np.int64), (n,)))
    table = np.zeros(width * depth, dtype=np.int64) if bins is None else np.asarray(bins).astype(np.int64).copy()
    vals = np.empty((n, depth), dtype=np.int64)
    small = np.uint16 if width <= 1 << 16 else np.int64  # (16-bit keys: numpy's radix sort)
    seg, ws, orders = [], [], []
    for s in range(depth):
        col = (h[:, s] % np.uint64(width)).astype(np.int64)
        order = np.argsort(col.astype(small), kind="stable")
        orders.append(order)
        seg.append(col[order] + s * width)
        ws.append(w[order])
    seg = np.concatenate(seg) if depth else np.zeros(0, dtype=np.int64)
    after, clamps = _segments(seg, np.concatenate(ws) if depth else w[:0], table[seg], rails)
    for s in range(depth):
        part = after[s * n:(s + 1) * n]
        vals[orders[s], s] = part
    if n:
        last = np.ones(seg.size, dtype=bool)
        last[:-1] = seg[1:] != seg[:-1]
        table[seg[last]] = after[last]
    names = (queries,) if isinstance(queries, str) else tuple(queries)
    els_after = np.empty(n, dtype=object)
    e = els
    lo, hi = els_rails
    for i, x in enumerate(w.tolist()):
        e = min(hi, max(lo, e + x))
        els_after[i] = e
    res = {q: query_values(vals, els_after, width, q) for q in names}
    return res, table, e, clamps


def threshold_dict(tracked, keys, weights, results, threshold):
    """StreamThreshold's dict over an ordered signed batch (countminsketch.py:800-803, :831-834), in op order"""
    for k, w, r in zip(keys, weights, results):
        r = int(r)
        if r >= threshold:
            tracked[k] = r
        elif w < 0:
            tracked.pop(k, None)
    return tracked


def results_sha(results):
    return hashlib.sha256(np.asarray(results, dtype=np.int64).tobytes()).hexdigest()


# ------------------------------------------------------------------ the streams of tests/golden/golden_signed_running.json
# From integers alone, on top of tests/hitters_recipe.py (keys: its skewed stream; preload: an export image).  The weights of op i by
# the case's "weights":
#   unit            +1 or -1, half of each
#   small           -7 .. 7
#   rail            a cycle of +INT32_MAX, -INT32_MAX, INT32_MIN, 0, +1, -1 and a signed 31-bit number
#   add_then_remove the first half adds 1 .. 7, the second half removes 1 .. 4 (the tests feed the halves to add_many / remove_many)
# preload: {"bins": "hi" | "lo" | "both", "below": d, "elements_added": e} -- every bin d counts from INT32_MAX, from INT32_MIN, or
# the even bins from one and the odd ones from the other.
def stream_weights(case):
    import hitters_recipe as R

    n, salt, kind = case["n"], case["salt"], case["weights"]
    r = [R.sm((R.SEED ^ 0x51A9ED) + salt * 7919 + i) for i in range(n)]
    if kind == "unit":
        w = [1 if x & 1 else -1 for x in r]
    elif kind == "small":
        w = [x % 15 - 7 for x in r]
    elif kind == "rail":
        cyc = (I32[1], -I32[1], I32[0], 0, 1, -1)
        w = [cyc[i % 7] if i % 7 < 6 else (x % 2**31) * (1 if x >> 40 & 1 else -1) for i, x in enumerate(r)]
    else:
        assert kind == "add_then_remove"
        w = [1 + x % 7 if i < n // 2 else -(1 + x % 4) for i, x in enumerate(r)]
    return np.array(w, dtype=np.int64)


def preload_bins(case):
    """int32[depth * width] the case starts from, or None"""
    p = case.get("preload")
    if not p:
        return None
    cells = case["width"] * case["depth"]
    hi, lo = I32[1] - p["below"], I32[0] + p["below"]
    if p["bins"] == "both":
        return np.where(np.arange(cells) % 2 == 0, hi, lo).astype(np.int32)
    return np.full(cells, hi if p["bins"] == "hi" else lo, dtype=np.int32)


def preload_bytes(case):
    import hitters_recipe as R

    b = preload_bins(case)
    return None if b is None else b.tobytes() + R.FOOTER.pack(case["width"], case["depth"], case["preload"]["elements_added"])
