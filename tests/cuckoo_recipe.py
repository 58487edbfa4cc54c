"""What the cuckoo filter's GPU tests share (tests/test_gpu_cuckoo.py, tests/test_gpu_cuckoo_edges.py): an op stream through the class, the
model that stream is compared with, and the parallel placement's iteration written out sequentially.  Plain Python: nothing here imports
the engine (the tests hand the package in)."""

import itertools
import random

import cuckoo_model as M

POLICIES = ["auto", "parallel", "sequential"]


def finger_bits(params) -> int:
    """the fingerprint width of a fixture's `params`: ``finger_size`` bytes, or ``finger_bits`` where an ``error_rate`` made it"""
    return params["finger_bits"] if "finger_bits" in params else params["finger_size"] * 8


def make_filter(pa, params):
    """``CuckooFilter(**params)``, or ``CuckooFilter.init_error_rate(**params)`` where `params` names an ``error_rate``"""
    p = dict(params)
    bits = p.pop("finger_bits", None)
    cf = pa.CuckooFilter.init_error_rate(**p) if "error_rate" in p else pa.CuckooFilter(**p)
    assert bits is None or cf.fingerprint_size_bits == bits
    return cf


def run_class(pa, params, keys, ops, seed, policy):
    """the op stream in batches cut where add turns into remove -> (filter, remove returns, error index, error message)"""
    random.seed(seed)
    cf = make_filter(pa, params)
    cf._insert_policy = policy
    rets, at = [], 0
    for op, group in itertools.groupby(ops, key=lambda o: o[0]):
        batch = [keys[k] for _, k in group]
        if op == "a":
            try:
                cf.add_many(batch)
            except pa.CuckooFilterFullError as ex:
                return cf, rets, at + ex.index, str(ex)
        else:
            rets += [int(r) for r in cf.remove_many(batch)]
        at += len(batch)
    return cf, rets, None, None


def model_of(params, seed=None, state=None):
    if state is None:
        random.seed(seed)
        state = random.getstate()
    return M.CuckooModel(params["capacity"], params["bucket_size"], params["max_swaps"], params["expansion_rate"], params["auto_expand"],
                         finger_bits(params), M.MT19937(state))


def assert_same(cf, m):
    assert bytes(cf) == m.export()
    assert (cf.elements_added, cf.capacity) == (m.elements_added, m.capacity)
    assert random.getstate() == m.rng.getstate()
    assert cf.buckets == m.buckets


def _active_before(segment, at, d, j, room, walk_limit):
    """the active claims (d[t] == which + 1) of other keys among segment[:at], walked backwards and counted up to `room`
    -> the count, or None once `walk_limit` claims were walked without an answer"""
    c = walked = 0
    while at > 0 and c < room:
        if walked == walk_limit:
            return None
        at -= 1
        walked += 1
        t, which = segment[at]
        if t != j and d[t] == which + 1:
            c += 1
    return c


def jacobi_sweeps(triples, B, max_sweeps=32, walk_limit=None, fill=None):
    """the placement's iteration, written out sequentially: every sweep decides each key (1: idx_1, 2: idx_2, 3: it needs a kick) from the
    PREVIOUS sweep's decisions of the keys in front of it, starting from "all 1".  Every key owns a claim on each of its two buckets; a
    bucket's claims stand in key order, and a key counts the active ones in front of its own.  With a `walk_limit`, a key that walks
    that many claims without an answer decides 3.  `fill`: fingerprints already in each bucket (default: an empty table).

    Yields (decisions, changed, kick) after every sweep: the first key whose decision changed in it and the first that decided 3 (None:
    no such key).  Stops after a fixed point, after a sweep whose first 3 lies in front of its first change, or after `max_sweeps`."""
    m = len(triples)
    segments, where = {}, {}
    for j, (_, i1, i2) in enumerate(triples):
        for which, b in enumerate((i1, i2)):
            where[j, which] = len(segments.setdefault(b, []))
            segments[b].append((j, which))
    d = [1] * m
    for _ in range(max_sweeps):
        new = []
        for j, (_, i1, i2) in enumerate(triples):
            decision = 3
            for which, b in enumerate((i1, i2)):
                room = B - (fill[b] if fill is not None else 0)
                if room <= 0:
                    continue
                c = _active_before(segments[b], where[j, which], d, j, room, walk_limit)
                if c is None:
                    break
                if c < room:
                    decision = which + 1
                    break
            new.append(decision)
        changed = next((j for j in range(m) if new[j] != d[j]), None)
        kick = next((j for j in range(m) if new[j] == 3), None)
        d = new
        yield list(d), changed, kick
        if changed is None or (kick is not None and kick < changed):
            break


def jacobi(triples, B, max_sweeps=32, walk_limit=None):
    """-> (sweeps, accepted prefix = min(first change of the last sweep, first 3)) of ``jacobi_sweeps`` on an empty table"""
    m = len(triples)
    sweeps = changed = kick = 0
    for sweeps, (_, changed, kick) in enumerate(jacobi_sweeps(triples, B, max_sweeps, walk_limit), start=1):
        pass
    return sweeps, min(m, m if changed is None else changed, m if kick is None else kick)
