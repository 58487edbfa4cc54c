"""Table addressing at its limits, through the pre-hashed batch entries (``*_alt_many``, ``add_alt_many_ordered``) and 64-bit hashes chosen
by tests/edge_hashes.py: the first and last cell of every candidate slice, ``h % m`` through a small value / the top of the range / a
random multiple / a hash whose quotient estimate is one short, keys whose probes all name one cell, probe fields at all ones next to
boundary weights, whole batches aimed at one block of 2^10 cells, and CountMinSketch keys that collide in one row only.

Everything is bit-exact against the helper's numpy references: the whole (padded) table is compared on the device with a tensor built from
the reference's indices, every answer and ``elements_added`` with the reference's.  Every batch goes in once as a host array and once as a
device tensor.  Paths are chosen with the engine's options; where a read-only counter tells which path ran, it is asserted."""

import gc

import numpy as np
import pytest

import edge_hashes as E

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OPTS = ("partition", "partition_min_keys", "partition_two_level_slices", "bloom_lookup", "dense_walk_groups", "nibble_min_lg_lookup",
        "nibble_min_lg_update", "lookup_nibble_slices", "update_nibble_slices", "cms_small_weights", "remove_optimistic")
WHERE = ("host", "device")


@pytest.fixture(scope="module")
def pa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pyprobables_amd

    return pyprobables_amd


@pytest.fixture()
def N():
    """every batch through the partitioned kernels wherever the table is eligible; the options are put back afterwards"""
    from pyprobables_amd import _native as N

    gc.collect()  # (the counters read below are process-wide: let no sketch of an earlier test flush in the middle of this one)
    old = [N.get_option(k) for k in OPTS]
    N.set_option("partition", 1)
    N.set_option("partition_min_keys", 1)
    yield N
    for k, v in zip(OPTS, old):
        N.set_option(k, v)


def _dev(a):
    a = np.ascontiguousarray(a)  # (unsigned words travel as the signed tensors of the same bits)
    return torch.from_numpy(a.view({np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype))).cuda()


def _give(a, where):
    return a if where == "host" or a is None else _dev(a)


def _host(x):
    return x.cpu().numpy() if hasattr(x, "is_cuda") else np.asarray(x)


def _rows(vals, k, rng):
    """a flat run of hashes as rows of k (filled up with repeats of its own values)"""
    vals = np.asarray(vals, dtype=np.uint64)
    fill = (-vals.size) % k
    return np.concatenate([vals, rng.choice(vals, size=fill)]).reshape(-1, k)


def _noise(rng, n, cols):
    return rng.integers(0, 2**63, size=(n, cols), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, cols), dtype=np.uint64)


def _expect_bits(t, set_cells):
    """the Bloom table tensor (int32 words, little-endian bit order) with exactly `set_cells` set"""
    u = np.unique(np.asarray(set_cells, dtype=np.int64))
    words, inv = np.unique(u >> 5, return_inverse=True)
    masks = np.zeros(words.size, dtype=np.uint32)
    np.bitwise_or.at(masks, inv, (np.uint32(1) << (u & 31).astype(np.uint32)))
    exp = torch.zeros_like(t)
    exp[torch.from_numpy(words).to(t.device)] = torch.from_numpy(masks.view(np.int32)).to(t.device)
    return exp


def _expect_counters(t, ref, np_dtype):
    """the counter table tensor (padding included) as the reference has it"""
    nz = np.flatnonzero(ref.exact)
    vals = np.minimum(ref.exact[nz], ref.rail).astype(np_dtype).view(np.int32)
    exp = torch.zeros_like(t)
    exp[torch.from_numpy(nz).to(t.device)] = torch.from_numpy(vals).to(t.device)
    return exp


def _same_counters(sk, ref, np_dtype):
    assert torch.equal(sk.table_tensor, _expect_counters(sk.table_tensor, ref, np_dtype))
    assert sk.elements_added == ref.els
    if hasattr(sk, "table_released"):
        sk.table_released()


def _one_cell_rows(m, k, rng, n, hows=("low", "high", "mid")):
    """n rows whose k hashes all name ONE boundary cell (each through its own route), then n rows with k - 1 on one cell"""
    cells = E.edge_cells(m)
    pick = np.repeat(rng.choice(cells, size=2 * n), k)
    per_how = [E.hashes_for(pick, m, how, 5) for how in hows]
    h = np.choose(rng.integers(0, len(hows), size=pick.size), per_how).astype(np.uint64).reshape(-1, k)
    if k > 1:
        h[n:, k - 1] = E.hashes_for(rng.choice(cells, size=n), m, hows[-1], 6)
    return h


# ------------------------------------------------------------------ Bloom: a, b
BLOOM_CASES = [("direct", E.BLOOM_DIRECT, 0), ("2p28", E.BLOOM_2P28, 0), ("2p28-two-level", E.BLOOM_2P28, 2), ("np2", E.BLOOM_NP2, 0),
               ("np2-two-level", E.BLOOM_NP2, 2), ("2p31", E.BLOOM_2P31, 0), ("2p31-two-level", E.BLOOM_2P31, 2)]
_bloom_streams = {}


def _bloom_stream(m, k, hows):
    """(present rows, check rows, the reference's set cells, its answers): built once per geometry"""
    key = (m, k, hows)
    if key in _bloom_streams:
        return _bloom_streams[key]
    rng = np.random.default_rng(m % 1000)
    cells = E.edge_cells(m)
    parts = [_rows(E.hashes_for(cells, m, how, 1), k, rng) for how in hows]
    limits = [0, 2**64 - 1, m, (2**64 - 1) // m * m, 2**32 - 1, 2**32, 2**63, 2**63 - 1]  # h = 0, 2^64 - 1, exact multiples of m
    parts.append(_rows(np.array(limits, dtype=np.uint64), k, rng))
    if not E.is_pow2(m):
        sc = E.short_cells(m)
        parts.append(_rows(np.concatenate([E.hashes_for(sc * 16, m, "short", None), E.hashes_for(sc * 48, m, "short", 7)]), k, rng))
    parts.append(_one_cell_rows(m, k, rng, 100, hows))
    n_edge = sum(p.shape[0] for p in parts)
    if len(hows) > 1:
        parts.append(_noise(rng, min(2000, m // (8 * k)), k))  # ordinary keys around them (a small table stays sparse: absent keys exist)
    present = np.concatenate(parts)
    present = present[rng.permutation(present.shape[0])]
    idx = E.indices(present, m, k)
    set_cells = np.unique(idx)
    # absent keys that differ from a present key in ONE probe: the neighbour cell c +- 1, and the same cell-in-slice one slice of 2^s further
    base = present[:min(n_edge, 1500)].copy()
    bidx = idx[: base.shape[0]]
    r = np.arange(base.shape[0])
    j = r % k
    c = bidx[r, j]
    near = np.where(c % 2 == 0, c + 1, c - 1)  # (away from the boundary's other cell, which is present itself)
    near = np.where(near < 0, c + 1, np.where(near >= m, c - 1, near))
    step = np.int64(1) << (10 + (r % 11))
    far = np.where((r // 11) % 2 == 0, c + step, c - step)
    far = np.where(far < 0, c + step, np.where(far >= m, c - step, far))
    far = np.where((far < 0) | (far >= m), near, far)
    absent = []
    for cells_new in (near, far):
        a = base.copy()
        a[r, j] = E.hashes_for(cells_new, m, hows[-1], 9)
        absent.append(a)
    check = np.concatenate([present, *absent])
    want = E.bloom_member(set_cells, E.indices(check, m, k))
    assert want[: present.shape[0]].all() and int((~want).sum()) > base.shape[0] // 2  # (a moved probe may land on another present cell)
    _bloom_streams[key] = (present, check, set_cells, want)
    return _bloom_streams[key]


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name,geom,two_level", BLOOM_CASES, ids=[c[0] for c in BLOOM_CASES])
def test_bloom_boundary_cells_and_one_cell_keys(pa, N, name, geom, two_level, where):
    """direct kernels (m < 2^16), single-level pass 1 + apply, the forced two-level insert, and the lookup schemes 0 / 1 / 3 / 4 beside the default;
    2^28 bits: the low-word route under a high word of all ones; 9.6e7 bits: reduce_small and a partial last slice; m just below 2^31: boundary
    cells through `high` alone, the `short` hashes and a handful of limit values (0, 2^64 - 1, m, 2^32 ...), no ordinary keys (r = h - q * m
    just below 2 m ~ 2^32), compared on the device"""
    if two_level:
        N.set_option("partition_two_level_slices", two_level)
    blm = pa.BloomFilter(est_elements=geom[0], false_positive_rate=geom[1])
    m, k = blm.number_bits, blm.number_hashes
    assert m == E.bloom_bits(*geom)
    present, check, set_cells, want = _bloom_stream(m, k, ("high",) if name.startswith("2p31") else ("low", "high", "mid"))
    assert present.shape[0] < 20_000
    blm.add_alt_many(_give(present, where))
    assert torch.equal(blm.table_tensor, _expect_bits(blm.table_tensor, set_cells))  # (the words beyond m included: they stay clear)
    assert blm.elements_added == present.shape[0]
    if m < 2**20:
        assert np.array_equal(np.frombuffer(bytes(blm.bloom), dtype=np.uint8), E.bloom_table(m, set_cells))
    given = _give(check, where)
    for scheme in ((2,) if name == "direct" else (2, 0, 1, 3, 4)):
        N.set_option("bloom_lookup", scheme)
        got = blm.check_alt_many(given)
        assert np.array_equal(_host(got).astype(bool), want), scheme
    blm.add_alt_many(given)  # a second batch ORs into the table: the absent keys' cells join
    assert torch.equal(blm.table_tensor, _expect_bits(blm.table_tensor, E.indices(check, m, k)))
    assert blm.elements_added == present.shape[0] + check.shape[0]


# ------------------------------------------------------------------ CountingBloom: a, b, c
CBF_CASES = [("direct", E.CBF_DIRECT), ("slices32", E.CBF_SLICES32), ("nibble", E.CBF_NIBBLE), ("window", E.CBF_WINDOW),
             ("two-level", E.CBF_SLICES32)]


def _cbf(pa, N, name, geom):
    if name == "nibble":  # 4-bit images for updates and lookups on a table of 2^23 .. 2^24 counters
        N.set_option("nibble_min_lg_lookup", 20)
        N.set_option("nibble_min_lg_update", 20)
    if name == "two-level":  # no 4-bit images, and every table of more than two slices through the two-level split
        N.set_option("update_nibble_slices", 0)
        N.set_option("partition_two_level_slices", 2)
    N.set_option("lookup_nibble_slices", 2)
    cbf = pa.CountingBloomFilter(est_elements=geom[0], false_positive_rate=geom[1])
    assert cbf.number_bits == E.bloom_bits(*geom)
    return cbf, E.cbf_counters(cbf.number_bits)


def _ordinary_rows(name, m, k):
    """how many ordinary keys travel with the chosen ones.  The 4-bit update images, the optimistic decrement and the two-level split are
    taken only by a batch that brings at least cells / 8 probes (a pass over the whole table has to pay): there the ordinary keys alone
    bring that many, so that the boundary cells and one-cell keys among them go down those paths"""
    return m // (8 * k) + 1024 if name in ("nibble", "two-level") else 2000


def _window_prelude(cbf, ref, oracle, N):
    """the update window takes 16-byte keys only: real keys wait in it (adds and a remove: two kinds of phases, and together the
    table's cells / 8 probes that make a fold worth a pass), the first pre-hashed batch behind them makes it fold"""
    keys = oracle.gen_keys16(17, 600_000)
    oc = oracle.OracleCBF(cbf.number_bits, cbf.number_hashes)
    folds = N.get_option("update_window_folds")
    for remove, part in ((False, keys[:300_000]), (True, keys[:150_000]), (False, keys[300_000:])):
        (cbf.remove_many if remove else cbf.add_many)(torch.from_numpy(part).cuda())
        oc.update_keys(part, -np.ones(part.shape[0], dtype=np.int64) if remove else None)
    assert cbf.get_engine_option("window_pending_batches") == 3
    ref.exact += oc.bloom
    ref.els += oc.els_added
    return folds


def _check_cbf(cbf, ref, h, where, k):
    got = _host(cbf.check_alt_many(_give(h, where))).view(np.uint32)
    assert np.array_equal(got, ref.values(E.indices(h, cbf.number_bits, h.shape[1])).min(axis=1).astype(np.uint32))


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name,geom", CBF_CASES, ids=[c[0] for c in CBF_CASES])
def test_cbf_boundary_cells_and_one_cell_keys(pa, oracle, N, name, geom, where):
    """add (unit, 7, 3000, unit), check and remove (optimistic decrement on / off) of keys on boundary cells and of keys whose k probes name one
    cell (k * w goes in, check returns it, a remove takes k * w out).  direct: the direct kernels; slices32 and window: small batches, single-level
    32-bit slices for updates and removes (the window table after a fold of real keys; its lookups through the 4-bit images); nibble and
    two-level: batches of cells / 8 probes and more -- unit adds through the 4-bit delta images resp. the two-level split, weighted ones
    through the 32-bit slices resp. the split, unit removes through the optimistic decrement (option on) or lookup + checked decrement"""
    cbf, ref = _cbf(pa, N, name, geom)
    m, k = cbf.number_bits, cbf.number_hashes
    rng = np.random.default_rng(3)
    cells = E.edge_cells(m)
    parts = [_rows(E.hashes_for(cells, m, how, 2), k, rng) for how in ("low", "high", "mid")]
    if not E.is_pow2(m):
        sc = E.short_cells(m)
        parts.append(_rows(np.concatenate([E.hashes_for(sc * 16, m, "short", None), E.hashes_for(sc * 48, m, "short", 7)]), k, rng))
    ones = _one_cell_rows(m, k, rng, 150)
    parts.append(ones)
    n_chosen = sum(p.shape[0] for p in parts)
    n_ordinary = _ordinary_rows(name, m, k)
    h = np.concatenate([*parts, _noise(rng, n_ordinary, k)])
    order = rng.permutation(h.shape[0])
    h = h[order]
    idx = E.indices(h, m, k)
    folds = _window_prelude(cbf, ref, oracle, N) if name == "window" else None
    replays = N.get_option("cbf_ordered_replays")
    for w in (None, 7, 3000, None):
        wv = None if w is None else np.full(h.shape[0], w, dtype=np.uint32)
        cbf.add_alt_many(_give(h, where), _give(wv, where))
        ref.add(idx, 1 if w is None else w)
        if folds is not None:
            assert N.get_option("update_window_folds") == folds + 1  # the waiting real-key batches were folded in front of this one
        _same_counters(cbf, ref, np.uint32)
    # a key whose k probes name one cell put k * (1 + 7 + 3000 + 1) into it
    oi = E.indices(ones[:150], m, k)
    assert (oi == oi[:, :1]).all() and (ref.exact[oi[:, 0]] >= k * 3009).all()
    probe = np.concatenate([h[:20_000], h[order < n_chosen], _noise(rng, 1000, k)])
    shadow = N.get_option("cbf_lookup_shadow_hits")
    for _ in range(3):
        _check_cbf(cbf, ref, probe, where, k)
    if name in ("nibble", "window"):  # the third lookup of an unchanged table loads the kept 4-bit images: the nibble-slice lookup ran
        assert N.get_option("cbf_lookup_shadow_hits") > shadow
    # removed again: every other key -- and, where the batch has to bring cells / 8 probes, every ordinary key besides
    half = np.flatnonzero((np.arange(h.shape[0]) % 2 == 0) | ((order >= n_chosen) & (n_ordinary > 2000)))
    assert n_ordinary == 2000 or min(h.shape[0], half.size) * k >= m // 8
    for optimistic, w in ((1, None), (0, None), (1, 7), (0, 3000)):
        N.set_option("remove_optimistic", optimistic)
        wv = None if w is None else np.full(half.size, w, dtype=np.uint32)
        cbf.remove_alt_many(_give(h[half], where), _give(wv, where))
        ref.remove(idx[half], 1 if w is None else w)
        _same_counters(cbf, ref, np.uint32)
    assert N.get_option("cbf_ordered_replays") == replays  # every remove was well-formed: none needed the sequential replay
    assert cbf.batch_diagnostics() == {"violations": 0, "saturated": 0}
    _check_cbf(cbf, ref, probe, where, k)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name,geom", CBF_CASES[:3] + CBF_CASES[4:], ids=[c[0] for c in CBF_CASES[:3] + CBF_CASES[4:]])
def test_cbf_counters_through_the_nibble_escape_and_up_to_the_rail(pa, N, name, geom, where):
    """counters on boundary cells carried through 14, 15, 16 (15 is the 4-bit image's escape) by unit adds, then to 2^32 - 2, 2^32 - 1 and
    against the rail by weighted ones; every probe of these keys has its own cell (next to the rail the reference's repeated-index add raises).
    nibble / two-level: every batch brings cells / 8 probes, so the unit steps run through the 4-bit delta images resp. the two-level split"""
    cbf, ref = _cbf(pa, N, name, geom)
    m, k = cbf.number_bits, cbf.number_hashes
    rng = np.random.default_rng(8)
    cells = E.edge_cells(m)
    cells = cells[: cells.size // k * k]
    carry = E.any_how(cells, m, 4).reshape(-1, k)  # each boundary cell belongs to exactly one key
    cidx = E.indices(carry, m, k)
    noise = _noise(rng, min(1500, m // (32 * k)) if name in ("direct", "slices32") else _ordinary_rows(name, m, k), k)
    clean = ~np.isin(cidx, E.indices(noise, m, k))  # (the boundary cells no ordinary key touches hold exactly the carried value)
    assert clean.sum() > clean.size // 2
    for step, w in enumerate((14, None, None, 2**32 - 2 - 16, None, None, 5)):
        if w is None:
            h, wv = np.concatenate([carry, noise]), None
        else:
            h = np.concatenate([carry, noise])
            wv = np.concatenate([np.full(carry.shape[0], w, dtype=np.uint32), rng.integers(0, 20, size=noise.shape[0]).astype(np.uint32)])
        order = rng.permutation(h.shape[0])
        h, wv = h[order], (None if wv is None else wv[order])
        cbf.add_alt_many(_give(h, where), _give(wv, where))
        ref.add(E.indices(h, m, k), 1 if wv is None else wv)
        _same_counters(cbf, ref, np.uint32)
        _check_cbf(cbf, ref, np.concatenate([carry, noise[:20_000]]), where, k)
        if step < 5:
            assert (ref.values(cidx)[clean] == (14, 15, 16, 2**32 - 2, 2**32 - 1)[step]).all()
    assert int(ref.values(cidx).min()) == 2**32 - 1 and int(ref.exact[cidx].max()) > 2**32


# ------------------------------------------------------------------ CountMinSketch: a, c
CMS_WEIGHTS = [0, 15, 16] + [v for s in (15, 16, 18, 20) for v in (2 ** (31 - s) - 1, 2 ** (31 - s))]


def _cms_stream(width, depth):
    rng = np.random.default_rng(width % 1000 + depth)
    cells = E.edge_cells(width)
    parts = [_rows(E.hashes_for(cells, width, how, 3), depth, rng) for how in ("low", "high", "mid")]
    if not E.is_pow2(width):
        sc = E.short_cells(width)
        parts.append(_rows(np.concatenate([E.hashes_for(sc * 16, width, "short", None), E.hashes_for(sc * 48, width, "short", 7)]), depth, rng))
    # cell-in-slice at all ones of the TABLE index column + row * width, for slices of 2^15, 2^16, 2^18 and 2^20 cells, under every weight
    cols = []
    for s in (15, 16, 18, 20):
        for _ in range(2 * len(CMS_WEIGHTS)):
            row = []
            for i in range(depth):
                lo, hi = (i * width + (1 << s)) >> s, ((i + 1) * width) >> s
                row.append((int(rng.integers(lo, hi + 1)) << s) - 1 - i * width if lo <= hi else int(rng.integers(0, width)))
            cols.append(row)
    parts.append(E.any_how(np.array(cols).reshape(-1), width, 6).reshape(-1, depth))
    n_edge = sum(p.shape[0] for p in parts)
    h = np.concatenate([*parts, _noise(rng, 2000, depth)])
    w = np.concatenate([np.resize(np.array(CMS_WEIGHTS, dtype=np.int32), n_edge), rng.integers(0, 16, size=2000).astype(np.int32)])
    order = rng.permutation(h.shape[0])
    return h[order], w[order]


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("width,depth", E.CMS_SHAPES)
def test_cms_boundary_cells_and_field_limits(pa, N, width, depth, where):
    """add, weighted add (inline probe format, weight << shift | cell: weights 0, 15, 16, 2^(31-s) - 1, 2^(31-s) beside a cell-in-slice of
    all ones), remove and check under min / mean / mean-min"""
    N.set_option("cms_small_weights", 2)  # "always compact" -- which a pre-hashed batch cannot be, see below
    cms = pa.CountMinSketch(width=width, depth=depth)
    ref = E.cms_counters(width, depth)
    h, w = _cms_stream(width, depth)
    idx = E.cms_indices(h, width, depth)
    used = N.get_option("cms_small_weights_used")
    cms.add_alt_many(_give(h, where))
    ref.add(idx)
    _same_counters(cms, ref, np.int32)
    for _ in range(2):
        cms.add_alt_many(_give(h, where), _give(w, where))
        ref.add(idx, w)
        _same_counters(cms, ref, np.int32)
    # the compact format is built for the 16-byte key layout alone: whatever the option says, a pre-hashed batch travels in the plain inline one
    assert N.get_option("cms_small_weights_used") == used
    probe = np.concatenate([h, _noise(np.random.default_rng(1), 1000, depth)])
    pidx = E.cms_indices(probe, width, depth)

    def checks():
        for query in ("min", "mean", "mean-min"):
            cms.query_type = query
            got = _host(cms.check_alt_many(_give(probe, where))).astype(np.int64)
            assert np.array_equal(got, E.cms_query(ref.values(pidx), query, width, ref.els)), query

    checks()
    half = np.arange(0, h.shape[0], 2)
    cms.remove_alt_many(_give(h[half], where), _give(w[half], where))
    ref.remove(idx[half], w[half])
    cms.remove_alt_many(_give(h[half], where))
    ref.remove(idx[half])
    _same_counters(cms, ref, np.int32)
    checks()
    assert cms.batch_diagnostics() == {"saturated": 0}


# ------------------------------------------------------------------ d: one block of 2^10 cells, pre-hashed
def _one_block(m, k, n, rng, block=None):
    """n rows whose probes all fall inside one aligned block of 2^10 cells (default: the last full one) + 200 rows spread over the table"""
    block = ((m >> 10) - 1) if block is None else block
    cells = (block << 10) + rng.integers(0, 1 << 10, size=(n, k))
    return np.concatenate([E.lift(cells, m, 11), _noise(rng, 200, k)])


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("geom", (E.BLOOM_2P28, E.BLOOM_NP2), ids=("2p28", "np2"))
def test_bloom_whole_batch_into_one_block(pa, N, geom, where):
    """200 000 keys aimed at 1024 bits: one slice takes every probe (segment overflow / spill), pass 2 walked by chunks and end to end"""
    rng = np.random.default_rng(21)
    tables = []
    for dense in (0, 1 << 30):
        N.set_option("dense_walk_groups", dense)
        blm = pa.BloomFilter(est_elements=geom[0], false_positive_rate=geom[1])
        m, k = blm.number_bits, blm.number_hashes
        if not tables:
            h = _one_block(m, k, 200_000, rng)
            idx = E.indices(h, m, k)
            probe = np.concatenate([h[::50], _one_block(m, k, 2000, rng), _one_block(m, k, 2000, rng, block=(m >> 10) - 2)])
            want = E.bloom_member(np.unique(idx), E.indices(probe, m, k))
            assert 0 < int(want.sum()) < want.size
        blm.add_alt_many(_give(h, where))
        assert torch.equal(blm.table_tensor, _expect_bits(blm.table_tensor, idx))
        assert blm.elements_added == h.shape[0]
        tables.append(blm)
    given = _give(probe, where)
    big = _give(np.concatenate([h, probe]), where)
    for scheme in (2, 0, 1, 3, 4):
        N.set_option("bloom_lookup", scheme)
        assert np.array_equal(_host(tables[0].check_alt_many(given)).astype(bool), want), scheme
        assert np.array_equal(_host(tables[1].check_alt_many(big)).astype(bool), np.concatenate([np.ones(h.shape[0], dtype=bool), want])), scheme


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("name,geom", CBF_CASES[1:3], ids=[c[0] for c in CBF_CASES[1:3]])
def test_cbf_whole_batch_into_one_block(pa, N, name, geom, where):
    cbf, ref = _cbf(pa, N, name, geom)
    m, k = cbf.number_bits, cbf.number_hashes
    rng = np.random.default_rng(22)
    h = _one_block(m, k, 200_000, rng)
    for w in (None, 3):
        cbf.add_alt_many(_give(h, where), None if w is None else _give(np.full(h.shape[0], w, dtype=np.uint32), where))
        ref.add(E.indices(h, m, k), 1 if w is None else w)
        _same_counters(cbf, ref, np.uint32)
    _check_cbf(cbf, ref, np.concatenate([h[::40], _one_block(m, k, 3000, rng, block=(m >> 10) - 2)]), where, k)


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("width,depth", E.CMS_SHAPES[2:])
def test_cms_whole_batch_into_one_block_per_row(pa, N, width, depth, where):
    cms = pa.CountMinSketch(width=width, depth=depth)
    ref = E.cms_counters(width, depth)
    rng = np.random.default_rng(23)
    h = _one_block(width, depth, 200_000, rng)
    idx = E.cms_indices(h, width, depth)
    w = rng.integers(0, 16, size=h.shape[0]).astype(np.int32)
    for wv in (None, w):
        cms.add_alt_many(_give(h, where), _give(wv, where))
        ref.add(idx, 1 if wv is None else wv)
        _same_counters(cms, ref, np.int32)
    probe = h[::40]
    got = _host(cms.check_alt_many(_give(probe, where))).astype(np.int64)
    assert np.array_equal(got, E.cms_query(ref.values(idx[::40]), "min", width, ref.els))


# ------------------------------------------------------------------ e: the running add, keys that collide in ONE row only
def _row_group(width, depth, shared_row, col, n, rng, seed):
    cols = np.stack([rng.permutation(width)[:n] for _ in range(depth)], axis=1)  # distinct columns in every row ...
    cols[:, shared_row] = col                                                   # ... but one: all n keys share it
    return E.lift(cols, width, seed)


_running_refs = {}


def _running_case(width, depth, variant, query):
    key = (width, depth, variant, query)
    if key not in _running_refs:
        rng = np.random.default_rng(depth * 7 + len(variant))
        if variant == "first":
            h, w = _row_group(width, depth, 0, width - 1, 5000, rng, 1), None
        elif variant == "last":
            h, w = _row_group(width, depth, depth - 1, 0, 5000, rng, 2), None
        else:  # two groups taking turns, weighted
            h = np.empty((5000, depth), dtype=np.uint64)
            h[0::2] = _row_group(width, depth, 0, width - 1, 2500, rng, 3)
            h[1::2] = _row_group(width, depth, depth - 1, (width - 1) >> 10 << 10, 2500, rng, 4)
            w = (1 + np.arange(5000) % 3).astype(np.int32)
        _running_refs[key] = (h, w, *E.cms_running(width, depth, h, w, query))
    return _running_refs[key]


@pytest.mark.parametrize("query", ("min", "mean", "mean-min"))
@pytest.mark.parametrize("variant", ("first", "last", "alternating"))
@pytest.mark.parametrize("width,depth", ((2**20, 5), (1_000_003, 5), (1_000_003, 8)))
def test_running_add_of_keys_that_share_one_row(pa, N, width, depth, variant, query):
    """5000 ordered adds that collide in one row (the first, the last) and nowhere else, and two such groups taking turns: every op's
    return value, the table and elements_added against the sequential loop"""
    h, w, want, bins, els = _running_case(width, depth, variant, query)
    nz = np.flatnonzero(bins)
    for where in WHERE:
        cms = pa.CountMinSketch(width=width, depth=depth)
        cms.query_type = query
        fast, seq = N.get_option("cms_running_fast"), N.get_option("cms_running_sequential")
        got = cms.add_alt_many_ordered(_give(h, where), _give(w, where))
        assert (N.get_option("cms_running_fast"), N.get_option("cms_running_sequential")) == (fast + 1, seq)  # the per-row segments, not the one-lane kernel
        assert _host(got).dtype == (np.int64 if query == "mean-min" else np.int32)
        assert np.array_equal(_host(got).astype(np.int64), want), where
        exp = torch.zeros_like(cms.table_tensor)
        exp[torch.from_numpy(nz).cuda()] = torch.from_numpy(bins[nz]).cuda()
        assert torch.equal(cms.table_tensor, exp)
        assert cms.elements_added == els


# ------------------------------------------------------------------ f: k + 3 columns, strided views, short matrices
def test_only_the_first_k_columns_count_and_short_matrices_are_refused(pa, N):
    rng = np.random.default_rng(31)
    blm = pa.BloomFilter(est_elements=E.BLOOM_NP2[0], false_positive_rate=E.BLOOM_NP2[1])
    cbf = pa.CountingBloomFilter(est_elements=E.CBF_SLICES32[0], false_positive_rate=E.CBF_SLICES32[1])
    width, depth = E.CMS_SHAPES[1]
    cms = pa.CountMinSketch(width=width, depth=depth)
    m, k = blm.number_bits, blm.number_hashes
    mc, kc = cbf.number_bits, cbf.number_hashes
    n = 3000

    def forms(mat, cols):
        """host, contiguous device tensor, and a strided device view of a wider matrix (which the Python layer copies into a contiguous
        tensor before the engine sees it: the engine itself reads whole rows of `cols` hashes, never strided ones)"""
        wider = np.concatenate([mat[:, :cols], _noise(rng, mat.shape[0], 5)], axis=1)
        return (mat[:, :cols], _dev(mat[:, :cols]), _dev(wider)[:, :cols])

    # Bloom: columns beyond k are ignored
    hb = _noise(rng, n, k + 3)
    hb[:500, :k] = np.resize(E.any_how(E.edge_cells(m), m, 1), (500, k))
    for i, given in enumerate(forms(hb, k + 3)):
        assert given.shape[1] == k + 3 and (i < 2 or not given.is_contiguous())
        blm.add_alt_many(given)
        assert torch.equal(blm.table_tensor, _expect_bits(blm.table_tensor, E.indices(hb, m, k)))
        probe = np.concatenate([hb, _noise(rng, 500, k + 3)])
        want = E.bloom_member(np.unique(E.indices(hb, m, k)), E.indices(probe, m, k))
        for pg in forms(probe, k + 3):
            assert np.array_equal(_host(blm.check_alt_many(pg)).astype(bool), want)
    # CountingBloom: add / remove take the first k; check takes the min over ALL supplied columns, as the reference's check_alt does
    hc = _noise(rng, n, kc + 3)
    hc[:500, :kc] = np.resize(E.any_how(E.edge_cells(mc)[1:], mc, 2), (500, kc))  # (cell 0 stays empty)
    ref = E.cbf_counters(mc)
    for given in forms(hc, kc + 3):
        cbf.add_alt_many(given, 2)
        ref.add(E.indices(hc, mc, kc), 2)
        _same_counters(cbf, ref, np.uint32)
    cbf.remove_alt_many(forms(hc, kc + 3)[2])
    ref.remove(E.indices(hc, mc, kc))
    _same_counters(cbf, ref, np.uint32)
    for cols in (kc + 3, kc, kc - 1, 1):  # (a short matrix is a shorter min: cell 0, empty here, is not probed in its place)
        for given in forms(hc, cols):
            got = _host(cbf.check_alt_many(given)).view(np.uint32)
            assert np.array_equal(got, ref.values(E.indices(hc, mc, cols)).min(axis=1).astype(np.uint32)), cols
    assert ref.exact[0] == 0 and int(_host(cbf.check_alt_many(hc[:, :1])).view(np.uint32).min()) >= 5
    # CountMinSketch: exactly `depth` columns (the reference walks ALL supplied hashes and runs off the table with more)
    hm = _noise(rng, n, depth + 3)
    hm[:500, :depth] = np.resize(E.any_how(E.edge_cells(width), width, 3), (500, depth))
    refm = E.cms_counters(width, depth)
    for given in forms(hm, depth):
        cms.add_alt_many(given, 3)
        refm.add(E.cms_indices(hm, width, depth), 3)
        _same_counters(cms, refm, np.int32)
        got = _host(cms.check_alt_many(given)).astype(np.int64)
        assert np.array_equal(got, E.cms_query(refm.values(E.cms_indices(hm, width, depth)), "min", width, refm.els))
    for given in forms(hm, depth + 3):
        for call in (cms.add_alt_many, cms.remove_alt_many, cms.check_alt_many, cms.add_alt_many_ordered):
            with pytest.raises(IndexError):
                call(given)
    # fewer than k columns: refused before anything runs
    for sk, mat, need, calls in ((blm, hb, k, ("add_alt_many", "check_alt_many")), (cbf, hc, kc, ("add_alt_many", "remove_alt_many")),
                                 (cms, hm, depth, ("add_alt_many", "remove_alt_many", "check_alt_many", "add_alt_many_ordered"))):
        for given in forms(mat, need - 1):
            for call in calls:
                with pytest.raises(ValueError):
                    getattr(sk, call)(given)
    assert torch.equal(blm.table_tensor, _expect_bits(blm.table_tensor, E.indices(hb, m, k)))
    _same_counters(cbf, ref, np.uint32)
    _same_counters(cms, refm, np.int32)
