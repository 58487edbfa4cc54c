"""BloomFilterBank: thousands of small Bloom filters of ONE geometry in one device table, built and queried a batch at a time.

Filter ``f`` of the bank is, byte for byte, the reference's ``BloomFilter(est_elements, false_positive_rate)`` after ``add()`` of the keys
sent to ``f`` (``probables/blooms/bloom.py:234-272``): one filter per row group, SSTable, shard, tenant or document, without one object,
one handle and one launch per filter.  Row ``f`` of :attr:`table_tensor` is that filter's bit array, padded to 16 bytes.

Two routes lead into the table (``include/psk.h``): *direct* -- every key carries a filter id, its k probes are atomics
into that row (``psk_bank_add``) -- and *grouped* -- the keys of a filter lie (or are sorted) together, one workgroup sets a filter's bits in
an LDS image of the row and ORs the image into the table once (``psk_bank_build``).

"Which filters may hold this key?" is answered from a second copy of the table, the *slice image*: the bank transposed (``psk_bank_slices``),
row ``p`` holding bit ``p`` of every filter.  All filters share the geometry and the hash family, so the answer for one key is the AND of
its k slice rows (``psk_bank_match``).  The image is allocated on the first match and refreshed lazily: updates only mark it stale.
A *query* -- a set of keys: the k-mers of a read, the terms of a document -- is scored against every filter by the same row-AND
(``psk_bank_score``: per filter, how many of the query's keys it may hold), and ``psk_bank_score_select`` keeps the filters at a threshold.

The filters as sets are read from the table alone: ``bits_set`` / ``estimate_elements`` (``psk_bank_popcount``), ``overlap`` /
``jaccard`` for all pairs of two lists of filters (``psk_bank_overlap``: a tiled GEMM over AND and popcount), and ``reduce``, the union or
intersection of groups of filters as a new bank (``psk_bank_reduce``).
"""

from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _native as N
from ._base import DeviceResident, _resolve_device, as_bool, require_device, result_buffer
from .bloom import BloomFilter
from .exceptions import NotSupportedError, SimilarityError
from .hashes import default_fnv_1a, device_digest, is_fused_fnv
from .keys import KeyBatch, hashed_batch, pack_hashes

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

# Device keys with ids take the grouped route (torch.sort of the ids + psk_bank_build) from this many keys on; None = never.  Measured
# (scripts/bench_bank.py part (b), profiles/bank_bench.txt: 4096 filters of 11 984 bytes, random ids, one MI355X): direct atomics win up to
# 2^20 keys (0.41 against 0.50 ms), sort + grouped from 2^21 on (0.60 against 0.69 ms; 2.3 x at 2^25).  What the sort buys is the LDS image:
# the automatic choice also wants a mean segment that takes it (`_grouped_pays`), else the grouped route would be the same atomics behind a sort.
BANK_GROUP_MIN_KEYS = 1 << 21
BANK_ROUTE_R = 16           # kBankRouteR of csrc/psk_bank.hip: route 0 takes the LDS image for a part with keys * k * R >= the row's words
BANK_LDS_ROW_BYTES = 65536  # rows beyond it never take the LDS image
BANK_MATCH_MAX_HASHES = 64  # psk_bank_match keeps a workgroup's k * 256 bit positions in LDS: 64 KiB at the cap
BANK_SLICE_MAX_GROUPS = 8   # more stale 32-filter column groups than this: the next match transposes the whole bank, not group by group
BANK_OVERLAP_T = 64         # kBankOvlT: psk_bank_overlap's workgroup owns a T x T tile of pairs ...
BANK_OVERLAP_C = 32         # kBankOvlC: ... and walks the rows in chunks of C words
BANK_GRID_CAP = 4096        # kBankGridCap: more rows (popcount), tiles (overlap) or row pieces (reduce) than this are walked with a stride
_ELEM = {N.KEYS_FIXED: 1, N.KEYS_VARLEN8: 1, N.KEYS_VARLEN32: 4, N.KEYS_HASHES: 8}


def group_ids(ids, num_filters: int):
    """ids[n] -> (perm uint32[n], seg uint64[num_filters + 1]): the keys of filter f, in their order of arrival, are perm[seg[f]:seg[f + 1]]
    (what ``psk_bank_build`` takes; the device route does the same with torch.sort + searchsorted).  An id outside [0, num_filters) raises."""
    a = np.asarray(ids)
    if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
        raise TypeError("ids must be a 1-D integer array")
    a = a.astype(np.int64, copy=False)
    if a.size and (int(a.min()) < 0 or int(a.max()) >= num_filters):
        raise ValueError(f"filter ids must lie in [0, {num_filters})")
    perm = np.argsort(a, kind="stable").astype(np.uint32)
    seg = np.zeros(num_filters + 1, dtype=np.uint64)
    np.cumsum(np.bincount(a, minlength=num_filters), out=seg[1:])
    return perm, seg


def score_thresholds(lengths, threshold) -> np.ndarray:
    """the per-query thresholds of ``score_many``: uint32[queries] for queries of ``lengths`` keys.  An ``int >= 1`` holds for every query; an
    integer array of ``queries`` values >= 1 gives each query its own; a ``float`` in (0, 1] is the COBS-style fraction of the query's keys,
    ``t_q = max(1, ceil(float64(threshold) * len_q))``.  Anything else raises ``TypeError`` / ``ValueError``.  Pure numpy: no GPU."""
    lengths = np.asarray(lengths)
    if lengths.ndim != 1 or (lengths.size and lengths.dtype.kind not in "iu"):
        raise TypeError("lengths must be a 1-D integer array")
    if isinstance(threshold, (bool, np.bool_)):
        raise TypeError("threshold must be an int, an integer array or a float, not a bool")
    if isinstance(threshold, (int, np.integer)):
        if not 1 <= int(threshold) < 2**32:
            raise ValueError("an integer threshold must lie in [1, 2^32)")
        return np.full(lengths.size, int(threshold), dtype=np.uint32)
    if isinstance(threshold, (float, np.floating)):
        if not 0.0 < float(threshold) <= 1.0:  # (NaN fails both comparisons)
            raise ValueError("a fractional threshold must lie in (0, 1]")
        t = np.ceil(np.float64(threshold) * lengths.astype(np.float64))
        return np.maximum(t, 1.0).astype(np.uint32)
    if torch is not None and isinstance(threshold, torch.Tensor):
        threshold = threshold.cpu().numpy()
    if isinstance(threshold, (str, bytes)) or not isinstance(threshold, (np.ndarray, list, tuple)):
        raise TypeError("threshold must be an int, an integer array or a float")
    a = np.asarray(threshold)
    if a.size == 0 and a.ndim == 1:  # (an empty list has no integer dtype of its own)
        a = a.astype(np.int64)
    if a.dtype.kind not in "iu" or a.ndim != 1:
        raise TypeError("per-query thresholds must be a 1-D integer array")
    if a.size != lengths.size:
        raise ValueError(f"per-query thresholds: {a.size} values for {lengths.size} queries")
    if a.size and (int(a.min()) < 1 or int(a.max()) >= 2**32):
        raise ValueError("per-query thresholds must lie in [1, 2^32)")
    return a.astype(np.uint32)


def _slice_batch(b: KeyBatch, lo: int, hi: int) -> KeyBatch:
    """keys [lo, hi) of a batch, without copying the keys"""
    if lo == 0 and hi == b.n:
        return b
    if b.layout in (N.KEYS_FIXED, N.KEYS_HASHES):
        stride = b.key_len * _ELEM[b.layout]
        return KeyBatch(b.layout, b.data + lo * stride if b.data else 0, 0, hi - lo, b.key_len, b.where, b.device, b.keep)
    if b.where == N.DEVICE:  # device offsets are positions in the blob: they need not start at 0
        return KeyBatch(b.layout, b.data, b.offsets + 8 * lo, hi - lo, 0, b.where, b.device, b.keep)
    offs = np.ctypeslib.as_array((C.c_uint64 * (b.n + 1)).from_address(b.offsets))
    o = offs[lo:hi + 1] - offs[lo]  # host blobs are staged from their first element
    return KeyBatch(b.layout, b.data + int(offs[lo]) * _ELEM[b.layout], o.ctypes.data, hi - lo, 0, b.where, b.device, [*b.keep, o])


class RowBank(DeviceResident):
    """what the banks share (BloomFilterBank here, CountMinSketchBank in cmsbank.py): ``_num_rows`` rows of one geometry in one device table, row
    ids and row offsets that arrive as arrays or tensors on either side, and the split of a grouped build.  A subclass sets ``_ROW`` (what the
    messages call a row), ``_num_rows``, ``_device``, ``_cus`` and ``_split``."""

    _NOUN = "bank"
    _ROW = "row"

    def _index(self, f) -> int:
        f = int(f)
        if not 0 <= f < self._num_rows:
            raise IndexError(f"{self._ROW} {f} out of range [0, {self._num_rows})")
        return f

    def _ids(self, ids, n: int, where: int, validate: bool):
        """-> the ids where the keys are: an int64 numpy array (host keys) or an int64 tensor (device keys), checked"""
        is_dev = torch is not None and isinstance(ids, torch.Tensor) and ids.is_cuda
        if is_dev:
            if ids.dim() != 1 or ids.is_floating_point() or ids.dtype == torch.bool:
                raise TypeError("ids must be a 1-D integer tensor")
            if ids.numel() != n:
                raise ValueError("ids length differs from the number of keys")
            if ids.device.index != self._device:
                raise ValueError(f"ids live on cuda:{ids.device.index}, the bank on cuda:{self._device}")
            if validate and n:  # one reduction, one synchronisation
                lo, hi = torch.aminmax(ids)
                if int(lo.item()) < 0 or int(hi.item()) >= self._num_rows:
                    raise ValueError(f"{self._ROW} ids must lie in [0, {self._num_rows})")
            return ids.to(torch.int64) if where == N.DEVICE else ids.cpu().numpy().astype(np.int64)
        a = ids.numpy() if torch is not None and isinstance(ids, torch.Tensor) else np.asarray(ids)
        if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
            raise TypeError("ids must be a 1-D integer array")
        if a.size != n:
            raise ValueError("ids length differs from the number of keys")
        a = a.astype(np.int64, copy=False)
        if a.size and (int(a.min()) < 0 or int(a.max()) >= self._num_rows):  # host ids are always checked
            raise ValueError(f"{self._ROW} ids must lie in [0, {self._num_rows})")
        return torch.from_numpy(np.ascontiguousarray(a)).to(self._dev) if where == N.DEVICE else a

    def _offsets(self, offs, n: int, where: int, validate: bool, count=None, what: str = "filter_offsets"):
        """offsets[count + 1] (filter_offsets / sketch_offsets: count = the bank's rows; query_offsets: any count >= 0, None) -> as _ids: where the keys are, checked
        (non-decreasing, from 0 to n)"""
        is_dev = torch is not None and isinstance(offs, torch.Tensor) and offs.is_cuda
        want = f"{count + 1} integers" if count is not None else "a 1-D integer array of queries + 1 entries"
        size = int(offs.numel()) if torch is not None and isinstance(offs, torch.Tensor) else None
        if is_dev:
            if offs.dim() != 1 or size < 1 or (count is not None and size != count + 1) or offs.is_floating_point() or offs.dtype == torch.bool:
                raise TypeError(f"{what} must be {want}")
            if offs.device.index != self._device:
                raise ValueError(f"{what} live on cuda:{offs.device.index}, the bank on cuda:{self._device}")
            o = offs.to(torch.int64).contiguous()
            if validate:  # one reduction, one synchronisation
                bad = (o[1:] < o[:-1]).any() | (o[0] != 0) | (o[-1] != n)
                if bool(bad.item()):
                    raise ValueError(f"{what} must be non-decreasing, start at 0 and end at the number of keys")
            return o if where == N.DEVICE else o.cpu().numpy()
        a = offs.numpy() if torch is not None and isinstance(offs, torch.Tensor) else np.asarray(offs)
        if a.ndim != 1 or a.size < 1 or (count is not None and a.size != count + 1) or a.dtype.kind not in "iu":
            raise TypeError(f"{what} must be {want}")
        a = np.ascontiguousarray(a.astype(np.int64, copy=False))
        if (np.diff(a) < 0).any() or int(a[0]) != 0 or int(a[-1]) != n:
            raise ValueError(f"{what} must be non-decreasing, start at 0 and end at the number of keys")
        return torch.from_numpy(a).to(self._dev) if where == N.DEVICE else a

    @staticmethod
    def _addr(x) -> int:
        if isinstance(x, np.ndarray):
            return x.ctypes.data if x.size else 0
        return x.data_ptr() if x.numel() else 0

    def _ids_u32(self, ids):
        """int64 ids -> the uint32 words the engine reads (fewer than 2^31 rows: the low word)"""
        if isinstance(ids, np.ndarray):
            return np.ascontiguousarray(ids.astype(np.uint32))
        return ids.to(torch.int32).contiguous()

    def split_for(self) -> int:
        """workgroups per row of a grouped build: 1 unless the bank has fewer than twice as many rows as the device has CUs"""
        if self._split is not None:
            return int(self._split)
        return 1 if self._num_rows >= 2 * self._cus else -(-2 * self._cus // self._num_rows)


class BloomFilterBank(RowBank):
    """``num_filters`` Bloom filters sized by ``(est_elements, false_positive_rate)`` as the reference sizes one (bloom.py:463-502).

    Keys are accepted as everywhere in the package (lists of ``str`` / ``bytes``, ``(n, L)`` uint8 arrays or tensors, ragged
    ``(blob, offsets)``); ``ids`` / ``filter_offsets`` are integer arrays or tensors, host or device.  A non-default ``hash_function`` is
    evaluated on the host (the digest families on the device) and travels as pre-computed hashes, as in :class:`BloomFilter`."""

    _CHUNK = 2**32 - 1  # keys per engine call
    _ROW = "filter"
    _num_rows = property(lambda self: self._num_filters)

    def __init__(self, num_filters, est_elements, false_positive_rate, hash_function=None, device=None):
        if not (isinstance(num_filters, (int, np.integer)) and 0 < int(num_filters) < 2**31):
            raise ValueError("num_filters must be an integer in [1, 2^31)")
        L = N.lib()
        self._fpr, self._number_hashes, self._num_bits = BloomFilter._get_optimized_params(est_elements, false_positive_rate)
        if self._num_bits > 2**31:
            raise ValueError("a bank's filters hold at most 2^31 bits each: use BloomFilter for big tables")
        self._est_elements = est_elements
        self._num_filters = int(num_filters)
        self._hash_arg = hash_function
        self._hash_func = default_fnv_1a if hash_function is None else hash_function
        self._is_fused = is_fused_fnv(hash_function)
        self._digest = device_digest(self._hash_func)
        self._row_bytes = int(L.psk_bank_row_bytes(self._num_bits))
        require_device("the bank's table lives in GPU memory")
        self._device = _resolve_device(device)
        self._table = torch.zeros(self._num_filters * (self._row_bytes // 4), dtype=torch.int32, device=self._dev)
        self._els = torch.zeros(self._num_filters, dtype=torch.int64, device=self._dev)
        self._cus = int(torch.cuda.get_device_properties(self._device).multi_processor_count)
        self._add_policy = "auto"  # "auto" | "direct" | "grouped" (tests force each)
        self._route = 0            # psk_bank_build's route: 0 auto per workgroup, 1 LDS image, 2 global atomics
        self._last_path = None     # "direct" / "grouped": the way the last update took
        self._split = None         # workgroups per filter; None: 1, or ceil(2 * CUs / num_filters) for a bank of fewer than 2 * CUs filters
        self._score_split = None   # workgroups per query of a score call; None: 1, or ceil(2 * CUs / queries) for fewer than 2 * CUs queries
        self._slice_row_bytes = int(L.psk_bank_slice_row_bytes(self._num_filters))
        self._slices = None        # the slice image (match_many), allocated on the first match
        self._stale_all = True     # the image lags behind the table: everywhere / in these 32-filter column groups
        self._stale_groups = set()
        self._last_refresh = None  # the (first, last) filter spans of the last refresh (tests)

    # ------------------------------------------------------------------ properties
    num_filters = property(lambda self: self._num_filters)
    number_bits = property(lambda self: self._num_bits)
    number_hashes = property(lambda self: self._number_hashes)
    row_bytes = property(lambda self: self._row_bytes)
    estimated_elements = property(lambda self: self._est_elements)
    false_positive_rate = property(lambda self: self._fpr)
    hash_function = property(lambda self: self._hash_func)

    @property
    def table_tensor(self):
        """the int32 tensor [num_filters, row_bytes / 4] backing the bank (a view: writes through it are the caller's business)"""
        return self._table.view(self._num_filters, self._row_bytes // 4)

    @property
    def elements_added(self) -> np.ndarray:
        """int64 per filter: the number of keys sent there, repeats counted (bloom.py:239)"""
        return self._els.cpu().numpy()

    def clear(self, f=None) -> None:
        """empty filter ``f``, or every filter"""
        if f is None:
            self._table.zero_()
            self._els.zero_()
            self._mark_stale()
        else:
            self.table_tensor[self._index(f)].zero_()
            self._els[self._index(f)] = 0
            self._mark_stale(self._index(f))

    # ------------------------------------------------------------------ batches, ids, offsets
    def _batch(self, keys) -> KeyBatch:
        return self._same_device(hashed_batch(keys, self._hash_func, self._is_fused, self._digest, self._number_hashes, self._device, self._stream))

    def _grouped_pays(self, n: int) -> bool:
        """the automatic choice for device keys with ids: sort + grouped build from BANK_GROUP_MIN_KEYS keys on, where a filter's mean share of
        the batch is a segment that route 0 gives the LDS image (and the row fits it)"""
        if BANK_GROUP_MIN_KEYS is None or n < BANK_GROUP_MIN_KEYS or self._row_bytes > BANK_LDS_ROW_BYTES:
            return False
        return n * self._number_hashes * BANK_ROUTE_R >= self._num_filters * (self._row_bytes // 4)

    # ------------------------------------------------------------------ updates
    def _add_direct(self, b: KeyBatch, ids) -> None:
        self._last_path = "direct"
        self._mark_stale()
        L = N.lib()
        for lo in range(0, b.n, self._CHUNK):
            hi = min(b.n, lo + self._CHUNK)
            c, w = _slice_batch(b, lo, hi), self._ids_u32(ids[lo:hi])
            N.check(L.psk_bank_add(self._table.data_ptr(), self._num_filters, self._num_bits, self._number_hashes, *c.args(), c.where,
                                   self._addr(w) or None, self._device, self._stream))

    def _build(self, b: KeyBatch, seg, perm) -> None:
        """seg int64[F + 1] on the device (positions in perm, or in the batch when perm is None), perm int32[n] on the device or None"""
        self._last_path = "grouped"
        self._mark_stale()
        L = N.lib()
        if b.n > self._CHUNK:
            raise ValueError("a grouped call takes fewer than 2^32 keys")
        N.check(L.psk_bank_build(self._table.data_ptr(), self._num_filters, self._num_bits, self._number_hashes, *b.args(), seg.data_ptr(),
                                 perm.data_ptr() if perm is not None else None, self.split_for(), int(self._route), self._device, self._stream))

    def _add_batch(self, b: KeyBatch, ids, filter_offsets, validate: bool) -> None:
        if (ids is None) == (filter_offsets is None):
            raise TypeError("pass either ids or filter_offsets")
        if self._add_policy not in ("auto", "direct", "grouped"):
            raise ValueError(f"unknown _add_policy {self._add_policy!r}")
        F = self._num_filters
        if filter_offsets is not None:
            offs = self._offsets(filter_offsets, b.n, b.where, validate, self._num_filters)
            if b.n == 0:
                return
            if b.where == N.DEVICE and self._add_policy != "direct":  # keys that arrive grouped: the build kernel as they lie
                self._build(b, offs, None)
            elif b.where == N.DEVICE:
                self._add_direct(b, torch.repeat_interleave(torch.arange(F, device=self._dev), offs[1:] - offs[:-1]))
            else:  # host keys always go direct
                self._add_direct(b, np.repeat(np.arange(F, dtype=np.int64), np.diff(offs)))
            counts = offs[1:] - offs[:-1]
            self._els += counts if b.where == N.DEVICE else torch.from_numpy(np.ascontiguousarray(counts)).to(self._dev)
            return
        idv = self._ids(ids, b.n, b.where, validate)
        if b.n == 0:
            return
        grouped = b.where == N.DEVICE and b.n <= self._CHUNK and (
            self._add_policy == "grouped" or (self._add_policy == "auto" and self._grouped_pays(b.n)))
        if b.where == N.HOST:
            self._add_direct(b, idv)
            self._els += torch.from_numpy(np.bincount(idv, minlength=F).astype(np.int64)).to(self._dev)
            return
        if not validate:  # unchecked device ids: the engine skips ids >= num_filters, the counts must skip them too
            counts = torch.bincount(torch.where((idv < 0) | (idv >= F), F, idv), minlength=F + 1)[:F]
        else:
            counts = torch.bincount(idv, minlength=F)
        if grouped:
            srt, perm = torch.sort(idv, stable=True)
            seg = torch.searchsorted(srt, torch.arange(F + 1, device=self._dev, dtype=torch.int64))
            self._build(b, seg.contiguous(), perm.to(torch.int32).contiguous())
        else:
            self._add_direct(b, idv)
        self._els += counts

    def add_many(self, keys, ids=None, filter_offsets=None, validate: bool = True) -> None:
        """filter ``ids[i]`` gets key ``i`` -- or, for keys that are already grouped by filter, filter ``f`` gets keys
        ``filter_offsets[f]:filter_offsets[f + 1]``.  An id outside the bank raises ``ValueError`` before anything is launched; device ids /
        offsets are checked with one reduction and one synchronisation unless ``validate=False`` (then an id beyond the bank is skipped)."""
        self._add_batch(self._batch(keys), ids, filter_offsets, validate)

    def add_alt_many(self, hashes, ids=None, filter_offsets=None, validate: bool = True) -> None:
        """:meth:`add_many` for pre-computed hashes: (n, >= k) uint64"""
        self._add_batch(self._same_device(pack_hashes(hashes, self._number_hashes)), ids, filter_offsets, validate)

    # ------------------------------------------------------------------ lookups
    def _check_batch(self, b: KeyBatch, ids, validate: bool):
        idv = self._ids(ids, b.n, b.where, validate)
        L = N.lib()
        out = result_buffer(b.where, b.n, np.uint8, torch.uint8, self._device)[1]()
        for lo in range(0, b.n, self._CHUNK):  # (n = 0 launches nothing)
            hi = min(b.n, lo + self._CHUNK)
            c, w = _slice_batch(b, lo, hi), self._ids_u32(idv[lo:hi])
            N.check(L.psk_bank_check(self._table.data_ptr(), self._num_filters, self._num_bits, self._number_hashes, *c.args(), c.where,
                                     self._addr(w) or None, self._addr(out[lo:hi]) or None, self._device, self._stream))
        return as_bool(out)

    def check_many(self, keys, ids, validate: bool = True):
        """``key_i in filter ids[i]`` for every key: numpy bool[n] for host keys, torch.bool on the device for device keys"""
        return self._check_batch(self._batch(keys), ids, validate)

    def check_alt_many(self, hashes, ids, validate: bool = True):
        return self._check_batch(self._same_device(pack_hashes(hashes, self._number_hashes)), ids, validate)

    # ------------------------------------------------------------------ which filters may hold a key: the slice image
    @property
    def slice_row_bytes(self) -> int:
        """bytes of one row of the slice image: ceil(num_filters / 8) rounded up to 16"""
        return self._slice_row_bytes

    @property
    def slice_tensor(self):
        """the int32 tensor [number_bits, slice_row_bytes / 4] of the slice image (row p holds bit p of every filter), or None before the
        first match; it may be stale: :meth:`refresh_slices` brings it up to date"""
        return None if self._slices is None else self._slices.view(self._num_bits, self._slice_row_bytes // 4)

    def drop_slices(self) -> None:
        """free the slice image; the next match builds it again"""
        self._slices = None
        self._mark_stale()

    def invalidate_slices(self) -> None:
        """for callers who wrote through :attr:`table_tensor`: the next match transposes the whole bank again"""
        self._mark_stale()

    def _mark_stale(self, f=None) -> None:
        """a host flag, no launch: every column of the image (f is None) or the 32-filter column group of filter f is out of date"""
        if f is None:
            self._stale_all = True
            self._stale_groups.clear()
        elif not self._stale_all:
            self._stale_groups.add(int(f) >> 5)
            if len(self._stale_groups) > BANK_SLICE_MAX_GROUPS:
                self._mark_stale()

    def refresh_slices(self) -> None:
        """bring the slice image up to date now (allocating it if need be): the whole bank, or one ranged transpose per stale column group"""
        if self._slices is None:
            self._slices = torch.zeros(self._num_bits * (self._slice_row_bytes // 4), dtype=torch.int32, device=self._dev)
            self._stale_all = True
        L, F = N.lib(), self._num_filters
        spans = [(0, F)] if self._stale_all else [(32 * g, min(32 * g + 32, F)) for g in sorted(self._stale_groups)]
        for lo, hi in spans:
            N.check(L.psk_bank_slices(self._table.data_ptr(), F, self._num_bits, self._slices.data_ptr(), lo, hi, self._device, self._stream))
        self._last_refresh = spans
        self._stale_all = False
        self._stale_groups.clear()

    def _image_ready(self, b: KeyBatch, what: str) -> None:
        """in front of every call that reads the slice image (match, score): the cap on k, the batch size, and the lazy refresh"""
        if self._number_hashes > BANK_MATCH_MAX_HASHES:
            raise NotSupportedError(f"{what}_many takes filters of at most {BANK_MATCH_MAX_HASHES} hashes (this bank has {self._number_hashes}): "
                                    "use check_many(keys, ids) with the filter ids spelled out")
        if b.n > self._CHUNK:
            raise ValueError(f"a {what} call takes fewer than 2^32 keys")
        if self._stale_all or self._stale_groups or self._slices is None:
            self.refresh_slices()

    def _match_batch(self, b: KeyBatch, form: str):
        if form not in ("mask", "count", "ids"):
            raise ValueError(f"form must be 'mask', 'count' or 'ids', not {form!r}")
        self._image_ready(b, "match")
        L, n, words = N.lib(), b.n, self._slice_row_bytes // 4
        host = b.where == N.HOST

        def call(mask=None, count=None, offs=None, ids=None):
            if n:
                N.check(L.psk_bank_match(self._slices.data_ptr(), self._num_filters, self._num_bits, self._number_hashes, *b.args(), b.where,
                                         *(None if t is None else t.data_ptr() for t in (mask, count, offs, ids)), self._device, self._stream))

        if form == "mask":
            mask = torch.empty((n, words), dtype=torch.int32, device=self._dev)
            call(mask=mask)
            return mask.cpu().numpy().view(np.uint32) if host else mask
        count = torch.empty(n, dtype=torch.int32, device=self._dev)
        call(count=count)
        if form == "count":
            return count.cpu().numpy() if host else count
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=self._dev)
        torch.cumsum(count, 0, out=offsets[1:])
        ids = torch.empty(int(offsets[-1].item()), dtype=torch.int32, device=self._dev)
        if ids.numel():
            call(offs=offsets, ids=ids)
        return (offsets.cpu().numpy(), ids.cpu().numpy()) if host else (offsets, ids)

    def match_many(self, keys, form: str = "mask"):
        """every filter that may hold each key (``key in filter f`` of bloom.py:261-272 for all f at once), read from the slice image.
        ``form="mask"``: int32 [n, slice_row_bytes / 4], bit ``f & 31`` of word ``f >> 5`` of row i is set when filter f may hold key i;
        ``"count"``: int32 [n], the number of such filters; ``"ids"``: ``(offsets int64[n + 1], ids int32[total])``, the filters of key i are
        ``ids[offsets[i]:offsets[i + 1]]``, ascending.  Device keys give tensors on the device, host keys numpy arrays (the mask as uint32)."""
        return self._match_batch(self._batch(keys), form)

    def match_alt_many(self, hashes, form: str = "mask"):
        """:meth:`match_many` for pre-computed hashes: (n, >= k) uint64"""
        return self._match_batch(self._same_device(pack_hashes(hashes, self._number_hashes)), form)

    def match(self, key) -> list:
        """the ids of the filters that may hold ``key``, ascending"""
        b = self._batch(key)
        if b.n != 1:
            raise TypeError("match takes one key; use match_many for a batch")
        _, ids = self._match_batch(b, "ids")
        return [int(f) for f in (ids if isinstance(ids, np.ndarray) else ids.cpu().numpy())]

    # ------------------------------------------------------------------ scoring a query: how many of its keys each filter may hold
    def score_split_for(self, queries: int) -> int:
        """workgroups per query of a score call: 1 unless there are fewer than twice as many queries as the device has CUs (the rule of
        :meth:`split_for`; ``_score_split`` overrides it).  Not measured: no run has compared splits yet."""
        if self._score_split is not None:
            return int(self._score_split)
        return 1 if queries == 0 or queries >= 2 * self._cus else -(-2 * self._cus // queries)

    def _score_batch(self, b: KeyBatch, query_offsets, threshold, validate: bool):
        qo = self._offsets(query_offsets, b.n, N.DEVICE, validate, None, "query_offsets")
        L, F, Q, host = N.lib(), self._num_filters, int(qo.numel()) - 1, b.where == N.HOST
        thr = None
        if threshold is not None:  # (offsets and thresholds are refused before the image is touched)
            fraction = isinstance(threshold, (float, np.floating))
            lengths = (qo[1:] - qo[:-1]).cpu().numpy() if fraction else np.zeros(Q, dtype=np.int64)
            thr = torch.from_numpy(score_thresholds(lengths, threshold).view(np.int32)).to(self._dev)
        self._image_ready(b, "score")
        scores = torch.empty((Q, F), dtype=torch.int32, device=self._dev)
        if Q:
            N.check(L.psk_bank_score(self._slices.data_ptr(), F, self._num_bits, self._number_hashes, *b.args(), b.where, qo.data_ptr(), Q,
                                     self.score_split_for(Q), scores.data_ptr(), self._device, self._stream))
        if thr is None:
            return scores.cpu().numpy() if host else scores

        def select(count=None, offs=None, ids=None, hit=None):
            if Q:
                N.check(L.psk_bank_score_select(scores.data_ptr(), Q, F, thr.data_ptr(), *(None if t is None else t.data_ptr() for t in (count, offs, ids, hit)),
                                                self._device, self._stream))

        count = torch.empty(Q, dtype=torch.int32, device=self._dev)
        select(count=count)
        offsets = torch.zeros(Q + 1, dtype=torch.int64, device=self._dev)
        torch.cumsum(count, 0, out=offsets[1:])
        total = int(offsets[-1].item())
        ids, hit = (torch.empty(total, dtype=torch.int32, device=self._dev) for _ in range(2))
        if total:
            select(offs=offsets, ids=ids, hit=hit)
        return tuple(t.cpu().numpy() for t in (offsets, ids, hit)) if host else (offsets, ids, hit)

    def score_many(self, keys, query_offsets, threshold=None, validate: bool = True):
        """whole queries against every filter: query q is ``keys[query_offsets[q]:query_offsets[q + 1]]`` (``query_offsets``: ``queries + 1``
        integers, host or device, non-decreasing from 0 to n; host arrays are always checked, device tensors with one reduction unless
        ``validate=False``), and ``score[q, f]`` is the number of its keys that filter f may hold -- the sum over the query of
        ``key in filter f`` (bloom.py:261-272), a repeated key counted each time.  The per-key mask of :meth:`match_many` is never written.
        ``threshold=None``: int32 ``[queries, num_filters]``.  With a threshold (see :func:`score_thresholds`: an int, one int per query, or a
        fraction of each query's length): ``(offsets int64[queries + 1], ids int32[total], scores int32[total])``, the filters of query q with
        ``score >= t_q`` are ``ids[offsets[q]:offsets[q + 1]]``, ascending, their scores beside them.  Device keys give tensors on the device,
        host keys numpy arrays.  Nothing here changes the table or marks the slice image stale."""
        return self._score_batch(self._batch(keys), query_offsets, threshold, validate)

    def score_alt_many(self, hashes, query_offsets, threshold=None, validate: bool = True):
        """:meth:`score_many` for pre-computed hashes: (n, >= k) uint64"""
        return self._score_batch(self._same_device(pack_hashes(hashes, self._number_hashes)), query_offsets, threshold, validate)

    def score(self, keys, threshold=None):
        """one query made of all the keys: numpy int32[num_filters], or with a threshold ``(ids, scores)`` as numpy arrays"""
        b = self._batch(keys)
        r = self._score_batch(b, np.array([0, b.n], dtype=np.int64), threshold, True)
        if threshold is None:
            return (r if isinstance(r, np.ndarray) else r.cpu().numpy())[0]
        return tuple(x if isinstance(x, np.ndarray) else x.cpu().numpy() for x in r[1:])

    # ------------------------------------------------------------------ the filters as sets: bit counts, estimates, overlap, folds
    def _rows(self, ids, validate: bool, what: str = "ids"):
        """a list of this bank's filters -> (n, int32 device tensor, or None for "every filter"), checked as `_ids` checks"""
        if ids is None:
            return self._num_filters, None
        is_dev = torch is not None and isinstance(ids, torch.Tensor) and ids.is_cuda
        n = int(ids.numel()) if torch is not None and isinstance(ids, torch.Tensor) else int(np.asarray(ids).size)
        if n >= 2**32:
            raise ValueError(f"{what} names 2^32 filters or more")
        return n, self._ids_u32(self._ids(ids, n, N.DEVICE, validate if is_dev else True))

    def _bits(self, rows, n: int):
        out = torch.empty(n, dtype=torch.int64, device=self._dev)
        if n == 0:
            return out
        N.check(N.lib().psk_bank_popcount(self._table.data_ptr(), self._num_filters, self._num_bits, None if rows is None else self._addr(rows) or None, n,
                                          self._addr(out) or None, self._device, self._stream))
        return out

    def bits_set(self, ids=None, validate: bool = True):
        """torch.int64[n] on the device: the number of set bits of filters ``ids`` (``None``: of every filter)"""
        n, rows = self._rows(ids, validate)
        return self._bits(rows, n)

    def _estimates(self, bits: np.ndarray) -> np.ndarray:
        """bloom.py:340-352 for each bit count: math.log on the host, once per distinct count (a vector log one ulp off could move the truncation)"""
        m, k = self._num_bits, self._number_hashes
        vals, inv = np.unique(bits, return_inverse=True)
        est = [-1 if int(c) >= m else int(-1 * (float(m) / float(k)) * math.log(1 - (float(int(c)) / float(m)))) for c in vals]
        return np.array(est, dtype=np.int64)[inv].reshape(bits.shape)

    def estimate_elements(self, ids=None, validate: bool = True) -> np.ndarray:
        """numpy int64[n]: entry i is ``bank.filter(ids[i]).estimate_elements()`` (bloom.py:340-352), -1 for a filter with every bit set"""
        return self._estimates(self.bits_set(ids, validate).cpu().numpy())

    def current_false_positive_rate(self) -> np.ndarray:
        """numpy float64[num_filters]: bloom.py:361-369 from each filter's ``elements_added``"""
        m, k = self._num_bits, self._number_hashes
        vals, inv = np.unique(self.elements_added, return_inverse=True)
        return np.array([math.pow((1 - math.exp(k * -1 * int(e) / m)), k) for e in vals], dtype=np.float64)[inv]

    def _similar(self, other):
        if other is None or other is self:
            return self
        if not isinstance(other, BloomFilterBank):
            raise TypeError("other must be a BloomFilterBank")
        if other._num_bits != self._num_bits or other._number_hashes != self._number_hashes or \
                list(other._hash_func("test", self._number_hashes)) != list(self._hash_func("test", self._number_hashes)):
            raise SimilarityError("the other bank's geometry or hash function differs from this bank's")
        if other._device != self._device:
            raise ValueError(f"the other bank lives on cuda:{other._device}, this bank on cuda:{self._device}")
        return other

    def _overlap(self, other, a, b, validate: bool):
        """-> (other, rows a, rows b, int32[na, nb] counts); the symmetric case (one bank, one list) computes the upper triangle only"""
        other = self._similar(other)
        if self._num_bits >= 2**31:
            raise NotSupportedError("overlap counts of filters of 2^31 bits do not fit the int32 tensor: call psk_bank_overlap with a uint32 buffer")
        na, ra = self._rows(a, validate, "a")
        if other is self and (b is a):
            nb, rb = na, ra
        else:
            nb, rb = other._rows(b, validate, "b")
        out = torch.empty((na, nb), dtype=torch.int32, device=self._dev)
        if na and nb:
            # (NULL lists take rows 0 .. n - 1: n == num_filters here)
            N.check(N.lib().psk_bank_overlap(self._table.data_ptr(), self._num_filters, None if ra is None else ra.data_ptr(), na, other._table.data_ptr(),
                                             other._num_filters, None if rb is None else rb.data_ptr(), nb, self._num_bits, out.data_ptr(), self._device,
                                             self._stream))
        return other, (na, ra), (nb, rb), out

    def overlap(self, other=None, a=None, b=None, validate: bool = True):
        """torch.int32[na, nb] on the device: entry (i, j) is the number of bits set in both filter ``a[i]`` of this bank and filter ``b[j]`` of
        ``other`` (``None``: this bank; ``a`` / ``b`` of ``None``: every filter) -- ``count_int`` of bloom.py:448-457 for every pair at once.
        ``other`` must share the geometry and the hash function (else ``SimilarityError``) and the device (else ``ValueError``)."""
        return self._overlap(other, a, b, validate)[3]

    def jaccard(self, other=None, a=None, b=None, validate: bool = True):
        """torch.float64[na, nb] on the device: ``blm[a[i]].jaccard_index(blm[b[j]])`` (bloom.py:430-460) for every pair, bit for bit -- the
        correctly rounded quotient of the same two integers, 1.0 where the union is empty"""
        other, (na, ra), (nb, rb), inter = self._overlap(other, a, b, validate)
        inter = inter.to(torch.int64)
        ca = self._bits(ra, na)
        cb = ca if (other is self and rb is ra and nb == na) else other._bits(rb, nb)
        union = ca[:, None] + cb[None, :] - inter
        return torch.where(union == 0, torch.ones((), dtype=torch.float64, device=self._dev), inter.to(torch.float64) / union.to(torch.float64).clamp_(min=1.0))

    def reduce(self, groups, op: str = "or", validate: bool = True):
        """a new bank of G filters (same geometry, hash function and device): filter g is the chained ``union`` (``op="or"``, bloom.py:401-428) or
        ``intersection`` (``"and"``, bloom.py:371-399) of this bank's filters ``groups[g]``.  ``groups``: a list of lists of filter ids, or
        ``(offsets[G + 1], members[total])`` arrays or tensors.  ``elements_added[g]`` of the new bank is ``estimate_elements()`` of its row (-1
        for a full row), as the reference's union / intersection leave it.  An empty group gives an empty filter under ``"or"`` and raises
        ``ValueError`` under ``"and"`` (unchecked device offsets: the zero row)."""
        if op not in ("or", "and"):
            raise ValueError(f"op must be 'or' or 'and', not {op!r}")
        if isinstance(groups, tuple) and len(groups) == 2:
            offs, members = groups
        else:
            groups = [np.asarray(g, dtype=np.int64).reshape(-1) if len(g) else np.zeros(0, dtype=np.int64) for g in groups]
            offs = np.zeros(len(groups) + 1, dtype=np.int64)
            np.cumsum([g.size for g in groups], out=offs[1:])
            members = np.concatenate(groups) if groups else np.zeros(0, dtype=np.int64)
        offs_dev = torch is not None and isinstance(offs, torch.Tensor) and offs.is_cuda
        if offs_dev:
            if offs.dim() != 1 or offs.numel() < 1 or offs.is_floating_point() or offs.dtype == torch.bool:
                raise TypeError("group offsets must be a 1-D integer tensor of G + 1 entries")
            if offs.device.index != self._device:
                raise ValueError(f"group offsets live on cuda:{offs.device.index}, the bank on cuda:{self._device}")
            seg = offs.to(torch.int64).contiguous()
            total = int(members.numel()) if isinstance(members, torch.Tensor) else int(np.asarray(members).size)
            if validate:  # one reduction, one synchronisation
                bad = (seg[1:] < seg[:-1]).any() | (seg[0] != 0) | (seg[-1] != total)
                empty = (seg[1:] == seg[:-1]).any()
                bad, empty = bool(bad.item()), bool(empty.item())
        else:
            o = offs.numpy() if torch is not None and isinstance(offs, torch.Tensor) else np.asarray(offs)
            if o.ndim != 1 or o.size < 1 or o.dtype.kind not in "iu":
                raise TypeError("group offsets must be a 1-D integer array of G + 1 entries")
            o = np.ascontiguousarray(o.astype(np.int64, copy=False))
            total = int(members.numel()) if torch is not None and isinstance(members, torch.Tensor) else int(np.asarray(members).size)
            bad = bool((np.diff(o) < 0).any()) or int(o[0]) != 0 or int(o[-1]) != total
            empty = bool((np.diff(o) == 0).any())
            seg = torch.from_numpy(o).to(self._dev)
        if not offs_dev or validate:
            if bad:
                raise ValueError("group offsets must be non-decreasing, start at 0 and end at the number of members")
            if empty and op == "and":
                raise ValueError("an empty group has no intersection")
        G = int(seg.numel()) - 1
        if G < 1:
            raise ValueError("reduce needs at least one group")
        if members is None:
            raise TypeError("members must be an integer array or tensor")
        _, rows = self._rows(members, validate, "members")
        out = BloomFilterBank(G, self._est_elements, self._fpr, hash_function=self._hash_arg, device=self._device)
        bits = torch.empty(G, dtype=torch.int64, device=self._dev)
        N.check(N.lib().psk_bank_reduce(self._table.data_ptr(), self._num_filters, self._num_bits, seg.data_ptr(), self._addr(rows) or None, G,
                                        1 if op == "and" else 0, out._table.data_ptr(), bits.data_ptr(), self._device, self._stream))
        out._els = torch.from_numpy(self._estimates(bits.cpu().numpy())).to(self._dev)
        return out

    # ------------------------------------------------------------------ single filters
    def filter(self, f) -> BloomFilter:
        """a :class:`BloomFilter` COPY of filter ``f`` (table and ``elements_added``): export, union, estimate_elements ... all work on it"""
        f = self._index(f)
        blm = BloomFilter(self._est_elements, self._fpr, hash_function=self._hash_arg, device=self._device)
        t = blm._tab
        N.check(N.lib().psk_table_or(t.ptr, self.table_tensor[f].data_ptr(), t.nwords, t.device, t.stream))  # (blm starts empty)
        blm.elements_added = int(self._els[f].item())
        return blm

    def set_filter(self, f, blm: BloomFilter) -> None:
        """copy ``blm`` (table and ``elements_added``) into filter ``f``; a filter of another geometry or hash family raises"""
        f = self._index(f)
        if not isinstance(blm, BloomFilter) or type(blm)._KIND != "bloom":
            raise TypeError("set_filter takes a BloomFilter")
        if blm.number_bits != self._num_bits or blm.number_hashes != self._number_hashes or \
                list(blm.hashes("test")) != list(self._hash_func("test", self._number_hashes)):
            raise SimilarityError("the filter's geometry or hash function differs from the bank's")
        if blm.device != self._device:
            raise ValueError(f"the filter lives on cuda:{blm.device}, the bank on cuda:{self._device}")
        blm._flush()
        _ = blm._tab.ptr  # (the engine applies what it deferred before the tensor is read)
        self.table_tensor[f].copy_(blm._tab.tensor)
        self._els[f] = int(blm.elements_added)
        self._mark_stale(f)

    def __str__(self) -> str:
        return (f"BloomFilterBank:\n\tfilters: {self._num_filters}\n\tbits per filter: {self._num_bits}\n\tnumber hashes: {self._number_hashes}\n"
                f"\trow bytes: {self._row_bytes}\n\telements added: {int(self._els.sum().item())}\n")
