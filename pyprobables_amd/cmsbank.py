"""CountMinSketchBank: thousands of small count-min sketches of ONE geometry in one device table, fed and queried a batch at a time.

Sketch ``s`` of the bank followed by the ``IIq`` footer is, byte for byte, ``bytes(CountMinSketch(width, depth))`` of the reference after
``add(key, num_els)`` of the ops sent to ``s`` (``probables/countminsketch/countminsketch.py:257-288, 342-354``): one frequency sketch per
tenant, shard or time window without one object, one handle and one launch per sketch.  Row ``s`` of :attr:`table_tensor` is that sketch's
``int32[depth][width]``, padded to 16 bytes.  Only adds enter a bank, with ``num_els >= 0``: every bin ends at
``min(old + the weights that reached it, INT32_MAX)`` whatever the order of execution.

Two routes lead into the table (``include/psk.h`` "CountMinSketchBank"): *direct* -- every key carries a sketch id, its
``depth`` probes are atomic adds into that row (``psk_cms_bank_add``) -- and *grouped* -- the keys of a sketch lie (or are sorted) together,
one workgroup counts them in an LDS image of the row and adds the image's non-zero counters to the table once (``psk_cms_bank_build``).

Beside ``elements_added`` the bank keeps a *bound* per sketch: an upper bound on the largest value any bin of the sketch can hold.  While it
is at most ``INT32_MAX`` no add to the sketch can reach the rail and the engine uses plain atomic adds; above it every add clamps.
"""

from __future__ import annotations

import numpy as np

from . import _native as N
from ._base import _resolve_device, require_device, result_buffer
from .bank import RowBank, _slice_batch
from .countminsketch import _I32_MAX, _I64_MAX, _QUERIES, CountMinSketch
from .exceptions import CountMinSketchError, NotSupportedError
from .hashes import default_fnv_1a, device_digest, is_fused_fnv
from .keys import KeyBatch, hashed_batch, pack_hashes

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

# Device keys with ids take the grouped route (torch.sort of the ids + psk_cms_bank_build) from this many keys on; None = never.  Measured
# (scripts/bench_cms_bank.py part (b), profiles/cms_bank_bench.txt: 4096 sketches of 2048 x 5, random ids, one MI355X): direct atomics win up to
# 2^22 keys (0.97 against 1.02 ms), sort + grouped from 2^23 on (1.47 against 1.81 ms; 1.64 x at 2^25).  What the sort buys is the LDS image:
# the automatic choice also wants a mean segment that takes it (`_grouped_pays`).
CMS_BANK_GROUP_MIN_KEYS = 1 << 23
CMS_BANK_ROUTE_R = 8         # kCmsBankRouteR of csrc/psk_cms_bank.hip: route 0 takes the LDS image for a part with keys * depth * R >= the row's ints
CMS_BANK_LDS_INTS = 16384    # kCmsBankLdsInts: rows beyond it never take the LDS image
CMS_BANK_MAX_DEPTH = 64      # kMaxDepthMeanMin: the mean-min query keeps a key's `depth` values in registers
CMS_BANK_BUILD_MAX_INTS = 2**32  # psk_cms_bank_build / _reduce index a row with 32 bits: wider rows go direct, and are not reduced
CMS_BANK_GRID_CAP = 4096     # kCmsBankGridCap: more sketches (build) or groups x row pieces (reduce) than this are walked with a stride


def sat_add_i64(a, b):
    """``min(a + b, INT64_MAX)`` per element for ``b >= 0`` without leaving int64: numpy arrays or torch tensors (``a`` may be negative)"""
    xp = torch if torch is not None and isinstance(a, torch.Tensor) else np
    zero = xp.zeros_like(a)
    return a + xp.minimum(b, _I64_MAX - xp.maximum(a, zero))


def reduce_bounds(bound, offsets, members) -> np.ndarray:
    """the bounds a :meth:`CountMinSketchBank.reduce` leaves: per group the sum of its members' bounds, clamped at INT64_MAX; a member outside
    the bank is an empty sketch.  Pure numpy / Python integers: no GPU."""
    bound, offsets, members = (np.asarray(x, dtype=np.int64) for x in (bound, offsets, members))
    out = np.zeros(offsets.size - 1, dtype=np.int64)
    for g in range(out.size):
        m = members[offsets[g]:offsets[g + 1]]
        m = m[(m >= 0) & (m < bound.size)]
        out[g] = min(sum(int(bound[i]) for i in m), _I64_MAX)
    return out


def loaded_bound(bins) -> int:
    """the bound of a sketch whose bins were loaded: ``max(0, max bin)``"""
    bins = np.asarray(bins)
    return max(0, int(bins.max())) if bins.size else 0


def host_weights(num_els, n: int):
    """``num_els`` of a host call, checked: None (every key counts once) or int64[n] with every value in [0, INT32_MAX]"""
    if num_els is None:
        return None
    a = np.asarray(num_els)
    if a.dtype.kind not in "iu" or a.dtype == np.bool_:
        raise TypeError("num_els must be integers")
    if a.ndim == 0:
        a = np.full(n, int(a), dtype=np.int64)
    if a.ndim != 1 or a.size != n:
        raise ValueError("weights length differs from the number of keys")
    if a.size and int(a.min()) < 0:
        raise ValueError("num_els must be >= 0: a bank takes adds only")
    if a.size and int(a.max()) > _I32_MAX:
        raise OverflowError(f"num_els outside [0, {_I32_MAX}]")
    return a.astype(np.int64)


class CountMinSketchBank(RowBank):
    """``num_sketches`` count-min sketches sized by ``(width, depth)`` or ``(confidence, error_rate)`` as the reference sizes one
    (countminsketch.py:88-113).

    Keys are accepted as everywhere in the package; ``ids`` / ``sketch_offsets`` / ``num_els`` are integer arrays or tensors, host or device.
    A non-default ``hash_function`` is evaluated on the host (the digest families on the device) and travels as pre-computed hashes."""

    _CHUNK = 2**32 - 1  # keys per engine call
    _ROW = "sketch"
    _num_rows = property(lambda self: self._num_sketches)

    def __init__(self, num_sketches, width=None, depth=None, confidence=None, error_rate=None, hash_function=None, device=None):
        if not (isinstance(num_sketches, (int, np.integer)) and 0 < int(num_sketches) < 2**31):
            raise ValueError("num_sketches must be an integer in [1, 2^31)")
        self._width, self._depth, self._confidence, self._error_rate = CountMinSketch._geometry(width, depth, confidence, error_rate)
        if self._depth > CMS_BANK_MAX_DEPTH:
            raise NotSupportedError(f"a bank's sketches are at most {CMS_BANK_MAX_DEPTH} deep ({self._depth} was asked for): use CountMinSketch")
        if self._width > 2**31:
            raise ValueError("a bank's sketches are at most 2^31 wide: use CountMinSketch for big tables")
        L = N.lib()
        self._num_sketches = int(num_sketches)
        self._hash_arg = hash_function
        self._hash_func = default_fnv_1a if hash_function is None else hash_function
        self._is_fused = is_fused_fnv(hash_function)
        self._digest = device_digest(self._hash_func)
        self._row_bytes = int(L.psk_cms_table_bytes(self._width, self._depth))
        self._query = "min"
        require_device("the bank's table lives in GPU memory")
        self._device = _resolve_device(device)
        self._table = torch.zeros(self._num_sketches * (self._row_bytes // 4), dtype=torch.int32, device=self._dev)
        self._els = torch.zeros(self._num_sketches, dtype=torch.int64, device=self._dev)
        self._bound = torch.zeros(self._num_sketches, dtype=torch.int64, device=self._dev)  # per sketch: no bin exceeds it (clamped at INT64_MAX)
        self._sat = torch.zeros(1, dtype=torch.int64, device=self._dev)                    # clamping adds that met the rail
        self._cus = int(torch.cuda.get_device_properties(self._device).multi_processor_count)
        self._add_policy = "auto"  # "auto" | "direct" | "grouped" (tests force each)
        self._route = 0            # psk_cms_bank_build's route: 0 auto per workgroup, 1 LDS image, 2 global atomics
        self._last_path = None     # "direct" / "grouped": the way the last update took
        self._undo = None          # (bound, elements_added) in front of the bookkeeping of the call in flight
        self._last_chunk = 0
        self._split = None         # workgroups per sketch; None: 1, or ceil(2 * CUs / num_sketches) for a bank of fewer than 2 * CUs sketches

    # ------------------------------------------------------------------ properties
    num_sketches = property(lambda self: self._num_sketches)
    width = property(lambda self: self._width)
    depth = property(lambda self: self._depth)
    confidence = property(lambda self: self._confidence)
    error_rate = property(lambda self: self._error_rate)
    row_bytes = property(lambda self: self._row_bytes)
    hash_function = property(lambda self: self._hash_func)

    @property
    def query_type(self) -> str:
        return self._query

    @query_type.setter
    def query_type(self, val):
        """'min' | 'mean' | 'mean-min'; anything else means 'min' (countminsketch.py:223-238)"""
        val = val.lower() if isinstance(val, str) else None
        self._query = val if val in ("mean", "mean-min") else "min"

    @property
    def table_tensor(self):
        """the int32 tensor [num_sketches, row_bytes / 4] backing the bank (a view: a caller who writes through it keeps the bound right himself)"""
        return self._table.view(self._num_sketches, self._row_bytes // 4)

    @property
    def elements_added(self) -> np.ndarray:
        """int64 per sketch: the sum of ``num_els`` sent there, clamped at INT64_MAX (countminsketch.py:285-287)"""
        return self._els.cpu().numpy()

    def batch_diagnostics(self) -> dict:
        """{"saturated": the clamping adds that met INT32_MAX so far}"""
        return {"saturated": int(self._sat.item())}

    def clear(self, s=None) -> None:
        """empty sketch ``s``, or every sketch"""
        if s is None:
            self._table.zero_()
            self._els.zero_()
            self._bound.zero_()
        else:
            s = self._index(s)
            self.table_tensor[s].zero_()
            self._els[s] = 0
            self._bound[s] = 0

    def _batch(self, keys) -> KeyBatch:
        return self._same_device(hashed_batch(keys, self._hash_func, self._is_fused, self._digest, self._depth, self._device, self._stream))

    def _alt(self, hashes) -> KeyBatch:
        b = pack_hashes(hashes, self._depth)
        if b.n and b.key_len != self._depth:  # countminsketch.py:275 enumerates ALL supplied hashes
            raise IndexError("array index out of range")
        return self._same_device(b)

    def _grouped_pays(self, n: int) -> bool:
        """the automatic choice for device keys with ids: sort + grouped build from CMS_BANK_GROUP_MIN_KEYS keys on, where a sketch's mean share of
        the batch is a segment that route 0 gives the LDS image (and the row fits it)"""
        ints = self._row_bytes // 4
        if CMS_BANK_GROUP_MIN_KEYS is None or n < CMS_BANK_GROUP_MIN_KEYS or ints > CMS_BANK_LDS_INTS:
            return False
        return n * self._depth * CMS_BANK_ROUTE_R >= self._num_sketches * ints

    # ------------------------------------------------------------------ updates
    def _weights(self, num_els, b: KeyBatch, validate: bool):
        """-> (w: None, or the int32 weights where the keys are; w64: None, or the same as int64 for the sums; flags: what is still to be read
        back about a device tensor of the caller's, as (device bool, exception) pairs).  Host weights are always checked, here; unchecked device
        weights are clamped into [0, INT32_MAX]"""
        if num_els is None:
            return None, None, []
        if not (torch is not None and isinstance(num_els, torch.Tensor) and num_els.is_cuda):
            h = host_weights(num_els.numpy() if torch is not None and isinstance(num_els, torch.Tensor) else num_els, b.n)
            if b.where == N.HOST:
                return np.ascontiguousarray(h.astype(np.int32)), h, []
            t = torch.from_numpy(h).to(self._dev)
            return t.to(torch.int32), t, []
        t = num_els
        if b.where != N.DEVICE:
            raise ValueError("device weights need a device key batch")
        if t.device.index != self._device:
            raise ValueError(f"weights live on cuda:{t.device.index}, the bank on cuda:{self._device}")
        if t.is_floating_point() or t.dtype == torch.bool:
            raise TypeError("num_els must be integers")
        if t.dim() != 1 or t.numel() != b.n:
            raise ValueError("weights length differs from the number of keys")
        flags = []
        if validate and b.n:
            flags.append(((t < 0).any(), ValueError("num_els must be >= 0: a bank takes adds only")))
            if t.element_size() > 4:
                flags.append(((t > _I32_MAX).any(), OverflowError(f"num_els outside [0, {_I32_MAX}]")))
        w64 = t.to(torch.int64).clamp(0, _I32_MAX)
        return w64.to(torch.int32), w64, flags

    @staticmethod
    def _read_flags(flags) -> None:
        """ONE read-back (one synchronisation) for everything a call has to know about its device arguments; the first raised flag raises"""
        if flags:
            for hit, (_, exc) in zip(torch.stack([f for f, _ in flags]).cpu().tolist(), flags):
                if hit:
                    raise exc

    def _clip_ids(self, idv):
        """unchecked ids as the engine's 32-bit words may carry them: everything outside the bank becomes num_sketches, which the engine skips
        (an id of 2^32 + 1 must not alias sketch 1)"""
        S = self._num_sketches
        if isinstance(idv, np.ndarray):
            return np.where((idv < 0) | (idv >= S), S, idv)
        return torch.where((idv < 0) | (idv >= S), S, idv)

    def _account(self, sums) -> None:
        """BEFORE the launch: the bound and elements_added of every sketch rise by the weight sent to it"""
        if isinstance(sums, np.ndarray):
            sums = torch.from_numpy(np.ascontiguousarray(sums.astype(np.int64))).to(self._dev)
        self._undo = (self._bound, self._els)
        self._bound = sat_add_i64(self._bound, sums)
        self._els = sat_add_i64(self._els, sums)

    def _launch(self, call) -> None:
        """the engine call behind `_account`: a call that is refused or fails puts the bookkeeping back (a batch of more than `_CHUNK` keys
        that fails after its first engine call leaves those keys in the table: the bound then only errs upwards)"""
        try:
            call()
        except Exception:
            if self._last_chunk == 0:
                self._bound, self._els = self._undo
            raise
        finally:
            self._undo = None

    def _add_direct(self, b: KeyBatch, ids, w) -> None:
        self._last_path = "direct"
        L = N.lib()
        for lo in range(0, b.n, self._CHUNK):
            self._last_chunk = lo
            hi = min(b.n, lo + self._CHUNK)
            c, i32 = _slice_batch(b, lo, hi), self._ids_u32(ids[lo:hi])
            wc = None if w is None else w[lo:hi]
            N.check(L.psk_cms_bank_add(self._table.data_ptr(), self._num_sketches, self._width, self._depth, *c.args(), c.where, self._addr(i32) or None,
                                       None if wc is None else self._addr(wc) or None, self._bound.data_ptr(), self._sat.data_ptr(), self._device, self._stream))

    def _build(self, b: KeyBatch, seg, perm, w) -> None:
        """seg int64[S + 1] on the device (positions in perm, or in the batch when perm is None), perm int32[n] on the device or None"""
        self._last_path = "grouped"
        self._last_chunk = 0
        if b.n > self._CHUNK:
            raise ValueError("a grouped call takes fewer than 2^32 keys")
        N.check(N.lib().psk_cms_bank_build(self._table.data_ptr(), self._num_sketches, self._width, self._depth, *b.args(), seg.data_ptr(),
                                           perm.data_ptr() if perm is not None else None, None if w is None else self._addr(w) or None,
                                           self._bound.data_ptr(), self._sat.data_ptr(), self.split_for(), int(self._route), self._device, self._stream))

    def _add_batch(self, b: KeyBatch, ids, sketch_offsets, num_els, validate: bool) -> None:
        if (ids is None) == (sketch_offsets is None):
            raise TypeError("pass either ids or sketch_offsets")
        if self._add_policy not in ("auto", "direct", "grouped"):
            raise ValueError(f"unknown _add_policy {self._add_policy!r}")
        if int(self._route) not in (0, 1, 2):
            raise ValueError("route must be 0 (auto), 1 (LDS image) or 2 (global atomics)")
        ints = self._row_bytes // 4
        if int(self._route) == 1 and self._add_policy != "direct" and ints > CMS_BANK_LDS_INTS:  # (refused before the bookkeeping moves)
            raise ValueError(f"rows of {ints} ints do not fit the LDS image (at most {CMS_BANK_LDS_INTS})")
        if self._add_policy == "grouped" and ints >= CMS_BANK_BUILD_MAX_INTS:
            raise ValueError(f"the grouped build takes rows of fewer than 2^32 ints (these have {ints}): the direct route takes them")
        can_build = ints < CMS_BANK_BUILD_MAX_INTS
        S, dev = self._num_sketches, b.where == N.DEVICE
        w, w64, flags = self._weights(num_els, b, validate)
        if sketch_offsets is not None:
            fold = dev and torch is not None and isinstance(sketch_offsets, torch.Tensor) and sketch_offsets.is_cuda
            offs = self._offsets(sketch_offsets, b.n, b.where, validate and not fold, S, "sketch_offsets")
            if fold and validate:  # device offsets and device weights: one reduction, one synchronisation
                flags.insert(0, ((offs[1:] < offs[:-1]).any() | (offs[0] != 0) | (offs[-1] != b.n),
                                 ValueError("sketch_offsets must be non-decreasing, start at 0 and end at the number of keys")))
            self._read_flags(flags)
            if b.n == 0:
                return
            oc = offs.clamp(0, b.n) if dev else offs  # (unchecked device offsets: the engine reads no key at or beyond n, nor do the sums)
            if w64 is None:
                sums = oc[1:] - oc[:-1]
            else:  # segment sums from one prefix sum (n < 2^32 weights below 2^31: below 2^63)
                cs = torch.cat([torch.zeros(1, dtype=torch.int64, device=self._dev), torch.cumsum(w64, 0)]) if dev else np.concatenate([[0], np.cumsum(w64)])
                sums = cs[oc[1:]] - cs[oc[:-1]]
            if dev:
                sums = sums.clamp(min=0)
            self._account(sums)
            if dev and self._add_policy != "direct" and can_build:  # keys that arrive grouped: the build kernel as they lie
                self._launch(lambda: self._build(b, offs, None, w))
            elif dev:
                self._launch(lambda: self._add_direct(b, torch.repeat_interleave(torch.arange(S, device=self._dev), offs[1:] - offs[:-1]), w))
            else:  # host keys always go direct
                self._launch(lambda: self._add_direct(b, np.repeat(np.arange(S, dtype=np.int64), np.diff(offs)), w))
            return
        ids_dev = torch is not None and isinstance(ids, torch.Tensor) and ids.is_cuda
        idv = self._ids(ids, b.n, b.where, validate and not ids_dev)
        if ids_dev and validate and b.n:  # device ids and device weights: one reduction, one synchronisation
            lo, hi = torch.aminmax(ids)
            flags.insert(0, ((lo < 0) | (hi >= S), ValueError(f"{self._ROW} ids must lie in [0, {S})")))
        self._read_flags(flags)
        if b.n == 0:
            return
        at = idv if validate else self._clip_ids(idv)  # unchecked ids: the engine skips num_sketches, and so do the sums
        if not dev:
            sums = np.bincount(at, minlength=S + 1).astype(np.int64) if w64 is None else np.zeros(S + 1, dtype=np.int64)
            if w64 is not None:
                np.add.at(sums, at, w64)
            self._account(sums[:S])
            self._launch(lambda: self._add_direct(b, at, w))
            return
        if w64 is None:
            self._account(torch.bincount(at, minlength=S + 1)[:S])
        else:
            self._account(torch.zeros(S + 1, dtype=torch.int64, device=self._dev).index_add_(0, at, w64)[:S])
        grouped = can_build and b.n <= self._CHUNK and (self._add_policy == "grouped" or (self._add_policy == "auto" and self._grouped_pays(b.n)))
        if grouped:
            srt, perm = torch.sort(at, stable=True)
            seg = torch.searchsorted(srt, torch.arange(S + 1, device=self._dev, dtype=torch.int64))
            self._launch(lambda: self._build(b, seg.contiguous(), perm.to(torch.int32).contiguous(), w))
        else:
            self._launch(lambda: self._add_direct(b, at, w))

    def add_many(self, keys, ids=None, sketch_offsets=None, num_els=None, validate: bool = True) -> None:
        """sketch ``ids[i]`` gets ``add(key_i, num_els_i)`` -- or, for keys that are already grouped by sketch, sketch ``s`` gets keys
        ``sketch_offsets[s]:sketch_offsets[s + 1]``.  ``num_els``: None (= 1), an int, or one integer in [0, 2^31) per key.  An id outside the
        bank or a negative ``num_els`` raises ``ValueError`` before anything changes; device ids and device weights are checked together with
        one reduction and one synchronisation unless ``validate=False`` (then an id beyond the bank is skipped and a weight is clamped into
        [0, 2^31)).  ``elements_added`` and the bound move before the launch; a call the engine refuses puts them back."""
        self._add_batch(self._batch(keys), ids, sketch_offsets, num_els, validate)

    def add_alt_many(self, hashes, ids=None, sketch_offsets=None, num_els=None, validate: bool = True) -> None:
        """:meth:`add_many` for pre-computed hashes: (n, depth) uint64"""
        self._add_batch(self._alt(hashes), ids, sketch_offsets, num_els, validate)

    # ------------------------------------------------------------------ lookups
    def _check_batch(self, b: KeyBatch, ids, validate: bool):
        idv = self._ids(ids, b.n, b.where, validate)
        if not validate:
            idv = self._clip_ids(idv)
        L, wide = N.lib(), self._query == "mean-min"
        out = result_buffer(b.where, b.n, np.int64 if wide else np.int32, torch.int64 if wide else torch.int32, self._device)[1]()
        for lo in range(0, b.n, self._CHUNK):  # (n = 0 launches nothing)
            hi = min(b.n, lo + self._CHUNK)
            c, i32 = _slice_batch(b, lo, hi), self._ids_u32(idv[lo:hi])
            head = (self._table.data_ptr(), self._num_sketches, self._width, self._depth, *c.args(), c.where, self._addr(i32) or None)
            if wide:
                N.check(L.psk_cms_bank_check_meanmin(*head, self._els.data_ptr(), self._addr(out[lo:hi]) or None, self._device, self._stream))
            else:
                N.check(L.psk_cms_bank_check(*head, _QUERIES[self._query], self._addr(out[lo:hi]) or None, self._device, self._stream))
        return out

    def check_many(self, keys, ids, validate: bool = True):
        """the reference's ``check(key_i)`` on sketch ``ids[i]`` under :attr:`query_type` (countminsketch.py:323-340, 429-453): int32 (int64 for
        'mean-min'), numpy for host keys, a torch tensor on the device for device keys"""
        return self._check_batch(self._batch(keys), ids, validate)

    def check_alt_many(self, hashes, ids, validate: bool = True):
        return self._check_batch(self._alt(hashes), ids, validate)

    # ------------------------------------------------------------------ folds
    def reduce(self, groups, validate: bool = True):
        """a new bank of G sketches (same geometry, hash function and device): sketch g is this bank's sketches ``groups[g]`` joined in that order
        onto an empty sketch (countminsketch.py:356-399: an accumulator on a rail stays frozen, ``elements_added`` clamps).  ``groups``: a list of
        lists of sketch ids, or ``(members[total], offsets[G + 1])`` arrays or tensors.  An empty group gives an empty sketch; with
        ``validate=False`` a member beyond the bank counts as an empty sketch."""
        if isinstance(groups, tuple) and len(groups) == 2:
            members, offs = groups
        else:
            groups = [np.asarray(g, dtype=np.int64).reshape(-1) if len(g) else np.zeros(0, dtype=np.int64) for g in groups]
            offs = np.zeros(len(groups) + 1, dtype=np.int64)
            np.cumsum([g.size for g in groups], out=offs[1:])
            members = np.concatenate(groups) if groups else np.zeros(0, dtype=np.int64)
        if self._row_bytes // 4 >= CMS_BANK_BUILD_MAX_INTS:
            raise NotSupportedError("reduce takes rows of fewer than 2^32 ints: join the sketches one by one through sketch(s)")
        total = int(members.numel()) if torch is not None and isinstance(members, torch.Tensor) else int(np.asarray(members).size)
        if total >= 2**31:  # (the device fold of the bounds adds 32-bit halves in int64)
            raise ValueError("members names 2^31 sketches or more")
        seg = self._offsets(offs, total, N.DEVICE, validate, None, "group offsets")
        G = int(seg.numel()) - 1
        if G < 1:
            raise ValueError("reduce needs at least one group")
        m_dev = torch is not None and isinstance(members, torch.Tensor) and members.is_cuda
        if m_dev or validate:
            rows = self._ids(members, total, N.DEVICE, validate)
        else:  # unchecked host members
            rows = torch.from_numpy(np.ascontiguousarray(np.asarray(members).astype(np.int64))).to(self._dev)
        rows = torch.where((rows < 0) | (rows >= self._num_sketches), self._num_sketches, rows)
        out = CountMinSketchBank(G, self._width, self._depth, hash_function=self._hash_arg, device=self._device)
        out._confidence, out._error_rate, out._query = self._confidence, self._error_rate, self._query
        r32 = self._ids_u32(rows)
        N.check(N.lib().psk_cms_bank_reduce(self._table.data_ptr(), self._els.data_ptr(), self._num_sketches, self._width, self._depth, seg.data_ptr(),
                                            self._addr(r32) or None, G, out._table.data_ptr(), out._els.data_ptr(), self._device, self._stream))
        out._bound = self._reduce_bounds(seg, rows, G, total)
        return out

    def _reduce_bounds(self, seg, rows, G: int, total: int):
        """`reduce_bounds` on the device, no read-back: the members' bounds as 31-bit halves, summed per group (fewer than 2^31 members: no
        int64 sum wraps), put together again with the clamp at INT64_MAX.  `rows` holds num_sketches for a member beyond the bank."""
        m31 = 2**31 - 1
        v = torch.cat([self._bound, torch.zeros(1, dtype=torch.int64, device=self._dev)])[rows]
        grp = torch.searchsorted(seg[1:].contiguous(), torch.arange(total, device=self._dev, dtype=torch.int64), right=True).clamp_(max=G)
        lo = torch.zeros(G + 1, dtype=torch.int64, device=self._dev).index_add_(0, grp, v & m31)[:G]
        hi = torch.zeros(G + 1, dtype=torch.int64, device=self._dev).index_add_(0, grp, v >> 31)[:G]
        top = hi + (lo >> 31)
        return torch.where(top >= 2**32, torch.full_like(top, _I64_MAX), (top.clamp(max=2**32 - 1) << 31) | (lo & m31))

    # ------------------------------------------------------------------ single sketches
    def _similar(self, cms) -> None:
        if not isinstance(cms, CountMinSketch):
            raise TypeError(f"Unable to merge a count-min sketch with {type(cms)}")
        if cms.width != self._width or cms.depth != self._depth or list(cms.hashes("test")) != list(self._hash_func("test", self._depth)):
            raise CountMinSketchError("Unable to merge as the count-min sketches are mismatched")
        if cms.device != self._device:
            raise ValueError(f"the sketch lives on cuda:{cms.device}, the bank on cuda:{self._device}")

    def sketch(self, s) -> CountMinSketch:
        """a :class:`CountMinSketch` COPY of sketch ``s`` (bins, ``elements_added``, ``query_type``): ``bytes()`` of it is the reference's export"""
        s = self._index(s)
        cms = CountMinSketch(width=self._width, depth=self._depth, hash_function=self._hash_arg, device=self._device)
        cms._confidence, cms._error_rate = self._confidence, self._error_rate
        t = cms._tab
        N.check(N.lib().psk_table_add_sat_i32(t.ptr, self.table_tensor[s].data_ptr(), self._width * self._depth, t.device, t.stream))  # (cms starts empty)
        N.check(N.lib().psk_rescan_bound(t.handle, t.stream))  # the copied bins may sit on a rail
        cms._els_added = int(self._els[s].item())
        cms.query_type = self._query
        return cms

    def set_sketch(self, s, cms: CountMinSketch) -> None:
        """copy ``cms`` (bins -- any, negative ones included -- and ``elements_added``) into sketch ``s``; a sketch of another geometry or hash
        family raises ``CountMinSketchError`` as ``join`` does"""
        s = self._index(s)
        self._similar(cms)
        _ = cms._tab.ptr  # (the engine applies what it deferred before the tensor is read)
        row = self.table_tensor[s]
        row.copy_(cms._tab.tensor)
        self._els[s] = int(cms.elements_added)
        self._bound[s] = torch.clamp(row.max(), min=0).to(torch.int64)

    def __str__(self) -> str:
        return (f"CountMinSketchBank:\n\tsketches: {self._num_sketches}\n\twidth: {self._width}\n\tdepth: {self._depth}\n"
                f"\trow bytes: {self._row_bytes}\n")
