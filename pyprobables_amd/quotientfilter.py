"""QuotientFilter on the GPU (reference: ``probables/quotientfilter/quotientfilter.py``).

The reference drops duplicates (``add_alt`` inserts only what ``_contained_at_loc`` does not find), keeps every run sorted by
remainder and the runs of a cluster in quotient order, so its four arrays -- ``_filter``, ``_is_occupied``, ``_is_continuation``,
``_is_shifted`` -- are a function of the SET of 32-bit hashes it holds, not of their order.  That makes a bulk build exact: sort and
deduplicate the hashes (torch: rocPRIM's radix sort), place them with one prefix-max scan (``psk_qf_build``), and the table is the
reference's bit for bit (DESIGN.md "Quotient filter"; tests/test_quotient_model.py ties the layout rule to the live reference).
Adding a batch to a loaded filter is exact for the same reason however it is carried out: by rewriting the touched regions in place
(``psk_qf_add_alt``, DESIGN.md "Quotient filter: insertion in place") when the quotient stays and an empty slot remains, or by
decode + concatenate + sort/unique + rebuild (an empty filter, q < 5, a stream that reaches the load threshold, a batch that fills the table).

Removal is a batch call, ``remove_many`` / ``remove_alt_many``: the reference's ``remove_alt`` leaves the canonical table of the remaining set
whenever the table has an empty slot (tests/test_quotient_remove_model.py), so a batch is exact however it is carried out -- by repairing the
hit clusters in place (``psk_qf_remove_alt``, DESIGN.md "Quotient filter: removal") or by decode + set difference + rebuild.  The reference
never decrements ``_elements_added`` in a removal and resets it only in a resize; ``elements_added``, ``load_factor``, the auto-expand test and
the "insufficient space" test follow that counter (held + removals since the last resize), ``elements_held`` is the true count.

Deviations from the reference, all deliberate:

* the per-key ``remove`` / ``remove_alt`` still raise :class:`NotSupportedError`; removal is available as ``remove_many`` / ``remove_alt_many``.
* ``remove_many`` / ``remove_alt_many`` on a completely full table give the canonical table of the remaining set (the reference's removal can
  spin forever there or leave a table that is not canonical).
* ``auto_expand=False`` and more distinct hashes than slots: :class:`QuotientFilterError` with the reference's message, raised BEFORE
  the table changes (the reference raises mid-stream and keeps the part it had inserted).
* ``get_hashes()`` of a completely full table returns the hashes in ascending order (the reference's walk to the first empty slot
  runs off the table there).

Per-key ``add`` goes the batch's way with a batch of one: this class is for batches (``add_many`` / ``check_many``).
"""

from __future__ import annotations

import math
from collections.abc import Iterator

import numpy as np

from . import _native as N
from ._base import DeviceResident, _resolve_device, as_bool, equal_groups, require_device, result_buffer
from .exceptions import NotSupportedError, QuotientFilterError
from .hashes import KeyT, fnv_1a_32
from .keys import pack_keys

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

_I32_MIN = -(2**31)
# ``_remove_policy = "auto"``: a batch of up to this fraction of the hashes held is repaired in place, a larger one rebuilds the table.
# profiles/quotient_remove_bench.txt (scripts/bench_quotient_remove.py; load 0.8, end to end, m distinct present hashes of `held`):
#   q = 24 (13.4 M held)  in place 0.29 ms at m = 2^10, 0.38 ms at 2^16, 2.0 ms at 2^22 (0.31 of held); the rebuild 3.2 - 3.4 ms at every m
#   q = 20 (839 K held)   in place 0.27 ms at 2^10, 0.44 ms at 2^18 (0.31 of held), 0.59 ms at 2^19 (0.62); the rebuild 0.48 - 0.58 ms
# In place wins up to 0.31 of held at both sizes (by 1.7 x and 1.2 x there) and ties at 0.62 at q = 20; the constant lies between the two.
REMOVE_LOCAL_MAX_FRACTION = 0.5
# ``_add_policy = "auto"``: a stream of up to this fraction of the hashes held, into a table of at least 2^ADD_LOCAL_MIN_QUOTIENT slots, is inserted
# in place; anything else rebuilds the table.  profiles/quotient_add_bench.txt (scripts/bench_quotient_add.py; load 0.8, end to end, m new hashes):
#   q = 24 (13.4 M held)  in place 0.49 ms at m = 2^10, 0.85 ms at 2^16, 1.5 ms at 2^19, 2.8 ms at 2^20 (0.078 of held), 9.7 ms at 2^21 (0.156);
#                         the rebuild 3.5 - 3.6 ms at every m: in place wins by 7.1 x at 2^10 and 1.3 x at 2^20, and loses (0.38 x) at 2^21
#   q = 22 (3.36 M held)  in place 0.62 ms at 2^10, 0.94 ms at 2^16 (0.020 of held), 1.10 ms at 2^17 (0.039), 4.8 ms at 2^19; the rebuild
#                         1.02 - 1.07 ms: in place wins by 1.65 x at 2^10 and 1.10 x at 2^16, and loses (0.94 x) at 2^17
#   q = 20 (839 K held)   in place 0.82 ms at 2^10 .. 2^14, 1.07 ms at 2^16, 2.9 ms at 2^17; the rebuild 0.54 - 0.56 ms: in place never wins --
#                         its kernels alone take 0.46 ms for 2^10 hashes (three dependent launches, each as long as its longest walk), which is
#                         what decoding and rebuilding 2^20 slots costs
# (m stops at 0.8 * 2^q + m < 2^q: 2^22 new hashes do not fit a table of 2^24 slots at load 0.8.)  The crossover is not one fraction: it lies
# between 0.078 and 0.156 of held at q = 24 and between 0.020 and 0.039 at q = 22.  The constant sits in the smaller table's bracket, which is a
# win at both sizes; the quotient floor is the smallest size measured at which in place wins at all.
ADD_LOCAL_MAX_FRACTION = 0.03
ADD_LOCAL_MIN_QUOTIENT = 22


def _check_quotient(quotient: int) -> None:
    if quotient < 3 or quotient > 31:
        raise QuotientFilterError(f"Invalid quotient setting; quotient must be between 3 and 31; {quotient} was provided")


def bits_per_element(quotient: int) -> int:
    """the reference's three width classes (quotientfilter.py:66-75)"""
    r = 32 - quotient
    return 8 if r <= 8 else (16 if r <= 16 else 32)


def resize_threshold(quotient: int, max_load_factor: float) -> int:
    """the smallest element count n with ``n / size >= max_load_factor`` -- the reference's own float test (quotientfilter.py:161)"""
    size = 1 << quotient
    t = max(0, math.ceil(max_load_factor * size))
    while t > 0 and (t - 1) / size >= max_load_factor:
        t -= 1
    while t / size < max_load_factor:
        t += 1
    return t


def _after_resize(quotient: int, held: int, max_load_factor: float) -> int:
    """the quotient after the ``resize()`` that ``add_alt`` triggers with `held` elements in the table: one doubling, and one more for
    every re-inserting call that again meets a load at the threshold (only a small ``max_load_factor`` gets there)"""
    quotient += 1
    while quotient <= 31 and held - 1 >= resize_threshold(quotient, max_load_factor):
        quotient += 1
    return quotient


def expanded_quotient(quotient: int, held: int, counts_after, max_load_factor: float = 0.85, stale: int = 0) -> int:
    """The quotient an auto-expanding filter ends with.  ``held`` distinct hashes are in the table, ``counts_after[i]`` (ascending; a
    torch tensor or anything ``torch.as_tensor`` takes) is the distinct count after call i of the stream.

    The reference tests ``load_factor >= max_load_factor`` at the START of every ``add_alt`` call, duplicates included
    (quotientfilter.py:161), so the table doubles only if another call FOLLOWS the one that reached the threshold: the crossing index
    is the first i with ``counts_after[i] >= threshold``; a resize happens iff it is not the last call.  Repeats at the new size.

    ``stale``: successful removals since the last resize.  The reference's counter is the true count plus these until the first doubling
    of the stream resets it (``resize`` re-adds what the table holds into fresh parameters); behind that the stream is judged on true counts."""
    cum = torch.as_tensor(counts_after, dtype=torch.int64)
    m = int(cum.numel())
    nxt = 0  # the first call whose load test has not run yet
    while nxt < m:
        t = resize_threshold(quotient, max_load_factor)
        if held + stale >= t:
            call = nxt
        else:  # calls behind the first j with cum[j] + stale >= t start with the threshold reached
            call = max(nxt, int(torch.searchsorted(cum, torch.tensor([t - stale], dtype=torch.int64, device=cum.device))[0]) + 1)
        if call >= m:
            break
        quotient = _after_resize(quotient, held if call == 0 else int(cum[call - 1]), max_load_factor)
        _check_quotient(quotient)
        stale = 0
        nxt = call + 1  # that call inserts into the larger table without another test
    return quotient


def plan_add(quotient: int, held: int, stale: int, counts_after, auto_expand: bool, max_load_factor: float = 0.85) -> tuple[int, int]:
    """The host side of one ``add_alt`` stream: -> (quotient, stale) behind it.  ``held`` distinct hashes are in the table, ``stale`` removals
    have succeeded since the last resize, ``counts_after[i]`` is the true distinct count after call i (non-empty).  Raises the reference's
    "insufficient space" (quotientfilter.py:357-358: ``_add`` compares ITS counter with the size, so slots may be free) before anything changes."""
    cum = torch.as_tensor(counts_after, dtype=torch.int64)
    total = int(cum[-1])
    q = quotient
    if auto_expand and total + stale >= resize_threshold(q, max_load_factor):
        q = expanded_quotient(q, held, cum, max_load_factor, stale)  # the threshold is reached inside this stream: whether (and how often) the table doubles depends on WHERE
    if q != quotient:
        stale = 0
    if total + stale > (1 << q):
        raise QuotientFilterError("Unable to insert the element due to insufficient space")
    return q, stale


def _is_default_hash(hash_function) -> bool:
    if hash_function is None or hash_function is fnv_1a_32:
        return True
    if getattr(hash_function, "__module__", None) == "probables.hashes" and getattr(hash_function, "__name__", None) == "fnv_1a_32":
        try:
            return hash_function("this is a test €", 0) == fnv_1a_32("this is a test €", 0)
        except Exception:
            return False
    return False


class QuotientFilter(DeviceResident):
    """Quotient filter with the table in GPU memory; same surface as the reference's class plus the batch calls.

    Args:
        quotient (int): The size of the quotient to use (3 .. 31); the table has ``2**quotient`` slots
        auto_expand (bool): Automatically expand or not
        hash_function (function): ``hf(key, 0) -> int`` (32 bits are used); ``None``: the reference's ``fnv_1a_32``, hashed on the GPU.
            Any other function is evaluated per key on the host and its hashes are handed to the kernels.
        device: HIP device index (default: torch's current device)
    Raises:
        QuotientFilterError: Raised when unable to initialize
    """

    _NOUN = "filter"

    def __init__(self, quotient: int = 20, auto_expand: bool = True, hash_function=None, device=None):
        _check_quotient(quotient)
        self._device = _resolve_device(device)
        self._hash_func = fnv_1a_32 if hash_function is None else hash_function
        self._fused = _is_default_hash(hash_function)
        self._auto_resize = bool(auto_expand)
        self._max_load_factor = 0.85
        self._set_params(quotient)

    def _set_params(self, quotient: int) -> None:
        self._q, self._r, self._size = quotient, 32 - quotient, 1 << quotient
        self._bits_per_elm = bits_per_element(quotient)
        self._held = self._stale = 0  # slots in use; successful removals since these parameters were set (the reference's counter is their sum)
        self._filter = self._occ = self._cont = self._sh = None  # allocated by the first call that touches the table (_alloc)
        self._remove_scratch = None

    def _alloc(self) -> None:
        """the four arrays, zeroed, in HBM.  No device, no table: every call that needs one raises (there is no CPU fallback); the
        parameters and properties above exist without one."""
        if self._filter is not None:
            return
        require_device("the quotient filter's table lives in GPU memory")
        dev = self._dev
        dtype = {8: torch.uint8, 16: torch.int16, 32: torch.int32}[self._bits_per_elm]
        words = max(self._size // 32, 1)
        self._filter = torch.zeros(self._size, dtype=dtype, device=dev)
        self._occ, self._cont, self._sh = (torch.zeros(words, dtype=torch.int32, device=dev) for _ in range(3))

    # ------------------------------------------------------------------ properties (quotientfilter.py:86-142)
    @property
    def quotient(self) -> int:
        """int: The size of the quotient, in bits"""
        return self._q

    @property
    def remainder(self) -> int:
        """int: The size of the remainder, in bits"""
        return self._r

    @property
    def num_elements(self) -> int:
        """int: The total size of the filter"""
        return self._size

    @property
    def size(self) -> int:
        """int: The number of bins available in the filter (same as `num_elements`)"""
        return self._size

    @property
    def elements_added(self) -> int:
        """int: The reference's counter: the (distinct) elements added since the last resize, removed ones included"""
        return self._held + self._stale

    @property
    def elements_held(self) -> int:
        """int: The number of (distinct) elements in the filter"""
        return self._held

    @property
    def bits_per_elm(self) -> int:
        """int: The number of bits used per element"""
        return self._bits_per_elm

    @property
    def load_factor(self) -> float:
        """float: The load factor of the filter"""
        return self.elements_added / self._size

    @property
    def auto_expand(self) -> bool:
        """bool: Will the quotient filter automatically expand"""
        return self._auto_resize

    @auto_expand.setter
    def auto_expand(self, val: bool):
        self._auto_resize = bool(val)

    @property
    def max_load_factor(self) -> float:
        """float: The maximum allowed load factor after which auto expanding should occur"""
        return self._max_load_factor

    @max_load_factor.setter
    def max_load_factor(self, val: float):
        self._max_load_factor = float(val)

    @property
    def hash_function(self):
        return self._hash_func

    # the four arrays as they lie in HBM (include/psk.h "QuotientFilter")
    @property
    def filter_tensor(self):
        """remainders, one per slot: uint8 / int16 / int32 holding the unsigned 8 / 16 / 32-bit values"""
        self._alloc()
        return self._filter

    @property
    def occupied_tensor(self):
        """``_is_occupied`` packed LSB-first into int32 words"""
        self._alloc()
        return self._occ

    @property
    def continuation_tensor(self):
        self._alloc()
        return self._cont

    @property
    def shifted_tensor(self):
        self._alloc()
        return self._sh

    def tables(self) -> dict:
        """host copies in the reference's shape: ``filter`` (unsigned), ``occupied`` / ``continuation`` / ``shifted`` (uint8 0 / 1 per slot)"""
        self._alloc()
        udt = {8: np.uint8, 16: np.uint16, 32: np.uint32}[self._bits_per_elm]
        out = {"filter": self._filter.cpu().numpy().view(udt)}
        for name, t in (("occupied", self._occ), ("continuation", self._cont), ("shifted", self._sh)):
            out[name] = np.unpackbits(t.cpu().numpy().view(np.uint8), bitorder="little")[: self._size]
        return out

    def synchronize(self) -> None:
        self._alloc()
        super().synchronize()

    # ------------------------------------------------------------------ hashes in, as uint32 bit patterns in int32 device tensors
    def _hash_keys(self, keys):
        """keys -> (int32 device tensor of the 32-bit hashes in stream order)"""
        self._alloc()
        if not self._fused:
            if isinstance(keys, (str, bytes, bytearray, memoryview)):
                keys = [keys]
            return self._as_bits(np.fromiter((int(self._hash_func(k, 0)) & 0xFFFFFFFF for k in keys), dtype=np.uint64))
        b = self._same_device(pack_keys(keys))
        addr, fin = result_buffer(b.where, b.n, np.int32, torch.int32, self._device)
        N.check(N.lib().psk_qf_hash(*b.args(), b.where, addr, self._device, self._stream))
        return fin() if b.where == N.DEVICE else torch.from_numpy(fin()).to(self._dev)

    def _as_bits(self, hashes):
        """ints / numpy / torch (any integer type holding 0 .. 2^32 - 1) -> int32 device tensor of the bit patterns"""
        self._alloc()
        if torch is not None and isinstance(hashes, torch.Tensor):
            t = hashes.to(self._dev).reshape(-1)
            if t.dtype == torch.int32:
                return t.contiguous()
            t = t.to(torch.int64) & 0xFFFFFFFF
            return torch.where(t >= 2**31, t - 2**32, t).to(torch.int32)
        if isinstance(hashes, (int, np.integer)):
            hashes = [hashes]
        a = np.asarray(hashes if isinstance(hashes, np.ndarray) else [int(h) & 0xFFFFFFFF for h in hashes], dtype=np.uint64)
        a = (a.reshape(-1) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        return torch.from_numpy(a.view(np.int32)).to(self._dev)

    @staticmethod
    def _usort(bits, unique: bool):
        """ascending as UNSIGNED 32-bit values (the sign bit flipped turns that into int32 order)"""
        s = torch.sort(bits ^ _I32_MIN).values
        if unique:
            s = torch.unique_consecutive(s)
        return s ^ _I32_MIN

    @staticmethod
    def _to_ints(bits) -> list[int]:
        return (bits.cpu().numpy().view(np.uint32)).tolist()

    # ------------------------------------------------------------------ the three kernels' call sites
    def _build(self, sorted_bits) -> None:
        self._alloc()
        n = int(sorted_bits.numel())
        scratch = torch.empty(n // 1024 + 2, dtype=torch.int32, device=self._dev)
        N.check(N.lib().psk_qf_build(self._q, sorted_bits.data_ptr() if n else None, n, self._filter.data_ptr(), self._occ.data_ptr(),
                                     self._cont.data_ptr(), self._sh.data_ptr(), scratch.data_ptr(), self._device, self._stream))
        self._held = n

    def _table_args(self):
        self._alloc()
        return (self._q, self._filter.data_ptr(), self._occ.data_ptr(), self._cont.data_ptr(), self._sh.data_ptr())

    def _decode(self):
        """-> (hashes of the table ascending, int32 bit patterns on the device; first empty slot or None)"""
        n = self._held
        if n == 0:
            return torch.empty(0, dtype=torch.int32, device=self._dev), 0
        words = int(self._occ.numel())
        counts = torch.empty((3, words), dtype=torch.int64, device=self._dev)
        marks = torch.empty(2, dtype=torch.int32, device=self._dev)
        L = N.lib()
        N.check(L.psk_qf_decode(*self._table_args(), counts.data_ptr(), marks.data_ptr(), None, 0, self._device, self._stream))
        inc = torch.cumsum(counts, dim=1).contiguous()
        out = torch.empty(n, dtype=torch.int32, device=self._dev)
        N.check(L.psk_qf_decode(*self._table_args(), inc.data_ptr(), marks.data_ptr(), out.data_ptr(), n, self._device, self._stream))
        first_empty = int(marks[1].item()) & 0xFFFFFFFF
        return self._usort(out, unique=False), (None if first_empty == 0xFFFFFFFF else first_empty)

    def _reference_order(self):
        """the hashes in the order of the reference's ``hashes()``: slot order from the first empty slot on, i.e. the ascending list
        rotated to the first hash whose quotient lies behind that slot (quotientfilter.py:208-238)"""
        s, first_empty = self._decode()
        if first_empty is None or s.numel() == 0:
            return s
        bound = (first_empty + 1) << self._r  # > every hash of a quotient <= first_empty
        k = int(((s.to(torch.int64) & 0xFFFFFFFF) < bound).sum().item())
        return torch.cat([s[k:], s[:k]])

    # ------------------------------------------------------------------ insert
    _add_policy = "auto"  # "local": insert in place where that is possible; "rebuild": decode, merge, build; "auto": by batch size (tests force each)

    def _add_bits(self, bits) -> None:
        """the stream `bits` (int32 bit patterns, in order) through ``add_alt`` one after the other"""
        if self._add_policy not in ("auto", "local", "rebuild"):
            raise ValueError(f"unknown _add_policy {self._add_policy!r}")
        if int(bits.numel()) == 0:
            return
        # an empty filter bulk-builds; q < 5: the table's metadata is one replicated word, which the in-place kernels do not take.
        # "auto" goes by the LENGTH of the stream (an upper bound of its distinct count, known without a sort): a long stream of few distinct
        # hashes takes the rebuild, which costs time and nothing else
        held = self._held
        local = self._add_policy == "local" or (self._add_policy == "auto" and self._q >= ADD_LOCAL_MIN_QUOTIENT
                                                and int(bits.numel()) <= held * ADD_LOCAL_MAX_FRACTION)
        if local and held and self._q >= 5 and self._add_local(bits):
            return
        self._add_rebuild(bits)

    def _add_local(self, bits) -> bool:
        """in place, if the stream neither changes the quotient nor fills the table -> False: nothing was changed, the rebuild is to take it"""
        held, stale, q = self._held, self._stale, self._q
        batch = self._usort(bits, unique=True)
        n = int(batch.numel())
        limit = resize_threshold(q, self._max_load_factor) if self._auto_resize else self._size
        if held + n + stale >= limit:
            # close to the threshold (or the last slot): the exact count of new hashes decides, and psk_qf_check_alt gives it
            present = torch.empty(n, dtype=torch.uint8, device=self._dev)
            N.check(N.lib().psk_qf_check_alt(*self._table_args(), batch.data_ptr(), n, present.data_ptr(), self._device, self._stream))
            batch = batch[present == 0]
            n = int(batch.numel())
            total = held + n
            if self._auto_resize and total + stale >= limit:
                return False  # the threshold is reached inside this stream: where decides whether the table doubles
            plan_add(q, held, stale, [total], False)  # "insufficient space", before anything changes
            if total >= self._size:
                return False  # the last slot: a region may come round to its own start, the build places such a table
            if n == 0:
                return True
        # (else: even if every hash of the batch is new the quotient stays and slots remain; hashes in the table already are no-ops of the kernels)
        scratch = self._take_scratch(n)
        result = torch.empty(2, dtype=torch.int32, device=self._dev)
        N.check(N.lib().psk_qf_add_alt(*self._table_args(), batch.data_ptr(), n, scratch.data_ptr(), result.data_ptr(), self._device, self._stream))
        added, status = result.tolist()
        self._remove_scratch = scratch
        if status:
            return False  # refused: nothing was written
        self._held = held + added
        return True

    def _take_scratch(self, n: int):
        """the one scratch of the in-place kernels (2 * words + 2 + n for both), zeroed; both hand it back zeroed.  A call
        that fails may leave bits behind: only a call that ran gives it back"""
        words = int(self._occ.numel())
        if self._remove_scratch is None or int(self._remove_scratch.numel()) < 2 * words + 2 + n:
            self._remove_scratch = torch.zeros(2 * words + 2 + max(n, 1024), dtype=torch.int32, device=self._dev)
        scratch, self._remove_scratch = self._remove_scratch, None
        return scratch

    def _add_rebuild(self, bits) -> None:
        m = int(bits.numel())
        held, stale = self._held, self._stale
        old = self._decode()[0] if held else None
        union = self._usort(bits if old is None else torch.cat([old, bits]), unique=True)
        total = int(union.numel())
        q = self._q
        if self._auto_resize and total + stale >= resize_threshold(q, self._max_load_factor):
            # the threshold is reached inside this stream: whether (and how often) the table doubles depends on WHERE
            order, first = equal_groups(bits ^ _I32_MIN)
            if old is not None:
                first &= ~torch.isin(order.values, old ^ _I32_MIN)
            new = torch.zeros(m, dtype=torch.int64, device=bits.device)
            new[order.indices] = first.to(torch.int64)
            q, stale = plan_add(q, held, stale, held + torch.cumsum(new, 0), True, self._max_load_factor)
        else:
            q, stale = plan_add(q, held, stale, [total], False)  # (quotientfilter.py:357-358, raised there by the insert that finds its counter at the size)
        if q != self._q:
            self._set_params(q)
        self._build(union)
        self._stale = stale

    def add(self, key: KeyT) -> None:
        """Add key to the quotient filter (quotientfilter.py:144-152)"""
        self._add_bits(self._hash_keys(key))

    def add_alt(self, _hash: int) -> None:
        """Add the pre-hashed value to the quotient filter (quotientfilter.py:154-166)"""
        self._add_bits(self._as_bits(int(_hash)))

    def add_many(self, keys) -> None:
        """``for key in keys: add(key)`` as one batch; keys as everywhere in this package (lists, (n, L) uint8 arrays / tensors,
        ragged ``(blob, offsets)`` pairs, host or device)"""
        self._add_bits(self._hash_keys(keys))

    def add_alt_many(self, hashes) -> None:
        """``for h in hashes: add_alt(h)`` as one batch; ints, a numpy array or a torch tensor of 32-bit hashes"""
        self._add_bits(self._as_bits(hashes))

    def remove(self, key: KeyT) -> None:
        raise NotSupportedError("QuotientFilter.remove is not supported: the reference's removal fails on ordinary inputs "
                                "(IndexError: pop from empty list in _fixup_cluster), so there is no behaviour to match")

    def remove_alt(self, _hash: int) -> None:
        self.remove(b"")

    # ------------------------------------------------------------------ batch removal
    _remove_policy = "auto"  # "local": repair the hit clusters in place; "rebuild": decode, drop, build; "auto": by batch size (tests force each)

    def _remove_bits(self, bits) -> int:
        """the stream `bits` (int32 bit patterns) through ``remove_alt`` one after the other -> how many hashes left the table"""
        if self._remove_policy not in ("auto", "local", "rebuild"):
            raise ValueError(f"unknown _remove_policy {self._remove_policy!r}")
        held = self._held
        if int(bits.numel()) == 0 or held == 0:
            return 0
        gone = self._usort(bits, unique=True)
        local = self._remove_policy == "local" or (self._remove_policy == "auto" and int(gone.numel()) <= held * REMOVE_LOCAL_MAX_FRACTION)
        # a full table: the reference may not return, the canonical table of the rest is the defined answer and the rebuild gives it;
        # q < 5: the table's metadata is one replicated word, which the in-place kernels do not take
        if held == self._size or self._q < 5:
            local = False
        removed = self._remove_local(gone) if local else self._remove_rebuild(gone)
        self._held = held - removed
        self._stale += removed  # (the reference's `_elements_added` does not go down: quotientfilter.py:396-414 never touches it)
        return removed

    def _remove_local(self, gone) -> int:
        n = int(gone.numel())
        count = torch.empty(1, dtype=torch.int32, device=self._dev)
        scratch = self._take_scratch(n)
        N.check(N.lib().psk_qf_remove_alt(*self._table_args(), gone.data_ptr(), n, scratch.data_ptr(), count.data_ptr(), self._device, self._stream))
        removed = int(count.item())
        self._remove_scratch = scratch
        return removed

    def _remove_rebuild(self, gone) -> int:
        old = self._decode()[0]
        at = torch.searchsorted(gone ^ _I32_MIN, old ^ _I32_MIN).clamp_(max=int(gone.numel()) - 1)
        keep = old[gone[at] != old]
        removed = int(old.numel() - keep.numel())
        if removed:
            self._build(keep)
        return removed

    def remove_many(self, keys) -> int:
        """``for key in keys: remove(key)`` of the reference as one batch; keys as for ``add_many``.  Absent keys are no-ops.
        Returns the number of hashes removed."""
        return self._remove_bits(self._hash_keys(keys))

    def remove_alt_many(self, hashes) -> int:
        """``for h in hashes: remove_alt(h)`` of the reference as one batch; hashes as for ``add_alt_many``.  Returns the number removed."""
        return self._remove_bits(self._as_bits(hashes))

    # ------------------------------------------------------------------ lookup
    def check_many(self, keys):
        """bool per key (numpy for host keys, a torch tensor for device keys)"""
        if not self._fused:
            return self.check_alt_many(self._hash_keys(keys).cpu().numpy().view(np.uint32))
        b = self._same_device(pack_keys(keys))
        addr, fin = result_buffer(b.where, b.n, np.uint8, torch.uint8, self._device)
        N.check(N.lib().psk_qf_check(*self._table_args(), *b.args(), b.where, addr, self._device, self._stream))
        return as_bool(fin())

    def check_alt_many(self, hashes):
        on_device = torch is not None and isinstance(hashes, torch.Tensor) and hashes.is_cuda
        bits = self._as_bits(hashes)
        out = torch.empty(bits.numel(), dtype=torch.uint8, device=self._dev)
        N.check(N.lib().psk_qf_check_alt(*self._table_args(), bits.data_ptr() if bits.numel() else None, bits.numel(), out.data_ptr(), self._device,
                                         self._stream))
        return as_bool(out if on_device else out.cpu().numpy())

    def check(self, key: KeyT) -> bool:
        """Check to see if key is likely in the quotient filter (quotientfilter.py:187-195)"""
        return bool(self.check_many(key)[0])

    def check_alt(self, _hash: int) -> bool:
        return bool(self.check_alt_many([int(_hash)])[0])

    def __contains__(self, val: KeyT) -> bool:
        return self.check(val)

    # ------------------------------------------------------------------ contents
    def hashes(self) -> Iterator[int]:
        """A generator over the hashes in the quotient filter, in the reference's order"""
        yield from self.get_hashes()

    def get_hashes(self) -> list[int]:
        """Get the hashes from the quotient filter as a list (quotientfilter.py:240-245)"""
        return self._to_ints(self._reference_order())

    def resize(self, quotient: int | None = None) -> None:
        """Resize the quotient filter to use the new quotient size; ``None`` doubles it (quotientfilter.py:247-274)"""
        if quotient is None:
            quotient = self._q + 1
        if self.elements_added >= (1 << quotient):
            raise QuotientFilterError("Unable to shrink since there will be too many elements in the quotient filter")
        _check_quotient(quotient)
        stream = self._reference_order()
        self._set_params(quotient)
        self._add_bits(stream)  # the reference re-adds through add_alt too: a table left at its load threshold expands again

    def merge(self, second: "QuotientFilter") -> None:
        """Merge the `second` quotient filter into the first (quotientfilter.py:276-289)"""
        if self._hash_func("test", 0) != second._hash_func("test", 0):
            raise QuotientFilterError("Hash functions do not match")
        theirs = second._reference_order() if isinstance(second, QuotientFilter) else self._as_bits(list(second.hashes()))
        self._add_bits(theirs.to(self._dev))

    def validate_metadata(self, verbose=False) -> bool:
        """Check for invalid bit settings: a continuation that is not shifted (quotientfilter.py:521-538 names both such rows)"""
        self._alloc()
        bad = self._cont & ~self._sh
        if not bool(bad.any().item()):
            return True
        if verbose:
            rows = np.flatnonzero(np.unpackbits(bad.cpu().numpy().view(np.uint8), bitorder="little")[: self._size])
            for i in rows:
                print(f"Row failed: {i}")
        return False
