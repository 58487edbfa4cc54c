"""CuckooFilter on the GPU (reference: ``probables/cuckoo/cuckoo.py``).

The reference's layout depends on the order of the keys and, once a bucket pair is full, on ``random.choice`` / ``random.randint``.
Both are reproducible (DESIGN.md "Cuckoo filter"):

* in front of the first key that needs a kick nothing is random, and where each key lands is the unique fixed point of a triangular
  system -- ``psk_ck_place_sweep`` / ``psk_ck_place_apply`` place that prefix of a batch in parallel, exactly;
* the kicks draw from ``random``'s MT19937.  ``psk_ck_insert`` walks the keys in order on one lane with the generator's 625 words in
  device memory: every insert call reads ``random.getstate()`` before it touches the table and calls ``random.setstate()`` afterwards,
  so the table AND the generator are left as the reference's loop would leave them;
* lookups and removals never draw: one lane per key.

``add_many`` alternates the two insert paths (both exact, so any policy is); ``_insert_policy`` forces one ("parallel": the sequential
kernel gets one key at a time, "sequential": everything) for the tests.

Limits, each a :class:`NotSupportedError` at construction: a ``hash_function`` other than ``fnv_1a`` (a kick needs ``idx_2`` of a
resident fingerprint on the device), more than 32 fingerprint bits (the reference's own ``uint32`` export overflows there), more than 32
fingerprints per bucket.  Tables are taken to be the reference's: every fingerprint in one of its own two buckets.
"""

from __future__ import annotations

import math
import random
import struct
import time
from io import IOBase
from mmap import mmap
from numbers import Number
from pathlib import Path

import numpy as np

from . import _native as N
from ._base import DeviceResident, _resolve_device, as_bool, equal_groups, require_device, result_buffer
from .exceptions import CuckooFilterFullError, InitializationError, NativeLibraryError, NotSupportedError
from .hashes import KeyT, fnv_1a
from .keys import KeyBatch, pack_keys

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

MAX_BUCKET_SIZE = 32
_FOOTER = struct.Struct("II")
_NONE = 0xFFFFFFFF

# one psk_ck_insert launch: at most this many steps (a key and a swap are one step each).  Measured on one MI355X: 1303 .. 1315 ns per step
# with the table in L2, 1523 ns with a 512 MiB table (profiles/cuckoo_bench.txt), so 2^19 steps are 0.69 .. 0.80 s: the largest power of
# two that keeps a launch under a second
SEQ_BUDGET = 1 << 19
SEQ_CHUNK = 1 << 16      # keys handed to the sequential kernel before the parallel path gets another try
PAR_WINDOW = 1 << 22     # keys whose claims one parallel pass sorts
PAR_MIN = 1 << 12        # a parallel pass that places fewer keys than this is not tried again until the table has grown
MAX_SWEEPS = 32


def state_to_words(state) -> np.ndarray:
    """``random.getstate()`` -> the 625 uint32 words ``psk_ck_insert`` reads (624 of MT19937 and the index)"""
    version, internal, _ = state
    if version != 3 or len(internal) != 625:
        raise ValueError("not a random.getstate() tuple of version 3")
    return np.asarray(internal, dtype=np.uint32)


def words_to_state(words, like) -> tuple:
    """the 625 words back into a ``random.setstate()`` tuple; ``gauss_next`` is `like`'s (choice / randint never touch it)"""
    w = np.asarray(words, dtype=np.uint32).reshape(-1)
    if w.size != 625 or int(w[624]) > 624:
        raise ValueError("need 624 generator words and an index of at most 624")
    return (3, tuple(int(x) for x in w), like[2])


def _is_default_hash(hash_function) -> bool:
    if hash_function is None or hash_function is fnv_1a:
        return True
    if getattr(hash_function, "__module__", None) == "probables.hashes" and getattr(hash_function, "__name__", None) == "fnv_1a":
        try:
            return hash_function("this is a test €") == fnv_1a("this is a test €")
        except Exception:
            return False
    return False


class CuckooFilter(DeviceResident):
    """Cuckoo filter with the buckets in GPU memory; same surface as the reference's class plus the batch calls.

    Args:
        capacity (int): The number of bins
        bucket_size (int): The number of buckets per bin (at most 32 here)
        max_swaps (int): The number of cuckoo swaps before stopping
        expansion_rate (int): The rate at which to expand
        auto_expand (bool): If the filter should automatically expand
        finger_size (int): The size of the fingerprint to use in bytes (between 1 and 4)
        filepath (str): The path to the file to load or None if no file
        hash_function (function): ``None`` or ``fnv_1a``; anything else raises :class:`NotSupportedError`
        device: HIP device index (default: torch's current device)
    """

    _NOUN = "filter"

    def __init__(self, capacity: int = 10000, bucket_size: int = 4, max_swaps: int = 500, expansion_rate: int = 2, auto_expand: bool = True,
                 finger_size: int = 4, filepath=None, hash_function=None, device=None):
        valid_prms = (isinstance(capacity, Number) and capacity >= 1 and isinstance(bucket_size, Number) and bucket_size >= 1
                      and isinstance(max_swaps, Number) and max_swaps >= 1)
        if not valid_prms:
            raise InitializationError("CuckooFilter: capacity, bucket_size, and max_swaps must be an integer greater than 0")
        if not _is_default_hash(hash_function):
            raise NotSupportedError("CuckooFilter: only the default hash_function (fnv_1a) is supported: a kick needs the second index of "
                                    "a resident fingerprint on the device")
        self._device = _resolve_device(device)
        self._hash_func = fnv_1a
        self._bucket_size = int(bucket_size)
        self._capacity = int(capacity)
        self._max_swaps = int(max_swaps)
        self._expansion_rate = expansion_rate
        self._auto_expand = bool(auto_expand)
        self._fingerprint_size = 32
        self.fingerprint_size = finger_size
        self._elements_added = 0
        self._buckets = self._fill = self._marks = None
        self._pending = None  # (buckets, fill) of a loaded filter, on the host until the first call that needs the table
        self._insert_policy = "auto"
        self.last_insert_stats = {}
        if filepath is not None:
            path = Path(filepath).expanduser() if isinstance(filepath, (str, Path)) else None
            if path is None or not path.is_file():
                raise InitializationError("CuckooFilter: failed to load provided file")
            self._load(path.read_bytes())
        self._check_limits()
        self._error_rate = float(self._calc_error_rate())

    def _check_limits(self) -> None:
        if self._bucket_size > MAX_BUCKET_SIZE:
            raise NotSupportedError(f"CuckooFilter: bucket_size up to {MAX_BUCKET_SIZE} is supported; {self._bucket_size} was provided")
        if self._fingerprint_size > 32:
            raise NotSupportedError(f"CuckooFilter: fingerprints of up to 32 bits are supported ({self._fingerprint_size} asked for): the "
                                    "export format holds 32-bit words")
        if self._capacity >= 2**31:
            raise NotSupportedError("CuckooFilter: capacity below 2^31 is supported")

    @classmethod
    def init_error_rate(cls, error_rate: float, capacity: int = 10000, bucket_size: int = 4, max_swaps: int = 500, expansion_rate: int = 2,
                        auto_expand: bool = True, hash_function=None, device=None):
        """Initialize a simple Cuckoo Filter based on error rate (cuckoo.py:102-135)"""
        cku = cls(capacity=capacity, bucket_size=bucket_size, auto_expand=auto_expand, max_swaps=max_swaps, expansion_rate=expansion_rate,
                  hash_function=hash_function, device=device)
        cku._set_error_rate(error_rate)
        return cku

    @classmethod
    def load_error_rate(cls, error_rate: float, filepath, hash_function=None, device=None):
        """Initialize a previously exported Cuckoo Filter based on error rate (cuckoo.py:137-155)"""
        cku = cls(filepath=filepath, hash_function=hash_function, device=device)
        cku._set_error_rate(error_rate)
        return cku

    @classmethod
    def frombytes(cls, b, error_rate: float | None = None, hash_function=None, device=None) -> "CuckooFilter":
        """Load an exported filter from bytes (cuckoo.py:157-177)"""
        cku = cls(hash_function=hash_function, device=device)
        cku._load(bytes(b))
        cku._check_limits()
        cku._set_error_rate(error_rate)
        return cku

    # ------------------------------------------------------------------ properties (cuckoo.py:196-289)
    def __contains__(self, key: KeyT) -> bool:
        return self.check(key)

    def __str__(self):
        return (f"{self.__class__.__name__}:\n"
                f"\tCapacity: {self.capacity}\n"
                f"\tTotal Bins: {self.capacity * self.bucket_size}\n"
                f"\tLoad Factor: {self.load_factor() * 100}%\n"
                f"\tInserted Elements: {self.elements_added}\n"
                f"\tMax Swaps: {self.max_swaps}\n"
                f"\tExpansion Rate: {self.expansion_rate}\n"
                f"\tAuto Expand: {self.auto_expand}")

    @property
    def elements_added(self) -> int:
        """int: The number of elements added"""
        return self._elements_added

    @property
    def capacity(self) -> int:
        """int: The number of bins"""
        return self._capacity

    @property
    def max_swaps(self) -> int:
        """int: The maximum number of swaps to perform"""
        return self._max_swaps

    @property
    def bucket_size(self) -> int:
        """int: The number of buckets per bin"""
        return self._bucket_size

    @property
    def buckets(self) -> list[list[int]]:
        """list(list): The buckets holding the fingerprints (a host copy)"""
        self._alloc()
        rows, fill = self._buckets.cpu().numpy().view(np.uint32), self._fill.cpu().numpy()
        return [rows[r, : fill[r]].tolist() for r in range(self._capacity)]

    @property
    def expansion_rate(self) -> int:
        """int: The rate at expansion when the filter grows"""
        return self._expansion_rate

    @expansion_rate.setter
    def expansion_rate(self, val: int):
        self._expansion_rate = val

    @property
    def error_rate(self) -> float:
        """float: The error rate of the cuckoo filter"""
        return self._error_rate

    @property
    def auto_expand(self) -> bool:
        """bool: True if the cuckoo filter will expand automatically"""
        return self._auto_expand

    @auto_expand.setter
    def auto_expand(self, val: bool):
        self._auto_expand = bool(val)

    @property
    def fingerprint_size_bits(self) -> int:
        """int: The size in bits of the fingerprint"""
        return self._fingerprint_size

    @property
    def fingerprint_size(self) -> int:
        """int: The size in bytes of the fingerprint"""
        return math.ceil(self.fingerprint_size_bits / 8)

    @fingerprint_size.setter
    def fingerprint_size(self, val: int):
        if not 1 <= val <= 4:
            raise ValueError(f"{self.__class__.__name__}: fingerprint size must be between 1 and 4")
        self._fingerprint_size = val * 8
        self._calc_error_rate()

    @property
    def hash_function(self):
        return self._hash_func

    def load_factor(self) -> float:
        """float: How full the Cuckoo Filter is currently"""
        return self.elements_added / (self.capacity * self.bucket_size)

    def _calc_error_rate(self):
        return float(1 / (2 ** (self.fingerprint_size_bits - (math.log2(self.bucket_size) + 1))))

    def _calc_fingerprint_size(self) -> int:
        return int(math.ceil(math.log2(1.0 / self.error_rate) + math.log2(self.bucket_size) + 1))

    def _set_error_rate(self, error_rate) -> None:
        if error_rate is not None:
            self._error_rate = error_rate
            self._fingerprint_size = self._calc_fingerprint_size()
            self._check_limits()

    # ------------------------------------------------------------------ the table
    def _alloc(self) -> None:
        """buckets and fill in HBM.  No device, no table: every call that needs one raises (there is no CPU fallback)"""
        if self._buckets is not None:
            return
        require_device("the cuckoo filter's buckets live in GPU memory")
        if self._pending is not None:
            rows, fill = self._pending
            self._buckets = torch.from_numpy(rows.view(np.int32)).to(self._dev)
            self._fill = torch.from_numpy(fill.view(np.int32)).to(self._dev)
            self._pending = None
        else:
            self._new_table()

    def _new_table(self) -> None:
        self._buckets = torch.zeros((self._capacity, self._bucket_size), dtype=torch.int32, device=self._dev)
        self._fill = torch.zeros(self._capacity, dtype=torch.int32, device=self._dev)
        self._marks = None

    @property
    def buckets_tensor(self):
        """``uint32[capacity][bucket_size]`` as an int32 device tensor: rows filled from the left, unused slots 0"""
        self._alloc()
        return self._buckets

    @property
    def fill_tensor(self):
        """fingerprints per row, int32 device tensor"""
        self._alloc()
        return self._fill

    def synchronize(self) -> None:
        self._alloc()
        super().synchronize()

    def _geom(self):
        return (self._capacity, self._bucket_size)

    def _table(self):
        return (self._buckets.data_ptr(), self._fill.data_ptr())

    # ------------------------------------------------------------------ export / load (cuckoo.py:332-355, :394-431)
    def __bytes__(self) -> bytes:
        if self._pending is not None:
            rows = self._pending[0]
        else:
            self._alloc()
            rows = self._buckets.cpu().numpy()
        return rows.astype("<u4", copy=False).tobytes() + _FOOTER.pack(self._bucket_size, self._max_swaps)

    def export(self, file) -> None:
        """Export cuckoo filter to a path or an open binary file"""
        if isinstance(file, (IOBase, mmap)):
            file.write(bytes(self))
        else:
            Path(file).expanduser().write_bytes(bytes(self))

    def _load(self, data: bytes) -> None:
        size = len(data) - _FOOTER.size
        if size < 0:
            raise InitializationError("CuckooFilter: failed to load provided file")
        self._bucket_size, self._max_swaps = _FOOTER.unpack(data[size:])
        if self._bucket_size < 1:
            raise InitializationError("CuckooFilter: failed to load provided file")
        self._capacity = size // 4 // self._bucket_size
        rows = np.frombuffer(data, dtype="<u4", count=self._capacity * self._bucket_size).reshape(self._capacity, self._bucket_size).astype(np.uint32)
        # zero entries vanish wherever they are in a row: the others move left, in order
        order = np.argsort(rows == 0, axis=1, kind="stable")
        rows = np.ascontiguousarray(np.take_along_axis(rows, order, axis=1))
        fill = np.count_nonzero(rows, axis=1).astype(np.uint32)
        self._pending = (rows, fill)
        self._buckets = self._fill = self._marks = None
        self._elements_added = int(fill.sum())

    # ------------------------------------------------------------------ keys -> triples
    @staticmethod
    def _as_batch(keys) -> KeyBatch:
        if isinstance(keys, KeyBatch):
            return keys
        if isinstance(keys, (str, bytes, bytearray, memoryview)):
            keys = [keys]
        return pack_keys(keys)

    def _triples(self, keys):
        """-> int32 device tensor (3, n): fingerprints, idx_1, idx_2 (uint32 bit patterns) in stream order"""
        self._alloc()
        b = self._same_device(self._as_batch(keys))
        addr, fin = result_buffer(b.where, (3, b.n), np.int32, torch.int32, self._device)
        N.check(N.lib().psk_ck_triples(self._capacity, self._fingerprint_size, *b.args(), b.where, addr, self._device, self._stream))
        return fin() if b.where == N.DEVICE else torch.from_numpy(fin()).to(self._dev)

    def _triples_of_fingerprints(self, fps):
        """fingerprints (int32 bit patterns, device) -> their triples at the CURRENT capacity"""
        n = int(fps.numel())
        rows = (fps.to(torch.int64) & 0xFFFFFFFF).contiguous()
        out = torch.empty((3, n), dtype=torch.int32, device=self._dev)
        if n:
            N.check(N.lib().psk_ck_triples(self._capacity, 32, N.KEYS_HASHES, rows.data_ptr(), None, n, 1, N.DEVICE, out.data_ptr(), self._device, self._stream))
        return out

    # ------------------------------------------------------------------ insert
    # What CountingCuckooFilter (countingcuckoo.py) replaces: the entries that know the slot layout, what a placed fingerprint adds to the
    # totals, what a failed walk leaves over, and what has to happen to the batch before that leftover is dealt with.
    _EXPAND_FAILED = "The CuckooFilter failed to expand"
    _HOST_DEDUP = False  # True: the insert kernel has no dedup of its own, every policy takes the survivors on the host

    def _present(self, tr):
        n = int(tr.shape[1])
        out = torch.empty(n, dtype=torch.uint8, device=self._dev)
        if n:
            N.check(self._present_entry()(*self._geom(), *self._table(), tr.data_ptr(), n, out.data_ptr(), self._device, self._stream))
        return out.view(torch.bool)

    def _present_entry(self):
        return N.lib().psk_ck_present

    def _slots_used(self) -> int:
        return self._elements_added

    def _added(self, k: int) -> None:
        self._elements_added += k

    def _place_apply(self, window, claims, pos, w: int, d, prefix: int, counts) -> None:
        N.check(N.lib().psk_ck_place_apply(*self._geom(), *self._table(), window.data_ptr(), claims.data_ptr(), pos.data_ptr(), w, d.data_ptr(), prefix,
                                           self._device, self._stream))

    def _insert_launch(self, tr, start: int, end: int, dedup: bool, mt, res, counts) -> None:
        N.check(N.lib().psk_ck_insert(*self._geom(), min(self._max_swaps, _NONE), *self._table(), tr.data_ptr(), int(tr.shape[1]), start, end, int(dedup),
                                      SEQ_BUDGET, mt.data_ptr(), res.data_ptr(), self._device, self._stream))

    def _leftover(self, res):
        """what a failed walk leaves over, from the words of its launch"""
        return int(res[2]) & _NONE

    def _walk_failed(self, at: int, leftover):
        """the walk of the key at batch position `at` failed -> the leftover to expand with (or to drop)"""
        return leftover

    def _survivors(self, tr):
        """the keys an ``add`` loop would insert: first occurrence of their fingerprint in the batch, fingerprint not in the table
        -> (their triples, their positions in the batch)"""
        order, first = equal_groups(tr[0])
        keep = torch.zeros(int(tr.shape[1]), dtype=torch.bool, device=tr.device)
        keep[order.indices] = first
        keep &= ~self._present(tr)
        at = torch.nonzero(keep).reshape(-1)
        return tr[:, at].contiguous(), at

    def _place(self, window, counts=None) -> int:
        """parallel placement of the longest provably final prefix of `window` ((3, w) triples) -> keys placed.  The triples are distinct and
        not in the table, so each placed one takes a free slot: no more than the free slots can be placed and the window ends there (which
        also keeps a bucket's claim segment, walked by every sweep, at 2 * bucket_size claims on average)"""
        free = self._capacity * self._bucket_size - self._slots_used()
        window = window[:, :max(free, 1)].contiguous()
        w = int(window.shape[1])
        if w == 0:
            return 0
        L, dev = N.lib(), self._dev
        j2 = torch.arange(w, dtype=torch.int64, device=dev) << 1
        claims = torch.cat([(window[1].to(torch.int64) << 32) | j2, (window[2].to(torch.int64) << 32) | j2 | 1])
        order = torch.sort(claims)
        pos = torch.empty(2 * w, dtype=torch.int32, device=dev)
        pos[order.indices] = torch.arange(2 * w, dtype=torch.int32, device=dev)
        claims = order.values
        d_new, d_old = torch.empty(w, dtype=torch.uint8, device=dev), torch.ones(w, dtype=torch.uint8, device=dev)
        marks = torch.empty(2, dtype=torch.int32, device=dev)
        prefix = sweeps = 0
        for sweeps in range(1, MAX_SWEEPS + 1):
            N.check(L.psk_ck_place_sweep(*self._geom(), self._fill.data_ptr(), window.data_ptr(), claims.data_ptr(), pos.data_ptr(), w, d_old.data_ptr(),
                                         d_new.data_ptr(), marks.data_ptr(), self._device, self._stream))
            d_new, d_old = d_old, d_new  # d_old: the decisions of the sweep just done
            changed, kick = (int(x) & _NONE for x in marks.tolist())
            prefix = min(w, changed, kick)
            if changed == _NONE or kick < changed:  # a fixed point, or the first kick already lies in the final prefix
                break
        stats = self.last_insert_stats
        stats["sweeps"] = stats.get("sweeps", 0) + sweeps
        stats.setdefault("first_place", (sweeps, prefix))  # of the first placement of the call: (sweeps it took, keys it placed)
        if prefix:
            self._place_apply(window, claims, pos, w, d_old, prefix, counts)
            self._added(prefix)
        return prefix

    def _sequential(self, tr, start: int, end: int, dedup: bool, mt, counts=None):
        """-> (status, first key not done, what the failed walk left over, keys that walked)"""
        res = torch.zeros(12, dtype=torch.int32, device=self._dev)
        walked, stats, t0 = 0, self.last_insert_stats, time.perf_counter()
        while True:  # one launch, or as many as a walk that outlives the launch's budget needs: `res` carries it from one to the next
            self._insert_launch(tr, start, end, dedup, mt, res, counts)
            words = res.tolist()
            status, start, _, added, began = (int(x) & _NONE for x in words[:5])
            if status == 2:
                raise NativeLibraryError("psk_ck_insert: the table or the key stream is not a cuckoo filter's (index outside the table, or no draw accepted)")
            self._added(added)
            walked += began
            # (the read of `res` waited for the kernel: steps and seconds of the launches, what SEQ_BUDGET is sized from)
            stats["sequential_steps"] = stats.get("sequential_steps", 0) + (int(words[5]) & _NONE)
            if status != 3:
                stats["sequential_seconds"] = stats.get("sequential_seconds", 0.0) + time.perf_counter() - t0
                return status, start, self._leftover(words) if status == 1 else None, walked

    def _run(self, tr, dedup: bool, mt, expanding: bool = False, counts=None) -> None:
        """the stream `tr` through ``add`` (dedup) or through the re-insert loop of ``_expand_logic`` (not dedup; `counts`: what the counting
        filter's bins carry)"""
        policy, stats = self._insert_policy, self.last_insert_stats
        at = None
        if dedup and (policy != "sequential" or self._HOST_DEDUP):
            tr, at = self._survivors(tr)
        m = int(tr.shape[1])
        done, parallel = 0, policy != "sequential"
        while done < m:
            if parallel:
                placed = self._place(tr[:, done:done + PAR_WINDOW], None if counts is None else counts[done:done + PAR_WINDOW])
                stats["parallel_keys"] = stats.get("parallel_keys", 0) + placed
                done += placed
                if done >= m:
                    break
                if policy == "auto" and placed < PAR_MIN:
                    parallel = False
            end = done + 1 if policy == "parallel" else min(m, done + SEQ_CHUNK)
            status, nxt, leftover, walked = self._sequential(tr, done, end, dedup, mt, counts)
            stats["sequential_keys"] = stats.get("sequential_keys", 0) + nxt - done + (status == 1)
            stats["kicked_keys"] = stats.get("kicked_keys", 0) + walked
            done = nxt
            if status != 1:
                continue
            if expanding:
                raise CuckooFilterFullError(self._EXPAND_FAILED)
            failed = int(at[done]) if at is not None else done  # the key of the batch that could not be inserted
            leftover = self._walk_failed(failed, leftover)
            if not self._auto_expand:
                err = CuckooFilterFullError(f"The {self.__class__.__name__} is currently full")
                err.index = failed
                raise err
            try:
                self._expand_with(leftover, mt)
            except CuckooFilterFullError as err:
                err.index = failed
                raise
            done += 1
            tr = self._triples_of_fingerprints(tr[0])  # the rest of the caller's stream, at the new capacity
            parallel = policy != "sequential"

    def _expand_with(self, leftover, mt) -> None:
        """cuckoo.py:455-481: [leftover] + every fingerprint in bucket then slot order, re-inserted into a table `expansion_rate` times as large"""
        self._alloc()
        B = self._bucket_size
        live = torch.arange(B, dtype=torch.int32, device=self._dev)[None, :] < self._fill[:, None]
        fps = self._buckets[live]
        if leftover is not None:
            fps = torch.cat([torch.tensor([leftover if leftover < 2**31 else leftover - 2**32], dtype=torch.int32, device=self._dev), fps])
        capacity = self._capacity * self._expansion_rate
        if not isinstance(capacity, int) or capacity < 1 or capacity >= 2**31:
            raise NotSupportedError(f"CuckooFilter: cannot expand to a capacity of {capacity}")
        self._capacity = capacity
        self._elements_added = 0
        self._new_table()
        self.last_insert_stats["expansions"] = self.last_insert_stats.get("expansions", 0) + 1
        self._run(self._triples_of_fingerprints(fps), False, mt, expanding=True)

    def _with_random(self, body) -> None:
        """run `body(mt)` between ``random.getstate()`` and ``random.setstate()``: the state is read before the table is first written"""
        self._alloc()
        state = random.getstate()
        mt = torch.from_numpy(state_to_words(state).view(np.int32)).to(self._dev)
        self.last_insert_stats = {}
        try:
            body(mt)
        finally:
            random.setstate(words_to_state(mt.cpu().numpy().view(np.uint32), state))

    def add_many(self, keys) -> None:
        """``for key in keys: add(key)`` as one batch; keys as everywhere in this package (lists, (n, L) uint8 arrays / tensors, ragged
        ``(blob, offsets)`` pairs, host or device).  Raises :class:`CuckooFilterFullError` where the loop would, with the table as the
        loop would leave it and ``.index`` = the position of the key in the batch (the keys behind it are not added)."""
        tr = self._triples(keys)
        self._with_random(lambda mt: self._run(tr, True, mt))

    def add(self, key: KeyT) -> None:
        """Add element key to the filter (cuckoo.py:291-304)"""
        self.add_many(key)

    def expand(self) -> None:
        """Expand the cuckoo filter (cuckoo.py:357-359)"""
        self._with_random(lambda mt: self._expand_with(None, mt))

    # ------------------------------------------------------------------ lookup / removal
    def check_many(self, keys):
        """bool per key (numpy for host keys, a torch tensor for device keys)"""
        return as_bool(self._lookup(N.lib().psk_ck_check, keys, np.uint8, torch.uint8))

    def _lookup(self, entry, keys, np_dtype, torch_dtype):
        """``psk_ck_check`` / ``psk_cck_check``: one answer per key, where the keys are"""
        self._alloc()
        b = self._same_device(self._as_batch(keys))
        addr, fin = result_buffer(b.where, b.n, np_dtype, torch_dtype, self._device)
        N.check(entry(*self._geom(), self._fingerprint_size, *self._table(), *b.args(), b.where, addr, self._device, self._stream))
        return fin()

    def check(self, key: KeyT) -> bool:
        """Check if an element is in the filter (cuckoo.py:306-315)"""
        return bool(self.check_many(key)[0])

    def remove_many(self, keys):
        """``[remove(key) for key in keys]`` as one batch: bool per key (numpy for host keys, a torch tensor for device keys)"""
        b = self._as_batch(keys)
        on_device = b.where == N.DEVICE
        tr = self._triples(b)
        n = int(tr.shape[1])
        out = torch.zeros(n, dtype=torch.uint8, device=self._dev)
        if n:
            # how many earlier requests carry the same fingerprint: position inside the fingerprint's group of a stable sort
            order, first = equal_groups(tr[0])
            idx = torch.arange(n, dtype=torch.int64, device=tr.device)
            group_start = torch.cummax(torch.where(first, idx, torch.zeros_like(idx)), 0).values
            rank = torch.empty(n, dtype=torch.int32, device=tr.device)
            rank[order.indices] = (idx - group_start).to(torch.int32)
            if self._marks is None:
                self._marks = torch.zeros(self._capacity, dtype=torch.int32, device=self._dev)
            N.check(N.lib().psk_ck_remove(*self._geom(), *self._table(), tr.data_ptr(), rank.data_ptr(), n, self._marks.data_ptr(), out.data_ptr(), self._device,
                                          self._stream))
            self._elements_added -= int(out.sum().item())
        return as_bool(out if on_device else out.cpu().numpy())

    def remove(self, key: KeyT) -> bool:
        """Remove an element from the filter (cuckoo.py:317-330)"""
        return bool(self.remove_many(key)[0])
