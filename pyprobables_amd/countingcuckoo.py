"""CountingCuckooFilter on the GPU (reference: ``probables/cuckoo/countingcuckoo.py``): the cuckoo filter as a multiset.

The table is ``uint32[capacity][bucket_size][2]``, (fingerprint, count) pairs, rows filled from the left: the reference's export byte for
byte.  The insert machinery is :class:`CuckooFilter`'s (parallel placement in front of the first kick, the one-lane walk that carries
``random``'s MT19937); three behaviours of the reference decide what a batch has to do on top of it:

* a repeat increments the first bin that holds its fingerprint and ``elements_added``; an evicted bin keeps its count;
* an expansion LOSES counts: the bin ``_insert_fingerprint_alt`` takes in hand is built with count 1 whatever it was handed, and every
  re-insert adds 1 (not its count) to ``elements_added`` -- so after an expansion ``elements_added == unique_elements``;
* the leftover of a failed walk is a bin, count included: it goes first into the expansion (or is dropped without ``auto_expand``).

So the increments of a batch cannot all be applied at the end: ``add_many`` keeps the position ``seg`` where the current segment starts,
applies the repeats of ``[seg, p)`` when the walk of the key at ``p`` fails -- those of the leftover's own fingerprint find no bin and go
onto the leftover -- expands, and goes on with ``seg = p + 1``; the repeats behind the last expansion are applied at the end.  Repeats are
applied per DISTINCT fingerprint with their multiplicity (``psk_cck_add_counts``): a key repeated a million times is one weighted add.

Deviations, both documented in DESIGN.md 3.12: a count that would pass 2^32 - 1 raises ``OverflowError`` AFTER the call (that bin is left as
it was, the rest of the batch is applied; the reference's ``array("I")`` raises at that add), and an import that holds a non-zero
fingerprint with count 0 raises :class:`InitializationError` (the reference keeps the bin and fails with ``OverflowError`` at its removal).
"""

from __future__ import annotations

import numpy as np

from . import _native as N
from ._base import equal_groups
from .cuckoo import _FOOTER, _NONE, CuckooFilter
from . import cuckoo as _ck
from .exceptions import InitializationError, NativeLibraryError, NotSupportedError
from .hashes import KeyT

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


class CountingCuckooBin:
    """one (fingerprint, count) pair of a bucket, as ``buckets`` lists them"""

    __slots__ = ("finger", "count")

    def __init__(self, fingerprint: int, count: int) -> None:
        self.finger, self.count = int(fingerprint), int(count)

    def __contains__(self, val: int) -> bool:
        return self.finger == val

    def __eq__(self, other) -> bool:
        return isinstance(other, CountingCuckooBin) and (self.finger, self.count) == (other.finger, other.count)

    def __hash__(self) -> int:
        return hash((self.finger, self.count))

    def __repr__(self) -> str:
        return f"(fingerprint:{self.finger} count:{self.count})"


class CountingCuckooFilter(CuckooFilter):
    """Counting cuckoo filter with the bins in GPU memory; the reference's surface plus the batch calls.  Arguments as for
    :class:`CuckooFilter`."""

    _EXPAND_FAILED = "The CountingCuckooFilter failed to expand"
    _HOST_DEDUP = True

    def __init__(self, capacity: int = 10000, bucket_size: int = 4, max_swaps: int = 500, expansion_rate: int = 2, auto_expand: bool = True,
                 finger_size: int = 4, filepath=None, hash_function=None, device=None):
        self._unique_elements = 0
        self._batch = None  # (fingerprints of the batch, positions of its repeats, seg) while an add_many runs
        super().__init__(capacity, bucket_size, max_swaps, expansion_rate, auto_expand, finger_size, filepath, hash_function, device)

    def __contains__(self, key: KeyT) -> bool:
        return self.check(key) > 0

    @property
    def unique_elements(self) -> int:
        """int: unique number of elements inserted"""
        return self._unique_elements

    @property
    def buckets(self) -> list[list[CountingCuckooBin]]:
        """list(list): The buckets holding the bins (a host copy)"""
        self._alloc()
        rows, fill = self._buckets.cpu().numpy().view(np.uint32), self._fill.cpu().numpy()
        return [[CountingCuckooBin(f, c) for f, c in rows[r, : fill[r]].tolist()] for r in range(self._capacity)]

    def load_factor(self) -> float:
        """float: How full the Cuckoo Filter is currently"""
        return self.unique_elements / (self.capacity * self.bucket_size)

    # ------------------------------------------------------------------ the table
    def _new_table(self) -> None:
        self._buckets = torch.zeros((self._capacity, self._bucket_size, 2), dtype=torch.int32, device=self._dev)
        self._fill = torch.zeros(self._capacity, dtype=torch.int32, device=self._dev)
        self._marks = None

    @property
    def bins_tensor(self):
        """``uint32[capacity][bucket_size][2]`` as an int32 device tensor: (fingerprint, count), rows filled from the left, unused pairs 0"""
        self._alloc()
        return self._buckets

    buckets_tensor = bins_tensor

    def _load(self, data: bytes) -> None:
        """countingcuckoo.py:275-303: pairs whose fingerprint is 0 vanish wherever they stand, the others move left, in order"""
        size = len(data) - _FOOTER.size
        if size < 0:
            raise InitializationError("CuckooFilter: failed to load provided file")
        self._bucket_size, self._max_swaps = _FOOTER.unpack(data[size:])
        if self._bucket_size < 1:
            raise InitializationError("CuckooFilter: failed to load provided file")
        B = self._bucket_size
        self._capacity = size // 8 // B
        rows = np.frombuffer(data, dtype="<u4", count=self._capacity * B * 2).reshape(self._capacity, B, 2).astype(np.uint32)
        gone = rows[:, :, 0] == 0
        order = np.argsort(gone, axis=1, kind="stable")
        rows = np.take_along_axis(rows, order[:, :, None], axis=1)
        fill = np.count_nonzero(~gone, axis=1).astype(np.uint32)
        live = np.arange(B)[None, :] < fill[:, None]
        rows[~live] = 0
        if np.any(rows[:, :, 1][live] == 0):
            raise InitializationError("CountingCuckooFilter: the provided filter holds a fingerprint whose count is 0")
        self._pending = (np.ascontiguousarray(rows), fill)
        self._buckets = self._fill = self._marks = None
        self._elements_added = int(rows[:, :, 1].sum(dtype=np.uint64))
        self._unique_elements = int(fill.sum())

    # ------------------------------------------------------------------ what the insert machinery of CuckooFilter asks
    def _present_entry(self):
        return N.lib().psk_cck_present

    def _slots_used(self) -> int:
        return self._unique_elements

    def _added(self, k: int) -> None:
        self._elements_added += k
        self._unique_elements += k

    def _place_apply(self, window, claims, pos, w: int, d, prefix: int, counts) -> None:
        N.check(N.lib().psk_cck_place_apply(*self._geom(), *self._table(), window.data_ptr(), claims.data_ptr(), pos.data_ptr(), w, d.data_ptr(), prefix,
                                            None if counts is None else counts.data_ptr(), self._device, self._stream))

    def _insert_launch(self, tr, start: int, end: int, dedup: bool, mt, res, counts) -> None:
        N.check(N.lib().psk_cck_insert(*self._geom(), min(self._max_swaps, _NONE), *self._table(), tr.data_ptr(), None if counts is None else counts.data_ptr(),
                                       int(tr.shape[1]), start, end, _ck.SEQ_BUDGET, mt.data_ptr(), res.data_ptr(), self._device, self._stream))

    def _leftover(self, res):
        return (int(res[2]) & _NONE, int(res[9]) & _NONE)

    def _survivors(self, tr):
        sub, at = super()._survivors(tr)
        if self._batch is not None and self._batch["repeats"] is None:
            repeat = torch.ones(int(tr.shape[1]), dtype=torch.bool, device=tr.device)
            repeat[at] = False
            self._batch["repeats"] = torch.nonzero(repeat).reshape(-1)
        return sub, at

    def _apply_repeats(self, end: int, leftover=None):
        """the repeats of the batch at positions [seg, end): every distinct fingerprint gets its multiplicity added to its first bin; what
        finds no bin belongs to `leftover` -> the leftover with those counted in"""
        b = self._batch
        rep = b["repeats"]
        sel = rep[(rep >= b["seg"]) & (rep < end)]
        b["seg"] = end + 1
        k = int(sel.numel())
        if not k:
            return leftover
        fps, mult = torch.unique(b["fps"][sel], return_counts=True)  # (one sort per segment)
        u = int(fps.numel())
        tr = self._triples_of_fingerprints(fps)
        weights = mult.to(torch.int32)  # (a batch holds fewer than 2^32 keys; the bit pattern is the uint32)
        missed = torch.empty(u, dtype=torch.uint8, device=self._dev)
        flags = torch.empty(2, dtype=torch.int32, device=self._dev)
        N.check(N.lib().psk_cck_add_counts(*self._geom(), *self._table(), tr.data_ptr(), weights.data_ptr(), u, missed.data_ptr(), flags.data_ptr(), self._device,
                                           self._stream))
        self._elements_added += k
        n_missed, n_over = (int(x) & _NONE for x in flags.tolist())
        if n_missed:
            at = torch.nonzero(missed == 1).reshape(-1)
            lost = [(int(f) & _NONE, int(m)) for f, m in zip(fps[at].tolist(), mult[at].tolist())]
            if leftover is None or len(lost) != 1 or lost[0][0] != leftover[0]:
                raise NativeLibraryError("psk_cck_add_counts: a repeated fingerprint is neither in the table nor the one a failed walk left over")
            if leftover[1] + lost[0][1] > _NONE:
                n_over += 1
                self._elements_added -= lost[0][1]
            else:
                leftover = (leftover[0], leftover[1] + lost[0][1])
        if n_over:
            self._elements_added -= int(mult[missed == 2].sum().item())
            b["overflow"] = True
        return leftover

    def _walk_failed(self, at: int, leftover):
        return self._apply_repeats(at, leftover) if self._batch is not None else leftover

    def _expand_with(self, leftover, mt) -> None:
        """countingcuckoo.py:305-316: [leftover] + every bin in bucket then slot order, each re-inserted with its count -- which only a bin
        that is placed directly keeps"""
        self._alloc()
        B = self._bucket_size
        live = torch.arange(B, dtype=torch.int32, device=self._dev)[None, :] < self._fill[:, None]
        bins = self._buckets[live]  # (k, 2)
        if leftover is not None:
            first = torch.tensor([[v if v < 2**31 else v - 2**32 for v in leftover]], dtype=torch.int32, device=self._dev)
            bins = torch.cat([first, bins])
        capacity = self._capacity * self._expansion_rate
        if not isinstance(capacity, int) or capacity < 1 or capacity >= 2**31:
            raise NotSupportedError(f"CountingCuckooFilter: cannot expand to a capacity of {capacity}")
        self._capacity = capacity
        self._elements_added = self._unique_elements = 0
        self._new_table()
        self.last_insert_stats["expansions"] = self.last_insert_stats.get("expansions", 0) + 1
        batch, self._batch = self._batch, None  # (the re-insert stream is no batch of keys: its failed walk is the end)
        try:
            self._run(self._triples_of_fingerprints(bins[:, 0].contiguous()), False, mt, expanding=True, counts=bins[:, 1].contiguous())
        finally:
            self._batch = batch

    # ------------------------------------------------------------------ the batch calls
    def add_many(self, keys) -> None:
        """``for key in keys: add(key)`` as one batch (keys as for :class:`CuckooFilter`).  Raises :class:`CuckooFilterFullError` where the
        loop would, with the table as the loop would leave it and ``.index`` = the position of the key in the batch."""
        tr = self._triples(keys)
        n = int(tr.shape[1])

        def body(mt):
            self._batch = {"fps": tr[0], "repeats": None, "seg": 0, "overflow": False}
            try:
                self._run(tr, True, mt)
                self._apply_repeats(n)
                overflow = self._batch["overflow"]
            finally:
                self._batch = None
            if overflow:
                raise OverflowError("CountingCuckooFilter: a count would pass 2^32 - 1; that bin was left as it was, the rest of the batch is applied")

        self._with_random(body)

    def check_many(self, keys):
        """the count per key: numpy uint32 for host keys, an int32 (bit pattern of the uint32) torch tensor for device keys"""
        return self._lookup(N.lib().psk_cck_check, keys, np.uint32, torch.int32)

    def check(self, key: KeyT) -> int:
        """The number of times an element was inserted (countingcuckoo.py:175-191)"""
        return int(self.check_many(key)[0]) & _NONE

    def remove_many(self, keys):
        """``[remove(key) for key in keys]`` as one batch: bool per key (numpy for host keys, a torch tensor for device keys)"""
        b = self._as_batch(keys)
        on_device = b.where == N.DEVICE
        tr = self._triples(b)
        n = int(tr.shape[1])
        out = torch.zeros(n, dtype=torch.bool, device=self._dev)
        if n:
            # the requests of one fingerprint stand together in a stable sort: rank = position inside the group, group = its number
            order, first = equal_groups(tr[0])
            idx = torch.arange(n, dtype=torch.int64, device=tr.device)
            starts = torch.nonzero(first).reshape(-1)
            group = torch.cumsum(first.to(torch.int64), 0) - 1
            rank = idx - starts[group]
            u = int(starts.numel())
            requests = torch.diff(starts, append=torch.tensor([n], dtype=torch.int64, device=tr.device)).to(torch.int32)
            distinct = tr[:, order.indices[starts]].contiguous()
            granted = torch.empty(u, dtype=torch.int32, device=self._dev)
            emptied = torch.empty(1, dtype=torch.int32, device=self._dev)
            if self._marks is None:
                self._marks = torch.zeros(self._capacity, dtype=torch.int32, device=self._dev)
            N.check(N.lib().psk_cck_remove(*self._geom(), *self._table(), distinct.data_ptr(), requests.data_ptr(), u, self._marks.data_ptr(), granted.data_ptr(),
                                           emptied.data_ptr(), self._device, self._stream))
            got = granted.to(torch.int64) & _NONE
            out[order.indices] = rank < got[group]
            self._elements_added -= int(got.sum().item())
            self._unique_elements -= int(emptied.item()) & _NONE
        return out if on_device else out.cpu().numpy()

    def remove(self, key: KeyT) -> bool:
        """Remove one occurrence of an element from the filter (countingcuckoo.py:193-210)"""
        return bool(self.remove_many(key)[0])
