"""CountMinSketch (+ Count-Mean / Count-Mean-Min query variants) with the width x depth int32 table in
HBM and add / remove / check as fused HIP kernels.

Drop-in for the hot path of ``probables.CountMinSketch`` (``probables/countminsketch/countminsketch.py``).
Single-key ``add`` / ``remove`` run the reference semantics literally (ordered kernel: exact return value,
exact int32 / int64 clamps); ``add_many`` / ``remove_many`` are unordered atomic batches whose final table is
bit-exact whenever it does not depend on the order (same-sign weights, or no bin touching a rail);
``add_many_ordered`` is the batch form of ``add``: what the reference's loop returns for every key of an ordered batch;
``update_many_ordered`` / ``remove_many_ordered`` are the same for batches with removes in them.

``StreamThreshold`` and ``HeavyHitters`` (countminsketch.py:532-843) track a dict that every ``add`` feeds with its return value;
their ``add_many`` is ``add_many_ordered`` plus the dict rule, written as the two pure functions ``threshold_rule`` / ``hitters_rule``.
"""

from __future__ import annotations

import math
import struct
from io import BytesIO, IOBase
from mmap import mmap
from numbers import Number
from pathlib import Path

import numpy as np

from . import _native as N
from ._base import DeviceTable, weights_arg
from .bloom import _existing_file, _torch_dtype
from .exceptions import CountMinSketchError, InitializationError, NotSupportedError
from .hashes import HashFuncT, HashResultsT, KeyT, default_fnv_1a, device_digest, is_fused_fnv
from .keys import KeyBatch, hashed_batch, one_key_bytes, pack_hashes

_I32_MAX, _I32_MIN = 2**31 - 1, -(2**31)
_I64_MAX, _I64_MIN = 2**63 - 1, -(2**63)
_FOOTER = struct.Struct("IIq")  # width, depth, elements_added (countminsketch.py:122)
_QUERIES = {"min": N.Q_MIN, "mean": N.Q_MEAN, "mean-min": N.Q_MEANMIN}


class CountMinSketch:
    """Count-Min sketch on the GPU.

    Args (identical to the reference, countminsketch.py:59-67):
        width, depth, confidence, error_rate, filepath, hash_function
    Extra: device.  Initialisation order: file, then width/depth, then confidence/error_rate."""

    _DEFAULT_QUERY = "min"

    def __init__(self, width=None, depth=None, confidence=None, error_rate=None, filepath=None,
                 hash_function: HashFuncT | None = None, device=None):
        self._dev_arg = device
        self._els_added = 0
        self._dirty = False
        self._query = self._DEFAULT_QUERY
        self._tab: DeviceTable | None = None
        self._hash_function = default_fnv_1a if hash_function is None else hash_function
        self._is_fused = is_fused_fnv(hash_function)
        self._digest = device_digest(self._hash_function)
        if filepath is not None and _existing_file(filepath):
            self._parse_bytes(Path(filepath).expanduser().resolve().read_bytes())
            return
        self._width, self._depth, self._confidence, self._error_rate = self._geometry(width, depth, confidence, error_rate)
        self._tab = DeviceTable("cms", self._width, self._depth, self._dev_arg)

    @staticmethod
    def _geometry(width, depth, confidence, error_rate):
        """-> (width, depth, confidence, error_rate) from either pair, as the reference sizes a sketch (countminsketch.py:88-113)"""
        if width is not None and depth is not None:
            if not (isinstance(width, Number) and width > 0 and isinstance(depth, Number) and depth > 0):
                raise InitializationError("CountMinSketch: width and depth must be greater than 0")
            width, depth = int(width), int(depth)
            return width, depth, 1 - (1 / math.pow(2, depth)), 2 / width
        if confidence is not None and error_rate is not None:
            if not (isinstance(confidence, Number) and confidence > 0 and isinstance(error_rate, Number) and error_rate > 0):
                raise InitializationError("CountMinSketch: width and depth must be greater than 0")
            width = math.ceil(2 / error_rate)                                   # countminsketch.py:102
            depth = math.ceil((-1 * math.log(1 - confidence)) / 0.6931471805599453)  # :103-104
            return width, depth, confidence, error_rate
        raise InitializationError(
            "Must provide one of the following to initialize the Count-Min Sketch:\n"
            "    A file to load,\n"
            "    The width and depth,\n"
            "    OR confidence and error rate"
        )

    # ------------------------------------------------------------------ properties
    @property
    def width(self) -> int:
        return self._width

    @property
    def depth(self) -> int:
        return self._depth

    @property
    def confidence(self) -> float:
        return self._confidence

    @property
    def error_rate(self) -> float:
        return self._error_rate

    def _fold_counters(self) -> None:
        if self._tab is None or not self._dirty:
            return
        c = self._tab.counters()
        e = self._els_added + c[N.CTR_ADDED] - c[N.CTR_REMOVED]
        self._els_added = max(min(e, _I64_MAX), _I64_MIN)  # countminsketch.py:285-287, 317-319 (per batch)
        self._saturated = getattr(self, "_saturated", 0) + c[N.CTR_SATURATED]
        self._tab.reset_counters()
        self._dirty = False

    @property
    def elements_added(self) -> int:
        self._fold_counters()
        return self._els_added

    def batch_diagnostics(self) -> dict:
        self._dirty = True
        self._fold_counters()
        return {"saturated": getattr(self, "_saturated", 0)}

    @property
    def query_type(self) -> str:
        return self._query

    @query_type.setter
    def query_type(self, val):
        """'min' | 'mean' | 'mean-min'; anything else means 'min' (countminsketch.py:223-238)"""
        val = val.lower() if isinstance(val, str) else None
        self._query = val if val in ("mean", "mean-min") else "min"

    @property
    def hash_function(self) -> HashFuncT:
        return self._hash_function

    @property
    def device(self) -> int:
        return self._tab.device

    @property
    def table_tensor(self):
        return self._tab.tensor

    def set_engine_option(self, name: str, value) -> None:
        """override an engine tunable for THIS sketch (``psk_sketch_set_option``); ``None`` = follow the process-wide default again"""
        self._tab.set_option(name, value)

    def get_engine_option(self, name: str) -> int:
        return self._tab.get_option(name)

    def scratch_bytes(self) -> dict:
        """device memory the engine holds for this sketch besides its table (``psk_scratch_bytes``)"""
        return self._tab.scratch_bytes()

    def release_scratch(self) -> None:
        self._tab.release_scratch()

    @property
    def _bins(self):
        """host SNAPSHOT of the bins (int32, row-major by depth)"""
        from array import array  # noqa: PLC0415

        return array("i", self._tab.read().tobytes())

    @property
    def _fused(self) -> bool:
        return self._is_fused

    # ------------------------------------------------------------------ dunder / io
    def __str__(self) -> str:
        return (
            "Count-Min Sketch:\n"
            f"\tWidth: {self.width}\n"
            f"\tDepth: {self.depth}\n"
            f"\tConfidence: {self.confidence}\n"
            f"\tError Rate: {self.error_rate}\n"
            f"\tElements Added: {self.elements_added}"
        )

    def __contains__(self, key: KeyT) -> bool:
        return self.check(key) != 0

    def __bytes__(self) -> bytes:
        with BytesIO() as f:
            self.export(f)
            return f.getvalue()

    def export(self, file) -> None:
        """bins + ``IIq`` footer (countminsketch.py:342-354)"""
        blob = self._tab.read().tobytes() + _FOOTER.pack(self.width, self.depth, self.elements_added)
        if isinstance(file, (IOBase, mmap)):
            file.write(blob)
        else:
            Path(file).expanduser().resolve().write_bytes(blob)

    @classmethod
    def frombytes(cls, b, hash_function: HashFuncT | None = None, device=None):
        width, depth, _ = _FOOTER.unpack_from(bytes(b[-_FOOTER.size:]))
        inst = cls(width=width, depth=depth, hash_function=hash_function, device=device)
        inst._parse_bytes(bytes(b))
        return inst

    def _parse_bytes(self, blob: bytes) -> None:
        """countminsketch.py:417-427"""
        width, depth, added = _FOOTER.unpack_from(blob[-_FOOTER.size:])
        self._width, self._depth = width, depth
        self._confidence = 1 - (1 / math.pow(2, depth))
        self._error_rate = 2 / width
        if self._tab is None or (self._tab.m, self._tab.k) != (width, depth):
            self._tab = DeviceTable("cms", width, depth, self._dev_arg)
        self._tab.write(blob[: 4 * width * depth])
        self._els_added, self._dirty = added, False

    def clear(self) -> None:
        self._els_added, self._dirty = 0, False
        self._tab.clear()

    def hashes(self, key: KeyT, depth: int | None = None) -> HashResultsT:
        """the plugin call site (countminsketch.py:246-255)"""
        return self._hash_function(key, self.depth if depth is None else depth)

    # ------------------------------------------------------------------ batches
    def _batch(self, keys) -> KeyBatch:
        b = hashed_batch(keys, self._hash_function, self._is_fused, self._digest, self._depth, self._tab.device, self._tab.stream)
        self._tab.check_batch(b)
        return b

    def _alt(self, hashes) -> KeyBatch:
        b = pack_hashes(hashes, self._depth)
        if b.n and b.key_len != self._depth:
            # countminsketch.py:275 enumerates ALL supplied hashes; more than `depth` runs off the table there
            raise IndexError("array index out of range")
        return b

    def _ordered(self, b: KeyBatch, num_els, opmode: int) -> np.ndarray:
        if b.where != N.HOST:
            raise ValueError("ordered updates take host batches")
        w = np.ascontiguousarray(np.broadcast_to(np.asarray(num_els, dtype=np.int64), (b.n,)))
        out = np.empty(b.n + 1, dtype=np.int64)  # n return values + elements_added after the batch
        els_in = self.elements_added
        N.check(N.lib().psk_cms_update_ordered(self._tab.handle, *b.args(), w.ctypes.data if b.n else None, opmode,
                                               _QUERIES[self._query], els_in, b.where, out.ctypes.data, self._tab.stream))
        self._els_added = int(out[b.n])
        return out[: b.n]

    def _ordered_one(self, key, num_els, opmode: int):
        """one ordered update of one key through the preallocated words (``_base.OneKey``); None: take the general path"""
        raw = one_key_bytes(key) if self._is_fused else None
        if raw is None or type(num_els) is not int or not -(1 << 62) < num_els < 1 << 62:
            return None
        t = self._tab
        one = t.one
        one.w[0] = num_els
        N.check(N.lib().psk_cms_update_ordered(t.handle, N.KEYS_FIXED, raw or None, None, 1, len(raw), one.w_addr, opmode,
                                               _QUERIES[self._query], self.elements_added, N.HOST, one.o_addr, t.stream))
        self._els_added = int(one.o[1])
        return int(one.o[0])

    def add(self, key: KeyT, num_els: int = 1) -> int:
        """countminsketch.py:257-265"""
        res = self._ordered_one(key, num_els, N.OP_ADD)
        return res if res is not None else int(self._ordered(self._batch(key), num_els, N.OP_ADD)[0])

    def add_alt(self, hashes: HashResultsT, num_els: int = 1) -> int:
        """countminsketch.py:267-288"""
        return int(self._ordered(self._alt(hashes), num_els, N.OP_ADD)[0])

    def remove(self, key: KeyT, num_els: int = 1) -> int:
        """countminsketch.py:290-298"""
        res = self._ordered_one(key, num_els, N.OP_REMOVE)
        return res if res is not None else int(self._ordered(self._batch(key), num_els, N.OP_REMOVE)[0])

    def remove_alt(self, hashes: HashResultsT, num_els: int = 1) -> int:
        """countminsketch.py:300-321"""
        return int(self._ordered(self._alt(hashes), num_els, N.OP_REMOVE)[0])

    def update_ordered(self, keys, signed_num_els) -> np.ndarray:
        """strictly ordered mixed stream on the device: ``w >= 0`` adds, ``w < 0`` removes ``-w``; returns
        every op's reference return value (int64[n])"""
        return self._ordered(self._batch(keys), signed_num_els, N.OP_SIGNED)

    def _check_batch(self, b: KeyBatch):
        L = N.lib()
        if self._query == "mean-min":
            addr, fin = self._tab.out_buffer(b, b.n, np.int64, _torch_dtype("int64"))
            N.check(L.psk_cms_check_meanmin(self._tab.handle, *b.args(), b.where, self.elements_added, addr, self._tab.stream))
        else:
            addr, fin = self._tab.out_buffer(b, b.n, np.int32, _torch_dtype("int32"))
            N.check(L.psk_cms_check(self._tab.handle, *b.args(), b.where, _QUERIES[self._query], addr, self._tab.stream))
        return fin()

    def check(self, key: KeyT) -> int:
        """countminsketch.py:323-330"""
        raw = one_key_bytes(key) if self._is_fused else None
        if raw is None:
            return int(self._check_batch(self._batch(key))[0])
        t = self._tab
        one = t.one
        if self._query == "mean-min":
            N.check(N.lib().psk_cms_check_meanmin(t.handle, N.KEYS_FIXED, raw or None, None, 1, len(raw), N.HOST, self.elements_added,
                                                  one.o_addr, t.stream))
            return int(one.o[0])
        N.check(N.lib().psk_cms_check(t.handle, N.KEYS_FIXED, raw or None, None, 1, len(raw), N.HOST, _QUERIES[self._query], one.o_addr,
                                      t.stream))
        return int(one.o_i32[0])

    def check_alt(self, hashes: HashResultsT) -> int:
        """countminsketch.py:332-340"""
        return int(self._check_batch(self._alt(hashes))[0])

    def _update_batch(self, fn, b: KeyBatch, num_els) -> None:
        keep: list = []
        w_addr, _ = weights_arg(num_els, b.n, np.int32, b.where, keep, _I32_MIN, _I32_MAX, self._tab.device)
        N.check(fn(self._tab.handle, *b.args(), w_addr, b.where, self._tab.stream))
        self._dirty = True

    def add_many(self, keys, num_els=None) -> None:
        """ONE kernel launch for the whole batch; ``num_els``: None (=1), an int, or one int32 per key
        (numpy, or a CUDA tensor next to CUDA keys)"""
        self._update_batch(N.lib().psk_cms_add, self._batch(keys), num_els)

    def remove_many(self, keys, num_els=None) -> None:
        self._update_batch(N.lib().psk_cms_remove, self._batch(keys), num_els)

    def _running(self, fn, b: KeyBatch, w, lo: int):
        """``psk_cms_add_running`` / ``psk_cms_update_running``: every op's return value of the ordered batch, on the batch's side"""
        keep: list = []
        w_addr, _ = weights_arg(w, b.n, np.int32, b.where, keep, lo, _I32_MAX, self._tab.device)
        wide = self._query == "mean-min"
        addr, fin = self._tab.out_buffer(b, b.n, np.int64 if wide else np.int32, _torch_dtype("int64" if wide else "int32"))
        els_addr, els = self._tab.out_buffer(b, 1, np.int64, _torch_dtype("int64"))  # elements_added behind the batch (read back for a device batch)
        N.check(fn(self._tab.handle, *b.args(), w_addr, b.where, _QUERIES[self._query], self.elements_added, addr, els_addr, self._tab.stream))
        self._els_added = int(els()[0])
        return fin()

    @staticmethod
    def _weight_range(w):
        """(min, max) of a weight argument as Python integers, None for an empty one (a device tensor costs one small reduction and a
        synchronisation here)"""
        if hasattr(w, "is_cuda"):
            return (int(w.min().item()), int(w.max().item())) if w.numel() else None
        a = np.asarray(w)
        return (int(a.min()), int(a.max())) if a.size else None

    def _add_running(self, b: KeyBatch, num_els):
        w = num_els
        if w is not None:
            if hasattr(w, "is_cuda"):  # a torch tensor (a device one costs one small reduction and a synchronisation here)
                neg = bool(w.numel()) and int(w.min().item()) < 0
            else:
                a = np.asarray(w)
                neg = bool(a.size) and int(a.min()) < 0
            if neg:
                raise ValueError("add_many_ordered: num_els must be >= 0 (removes are not part of an ordered add batch)")
        return self._running(N.lib().psk_cms_add_running, b, num_els, 0)

    def _update_running(self, b: KeyBatch, signed_num_els):
        w = signed_num_els
        if w is not None and not (hasattr(w, "is_cuda") and w.dtype.is_signed and w.element_size() <= 4):  # (an int32 tensor cannot be outside)
            r = self._weight_range(w)
            if r and (r[0] < _I32_MIN or r[1] > _I32_MAX):
                raise ValueError("update_many_ordered: weights must lie in [-2**31, 2**31 - 1]; update_ordered takes int64 weights "
                                 "(and walks the batch on its sequential kernel)")
        return self._running(N.lib().psk_cms_update_running, b, signed_num_els, _I32_MIN)

    def update_many_ordered(self, keys, signed_num_els):
        """the batch form of a mixed stream of ``add`` and ``remove`` (countminsketch.py:257-321): ``w >= 0`` adds ``w``, ``w < 0``
        removes ``-w``; the table and ``elements_added`` end as the loop of single calls leaves them and entry i of the result is what
        that loop's i-th call returns under the current ``query_type`` -- int32 (int64 for 'mean-min'), numpy for host batches, a torch
        tensor for device batches.  Weights are int32 (``-2**31`` removes 2^31); anything outside raises ValueError before anything
        changes -- ``update_ordered`` keeps its int64 weights and its sequential kernel."""
        return self._update_running(self._batch(keys), signed_num_els)

    def update_alt_many_ordered(self, hashes, signed_num_els):
        """``update_many_ordered`` for pre-computed hashes (a (n, depth) uint64 array / tensor)"""
        return self._update_running(self._alt(hashes), signed_num_els)

    @classmethod
    def _negated(cls, num_els):
        """the weights of ``remove_many_ordered`` as ``update_many_ordered`` takes them"""
        if num_els is None:
            return -1
        r = cls._weight_range(num_els)
        if r and (r[0] < 0 or r[1] > _I32_MAX):
            raise ValueError("remove_many_ordered: num_els must lie in [0, 2**31 - 1] (update_many_ordered removes 2**31 with the weight -2**31)")
        if hasattr(num_els, "is_cuda"):
            return -num_els
        return -np.asarray(num_els, dtype=np.int64) if np.ndim(num_els) else -int(num_els)

    def remove_many_ordered(self, keys, num_els=None):
        """the batch form of ``remove`` (countminsketch.py:290-321): ``update_many_ordered`` with the weights negated; ``num_els``
        must be >= 0"""
        return self._update_running(self._batch(keys), self._negated(num_els))

    def remove_alt_many_ordered(self, hashes, num_els=None):
        return self._update_running(self._alt(hashes), self._negated(num_els))

    def add_many_ordered(self, keys, num_els=None):
        """the batch form of ``add`` (countminsketch.py:257-288): the table and ``elements_added`` end as the loop
        ``for key, w in zip(keys, num_els): add(key, w)`` leaves them and entry i of the result is what that loop's i-th ``add`` returns
        under the current ``query_type`` -- int32 (int64 for 'mean-min'), numpy for host batches, a torch tensor for device batches.
        ``keys`` / ``num_els`` as for ``add_many``; ``num_els`` must be >= 0 (ValueError before anything changes)."""
        return self._add_running(self._batch(keys), num_els)

    def add_alt_many_ordered(self, hashes, num_els=None):
        """``add_many_ordered`` for pre-computed hashes (a (n, depth) uint64 array / tensor)"""
        return self._add_running(self._alt(hashes), num_els)

    def add_alt_many(self, hashes, num_els=None) -> None:
        self._update_batch(N.lib().psk_cms_add, self._alt(hashes), num_els)

    def remove_alt_many(self, hashes, num_els=None) -> None:
        self._update_batch(N.lib().psk_cms_remove, self._alt(hashes), num_els)

    def check_many(self, keys):
        """estimated count per key under the current ``query_type``"""
        return self._check_batch(self._batch(keys))

    def check_alt_many(self, hashes):
        return self._check_batch(self._alt(hashes))

    def synchronize(self) -> None:
        self._tab.synchronize()

    # ------------------------------------------------------------------ join (countminsketch.py:356-399)
    def join(self, second: "CountMinSketch") -> None:
        if not isinstance(second, CountMinSketch):
            raise TypeError(f"Unable to merge a count-min sketch with {type(second)}")
        if self.width != second.width or self.depth != second.depth or self.hashes("test") != second.hashes("test"):
            raise CountMinSketchError("Unable to merge as the count-min sketches are mismatched")
        if second._tab.device != self._tab.device:
            raise ValueError("join needs both sketches on the same device")
        t = self._tab
        N.check(N.lib().psk_table_add_sat_i32(t.ptr, second._tab.ptr, self.width * self.depth, t.device, t.stream))
        e = self.elements_added + second.elements_added
        self._els_added = max(min(e, _I64_MAX), _I64_MIN)
        N.check(N.lib().psk_rescan_bound(t.handle, t.stream))  # the joined table may sit on a rail


class CountMeanSketch(CountMinSketch):
    """default query 'mean' (countminsketch.py:456-491)"""

    _DEFAULT_QUERY = "mean"


class CountMeanMinSketch(CountMinSketch):
    """default query 'mean-min' (countminsketch.py:494-529)"""

    _DEFAULT_QUERY = "mean-min"


# ------------------------------------------------------------------ the tracked dicts of StreamThreshold / HeavyHitters
def threshold_rule(tracked: dict, keys, results, threshold: int) -> dict:
    """StreamThreshold's rule (countminsketch.py:800-803) over an ordered batch of adds: ``tracked[key] = res`` for every op with
    ``res >= threshold``, in op order (a later store overwrites an earlier one and keeps the key's place).  ``keys`` / ``results``: the
    ops that matter, or all of them.  Pure host code: dict in, the same dict out."""
    tracked.update((k, int(r)) for k, r in zip(keys, results) if r >= threshold)
    return tracked


def hitters_rule(state, keys, results, num_hitters: int):
    """HeavyHitters' rule (countminsketch.py:643-661) replayed in op order.  ``state`` = (top_x dict, smallest); returns the new state.
    An op that meets a full list, a key that is not tracked and ``res <= smallest`` changes nothing -- the common case of a long stream,
    one dict lookup and one compare here."""
    top, smallest = state
    get = top.get
    for key, res in zip(keys, results):
        res = int(res)
        if len(top) < num_hitters:  # still have room (:646-650; __top_x_size is len(top) at every point the rule reads it)
            top[key] = res
        elif key in top:            # :651-652
            top[key] = res
        elif res > smallest:        # :653-660 something in there is smaller
            top[key] = res
            top.pop(min(top, key=get), None)
            smallest = top[min(top, key=get)]
    return top, smallest


def _batch_keys(keys):
    """the dict keys of a batch: the caller's own str / bytes objects of a list, ``bytes`` for array / tensor batches; -> indexable"""
    if isinstance(keys, (str, bytes, bytearray, memoryview)):
        return [keys]
    if isinstance(keys, tuple) and len(keys) == 2 and hasattr(keys[0], "dtype"):  # ragged (blob, offsets)
        blob, offs = (x.cpu().numpy() if hasattr(x, "is_cuda") else np.asarray(x) for x in keys)
        if blob.dtype.itemsize != 1:
            raise TypeError("tracked keys of a (blob, offsets) batch: a uint8 blob")
        raw, o = blob.tobytes(), offs.astype(np.int64)
        return [raw[o[i]:o[i + 1]] for i in range(o.size - 1)]
    if hasattr(keys, "is_cuda"):
        keys = keys.cpu().numpy()
    if isinstance(keys, np.ndarray):
        a = np.ascontiguousarray(keys)
        a = a.view(np.uint8).reshape(a.shape[0], -1)
        raw, L = a.tobytes(), a.shape[1]
        return [raw[i * L:(i + 1) * L] for i in range(a.shape[0])]
    return keys if isinstance(keys, list) else list(keys)


class StreamThreshold(CountMinSketch):
    """the keys whose count reached ``threshold`` when they were added (countminsketch.py:694-843).

    Args as the reference: threshold, width, depth, confidence, error_rate, filepath, hash_function; extra: device."""

    def __init__(self, threshold=100, width=None, depth=None, confidence=None, error_rate=None, filepath=None,
                 hash_function: HashFuncT | None = None, device=None):
        super().__init__(width, depth, confidence, error_rate, filepath, hash_function, device)
        self._threshold = threshold
        self._meets: dict = {}

    @classmethod
    def frombytes(cls, b, threshold=100, hash_function: HashFuncT | None = None, device=None):
        width, depth, _ = _FOOTER.unpack_from(bytes(b[-_FOOTER.size:]))
        inst = cls(threshold=threshold, width=width, depth=depth, hash_function=hash_function, device=device)
        inst._parse_bytes(bytes(b))
        return inst

    def __str__(self) -> str:
        return f"Stream Threshold {super().__str__()}\n\tThreshold: {self.threshold}\n\tNumber Meeting Threshold: {len(self._meets)}"

    @property
    def meets_threshold(self) -> dict:
        return self._meets

    @property
    def threshold(self) -> int:
        return self._threshold

    def clear(self) -> None:
        super().clear()
        self._meets = {}

    def add(self, key, num_els: int = 1) -> int:
        """countminsketch.py:775-785"""
        res = super().add(key, num_els)
        threshold_rule(self._meets, (key,), (res,), self._threshold)
        return res

    def add_alt(self, key, hashes: HashResultsT, num_els: int = 1) -> int:
        """countminsketch.py:787-803 (key first: the reference's signature)"""
        res = super().add_alt(hashes, num_els)
        threshold_rule(self._meets, (key,), (res,), self._threshold)
        return res

    def _removed(self, key, res: int) -> int:  # :831-834
        if res < self._threshold:
            self._meets.pop(key, None)
        else:
            self._meets[key] = res
        return res

    def remove(self, key, num_els: int = 1) -> int:
        """countminsketch.py:805-815"""
        return self._removed(key, super().remove(key, num_els))

    def remove_alt(self, key, hashes: HashResultsT, num_els: int = 1) -> int:
        """countminsketch.py:817-835"""
        return self._removed(key, super().remove_alt(hashes, num_els))

    def _replay(self, keys, res, neg) -> None:
        """the dict after the ordered batch.  An add stores ``res >= threshold`` (:800-803), a remove stores it as well and pops the key
        otherwise (:831-834): every op at or above the threshold matters, and a remove below it matters only while the dict holds
        something -- it is empty and stays so when nothing of the batch reaches the threshold.  ``neg``: which ops remove, on the side of
        ``res`` (None: none, True: all).  The selected ops alone come to the host and are replayed in op order."""
        sel = res >= self._threshold
        if neg is not None and (self._meets or bool(sel.any())):
            sel = sel | neg
        if hasattr(res, "is_cuda"):
            import torch  # noqa: PLC0415

            at = torch.nonzero(sel).flatten()
            idx, vals = at.cpu().numpy(), res[at].cpu().numpy()
        else:
            idx = np.nonzero(sel)[0]
            vals = res[idx]
        if not idx.size:
            return
        if isinstance(keys, list):
            picked = [keys[i] for i in idx.tolist()]
        elif hasattr(keys, "is_cuda") and keys.is_cuda:  # only the selected rows leave the device
            import torch  # noqa: PLC0415

            picked = _batch_keys(keys[torch.from_numpy(idx).to(keys.device)])
        else:
            allk = _batch_keys(keys)
            picked = [allk[i] for i in idx.tolist()]
        if neg is None:
            threshold_rule(self._meets, picked, vals.tolist(), self._threshold)
            return
        for key, r in zip(picked, vals.tolist()):  # (selected and below the threshold: a remove)
            if r >= self._threshold:
                self._meets[key] = r
            else:
                self._meets.pop(key, None)

    def add_many(self, keys, num_els=None):
        """``add`` for every key of the ordered batch: the sketch through ``add_many_ordered``; of the results only those that reached
        the threshold matter to the dict -- they are selected where the results lie and stored in op order.  Returns the results."""
        res = self.add_many_ordered(keys, num_els)
        self._replay(keys, res, None)
        return res

    def remove_many(self, keys, num_els=None):
        """``remove`` for every key of an ordered batch, host or device: the sketch through ``remove_many_ordered`` (the parallel signed
        passes of ``psk_cms_update_running``), the dict replayed on the host in op order.  Returns the results."""
        res = self.remove_many_ordered(keys, num_els)
        self._replay(keys, res, True)
        return res

    def update_many(self, keys, signed_num_els):
        """a mixed ordered batch: ``w >= 0`` is ``add(key, w)``, ``w < 0`` is ``remove(key, -w)``.  The sketch goes through
        ``update_many_ordered``; the dict is replayed on the host in op order, add ops by ``threshold_rule``, remove ops by the rule of
        ``remove`` (countminsketch.py:831-834).  Returns the results."""
        res = self.update_many_ordered(keys, signed_num_els)
        w = signed_num_els
        if w is None:
            neg = None
        elif hasattr(w, "is_cuda"):
            neg = (w < 0).to(res.device) if hasattr(res, "is_cuda") else (w < 0).numpy()
        elif np.ndim(w) == 0:
            neg = True if int(w) < 0 else None
        else:
            neg = np.asarray(w) < 0
            if hasattr(res, "is_cuda"):
                import torch  # noqa: PLC0415

                neg = torch.from_numpy(neg).to(res.device)
        self._replay(keys, res, neg)
        return res

    def join(self, second) -> None:
        raise NotSupportedError("Joining is not supported for stream threshold")


class HeavyHitters(CountMinSketch):
    """the ``num_hitters`` most common keys seen so far (countminsketch.py:532-691).

    Args as the reference: num_hitters, width, depth, confidence, error_rate, filepath, hash_function; extra: device."""

    def __init__(self, num_hitters=100, width=None, depth=None, confidence=None, error_rate=None, filepath=None,
                 hash_function: HashFuncT | None = None, device=None):
        super().__init__(width, depth, confidence, error_rate, filepath, hash_function, device)
        self._top: dict = {}
        self._num_hitters = num_hitters
        self._smallest = 0

    @classmethod
    def frombytes(cls, b, num_hitters=100, hash_function: HashFuncT | None = None, device=None):
        width, depth, _ = _FOOTER.unpack_from(bytes(b[-_FOOTER.size:]))
        inst = cls(num_hitters=num_hitters, width=width, depth=depth, hash_function=hash_function, device=device)
        inst._parse_bytes(bytes(b))
        return inst

    def __str__(self) -> str:
        return f"Heavy Hitters {super().__str__()}\n\tNumber Hitters: {self.number_heavy_hitters}\n\tNumber Recorded: {len(self._top)}"

    @property
    def heavy_hitters(self) -> dict:
        return self._top

    @property
    def number_heavy_hitters(self) -> int:
        return self._num_hitters

    def _track(self, keys, results) -> None:
        self._top, self._smallest = hitters_rule((self._top, self._smallest), keys, results, self._num_hitters)

    def add(self, key, num_els: int = 1) -> int:
        """countminsketch.py:617-627"""
        res = super().add(key, num_els)
        self._track((key,), (res,))
        return res

    def add_alt(self, key, hashes: HashResultsT, num_els: int = 1) -> int:
        """countminsketch.py:629-661 (key first: the reference's signature)"""
        res = super().add_alt(hashes, num_els)
        self._track((key,), (res,))
        return res

    def add_many(self, keys, num_els=None):
        """``add`` for every key of the ordered batch: the sketch through ``add_many_ordered``, then the list rule replayed in op
        order on the host.  Returns the results."""
        res = self.add_many_ordered(keys, num_els)
        self._track(_batch_keys(keys), (res.cpu().numpy() if hasattr(res, "is_cuda") else res).tolist())
        return res

    _NO_REMOVE = ("Unable to remove elements in the HeavyHitters "
                  "class as it is an un supported action (and does not"
                  "make sense)!")

    def remove(self, key, num_els: int = 1):
        raise NotSupportedError(self._NO_REMOVE)

    def remove_alt(self, *args, **kwargs):
        """countminsketch.py:663-676"""
        raise NotSupportedError(self._NO_REMOVE)

    def remove_many(self, keys, num_els=None):
        raise NotSupportedError(self._NO_REMOVE)

    remove_alt_many = remove_many
    update_many_ordered = update_alt_many_ordered = remove_many_ordered = remove_alt_many_ordered = remove_many

    def clear(self) -> None:
        super().clear()
        self._top = {}
        self._smallest = 0

    def join(self, second) -> None:
        raise NotSupportedError("Joining is not supported for heavy hitters")
