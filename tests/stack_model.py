"""The stacked Bloom filters as plain Python, for the tests of the index kernels (csrc/psk_index_ops.hip) and of the seams of
``_add_batch`` (expandingbloom.py).  No torch, no numpy.

``resolve`` is the loop the kernels claim to reproduce for an ordered batch:

    for key in batch:  if key is not reported elsewhere and key not in table: table.add(key)

``StackModel`` is the reference's ExpandingBloomFilter (``queue=None``) or RotatingBloomFilter (``queue=N``) over chosen bit positions:
a filter is the set of its set bits plus its own ``elements_added``.  tests/test_stack_model.py ties it to the real reference through
tests/golden/golden_stack_seams.json."""

import struct


def resolve(table_bits, idx, present):
    """flags[i] = 1 iff the sequential loop inserts key i.  ``table_bits``: the set bits of the table before the batch (left unchanged);
    ``idx[i]``: the bit positions of key i (repeats allowed); ``present[i]`` true: the key is reported by another filter (no candidate)."""
    table = set(table_bits)
    flags = []
    for bits, p in zip(idx, present):
        if p or all(b in table for b in bits):
            flags.append(0)
            continue
        table.update(bits)
        flags.append(1)
    return flags


def table_after(table_bits, idx, flags):
    """the set bits once every key with flag 1 is ORed in"""
    table = set(table_bits)
    for bits, f in zip(idx, flags):
        if f == 1:
            table.update(bits)
    return table


def pack_bits(bits, nbytes):
    """bit b lives in byte b // 8 at 1 << (b % 8)  (bloom.py:247-249)"""
    raw = bytearray(nbytes)
    for b in bits:
        raw[b >> 3] |= 1 << (b & 7)
    return bytes(raw)


class StackModel:
    """expandingbloom.py: ``add_alt`` / ``check_alt`` / ``push`` / ``pop`` / ``export`` of both classes.  A hash is reduced ``% m``; only
    the first k hashes of a key are used (bloom.py:247)."""

    _FOOTER = struct.Struct("QQQf")
    _COUNT = struct.Struct("Q")

    def __init__(self, m, k, est_elements, queue=None, fpr=0.0):
        self.m, self.k, self.est, self.queue, self.fpr = m, k, est_elements, queue, fpr
        self.filters = [[set(), 0]]  # [set bits, elements_added], oldest first
        self.elements_added = 0

    # ---- loading a state (frombytes)
    @classmethod
    def from_state(cls, m, k, est_elements, queue, fpr, filters, elements_added):
        s = cls(m, k, est_elements, queue, fpr)
        s.filters = [[set(bits), int(count)] for bits, count in filters]
        s.elements_added = elements_added
        return s

    def _bits(self, hashes):
        return [h % self.m for h in hashes[: self.k]]

    def check_alt(self, hashes):
        bits = self._bits(hashes)
        return any(all(b in f[0] for b in bits) for f in self.filters)

    def _new(self):
        self.filters.append([set(), 0])

    def _make_room(self):
        newest = self.filters[-1]
        if self.queue is None:  # __check_for_growth
            if newest[1] >= self.est:
                self._new()
            return
        if newest[1] == self.est:  # __rotate_bloom_filter(force=False): `==` only
            if len(self.filters) >= self.queue:
                self.filters.pop(0)
            self._new()

    def add_alt(self, hashes, force=False):
        self.elements_added += 1
        if force or not self.check_alt(hashes):
            self._make_room()
            newest = self.filters[-1]
            newest[0].update(self._bits(hashes))
            newest[1] += 1

    def push(self):
        if self.queue is not None and len(self.filters) >= self.queue:
            self.filters.pop(0)
        self._new()

    def pop(self):
        if self.queue is None:
            raise AttributeError("only the rotating filter pops")
        if len(self.filters) == 1:
            raise ValueError("Popping a Bloom Filter will result in an unusable system!")
        self.filters.pop(0)

    def counts(self):
        return [f[1] for f in self.filters]

    def state(self):
        return {"filters": len(self.filters), "counts": self.counts(), "elements_added": self.elements_added}

    def export(self):
        nbytes = (self.m + 7) // 8
        parts = []
        for bits, count in self.filters:
            parts.append(self._COUNT.pack(count))
            parts.append(pack_bits(bits, nbytes))
        parts.append(self._FOOTER.pack(len(self.filters), self.est, self.elements_added, self.fpr))
        return b"".join(parts)


# ---------------------------------------------------------------- inputs shared by tests/test_stack_model.py and tests/test_gpu_stack_kernels.py
def exhaustive_stripes():
    """every ordered 3-key batch over a 4-bit table with k = 2 (16 keys, the two-equal-bits ones included), from every one of the 16
    starting tables, under every one of the 8 present masks: (table bits, idx, present) per stripe, 524 288 stripes"""
    keys = [(a, b) for a in range(4) for b in range(4)]
    for tab in range(16):
        bits = [b for b in range(4) if tab >> b & 1]
        for mask in range(8):
            present = [mask >> j & 1 for j in range(3)]
            for k0 in keys:
                for k1 in keys:
                    for k2 in keys:
                        yield bits, (k0, k1, k2), present


def _hand(name, m, k, table, idx, present=None):
    return {"name": name, "m": m, "k": k, "table": list(table), "idx": [list(x) for x in idx], "present": list(present) if present else [0] * len(idx)}


HAND_CASES = [
    _hand("chain_third_key_skipped", 64, 2, [], [[1, 2], [2, 3], [1, 3], [4, 1], [3, 3], [5, 6], [6, 5], [7, 1], [1, 7], [8, 8], [8, 9], [9, 1]]),
    _hand("covered_by_several_mixed_k", 64, 3, [], [[1, 1, 1], [2, 2, 2], [1, 2, 2], [1, 2, 5], [5, 5, 5], [5, 1, 2], [6, 1, 2], [6, 6, 5], [7, 7, 6], [7, 6, 1], [8, 7, 6], [8, 8, 8]]),
    _hand("same_key_5_times", 64, 3, [9], [[4, 9, 11]] * 5 + [[9, 9, 9]] * 3 + [[11, 4, 9], [4, 4, 12], [12, 4, 9], [12, 12, 12]]),
    _hand("k1", 40, 1, [3, 39], [[0], [3], [0], [39], [38], [38], [1], [2], [1], [3], [37], [0]], [0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0]),
    _hand("k64_all_bits_equal", 128, 64, [70], [[5] * 64, [5] * 64, [70] * 64, [6] * 64, [6] * 63 + [5], [7] + [6] * 63, [7] * 64, [127] * 64, [127] * 64, [0] * 64, [0] * 32 + [70] * 32, [1] * 64]),
    _hand("present_hands_the_bit_on", 64, 2, [], [[1, 2], [1, 2], [1, 2], [3, 4], [3, 5], [4, 5], [6, 6], [6, 6], [6, 7], [7, 6], [8, 9], [8, 9]], [1, 0, 0, 1, 1, 0, 1, 1, 0, 0, 1, 1]),
    _hand("bits_31_32_and_m_minus_1", 1000, 3, [32], [[31, 32, 999], [31, 31, 31], [32, 32, 32], [999, 32, 32], [998, 999, 31], [998, 998, 998], [0, 31, 32], [0, 0, 0], [33, 32, 31], [991, 992, 999], [992, 991, 32], [63, 64, 999]]),
]

