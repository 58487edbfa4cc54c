"""A sequential model of the reference's CountingCuckooFilter (probables/cuckoo/countingcuckoo.py), written for this project, over
``cuckoo_model.MT19937``.

What differs from the plain filter's model (cuckoo_model.py), each as the reference does it:

* a bucket holds bins ``[fingerprint, count]``; ``add`` of a present fingerprint increments the FIRST bin that holds it in the row
  ``_check_if_present`` names (idx_1's if it holds one, else idx_2's) and ``elements_added``;
* ``_insert_fingerprint_alt`` (countingcuckoo.py:230-265): a bin that is placed directly keeps the count it was handed, a bin that has to
  walk goes in hand as ``CountingCuckooBin(fingerprint, 1)``; swaps exchange whole bins; every placed bin adds 1 to ``elements_added`` and
  to ``unique_elements`` -- so an expansion, which re-inserts every bin with its count, ends with ``elements_added == unique_elements``;
* the leftover of a failed walk is a bin; it goes first into the expansion.

`kicks` counts the inserts that had to walk, `count_resets` those that went in hand with a count above 1 (an expansion's only).
"""

import struct

from cuckoo_model import MT19937, Full, fnv_1a, state_digest  # noqa: F401  (re-exported for the tests)

FULL = "The CountingCuckooFilter is currently full"
EXPAND_FAILED = "The CountingCuckooFilter failed to expand"


class CountingCuckooModel:
    def __init__(self, capacity=10000, bucket_size=4, max_swaps=500, expansion_rate=2, auto_expand=True, finger_bits=32, rng=None):
        self.capacity, self.bucket_size, self.max_swaps = capacity, bucket_size, max_swaps
        self.expansion_rate, self.auto_expand, self.finger_bits = expansion_rate, auto_expand, finger_bits
        self.rng = rng
        self.buckets = [[] for _ in range(capacity)]
        self.elements_added = self.unique_elements = 0
        self.kicks = self.count_resets = self.expansions = 0
        self.leftovers = []  # the bins failed walks left over, in order

    def fingerprint(self, key) -> int:
        return fnv_1a(key) & ((1 << self.finger_bits) - 1)

    def indices(self, fp):
        return fp % self.capacity, fnv_1a(str(fp)) % self.capacity

    def _where(self, fp):
        i1, i2 = self.indices(fp)
        if any(b[0] == fp for b in self.buckets[i1]):
            return i1
        if any(b[0] == fp for b in self.buckets[i2]):
            return i2
        return None

    def _bin(self, fp):
        idx = self._where(fp)
        return (None, None) if idx is None else (idx, next(b for b in self.buckets[idx] if b[0] == fp))

    def _put(self, fp, idx, count) -> bool:
        if len(self.buckets[idx]) < self.bucket_size:
            self.buckets[idx].append([fp, count])
            self.elements_added += 1
            self.unique_elements += 1
            return True
        return False

    # countingcuckoo.py:230-265: None, or the bin left over
    def _insert(self, fp, count=1):
        i1, i2 = self.indices(fp)
        if self._put(fp, i1, count) or self._put(fp, i2, count):
            return None
        self.kicks += 1
        self.count_resets += count > 1
        idx = (i1, i2)[self.rng.randbelow(2)]
        hand = [fp, 1]
        for _ in range(self.max_swaps):
            slot = self.rng.randbelow(self.bucket_size)
            hand, self.buckets[idx][slot] = self.buckets[idx][slot], hand
            j1, j2 = self.indices(hand[0])
            idx = j2 if idx == j1 else j1
            if self._put(hand[0], idx, hand[1]):
                return None
        self.leftovers.append(tuple(hand))
        return hand

    # cuckoo.py:467-481 and countingcuckoo.py:305-316
    def expand(self, extra=None):
        bins = ([] if extra is None else [extra]) + [b for row in self.buckets for b in row]
        self.capacity *= self.expansion_rate
        self.buckets = [[] for _ in range(self.capacity)]
        self.elements_added = self.unique_elements = 0
        self.expansions += 1
        for fp, count in bins:
            if self._insert(fp, count) is not None:
                raise Full(EXPAND_FAILED)

    def add(self, key):
        fp = self.fingerprint(key)
        _, b = self._bin(fp)
        if b is not None:
            b[1] += 1
            self.elements_added += 1
            return
        left = self._insert(fp)
        if left is None:
            return
        if not self.auto_expand:
            raise Full(FULL)
        self.expand(left)

    def check(self, key) -> int:
        _, b = self._bin(self.fingerprint(key))
        return 0 if b is None else b[1]

    def remove(self, key) -> bool:
        idx, b = self._bin(self.fingerprint(key))
        if b is None:
            return False
        b[1] -= 1
        self.elements_added -= 1
        if b[1] == 0:
            self.buckets[idx] = [x for x in self.buckets[idx] if x is not b]
            self.unique_elements -= 1
        return True

    def export(self) -> bytes:
        out = bytearray()
        for row in self.buckets:
            words = [w for b in row for w in b] + [0, 0] * (self.bucket_size - len(row))
            out += struct.pack(f"<{2 * self.bucket_size}I", *words)
        return bytes(out) + struct.pack("II", self.bucket_size, self.max_swaps)

    def load(self, data: bytes):
        """countingcuckoo.py:275-303: pairs whose fingerprint is 0 vanish wherever they stand in a row"""
        self.bucket_size, self.max_swaps = struct.unpack("II", data[-8:])
        B = self.bucket_size
        self.capacity = (len(data) - 8) // 8 // B
        words = struct.unpack(f"<{self.capacity * B * 2}I", data[: self.capacity * B * 8])
        self.buckets = [[[words[2 * s], words[2 * s + 1]] for s in range(r * B, (r + 1) * B) if words[2 * s]] for r in range(self.capacity)]
        self.elements_added = sum(b[1] for row in self.buckets for b in row)
        self.unique_elements = sum(map(len, self.buckets))
        return self

    def bins(self):
        """the buckets as lists of (fingerprint, count) tuples"""
        return [[tuple(b) for b in row] for row in self.buckets]


def run_ops(model: CountingCuckooModel, keys, ops):
    """ops: list of [op, key index] with op 'a' / 'r'.  -> (returns per op: None / bool, error index or None, error message or None)"""
    rets = []
    for at, (op, k) in enumerate(ops):
        try:
            rets.append(model.add(keys[k]) if op == "a" else model.remove(keys[k]))
        except Full as ex:
            return rets, at, str(ex)
    return rets, None, None
