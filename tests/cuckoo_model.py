"""A sequential model of the reference's CuckooFilter (probables/cuckoo/cuckoo.py), written for this project.

The reference draws its kicks from Python's global ``random``: ``random.choice([idx_1, idx_2])`` and one ``random.randint(0, bucket_size - 1)``
per swap.  ``random`` is MT19937 and both calls reduce to ``_randbelow(n)``: ``k = n.bit_length()``, ``r = genrand_uint32() >> (32 - k)``,
drawn again while ``r >= n``.  The model carries its own MT19937, started from a ``random.getstate()`` tuple, so its buckets, its counts, the
key at which it raises and the generator state it ends with can all be compared with the live class (tests/test_cuckoo_model.py) and with
the GPU kernels (tests/test_gpu_cuckoo.py).
"""

import struct

MASK64 = (1 << 64) - 1
FULL = "The CuckooFilter is currently full"
EXPAND_FAILED = "The CuckooFilter failed to expand"


def fnv_1a(key) -> int:
    """64-bit FNV-1a, seed 0 (hashes.py:86-103): a str goes in code point by code point, bytes byte by byte"""
    h = 14695981039346656037
    for e in (map(ord, key) if isinstance(key, str) else key):
        h = ((h ^ e) * 1099511628211) & MASK64
    return h


class MT19937:
    """the generator behind ``random``; ``state`` is a ``random.getstate()`` tuple"""

    def __init__(self, state):
        version, internal, self.gauss = state
        assert version == 3 and len(internal) == 625
        self.mt, self.idx = list(internal[:624]), internal[624]
        self.draws = 0

    def getstate(self):
        return (3, tuple(self.mt) + (self.idx,), self.gauss)

    def u32(self) -> int:
        mt = self.mt
        if self.idx >= 624:
            for k in range(624):
                y = (mt[k] & 0x80000000) | (mt[(k + 1) % 624] & 0x7FFFFFFF)
                mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
            self.idx = 0
        y = mt[self.idx]
        self.idx += 1
        self.draws += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        return y ^ (y >> 18)

    def randbelow(self, n: int) -> int:
        k = n.bit_length()
        r = self.u32() >> (32 - k)
        while r >= n:
            r = self.u32() >> (32 - k)
        return r


class Full(Exception):
    pass


class CuckooModel:
    def __init__(self, capacity=10000, bucket_size=4, max_swaps=500, expansion_rate=2, auto_expand=True, finger_bits=32, rng=None):
        self.capacity, self.bucket_size, self.max_swaps = capacity, bucket_size, max_swaps
        self.expansion_rate, self.auto_expand, self.finger_bits = expansion_rate, auto_expand, finger_bits
        self.rng = rng
        self.buckets = [[] for _ in range(capacity)]
        self.elements_added = 0
        self.kicks = 0  # keys whose insert had to walk

    # cuckoo.py:483-506
    def fingerprint(self, key) -> int:
        return fnv_1a(key) & ((1 << self.finger_bits) - 1)

    def indices(self, fp):
        return fp % self.capacity, fnv_1a(str(fp)) % self.capacity

    def _where(self, fp):
        i1, i2 = self.indices(fp)
        if fp in self.buckets[i1]:
            return i1
        if fp in self.buckets[i2]:
            return i2
        return None

    def _put(self, fp, idx) -> bool:
        if len(self.buckets[idx]) < self.bucket_size:
            self.buckets[idx].append(fp)
            self.elements_added += 1
            return True
        return False

    # cuckoo.py:361-392: None, or the fingerprint left over
    def _insert(self, fp):
        i1, i2 = self.indices(fp)
        if self._put(fp, i1) or self._put(fp, i2):
            return None
        self.kicks += 1
        idx = (i1, i2)[self.rng.randbelow(2)]
        for _ in range(self.max_swaps):
            slot = self.rng.randbelow(self.bucket_size)
            fp, self.buckets[idx][slot] = self.buckets[idx][slot], fp
            j1, j2 = self.indices(fp)
            idx = j2 if idx == j1 else j1
            if self._put(fp, idx):
                return None
        return fp

    # cuckoo.py:455-481
    def expand(self, extra=None):
        fps = ([] if extra is None else [extra]) + [fp for b in self.buckets for fp in b]
        self.capacity *= self.expansion_rate
        self.buckets = [[] for _ in range(self.capacity)]
        self.elements_added = 0
        for fp in fps:
            if self._insert(fp) is not None:
                raise Full(EXPAND_FAILED)

    def add(self, key):
        fp = self.fingerprint(key)
        if self._where(fp) is not None:
            return
        left = self._insert(fp)
        if left is None:
            return
        if not self.auto_expand:
            raise Full(FULL)
        self.expand(left)

    def check(self, key) -> bool:
        return self._where(self.fingerprint(key)) is not None

    def remove(self, key) -> bool:
        fp = self.fingerprint(key)
        idx = self._where(fp)
        if idx is None:
            return False
        self.buckets[idx].remove(fp)
        self.elements_added -= 1
        return True

    def export(self) -> bytes:
        out = bytearray()
        for b in self.buckets:
            out += struct.pack(f"<{self.bucket_size}I", *(list(b) + [0] * (self.bucket_size - len(b))))
        return bytes(out) + struct.pack("II", self.bucket_size, self.max_swaps)

    def load(self, data: bytes):
        """cuckoo.py:394-431: zero entries vanish wherever they are in a row"""
        self.bucket_size, self.max_swaps = struct.unpack("II", data[-8:])
        self.capacity = (len(data) - 8) // 4 // self.bucket_size
        words = struct.unpack(f"<{self.capacity * self.bucket_size}I", data[: self.capacity * self.bucket_size * 4])
        self.buckets = [[w for w in words[r * self.bucket_size:(r + 1) * self.bucket_size] if w] for r in range(self.capacity)]
        self.elements_added = sum(map(len, self.buckets))
        return self


def state_digest(state) -> str:
    """sha256 over the 625 words of a ``random.getstate()`` tuple, little-endian uint32"""
    import hashlib

    return hashlib.sha256(struct.pack("<625I", *state[1])).hexdigest()


def run_ops(model: CuckooModel, keys, ops):
    """ops: list of [op, key index] with op 'a' / 'r'.  -> (returns per op: None / bool, error index or None, error message or None)"""
    rets = []
    for at, (op, k) in enumerate(ops):
        try:
            rets.append(model.add(keys[k]) if op == "a" else model.remove(keys[k]))
        except Full as ex:
            return rets, at, str(ex)
    return rets, None, None
