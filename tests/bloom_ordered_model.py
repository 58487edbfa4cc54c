"""The ordered Bloom batch in Python integers: the plain loop and the ``first[]`` rule.

A key is the list of its k bit positions; a table is a Python set of the positions that are set.

* ``loop``   ``for key in stream: seen = key in table; table.add(key)`` -- what ``BloomFilter.add_many_ordered`` must answer;
* ``rule``   the parallel form: ``first[b]`` = the smallest position of the stream whose key touches bit ``b``, for the bits clear in
  the table in front; ``seen[i] == 0`` iff ``first[b] == i`` for one of key ``i``'s clear bits; the table afterwards is the table in
  front plus every bit touched.  ``chunk``: the stream cut into ordered pieces, each of which sees the table as the previous one left it.

Hash positions of real keys (the reference's ``default_fnv_1a`` / ``default_md5`` / ``default_sha256`` restated on integers and
``hashlib``), and the table as the reference's bytes.  Nothing here imports the engine or the reference.
"""

from __future__ import annotations

import hashlib
from itertools import product

U64 = 1 << 64
FNV_BASIS, FNV_PRIME = 14695981039346656037, 1099511628211


# ------------------------------------------------------------------ the two forms
def loop(table: set, stream):
    """-> (seen list of 0 / 1, table afterwards); ``table`` is not modified"""
    t = set(table)
    seen = []
    for key in stream:
        seen.append(1 if all(b in t for b in key) else 0)
        t.update(key)
    return seen, t


def loop_conditional(table: set, stream):
    """``if key not in table: table.add(key)``: -> (seen, table afterwards, number of adds)"""
    t = set(table)
    seen, adds = [], 0
    for key in stream:
        s = all(b in t for b in key)
        seen.append(1 if s else 0)
        if not s:
            t.update(key)
            adds += 1
    return seen, t, adds


def rule(table: set, stream, chunk: int | None = None):
    """the ``first[]`` rule, piece by piece: -> (seen, table afterwards)"""
    t = set(table)
    stream = list(stream)
    chunk = max(1, len(stream)) if chunk is None else int(chunk)
    seen = []
    for lo in range(0, len(stream), chunk):
        piece = stream[lo:lo + chunk]
        first = {}
        for i, key in enumerate(piece):
            for b in key:
                if b not in t and b not in first:  # (i only grows: the first writer holds the minimum)
                    first[b] = i
        for i, key in enumerate(piece):
            seen.append(0 if any(first.get(b) == i for b in key) else 1)
        t.update(first)  # the keys with seen == 0 write their bits: every first[b]'s key is one of them
    return seen, t


# ------------------------------------------------------------------ the exhaustive 4-bit space
KEYS_2BIT = [(a, b) for a in range(4) for b in range(4)]  # every 2-position key over a 4-bit table (a == b: a repeated bit)


def exhaustive_cases():
    """every (start state, 3-key stream) over a 4-bit table: 16 * 16^3 = 65 536 cases, as (start set, [key, key, key])"""
    for s in range(16):
        start = {b for b in range(4) if s >> b & 1}
        for ks in product(KEYS_2BIT, repeat=3):
            yield start, list(ks)


# ------------------------------------------------------------------ positions of real keys
def fnv_1a(key, seed: int = 0) -> int:
    h = (FNV_BASIS + 31 * seed) % U64
    for e in (map(ord, key) if isinstance(key, str) else bytes(key)):
        h = ((h ^ e) * FNV_PRIME) % U64
    return h


def hashes_fnv(key, k: int) -> list:
    return [fnv_1a(key, s) for s in range(k)]


def hashes_digest(key, k: int, name: str) -> list:
    """the reference's digest chain: digest of the key, digest of that digest ...; each hash the first 8 bytes, little endian"""
    tmp = key.encode("utf-8") if isinstance(key, str) else bytes(key)
    out = []
    for _ in range(k):
        tmp = hashlib.new(name, tmp).digest()
        out.append(int.from_bytes(tmp[:8], "little"))
    return out


def positions(hashes, m: int, k: int) -> list:
    return [int(h) % m for h in list(hashes)[:k]]


# ------------------------------------------------------------------ tables as bytes
def table_bytes(table: set, m: int) -> bytes:
    """the reference's array('B'): bit ``b % 8`` of byte ``b // 8``"""
    out = bytearray((m + 7) // 8)
    for b in table:
        out[b >> 3] |= 1 << (b & 7)
    return bytes(out)


def table_from_bytes(raw: bytes, m: int) -> set:
    return {b for b in range(m) if raw[b >> 3] >> (b & 7) & 1}
