"""The key streams of tests/golden/golden_hitters.json, from integers alone (no RNG state, no floats): the fixture stores what the
reference made of every stream, the tests build the same stream again from the case's recipe.

op i of a case:  x = sm(SEED + salt * 1000003 + i) % R;  idx = x**3 // R**2  (skewed towards 0);  key = "k%07d" % idx (8 latin-1
characters) or key16(idx) (the 16-byte synthetic key of SURVEY.md 8(d));  weight = 1, or 1 + sm((SEED ^ 0xC0FFEE) + salt * 7919 + i) % 7.
R = 1 is the stream of one repeated key."""

import hashlib
import struct

import numpy as np

M64 = 2**64 - 1
SEED = 0x5EED
I32_MAX = 2**31 - 1
FOOTER = struct.Struct("IIq")  # countminsketch.py:122


def sm(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key16(i):
    return struct.pack("<QQ", sm(SEED + 2 * i), sm(SEED + 2 * i + 1))


def stream_indices(case):
    n, R, salt = case["n"], case["R"], case["salt"]
    return [(sm(SEED + salt * 1000003 + i) % R) ** 3 // R**2 for i in range(n)]


def stream_keys(case):
    """the keys as the caller hands them over: str or bytes objects"""
    idx = stream_indices(case)
    if case["key_kind"] == "str":
        return ["k%07d" % i for i in idx]
    return [key16(i) for i in idx]


def stream_weights(case):
    """None (unit weights) or an int32 array"""
    if not case["weighted"]:
        return None
    salt = case["salt"]
    return np.array([1 + sm((SEED ^ 0xC0FFEE) + salt * 7919 + i) % 7 for i in range(case["n"])], dtype=np.int32)


def keys_matrix(keys):
    """(n, L) uint8: the bytes every engine hashes (a str by code point, all <= 255 here)"""
    raw = [k.encode("latin-1") if isinstance(k, str) else k for k in keys]
    return np.frombuffer(b"".join(raw), dtype=np.uint8).reshape(len(raw), len(raw[0])).copy()


def preload_bytes(case):
    """the export image a case starts from (None: an empty sketch): every bin `below` counts under INT32_MAX, so the stream clamps"""
    p = case.get("preload")
    if not p:
        return None
    bins = np.full(case["width"] * case["depth"], I32_MAX - p["below"], dtype=np.int32)
    return bins.tobytes() + FOOTER.pack(case["width"], case["depth"], p["elements_added"])


def results_sha(results):
    return hashlib.sha256(np.asarray(results, dtype=np.int64).tobytes()).hexdigest()


def dict_pairs(case, d):
    """a tracked dict as the fixture stores it: ordered [key, value] pairs, bytes keys in hex"""
    return [[k if case["key_kind"] == "str" else k.hex(), int(v)] for k, v in d.items()]
