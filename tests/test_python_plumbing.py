"""The device plumbing every structure shares (pyprobables_amd/_base.py, keys.hashed_batch), as far as it runs without a device."""

import numpy as np
import pytest

from pyprobables_amd import _base, _native as N
from pyprobables_amd.exceptions import NativeLibraryError
from pyprobables_amd.keys import hashed_batch, pack_hashes, pack_keys

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("np_dtype", [np.uint8, np.uint32, np.int64])
@pytest.mark.parametrize("n", [0, 1, 65, (3, 0), (3, 5)])
def test_result_buffer_on_the_host(n, np_dtype):
    addr, fin = _base.result_buffer(N.HOST, n, np_dtype, None, 0)
    a = fin()
    assert isinstance(a, np.ndarray) and a.dtype == np_dtype and a.shape == (n if isinstance(n, tuple) else (n,))
    assert fin() is a  # the array the engine wrote, not a copy
    assert addr == (a.ctypes.data if a.size else None)  # (an empty result is NULL to the engine)


def test_as_bool_on_numpy():
    flags = np.array([0, 1, 1, 0, 1], dtype=np.uint8)
    got = _base.as_bool(flags)
    assert got.dtype == np.bool_ and got.tolist() == [False, True, True, False, True]
    assert np.shares_memory(got, flags)
    assert _base.as_bool(np.zeros(0, dtype=np.uint8)).shape == (0,)
    t = _base.as_bool(torch.tensor([1, 0], dtype=torch.uint8))
    assert t.dtype == torch.bool and t.tolist() == [True, False]


@pytest.mark.parametrize("values", [[], [5], [3, 3, 3, 3], [4, 1, 3, 2, 0], [7, 2, 7, 2, 2, 9, 7], [1, 1, 5, 2, 9, 9], [-(2**31), 2**31 - 1, -(2**31), 0]],
                         ids=["empty", "one", "all-equal", "all-distinct", "mixed", "runs-at-both-ends", "int32-rails"])
def test_equal_groups_against_numpy(values):
    v = np.asarray(values, dtype=np.int32)
    order, first = _base.equal_groups(torch.from_numpy(v))
    want = np.argsort(v, kind="stable")
    assert order.indices.numpy().tolist() == want.tolist() and order.values.numpy().tolist() == v[want].tolist()
    s = v[want]
    assert first.dtype == torch.bool and first.numpy().tolist() == [i == 0 or s[i] != s[i - 1] for i in range(len(s))]


def _same_batch(a, b):
    assert (a.layout, a.n, a.key_len, a.where, a.device) == (b.layout, b.n, b.key_len, b.where, b.device)
    assert bool(a.offsets) == bool(b.offsets)

    def image(x):  # the bytes behind the batch's pointers, through what keeps them alive
        return [np.asarray(k).tobytes() if isinstance(k, np.ndarray) else bytes(k) for k in x.keep]

    assert image(a) == image(b)


@pytest.mark.parametrize("keys", [["a", "bc", "def"], [b"abcd", b"efgh"], "lone", b"lone", [], ["€ uro", "x"], np.arange(24, dtype=np.uint8).reshape(4, 6)],
                         ids=["ragged", "fixed", "one-str", "one-bytes", "empty", "wide", "array"])
def test_hashed_batch_fused_is_pack_keys(keys):
    def never(key, depth):
        raise AssertionError("the fused route hashes on the device")

    _same_batch(hashed_batch(keys, never, True, None, 4, 0, None), pack_keys(keys))


def _py_hash(key, depth):
    raw = key.encode() if isinstance(key, str) else bytes(key)
    return [(int.from_bytes(raw, "little") * 0x9E3779B97F4A7C15 + i * 0x100000001B3) & (2**64 - 1) for i in range(depth)]


@pytest.mark.parametrize("keys", [["a", "bc", "def"], [b"k%d" % i for i in range(65)], b"lone", "lone", bytearray(b"lone"), [], ()],
                         ids=["three", "65", "one-bytes", "one-str", "one-bytearray", "empty-list", "empty-tuple"])
def test_hashed_batch_custom_hash_is_pack_hashes_of_the_per_key_hashes(keys):
    depth = 5
    got = hashed_batch(keys, _py_hash, False, None, depth, 0, None)
    each = [keys] if isinstance(keys, (str, bytes, bytearray)) else list(keys)
    want = pack_hashes([_py_hash(k, depth) for k in each] if each else np.zeros((0, depth), dtype=np.uint64), depth)
    _same_batch(got, want)
    assert got.layout == N.KEYS_HASHES and got.where == N.HOST and got.n == len(each) and got.key_len == depth
    if each:
        assert np.array_equal(got.keep[0], np.array([_py_hash(k, depth) for k in each], dtype=np.uint64))
    else:
        assert got.data == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="a device is present: nothing to refuse")
@pytest.mark.parametrize("what, text", [
    ("the sketch table lives in GPU memory", "no HIP device available: the sketch table lives in GPU memory and there is no CPU fallback"),
    ("the bank's table lives in GPU memory", "no HIP device available: the bank's table lives in GPU memory and there is no CPU fallback"),
    ("the cuckoo filter's buckets live in GPU memory", "no HIP device available: the cuckoo filter's buckets live in GPU memory and there is no CPU fallback"),
    ("the quotient filter's table lives in GPU memory", "no HIP device available: the quotient filter's table lives in GPU memory and there is no CPU fallback"),
])
def test_require_device_refuses_without_a_device(what, text):
    with pytest.raises(NativeLibraryError) as err:
        _base.require_device(what)
    assert str(err.value) == text


@pytest.mark.skipif(torch.cuda.is_available(), reason="a device is present: nothing to refuse")
def test_the_structures_refuse_with_their_own_words():
    import pyprobables_amd as pa

    for make, text in [
        (lambda: pa.BloomFilter(100, 0.05), "no HIP device available: the sketch table lives in GPU memory and there is no CPU fallback"),
        (lambda: pa.BloomFilterBank(4, 100, 0.05), "no HIP device available: the bank's table lives in GPU memory and there is no CPU fallback"),
        (lambda: pa.CuckooFilter(capacity=8).check_many([b"k"]),
         "no HIP device available: the cuckoo filter's buckets live in GPU memory and there is no CPU fallback"),
        (lambda: pa.QuotientFilter(quotient=8).check_many([b"k"]),
         "no HIP device available: the quotient filter's table lives in GPU memory and there is no CPU fallback"),
    ]:
        with pytest.raises(NativeLibraryError) as err:
            make()
        assert str(err.value) == text


def test_same_device_names_the_structure():
    from pyprobables_amd.keys import KeyBatch

    far = KeyBatch(N.KEYS_FIXED, 16, 0, 1, 4, N.DEVICE, 3)
    with pytest.raises(ValueError, match=r"^key batch lives on cuda:3, the bank on cuda:1$"):
        _base.same_device(far, 1, "bank")
    assert _base.same_device(far, 3, "bank") is far
    host = KeyBatch(N.KEYS_FIXED, 16, 0, 1, 4, N.HOST)
    assert _base.same_device(host, 1, "filter") is host
