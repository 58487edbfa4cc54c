"""The index kernels of the stacked filters (csrc/psk_index_ops.hip), called through the entries of include/psk.h on tensors the test
owns: chosen bit positions instead of hashed keys.  Every resolver case runs under the dense ``first[]`` resolver and under the slot-map
one and must give the flags of the sequential loop (tests/stack_model.py ``resolve``).  All comparisons are exact."""

import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import stack_model as M  # noqa: E402

NONE = 0xFFFFFFFF
GRID_CAP = 65535 * 256


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def N(torch):
    from pyprobables_amd import _native

    _native.lib()
    return _native


def slot_of(b, lg):
    """the map's slot function, restated"""
    return ((b * 0x9E3779B1) & NONE) >> (32 - lg)


def dev_u32(torch, values):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(values, dtype=np.uint32)).view(np.int32).reshape(-1)).cuda()


def words_of(bits, nwords):
    w = np.zeros(nwords, dtype=np.uint32)
    for b in bits:
        w[b >> 5] |= np.uint32(1 << (b & 31))
    return w


def all_ones(torch, t):
    """an int32 tensor of any size holds nothing but 0xFFFFFFFF (two reductions, no temporary of its size)"""
    return int(t.min()) == -1 and int(t.max()) == -1


class Resolved:
    pass


def resolve_on_gpu(torch, N, how, table, idx, present, n, k, first_len=None, lg=None, map_slots=None, count0=5):
    """one call of a resolver on caller-owned tensors, then psk_idx_insert(flag); checks everything but the flags and the final table:
    the table is untouched by the resolve, the insert count, the scratch all-ones again, count_dev[1] == 0"""
    L = N.lib()
    before = table.clone() if table.numel() <= 1 << 22 else None
    flag = torch.full((max(n, 1),), 7, dtype=torch.uint8, device="cuda")
    pres = present.data_ptr() if present is not None else None
    r = Resolved()
    if how == "dense":
        first = torch.full((first_len,), -1, dtype=torch.int32, device="cuda")
        cnt = torch.tensor([99, 0], dtype=torch.int64, device="cuda")
        host = C.c_uint64(12345)
        N.check(L.psk_idx_resolve_ordered(table.data_ptr(), idx.data_ptr(), pres, n, k, first.data_ptr(), flag.data_ptr(), cnt.data_ptr(), C.addressof(host), 0, None))
        r.inserted, scratch = int(host.value), first
        assert cnt.tolist() == [r.inserted, 0]
    else:
        slots = torch.full((2 * (map_slots or (1 << lg)),), -1, dtype=torch.int32, device="cuda")
        cnt = torch.tensor([count0, 0], dtype=torch.int64, device="cuda")
        N.check(L.psk_idx_resolve_ordered_hashed(table.data_ptr(), idx.data_ptr(), pres, n, k, slots.data_ptr(), lg, flag.data_ptr(), cnt.data_ptr(), 0, None))
        got = cnt.tolist()
        assert got[1] == 0  # the map never overflows
        r.inserted, scratch = got[0] - count0, slots  # (count_dev[0] is ADDED to)
    torch.cuda.synchronize()
    if before is not None:
        assert torch.equal(table, before), "the resolve must not modify the table"
    assert all_ones(torch, scratch), "the scratch must be all-ones again"
    r.flags = flag[:n].cpu().numpy()
    N.check(L.psk_idx_insert(table.data_ptr(), idx.data_ptr(), flag.data_ptr(), n, k, 0, None))
    torch.cuda.synchronize()
    return r


def lg_for(n, k):
    return max(4, (2 * n * k - 1).bit_length())


HOWS = ["dense", "hashed"]


# ---------------------------------------------------------------- 1. exhaustive
@pytest.fixture(scope="module")
def exhaustive():
    """the model's answer for every stripe, once: flags (n), the idx (n x 2), present (n), the table words before and after"""
    stripes = 16 * 8 * 4096
    idx = np.empty((stripes * 3, 2), dtype=np.uint32)
    present = np.empty(stripes * 3, dtype=np.uint8)
    flags = np.empty(stripes * 3, dtype=np.uint8)
    nib0 = np.empty(stripes, dtype=np.uint32)
    nib1 = np.empty(stripes, dtype=np.uint32)
    for t, (bits, keys, pres) in enumerate(M.exhaustive_stripes()):
        f = M.resolve(bits, keys, pres)
        flags[3 * t:3 * t + 3] = f
        present[3 * t:3 * t + 3] = pres
        idx[3 * t:3 * t + 3] = keys
        idx[3 * t:3 * t + 3] += 4 * t
        nib0[t] = sum(1 << b for b in bits)
        nib1[t] = sum(1 << b for b in M.table_after(bits, keys, f))
    assert t == stripes - 1

    def pack(nib):
        return (nib.reshape(-1, 8) << (4 * np.arange(8, dtype=np.uint32))).sum(axis=1, dtype=np.uint32)

    return {"n": stripes * 3, "idx": idx, "present": present, "flags": flags, "before": pack(nib0), "after": pack(nib1)}


@pytest.mark.parametrize("how", HOWS)
def test_every_3_key_batch_over_4_bits_in_one_call(torch, N, exhaustive, how):
    e = exhaustive
    n, m = e["n"], 1 << 21
    assert n == 1_572_864 and len(e["before"]) * 32 == m
    table, idx, present = dev_u32(torch, e["before"]), dev_u32(torch, e["idx"]), torch.from_numpy(e["present"]).cuda()
    r = resolve_on_gpu(torch, N, how, table, idx, present, n, 2, first_len=m, lg=lg_for(n, 2))
    wrong = np.flatnonzero(r.flags != e["flags"])
    assert wrong.size == 0, f"first wrong key {wrong[0]} (stripe {wrong[0] // 3})"
    assert r.inserted == int(e["flags"].sum())
    assert np.array_equal(table.cpu().numpy().view(np.uint32), e["after"])


# ---------------------------------------------------------------- 2. hand-made
@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("case", M.HAND_CASES, ids=[c["name"] for c in M.HAND_CASES])
def test_hand_made_batches(torch, N, case, how):
    m, k, n = case["m"], case["k"], len(case["idx"])
    nwords = (m + 31) // 32
    want = M.resolve(case["table"], case["idx"], case["present"])
    table, idx = dev_u32(torch, words_of(case["table"], nwords)), dev_u32(torch, case["idx"])
    present = torch.tensor(case["present"], dtype=torch.uint8, device="cuda") if any(case["present"]) else None
    r = resolve_on_gpu(torch, N, how, table, idx, present, n, k, first_len=m, lg=lg_for(n, k))
    assert r.flags.tolist() == want
    assert r.inserted == sum(want)
    assert np.array_equal(table.cpu().numpy().view(np.uint32), words_of(M.table_after(case["table"], case["idx"], want), nwords))


@pytest.mark.parametrize("how", HOWS)
def test_bit_positions_past_2p31_on_a_512_mib_table(torch, N, how):
    """bits 0x80000000 and 0xFFFFFFFE: the word index, the first[] index and the slot hash all have to be unsigned 32-bit"""
    hi, top = 0x80000000, 0xFFFFFFFE
    keys = [[hi, top], [hi, hi], [top, 5], [5, 6], [top, top], [hi + 1, 7], [7, hi + 1], [6, top - 1], [top - 1, hi], [0, 31], [hi + 31, 0], [hi + 31, hi + 32]]
    start = [7]
    want = M.resolve(start, keys, [0] * len(keys))
    after = M.table_after(start, keys, want)
    table = torch.zeros(1 << 27, dtype=torch.int32, device="cuda")  # 2^32 bits
    touched = sorted({b >> 5 for key in keys for b in key} | {0})
    table[0] = 1 << 7
    r = resolve_on_gpu(torch, N, how, table, dev_u32(torch, keys), None, len(keys), 2, first_len=1 << 32, lg=lg_for(len(keys), 2))
    assert r.flags.tolist() == want and r.inserted == sum(want)
    got = table[torch.tensor(touched, device="cuda")].cpu().numpy().view(np.uint32).tolist()
    assert got == [sum(1 << (b & 31) for b in after if b >> 5 == w) for w in touched]
    assert int(torch.count_nonzero(table)) == len([w for w in touched if any(b >> 5 == w for b in after)])


# ---------------------------------------------------------------- 3. the slot map
def bits_on_slot(slot, lg, count, start=1):
    out, b = [], start
    while len(out) < count:
        if slot_of(b, lg) == slot:
            out.append(b)
        b += 1
    return out


def hashed_case(torch, N, m, k, start, keys, lg, map_slots=None):
    want = M.resolve(start, keys, [0] * len(keys))
    nwords = (m + 31) // 32
    table = dev_u32(torch, words_of(start, nwords))
    r = resolve_on_gpu(torch, N, "hashed", table, dev_u32(torch, keys), None, len(keys), k, lg=lg, map_slots=map_slots)
    assert r.flags.tolist() == want and r.inserted == sum(want)
    assert np.array_equal(table.cpu().numpy().view(np.uint32), words_of(M.table_after(start, keys, want), nwords))
    return want


def test_probes_wrap_around_the_end_of_a_map_loaded_to_one_half(torch, N):
    bits = bits_on_slot(15, 4, 8)  # all eight start at the last slot: they settle in 15, 0, 1 .. 6
    m = 32 * (max(bits) // 32 + 1)
    keys = [[bits[2 * i], bits[2 * i + 1]] for i in range(4)]  # n * k = 8 = half of 2^4
    assert hashed_case(torch, N, m, 2, [], keys, 4) == [1, 1, 1, 1]
    assert hashed_case(torch, N, m, 1, [], [[b] for b in bits], 4) == [1] * 8
    # the same eight bits twice over: 16 keys of one bit need 2^5 slots by the sizing rule; on slot 31 of that map they wrap as well
    bits5 = bits_on_slot(31, 5, 8)
    m5 = 32 * (max(bits5) // 32 + 1)
    assert hashed_case(torch, N, m5, 1, [], [[b] for b in bits5] * 2, 5) == [1] * 8 + [0] * 8
    assert hashed_case(torch, N, m5, 1, [], [[b] for b in bits5 + bits5[::-1]], 5) == [1] * 8 + [0] * 8
    # ... and as 8 keys of k = 2 that name every bit twice: n * k = 16 probes over the eight bits
    assert hashed_case(torch, N, m5, 2, [bits5[7]], [[bits5[i], bits5[7 - i]] for i in range(8)], 5) == [1, 1, 1, 1, 0, 0, 0, 0]


def test_a_map_of_2p12_slots_half_full_and_a_buffer_larger_than_the_map(torch, N):
    rng = np.random.default_rng(12)
    m = 1 << 20
    bits = rng.choice(m, size=2048, replace=False).tolist()
    keys = [[b] for b in bits]
    assert sum(hashed_case(torch, N, m, 1, bits[:100], keys, 12)) == 2048 - 100
    # the class keeps ONE buffer sized for its largest step and passes the lg of the step: the tail beyond 2^lg stays all-ones throughout.
    # Slots past 2^lg that the call wrote would be left behind (it resets 2^lg slots only), so all-ones afterwards pins the whole lifetime.
    pairs = [[bits[i], bits[(i * 7 + 1) % 2048]] for i in range(1024)]
    hashed_case(torch, N, m, 2, bits[:100], pairs, 12, map_slots=1 << 14)


# ---------------------------------------------------------------- 4. refusals
def test_refusals_leave_every_buffer_alone(torch, N):
    L = N.lib()
    table = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    idx = torch.tensor([1, 2, 3, 4, 5, 6, 7, 8, 9], dtype=torch.int32, device="cuda")
    flag = torch.full((16,), 7, dtype=torch.uint8, device="cuda")
    out = torch.full((16,), 9, dtype=torch.uint8, device="cuda")
    first = torch.full((128,), -1, dtype=torch.int32, device="cuda")
    slots = torch.full((2 << 5,), -1, dtype=torch.int32, device="cuda")
    cnt = torch.tensor([41, 42], dtype=torch.int64, device="cuda")
    host = C.c_uint64(77)
    p = {name: t.data_ptr() for name, t in (("table", table), ("idx", idx), ("flag", flag), ("out", out), ("first", first), ("slots", slots), ("cnt", cnt))}

    def dense(n, k):
        return L.psk_idx_resolve_ordered(p["table"], p["idx"], None, n, k, p["first"], p["flag"], p["cnt"], C.addressof(host), 0, None)

    def hashed(n, k, lg):
        return L.psk_idx_resolve_ordered_hashed(p["table"], p["idx"], None, n, k, p["slots"], lg, p["flag"], p["cnt"], 0, None)

    refused = [
        L.psk_idx_test(p["table"], p["idx"], 4, 0, p["out"], 0, 0, None),
        L.psk_idx_insert(p["table"], p["idx"], None, 4, 0, 0, None),
        dense(4, 0),
        hashed(4, 0, 5),
        hashed(2, 2, 3),
        hashed(2, 2, 32),
        hashed(9, 1, 4),  # 2 * n * k = 18 = 2^4 + 2
        dense(2**32 - 1, 1),
    ]
    torch.cuda.synchronize()
    assert refused == [N.PSK_EINVAL] * len(refused)
    assert hashed(8, 1, 4) == N.PSK_OK  # (2 * n * k = 2^lg is served)
    torch.cuda.synchronize()
    served = [1 - (0x5A5A5A5A >> b & 1) for b in range(1, 9)]  # bits 1 .. 8, distinct: the clear ones insert
    assert cnt.tolist() == [41 + sum(served), 42] and flag.tolist() == served + [7] * 8
    assert host.value == 77 and all_ones(torch, first) and all_ones(torch, slots)
    assert table.tolist() == [0x5A5A5A5A] * 4 and out.tolist() == [9] * 16


# ---------------------------------------------------------------- 5. the grid caps
N_CAP = GRID_CAP + 257
SUB = 1 << 18


@pytest.fixture(scope="module")
def capped():
    m = 1 << 20
    rng = np.random.default_rng(5)
    order = rng.permutation(m).astype(np.uint32)
    base = np.concatenate([order, order[:5]])  # 2^20 + 5 keys; the rest repeat them
    idx = base[np.arange(N_CAP) % base.size]
    start = rng.integers(0, 2**32, size=m // 32, dtype=np.uint32) & rng.integers(0, 2**32, size=m // 32, dtype=np.uint32)
    clear = ((start[idx >> 5] >> (idx & 31)) & 1) == 0
    bits, first_at = np.unique(idx, return_index=True)
    flags = np.zeros(N_CAP, dtype=np.uint8)
    flags[first_at] = 1
    flags &= clear.astype(np.uint8)
    return {"m": m, "idx": idx, "start": start, "flags": flags, "clear": clear}


def test_dense_resolver_past_the_grid_cap(torch, N, capped):
    c = capped
    table, idx = dev_u32(torch, c["start"]), dev_u32(torch, c["idx"])
    r = resolve_on_gpu(torch, N, "dense", table, idx, None, N_CAP, 1, first_len=c["m"])
    assert np.array_equal(r.flags, c["flags"]) and r.inserted == int(c["flags"].sum()) == int(c["clear"][: c["m"]].sum())
    assert all_ones(torch, table)  # every bit is named


def test_hashed_resolver_walked_in_sub_chunks_past_the_grid_cap(torch, N, capped):
    c, L = capped, N.lib()
    table, idx = dev_u32(torch, c["start"]), dev_u32(torch, c["idx"])
    lg = lg_for(SUB, 1)
    slots = torch.full((2 << lg,), -1, dtype=torch.int32, device="cuda")
    flag = torch.full((N_CAP,), 7, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    for s in range(0, N_CAP, SUB):  # resolve, insert, next: as _resolve_insert walks a chunk
        n = min(SUB, N_CAP - s)
        N.check(L.psk_idx_resolve_ordered_hashed(table.data_ptr(), idx.data_ptr() + 4 * s, None, n, 1, slots.data_ptr(), lg, flag.data_ptr() + s, cnt.data_ptr(), 0, None))
        N.check(L.psk_idx_insert(table.data_ptr(), idx.data_ptr() + 4 * s, flag.data_ptr() + s, n, 1, 0, None))
    torch.cuda.synchronize()
    assert np.array_equal(flag.cpu().numpy(), c["flags"])
    assert cnt.tolist() == [int(c["flags"].sum()), 0]
    assert all_ones(torch, slots) and all_ones(torch, table)


def test_idx_test_and_insert_past_the_grid_cap(torch, N, capped):
    c, L = capped, N.lib()
    table, idx = dev_u32(torch, c["start"]), dev_u32(torch, c["idx"])
    out = torch.full((N_CAP,), 7, dtype=torch.uint8, device="cuda")
    N.check(L.psk_idx_test(table.data_ptr(), idx.data_ptr(), N_CAP, 1, out.data_ptr(), 0, 0, None))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), (~c["clear"]).astype(np.uint8))
    # only keys of the grid-stride loop's second turn insert: the last 257, and every 4099th key of the first turn must not
    flag = torch.zeros(N_CAP, dtype=torch.uint8, device="cuda")
    flag[GRID_CAP:] = 1
    flag[:GRID_CAP:4099] = 2
    N.check(L.psk_idx_insert(table.data_ptr(), idx.data_ptr(), flag.data_ptr(), N_CAP, 1, 0, None))
    torch.cuda.synchronize()
    want = c["start"].copy()
    tail = c["idx"][GRID_CAP:]
    np.bitwise_or.at(want, tail >> 5, np.uint32(1) << (tail & 31))
    assert np.array_equal(table.cpu().numpy().view(np.uint32), want)


@pytest.mark.parametrize("n", [0, 1, 255, N_CAP])
def test_bytes_or(torch, N, n):
    rng = np.random.default_rng(n + 1)
    a, b = rng.integers(0, 256, size=n + 8, dtype=np.uint8), rng.integers(0, 256, size=n + 8, dtype=np.uint8)
    dst, src = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    N.check(N.lib().psk_bytes_or(dst.data_ptr(), src.data_ptr(), n, 0, None))
    torch.cuda.synchronize()
    want = a.copy()
    want[:n] |= b[:n]  # (the 8 bytes past n stay as they were)
    assert np.array_equal(dst.cpu().numpy(), want)


# ---------------------------------------------------------------- 6. psk_idx_test / psk_idx_insert
def test_idx_test_accumulates_over_three_tables_and_overwrites_without(torch, N):
    L, m, k = N.lib(), 96, 2
    tables = [[1, 2, 40], [2, 3, 95], [40, 41, 0]]
    keys = [[1, 2], [2, 3], [40, 41], [1, 3], [95, 95], [0, 40], [5, 6], [2, 2], [41, 0], [1, 40], [3, 2], [94, 95]]
    idx = dev_u32(torch, keys)
    pre = [0, 2, 0, 2, 0, 0, 2, 0, 0, 2, 0, 0]
    out = torch.tensor(pre, dtype=torch.uint8, device="cuda")
    want = list(pre)
    for bits in tables:
        N.check(L.psk_idx_test(dev_u32(torch, words_of(bits, 3)).data_ptr(), idx.data_ptr(), len(keys), k, out.data_ptr(), 1, 0, None))
        torch.cuda.synchronize()
        want = [w if w else int(all(b in bits for b in key)) for w, key in zip(want, keys)]  # non-zero: kept as it is
        assert out.tolist() == want
    assert want == [1, 2, 1, 2, 1, 1, 2, 1, 1, 2, 1, 0]
    N.check(L.psk_idx_test(dev_u32(torch, words_of(tables[0], 3)).data_ptr(), idx.data_ptr(), len(keys), k, out.data_ptr(), 0, 0, None))
    torch.cuda.synchronize()
    assert out.tolist() == [int(all(b in tables[0] for b in key)) for key in keys]


def test_idx_insert_flag_values_null_flag_and_one_hot_word(torch, N):
    L, k = N.lib(), 2
    keys = [[0, 1], [2, 3], [4, 5], [6, 7], [33, 34], [35, 36], [62, 63], [95, 64]]
    idx = dev_u32(torch, keys)
    table = torch.zeros(3, dtype=torch.int32, device="cuda")
    flag = torch.tensor([0, 1, 2, 255, 1, 0, 255, 1], dtype=torch.uint8, device="cuda")
    N.check(L.psk_idx_insert(table.data_ptr(), idx.data_ptr(), flag.data_ptr(), len(keys), k, 0, None))
    torch.cuda.synchronize()
    assert np.array_equal(table.cpu().numpy().view(np.uint32), words_of([2, 3, 33, 34, 95, 64], 3))  # only flag 1 inserts
    N.check(L.psk_idx_insert(table.data_ptr(), idx.data_ptr(), None, len(keys), k, 0, None))
    torch.cuda.synchronize()
    assert np.array_equal(table.cpu().numpy().view(np.uint32), words_of([b for key in keys for b in key], 3))  # NULL: every key
    # 100 000 keys whose bits all fall into one 32-bit word (word 1 of 3): every OR lands, the neighbours stay clear
    rng = np.random.default_rng(3)
    many = (32 + rng.integers(0, 31, size=(100_000, 3))).astype(np.uint32)  # bit 63 is never named
    table = torch.zeros(3, dtype=torch.int32, device="cuda")
    N.check(L.psk_idx_insert(table.data_ptr(), dev_u32(torch, many).data_ptr(), None, 100_000, 3, 0, None))
    torch.cuda.synchronize()
    assert table.cpu().numpy().view(np.uint32).tolist() == [0, 0x7FFFFFFF, 0]
