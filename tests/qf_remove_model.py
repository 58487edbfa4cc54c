"""Removal in place from a quotient filter's table: a plain-Python step model of the two launches behind ``psk_qf_remove_alt``
(pyprobables_amd/csrc/psk_quotient.hip k_qf_locate / k_qf_repack, psk_quotient.hpp qf_find; DESIGN.md "Quotient filter: removal").
Test infrastructure, no GPU.

The model keeps the kernels' names and their word-level structure, and never computes the canonical table of the rest:
tests/test_quotient_remove_model.py holds it against ``qf_model.canonical``.

    locate   per batch hash: the lookup walk over 32-bit metadata words.  A hit sets its slot's bit in `dead`; the first to set it counts the hit
             and sets the cluster start's bit in `dirty`; the first to set THAT bit appends the start to `list` (`cursor`).
    repack   per listed cluster start b: reads the cluster slot by slot through the cached words `wsh` / `wcont` / `wdead`, writes the survivors
             behind the read position and zeroes what nobody took.  Metadata bits are gathered per written word in `mmask` / `mc` / `ms` and
             reach the arrays only in ``flush()``, as and-not followed by or: what another cluster holds in the same word stays.

The lanes of a launch are run one after the other; the order in which the listed clusters are repaired is the caller's (`order`).
Every array is a ``Dev``: an index outside it is an error (never Python's wrap-around), and every loop reports its length to ``Run.longest``.
"""

from __future__ import annotations

import numpy as np

import qf_model as M

M32 = 0xFFFFFFFF


def popc(x: int) -> int:
    return bin(x).count("1")


def ffs(x: int) -> int:
    """__ffs: the 1-based position of the lowest set bit, 0 for 0"""
    return (x & -x).bit_length()


class Dev:
    """a device array of unsigned integers"""

    def __init__(self, a: np.ndarray):
        self.a = a

    def __len__(self):
        return int(self.a.size)

    def __getitem__(self, i: int) -> int:
        if not 0 <= i < self.a.size:
            raise IndexError(f"read at {i} of {self.a.size}")
        return int(self.a[i])

    def __setitem__(self, i: int, v: int) -> None:
        if not 0 <= i < self.a.size:
            raise IndexError(f"write at {i} of {self.a.size}")
        self.a[i] = v


def pack(bits: np.ndarray) -> np.ndarray:
    """uint8[size] of 0 / 1 -> uint32 words, LSB first"""
    return np.packbits(np.asarray(bits, dtype=np.uint8), bitorder="little").view(np.uint32).copy()


def unpack(words: np.ndarray, size: int) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:size]


class Table:
    """the four arrays as the kernels see them (q >= 5): remainders per slot, three bit arrays in 32-bit words"""

    def __init__(self, filt: np.ndarray, occ: np.ndarray, cont: np.ndarray, sh: np.ndarray, q: int):
        assert q >= 5 and filt.size == 1 << q and occ.size == cont.size == sh.size == 1 << (q - 5)
        self.q, self.size, self.words = q, 1 << q, 1 << (q - 5)
        self.filter, self.occ, self.cont, self.sh = Dev(filt), Dev(occ), Dev(cont), Dev(sh)

    def arrays(self):
        """-> (filter, occupied, continuation, shifted) in the shape of ``qf_model.canonical``"""
        return (self.filter.a, *(unpack(w.a, self.size) for w in (self.occ, self.cont, self.sh)))


def table_of(arrays, q: int) -> Table:
    filt, occ, cont, sh = arrays
    return Table(np.array(filt, dtype=M.remainder_dtype(q)), pack(occ), pack(cont), pack(sh), q)


class Run:
    """one call: the scratch as psk_qf_remove_alt lays it out -- dead[words], dirty[words], cursor, a pad word, n list entries -- and what the
    tests ask about the run"""

    def __init__(self, t: Table, n: int):
        self.scratch = Dev(np.zeros(2 * t.words + 2 + n, dtype=np.uint32))
        self.dead, self.dirty, self.cursor, self.list = 0, t.words, 2 * t.words, 2 * t.words + 2  # offsets into the scratch
        self.removed = 0
        self.longest = 0  # the most steps any single loop took
        self.starts = []  # the list as k_qf_locate left it

    def loop(self, steps: int) -> None:
        self.longest = max(self.longest, steps)


# ------------------------------------------------------------------ psk_quotient.hpp qf_find (q >= 5: rep = 1)
def qf_find(t: Table, h: int, run: Run):
    """-> (slot, start) of hash h, or None"""
    rbits, smask = 32 - t.q, t.size - 1
    quot, rem = h >> rbits, h & ((1 << rbits) - 1)
    wmask = smask >> 5
    w, b = (quot >> 5) & wmask, quot & 31
    if not (t.occ[w] >> b) & 1:
        return None

    upto = M32 >> (31 - b)
    before = upto >> 1
    skip = j = 0
    found = False
    guard = 0
    while guard <= wmask + 1:
        nsh, oc = ~t.sh[w] & upto, t.occ[w]
        if nsh:
            j = nsh.bit_length() - 1
            skip += popc(oc & before & (M32 << j) & M32)
            found = True
            break
        skip += popc(oc & before)
        w = (w - 1) & wmask
        upto = before = M32
        guard += 1
    run.loop(guard + 1)
    if not found:
        return None
    start = ((w << 5) | j) & smask

    frm, c = (M32 << j) & M32, 0
    found = False
    guard = 0
    while guard <= wmask + 1:
        c = t.cont[w]
        z = ~c & frm & M32
        pc = popc(z)
        if pc > skip:
            run.loop(skip)
            while skip:
                z &= z - 1
                skip -= 1
            j = ffs(z) - 1
            found = True
            break
        skip -= pc
        w = (w + 1) & wmask
        frm = M32
        guard += 1
    run.loop(guard + 1)
    if not found:
        return None

    steps = 0
    while steps <= smask:
        slot = ((w << 5) | j) & smask
        v = t.filter[slot]
        if v >= rem:
            run.loop(steps + 1)
            return (slot, start) if v == rem else None
        j += 1
        if j == 32:
            j = 0
            w = (w + 1) & wmask
            c = t.cont[w]
        if not (c >> j) & 1:
            run.loop(steps + 1)
            return None
        steps += 1
    run.loop(steps)
    return None


# ------------------------------------------------------------------ k_qf_locate
def locate(t: Table, hashes, run: Run) -> None:
    n, s = len(hashes), run.scratch
    for h in hashes:
        hit = qf_find(t, h, run)
        if hit is None:
            continue
        slot, start = hit
        bit = 1 << (slot & 31)
        old = s[run.dead + (slot >> 5)]
        s[run.dead + (slot >> 5)] = old | bit
        if old & bit:
            continue  # the same hash twice in the batch
        run.removed += 1
        sbit = 1 << (start & 31)
        old = s[run.dirty + (start >> 5)]
        s[run.dirty + (start >> 5)] = old | sbit
        if old & sbit:
            continue
        at = s[run.cursor]
        s[run.cursor] = at + 1
        if at < n:
            s[run.list + at] = start


# ------------------------------------------------------------------ k_qf_repack, one lane
def repack(t: Table, run: Run, i: int) -> None:
    filter, occ, cont, sh, s = t.filter, t.occ, t.cont, t.sh, run.scratch
    dead, dirty = run.dead, run.dirty
    smask = t.size - 1
    wmask = smask >> 5
    b = s[run.list + i] & smask
    mw, mmask, mc, ms = b >> 5, 0, 0, 0  # the metadata word being written: bits decided, continuation and shifted values

    def flush():
        nonlocal mmask, mc, ms
        c0, s0 = mmask & ~mc, mmask & ~ms
        if c0:
            cont[mw] = cont[mw] & ~c0 & M32
        if mc:
            cont[mw] = cont[mw] | mc
        if s0:
            sh[mw] = sh[mw] & ~s0 & M32
        if ms:
            sh[mw] = sh[mw] | ms
        mmask = mc = ms = 0

    def emit(off, c, sbit, rem):  # offsets arrive ascending, each once
        nonlocal mw, mmask, mc, ms
        p = (b + off) & smask
        bit = 1 << (p & 31)
        if (p >> 5) != mw:
            flush()
            mw = p >> 5
        mmask |= bit
        if c:
            mc |= bit
        if sbit:
            ms |= bit
        filter[p] = rem

    rw, wsh, wcont, wdead, dbits = M32, 0, 0, 0, 0  # the word being read, and the dead bits consumed in it
    oc, alive = b, 0  # the quotient of the run being read, its survivors so far
    nxt, eo = 0, 0  # the earliest offset the next survivor may take; the next offset to write
    moved, sound = False, True
    steps = 0
    while steps <= smask:
        p = (b + steps) & smask
        bit = 1 << (p & 31)
        if (p >> 5) != rw:
            if dbits:
                s[dead + rw] = s[dead + rw] & ~dbits & M32
            rw, dbits = p >> 5, 0
            wsh, wcont, wdead = sh[rw], cont[rw], s[dead + rw]
        if steps and not wsh & bit:
            break
        if steps and not wcont & bit:  # the next run starts here
            if not alive:
                occ[oc >> 5] = occ[oc >> 5] & ~(1 << (oc & 31)) & M32
            alive = 0
            x = (oc + 1) & smask
            w, m = x >> 5, occ[x >> 5] & (M32 << (x & 31)) & M32
            guard = 0
            while guard <= wmask and not m:
                w = (w + 1) & wmask
                m = occ[w]
                guard += 1
            run.loop(guard)
            if not m:  # more runs than occupied bits: not a quotient filter's table
                sound = False
                break
            oc = (w << 5) + ffs(m) - 1
        if wdead & bit:
            dbits |= bit
            if not moved:
                moved, eo = True, steps
            steps += 1
            continue
        qo = (oc - b) & smask
        wo = qo if qo > nxt else nxt
        nxt = wo + 1
        if moved:
            rem = filter[p]
            run.loop(max(wo - eo, 0))
            while eo < wo:
                emit(eo, False, False, 0)
                eo += 1
            emit(wo, alive != 0, wo != qo, rem)
            eo = wo + 1
        alive += 1
        steps += 1
    run.loop(steps)
    if sound and not alive:
        occ[oc >> 5] = occ[oc >> 5] & ~(1 << (oc & 31)) & M32
    if moved:
        run.loop(max(steps - eo, 0))
        while eo < steps:
            emit(eo, False, False, 0)
            eo += 1
    flush()
    if dbits:
        s[dead + rw] = s[dead + rw] & ~dbits & M32
    s[dirty + (b >> 5)] = s[dirty + (b >> 5)] & ~(1 << (b & 31)) & M32


# ------------------------------------------------------------------ psk_qf_remove_alt
def remove_in_place(t: Table, batch, order=None) -> Run:
    """the table `t` after ``remove_alt`` of every hash of `batch` (the ABI asks for sorted distinct hashes; the kernels do not need either)
    -> the run: ``removed``, ``scratch``, ``starts``, ``longest``.  `order(n)` gives the order in which the n listed clusters are repaired."""
    hs = [int(h) for h in batch]
    n = len(hs)
    run = Run(t, n)
    if n == 0:
        return run
    locate(t, hs, run)
    cursor = run.scratch[run.cursor]
    count = cursor if cursor < n else n
    run.starts = [run.scratch[run.list + i] for i in range(count)]
    lanes = list(range(count)) if order is None else list(order(count))
    assert sorted(lanes) == list(range(count)), "every listed cluster is repaired once"
    for i in lanes:
        repack(t, run, i)
    run.scratch[run.cursor] = 0  # the host's memset behind the launches
    return run


def scratch_is_zero(t: Table, run: Run) -> bool:
    """dead, dirty, cursor and pad (the list behind them is written before it is read)"""
    return not run.scratch.a[: 2 * t.words + 2].any()
