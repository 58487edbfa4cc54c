"""Host model of pass 1's fixed-capacity bins (psk_part_bins.hpp, bins_plan / launch_scatter_bins in psk_host.hpp) for power-of-two Bloom
tables: which probes a batch puts into which (tile, slice) bin, what a bin carries into the next tile, and how many probes find their bin
full and take the exact fallback.  Everything here follows from the keys alone (hashes.py:71-103, bloom.py:241-272), so the counts are exact,
not estimates.  Test infrastructure: numpy only."""

import numpy as np

FNV_BASIS, FNV_PRIME = 0xCBF29CE484222325, 0x100000001B3
BIN_THREADS, BIN_KPT, MAX_WGS = 768, 2, 512   # kBinThreads, kBinKpt, two workgroups on each of 256 CUs


def fnv_indices(keys: np.ndarray, k: int, m: int) -> np.ndarray:
    """uint64[n, k]: bit index of probe j of every 16-byte key = fnv_1a(key, seed=j) % m"""
    keys = np.ascontiguousarray(keys, dtype=np.uint8)
    out = np.empty((keys.shape[0], k), dtype=np.uint64)
    prime = np.uint64(FNV_PRIME)
    with np.errstate(over="ignore"):
        for j in range(k):
            h = np.full(keys.shape[0], (FNV_BASIS + 31 * j) & (2**64 - 1), dtype=np.uint64)
            for b in range(keys.shape[1]):
                h = (h ^ keys[:, b].astype(np.uint64)) * prime
            out[:, j] = h % np.uint64(m)
    return out


def plan(n: int, k: int, nslices: int, even_tiles: int = 1):
    """(keys per tile, workgroups, tiles per workgroup) as launch_scatter_bins lays a round of n keys out"""
    tile_full = BIN_THREADS * BIN_KPT
    ntiles = -(-n // tile_full)
    nwg = max(1, min(MAX_WGS, ntiles))
    per_wg = -(-ntiles // nwg)
    tk = tile_full
    if even_tiles and nwg * per_wg > ntiles:
        tk = min(tile_full, (-(-n // (nwg * per_wg)) + 63) & ~63)
    return tk, nwg, per_wg


def bin_capacity(k: int, nslices: int, carry_group: bool) -> int:
    """bins_plan: mean + 3.5 sigma of a full tile's load, in whole groups of six; + one group for the carried probes"""
    mean = BIN_THREADS * BIN_KPT * k / nslices
    cap = (int(mean + 3.5 * np.sqrt(mean) + 2.0) + 5) // 6 * 6
    return cap + 6 if carry_group else cap


def cms_indices(keys: np.ndarray, depth: int, width: int) -> np.ndarray:
    """uint64[n, depth]: cell of row j of every 16-byte key = j * width + fnv_1a(key, seed=j) % width (countminsketch.py:267-288)"""
    return fnv_indices(keys, depth, width) + np.arange(depth, dtype=np.uint64) * np.uint64(width)


def segment_capacity(n: int, k: int, nslices: int, even_tiles: int = 1) -> int:
    """groups a (workgroup, slice) segment has room for, as launch_scatter_bins sizes it from the round's mean load"""
    tk, _, per_wg = plan(n, k, nslices, even_tiles)
    mean = per_wg * tk * k / nslices
    return int(mean / 6.0 + 0.5 * per_wg + 8.0 * np.sqrt(mean) / 6.0 + 16.0)


def spills(idx: np.ndarray, nslices: int, shift: int, cap: int, carry: bool, even_tiles: int = 1, ids: np.ndarray = None,
           segcap: int = None, tile_tag: bool = False) -> dict:
    """idx = fnv_indices(...) of the batch's keys -- or, with ids, of a pool of keys, and key i of the batch is pool key ids[i].
    carry = False: every tile closes its bins with a padded group (the bins before the carry).
    -> bin_spills (probes that met a full bin), groups written, pad slots among them, thin = share of (tile, slice) bins with fewer than six
    probes of their own tile, forced_tag = bins that hold carried probes and stay short of six (a tile-flag pass 1, tile_tag, sends those
    out at once).  With segcap (carry only) the write-out's segment cursors are followed too, branch by branch as k_part_bins takes them:
    seg_full = write-outs that did not fit their segment, seg_full_rem = those whose bin held a remainder then, seg_full_after = write-outs
    that found the cursor past the segment's end already, seg_spills = probes such write-outs handed to the exact fallback, flush_spills =
    probes the flush behind the last tile found no room for."""
    k = idx.shape[1]
    n = idx.shape[0] if ids is None else ids.shape[0]
    tk, nwg, per_wg = plan(n, k, nslices, even_tiles)
    ntiles = -(-n // tk)
    tile_of = (np.arange(n, dtype=np.int64) // tk) * nslices
    slice_of = (idx >> np.uint64(shift)).astype(np.int64)
    cnt = np.zeros(ntiles * nslices, dtype=np.int64)
    for j in range(k):
        cnt += np.bincount(tile_of + (slice_of[:, j] if ids is None else slice_of[ids, j]), minlength=ntiles * nslices)
    cnt = cnt.reshape(ntiles, nslices)
    full = np.zeros((nwg * per_wg, nslices), dtype=np.int64)
    full[:ntiles] = cnt
    exists = np.zeros(nwg * per_wg, dtype=bool)
    exists[:ntiles] = True
    r = np.zeros((nwg, nslices), dtype=np.int64)
    cur = np.zeros((nwg, nslices), dtype=np.int64)
    room = np.iinfo(np.int64).max if segcap is None else segcap
    bin_spills = groups = pads = forced_tag = 0
    seg_full = seg_full_rem = seg_full_after = seg_spills = flush_spills = 0
    for o in range(per_wg):   # tile = o * nwg + workgroup
        own = full[o * nwg:(o + 1) * nwg]
        live = exists[o * nwg:(o + 1) * nwg][:, None] & np.ones((1, nslices), dtype=bool)
        c = np.minimum(r + own, cap)
        bin_spills += int((r + own - c).sum())
        whole, rem = c // 6, c % 6
        if carry:
            tail = (whole == 0) & (r > 0) & live     # PayTileTag only: carried probes never wait a second tile
            forced_tag += int(tail.sum())
            ngroups = whole + (tail if tile_tag else 0)
            fits = cur + ngroups <= room
            fast, slow = live & fits, live & ~fits
            nall = whole + (rem > 0)
            written = np.clip(room - cur, 0, nall)   # slow path: the groups in front of the segment's end
            seg_full += int(slow.sum())
            seg_full_rem += int((slow & (rem > 0)).sum())
            seg_full_after += int((slow & (cur > room)).sum())
            seg_spills += int(((c - np.minimum(c, 6 * written)) * slow).sum())
            groups += int((ngroups * fast).sum() + (written * slow).sum())
            pads += int((((6 - rem) % 6) * (fast & tail & tile_tag)).sum() + (((6 - rem) % 6) * (slow & (written == nall))).sum())
            r = np.where(fast, np.where(tail & tile_tag, 0, rem), np.where(slow, 0, r))
            cur = cur + np.where(fast, ngroups, 0) + np.where(slow, nall, 0)
        else:
            groups += int((whole + (rem > 0)).sum())
            pads += int(((6 - rem) % 6).sum())
    if carry:
        fits = cur < room
        groups += int(((r > 0) & fits).sum())
        pads += int((((6 - r) % 6) * fits).sum())
        flush_spills = int((r * ~fits).sum())
    return {"tile": tk, "nwg": nwg, "per_wg": per_wg, "probes": n * k, "bin_spills": bin_spills, "groups": groups, "pads": pads,
            "thin": float((cnt < 6).mean()), "forced_tag": forced_tag, "seg_full": seg_full, "seg_full_rem": seg_full_rem,
            "seg_full_after": seg_full_after, "seg_spills": seg_spills, "flush_spills": flush_spills}
