#!/usr/bin/env python3
"""BloomFilterBank as sets -- bit counts, all-pairs overlap, row folds -- against the two ways there were without them.

The geometry of DESIGN.md 3.13 / 3.14: `--filters` filters of (10000, 0.01) (m = 95 851 bits, k = 7, rows of 11 984 bytes), each holding
`--per-filter` keys.

(1) `bits_set()` over the bank.
(2) `overlap()` over all pairs (the symmetric case: the upper triangle of tiles is computed) and `overlap(a, b)` for 256 x `--filters`.
(3) `reduce` of 512 groups of 8 filters, both ops.
(4) baseline (i), the only way before: `bank.filter(a).jaccard_index(bank.filter(b))`, timed on 256 sampled pairs and SCALED to the pair counts
    of (2); baseline (ii), torch alone: the rows unpacked to 0 / 1 float16 (an operand 16 times the table's size) and `torch.matmul`; the
    unpacking time and the peak memory are reported apart from the matmul.  Both run in this process, after the kernel's own timings.

Beside the overlap times stands the VALU floor of DESIGN.md 3.14: pairs x row words x 2 VALU lane-operations (v_and_b32 + v_bcnt_u32_b32) at
32 lanes per cycle per SIMD, 4 SIMDs x 256 CUs, 2.4 GHz -- an estimate, not a measurement.

Every call is timed end to end as a user makes it, around a device synchronise.  Warm-up first, then the median of `--reps` (>= 7) calls.  The
tables go to `--out`, one JSON line to stdout."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

import pyprobables_amd as pa  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--filters", type=int, default=4096)
ap.add_argument("--per-filter", type=int, default=5000)
ap.add_argument("--sample", type=int, default=256)
ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "bank_stats_bench.txt")
args = ap.parse_args()
assert args.reps >= 7

EST, FPR = 10000, 0.01
F, per = args.filters, args.per_filter
gen = torch.Generator(device="cuda").manual_seed(41)
bank = pa.BloomFilterBank(F, EST, FPR)
m, k = bank.number_bits, bank.number_hashes
dev = torch.cuda.get_device_name(0)
for lo in range(0, F, 512):  # filled in slabs: the keys of the whole bank need not be resident at once
    hi = min(F, lo + 512)
    keys = torch.randint(0, 256, ((hi - lo) * per, 16), dtype=torch.uint8, device="cuda", generator=gen)
    offs = torch.zeros(F + 1, dtype=torch.int64, device="cuda")
    offs[lo + 1:hi + 1] = torch.arange(1, hi - lo + 1, device="cuda") * per
    offs[hi + 1:] = (hi - lo) * per
    bank.add_many(keys, filter_offsets=offs, validate=False)
    del keys
words = bank.row_bytes // 4
table_bytes = F * bank.row_bytes


def median_time(fn, warm=2, reps=None):
    ts = []
    for r in range(warm + (reps or args.reps)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warm:
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def valu_floor(pairs):
    return pairs * words * 2 / (32 * 4 * 256 * 2.4e9)


result = {"bench": "bank_stats", "device": dev, "filters": F, "m": m, "k": k, "row_bytes": bank.row_bytes, "per_filter": per, "reps": args.reps}
lines = [f"BloomFilterBank statistics, {F} filters of ({EST}, {FPR}) holding {per} keys each: m = {m}, k = {k}, rows of {bank.row_bytes} bytes, table of "
         f"{table_bytes / 1e6:.1f} MB; {dev}; median of {args.reps} calls, end to end", ""]

# ---- (1)
t_bits = median_time(bank.bits_set)
fill = bank.bits_set().double().mean().item() / m
lines += ["(1) bits_set() over the bank", f"    {t_bits * 1e3:>10.3f} ms   {table_bytes / t_bits / 1e9:>8.1f} GB/s read   (mean fill {fill:.3f})", ""]
result["1"] = {"bits_set_s": t_bits, "fill": fill}

# ---- (2)
A = min(256, F)
a_ids = torch.randperm(F, device="cuda", generator=gen)[:A].contiguous()
pairs_all_sym, pairs_all, pairs_rect = F * (F + 1) // 2, F * F, A * F
t_all = median_time(bank.overlap)
t_rect = median_time(lambda: bank.overlap(a=a_ids))
lines.append("(2) overlap: popcount(row a AND row b) for every pair")
lines.append(f"    {'shape':>14} {'ms':>10} {'G pair-words/s':>15} {'VALU floor ms (estimate)':>26}")
lines.append(f"    {f'{F} x {F} sym':>14} {t_all * 1e3:>10.3f} {pairs_all_sym * words / t_all / 1e9:>15.1f} {valu_floor(pairs_all_sym) * 1e3:>26.3f}   (upper triangle computed, "
             f"both halves stored: {pairs_all * 4 / 1e6:.0f} MB out)")
lines.append(f"    {f'{A} x {F}':>14} {t_rect * 1e3:>10.3f} {pairs_rect * words / t_rect / 1e9:>15.1f} {valu_floor(pairs_rect) * 1e3:>26.3f}")
lines.append("    floor: pairs x row words x 2 VALU lane-ops / (32 lanes x 4 SIMDs x 256 CUs x 2.4 GHz); whether v_bcnt_u32_b32 issues at the full rate is not known")
lines.append("")
result["2"] = {"all_s": t_all, "rect_s": t_rect, "floor_all_s": valu_floor(pairs_all_sym), "floor_rect_s": valu_floor(pairs_rect)}

# ---- (3)
Gn, gs = min(512, F), 8
members = torch.randint(0, F, (Gn * gs,), device="cuda", generator=gen)
goffs = torch.arange(Gn + 1, device="cuda", dtype=torch.int64) * gs
t_or = median_time(lambda: bank.reduce((goffs, members), op="or", validate=False))
t_and = median_time(lambda: bank.reduce((goffs, members), op="and", validate=False))
moved = (Gn * gs + Gn) * bank.row_bytes
lines.append(f"(3) reduce: {Gn} groups of {gs} filters -> a new bank (allocation, estimate_elements of every row and its copy to the host included)")
lines.append(f"    or   {t_or * 1e3:>10.3f} ms   {moved / t_or / 1e9:>8.1f} GB/s read + written")
lines.append(f"    and  {t_and * 1e3:>10.3f} ms   {moved / t_and / 1e9:>8.1f} GB/s read + written")
lines.append("")
result["3"] = {"or_s": t_or, "and_s": t_and}

# ---- (4) (i)
S = args.sample
pi = torch.randint(0, F, (S, 2), generator=torch.Generator().manual_seed(5)).tolist()


def per_object():
    for x, y in pi:
        bank.filter(x).jaccard_index(bank.filter(y))


t_obj = median_time(per_object, warm=1, reps=3) / S
jac = bank.jaccard(a=[p[0] for p in pi[:8]], b=[p[1] for p in pi[:8]]).cpu()
for j, (x, y) in enumerate(pi[:8]):
    assert float(jac[j, j]) == bank.filter(x).jaccard_index(bank.filter(y)), "jaccard and the per-object jaccard_index disagree"
lines.append("(4) baselines, same process")
lines.append(f"    (i) bank.filter(a).jaccard_index(bank.filter(b)): {t_obj * 1e3:.3f} ms a pair (median of 3 runs over {S} sampled pairs)")
lines.append(f"        SCALED, not run: {pairs_all_sym} pairs = {t_obj * pairs_all_sym:.0f} s ({t_obj * pairs_all_sym / t_all:.0f} x overlap()); "
             f"{pairs_rect} pairs = {t_obj * pairs_rect:.0f} s ({t_obj * pairs_rect / t_rect:.0f} x overlap(a, b))")
result["4i"] = {"pair_s": t_obj, "sampled_pairs": S}

# ---- (4) (ii)
torch.cuda.synchronize()
torch.cuda.reset_peak_memory_stats()
base_mem = torch.cuda.memory_allocated()
shifts = torch.arange(32, device="cuda", dtype=torch.int32)


def unpack(rows):
    out = torch.empty((rows.shape[0], words * 32), dtype=torch.float16, device="cuda")
    for lo in range(0, rows.shape[0], 256):  # (in slabs: the int32 intermediate of the whole bank would be 32 times the table)
        r = rows[lo:lo + 256]
        out[lo:lo + 256] = ((r.unsqueeze(-1) >> shifts) & 1).reshape(r.shape[0], -1).to(torch.float16)
    return out


tt = bank.table_tensor
t_unpack = median_time(lambda: unpack(tt), warm=1, reps=3)
U = unpack(tt)
t_mm = median_time(lambda: torch.matmul(U, U.T))
Ua = U[a_ids].contiguous()
t_mm_rect = median_time(lambda: torch.matmul(Ua, U.T))
got = torch.matmul(Ua, U.T)
torch.cuda.synchronize()
peak = torch.cuda.max_memory_allocated() - base_mem
exact = bool((got.float().round().to(torch.int32) == bank.overlap(a=a_ids)).all().item())
lines.append(f"    (ii) torch alone: rows unpacked to 0 / 1 float16 ({U.numel() * 2 / 1e9:.2f} GB, 16 x the table), then torch.matmul (float16 result)")
lines.append(f"        unpack {t_unpack * 1e3:>10.3f} ms;  matmul {F} x {F}: {t_mm * 1e3:>10.3f} ms;  matmul {A} x {F}: {t_mm_rect * 1e3:>10.3f} ms;  peak memory {peak / 1e9:.2f} GB "
             f"beside the table")
lines.append(f"        its float16 counts equal overlap(a, b): {exact}" + ("" if exact else "  (float16 holds integers up to 2048 exactly: counts beyond that are rounded)"))
win_all, win_rect = t_mm < t_all, t_mm_rect < t_rect
lines.append(f"        matmul alone against the kernel: {F} x {F}: {t_all / t_mm:.2f} x ({'matmul' if win_all else 'kernel'} ahead);  {A} x {F}: {t_rect / t_mm_rect:.2f} x "
             f"({'matmul' if win_rect else 'kernel'} ahead);  with the unpack: {F} x {F}: {t_all / (t_mm + t_unpack):.2f} x")
result["4ii"] = {"unpack_s": t_unpack, "matmul_all_s": t_mm, "matmul_rect_s": t_mm_rect, "peak_bytes": peak, "fp16_exact": exact}

args.out.parent.mkdir(parents=True, exist_ok=True)
args.out.write_text("\n".join(lines) + "\n")
print("\n".join(lines), flush=True)
print(json.dumps(result))
