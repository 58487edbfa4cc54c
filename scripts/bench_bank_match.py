#!/usr/bin/env python3
"""BloomFilterBank.match_many -- "which of my filters may hold this key?" -- against the only way the bank offered before: check_many over
every (key, filter) pair.

The geometry of DESIGN.md 3.13: `--filters` filters of (10000, 0.01) (m = 95 851 bits, k = 7), each holding 10000 keys, 16-byte device keys.

(1) the slice image: the full transpose (`psk_bank_slices` over the whole bank) and the refresh of ONE 32-filter column group.
(2) `match_many` in each form ("mask", "count", "ids") for 2^12, 2^16 and 2^20 keys: once with keys that are present in one filter, once with
    absent keys.  The image is current: the refresh is not part of these timings.
(3) the baseline: `check_many` over all pairs of 2^12 keys x `--filters` filters (2^24 pairs at 4096 filters, the size of
    profiles/bank_bench.txt part (c)), the id array built beforehand, outside the timing.

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
ap.add_argument("--per-filter", type=int, default=10000)
ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "bank_match_bench.txt")
args = ap.parse_args()
assert args.reps >= 7

EST, FPR = 10000, 0.01
F, per = args.filters, args.per_filter
n = F * per
gen = torch.Generator(device="cuda").manual_seed(31)
keys = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device="cuda", generator=gen)
absent = torch.randint(0, 256, (1 << 20, 16), dtype=torch.uint8, device="cuda", generator=gen)
bank = pa.BloomFilterBank(F, EST, FPR)
m, k = bank.number_bits, bank.number_hashes
dev = torch.cuda.get_device_name(0)
offs = torch.arange(F + 1, device="cuda", dtype=torch.int64) * per
bank.add_many(keys, filter_offsets=offs, validate=False)
# present probes: one key of every filter in turn, so that a probe's own filter walks over the columns
pick = (torch.arange(1 << 20, device="cuda") % F) * per + torch.randint(0, per, (1 << 20,), device="cuda", generator=gen)
present = keys[pick].contiguous()
own = (pick // per).to(torch.int64)


def median_time(fn, before=None, warm=2):
    ts = []
    for r in range(warm + args.reps):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warm:
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


image_bytes = m * bank.slice_row_bytes
result = {"bench": "bank_match", "device": dev, "filters": F, "m": m, "k": k, "slice_row_bytes": bank.slice_row_bytes, "image_bytes": image_bytes, "reps": args.reps}
lines = [f"BloomFilterBank.match_many, {F} filters of ({EST}, {FPR}) holding {per} keys each: m = {m}, k = {k}, slice rows of {bank.slice_row_bytes} bytes, "
         f"image of {image_bytes / 1e6:.1f} MB; {dev}; median of {args.reps} calls, end to end", ""]

# ---- (1)
t_full = median_time(bank.refresh_slices, bank.invalidate_slices)
t_group = median_time(bank.refresh_slices, lambda: bank._mark_stale(33))
lines.append("(1) the slice image")
lines.append(f"    full transpose ({F} filters)        {t_full * 1e3:>10.3f} ms   {2 * image_bytes / t_full / 1e9:>8.1f} GB/s read + written")
lines.append(f"    refresh of one 32-filter group     {t_group * 1e3:>10.3f} ms")
lines.append("")
result["1"] = {"full_s": t_full, "group_s": t_group}

# ---- (2)
lines.append("(2) match_many, image current")
lines.append(f"    {'keys':>8} {'probes':>8} {'form':>6} {'ms':>10} {'M keys/s':>10} {'G (key, filter) answers/s':>27}")
rows2 = []
for lg in (12, 16, 20):
    nn = 1 << lg
    for name, probes in (("present", present[:nn]), ("absent", absent[:nn])):
        for form in ("mask", "count", "ids"):
            t = median_time(lambda: bank.match_many(probes, form=form))
            rows2.append({"n": nn, "probes": name, "form": form, "s": t})
            lines.append(f"    {nn:>8} {name:>8} {form:>6} {t * 1e3:>10.3f} {nn / t / 1e6:>10.2f} {nn * F / t / 1e9:>27.1f}")
cnt_p = bank.match_many(present[: 1 << 12], form="count")
cnt_a = bank.match_many(absent[: 1 << 12], form="count")
lines.append(f"    filters per key: present {cnt_p.float().mean().item():.2f}, absent {cnt_a.float().mean().item():.2f} (mean over 2^12 keys)")
lines.append("")
result["2"] = rows2

# ---- (3)
nb = 1 << 12
pair_keys = present[:nb].repeat_interleave(F, dim=0).contiguous()
pair_ids = torch.arange(F, device="cuda", dtype=torch.int64).repeat(nb)
t_pairs = median_time(lambda: bank.check_many(pair_keys, pair_ids, validate=False))
pairs = bank.check_many(pair_keys, pair_ids, validate=False).view(nb, F)
mask = bank.match_many(present[:nb])
bits = ((mask.view(nb, -1, 1) >> torch.arange(32, device="cuda", dtype=torch.int32)) & 1).view(nb, -1)[:, :F].bool()
assert torch.equal(bits, pairs), "match_many and check_many over all pairs disagree"
assert bool(pairs[torch.arange(nb, device="cuda"), own[:nb]].all())
t_mask = next(r["s"] for r in rows2 if r["n"] == nb and r["probes"] == "present" and r["form"] == "mask")
lines.append(f"(3) the same answers for 2^12 present keys x {F} filters")
lines.append(f"    check_many over {nb * F} pairs (ids prebuilt) {t_pairs * 1e3:>10.3f} ms {nb * F / t_pairs / 1e9:>8.2f} G pairs/s")
lines.append(f"    match_many, form mask                  {t_mask * 1e3:>10.3f} ms {nb * F / t_mask / 1e9:>8.2f} G pairs/s   = {t_pairs / t_mask:.1f} x the pairs baseline"
             + ("" if t_mask < t_pairs else "   (match_many does NOT beat the baseline)"))
lines.append("    both answers compared bit for bit: equal")
result["3"] = {"pairs_s": t_pairs, "match_mask_s": t_mask}

args.out.parent.mkdir(parents=True, exist_ok=True)
args.out.write_text("\n".join(lines) + "\n")
print("\n".join(lines), flush=True)
print(json.dumps(result))
