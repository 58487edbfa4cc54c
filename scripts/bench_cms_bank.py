#!/usr/bin/env python3
"""CountMinSketchBank against the loop over CountMinSketch objects it replaces, and the measurements behind its constants.

(a) the grouped build: `--sketches` sketches of 2048 x 5 (rows of 40 KiB) and 2^`--log2-keys` 16-byte device keys grouped by offsets, through
    `CountMinSketchBank.add_many(keys, sketch_offsets=...)` under the build's three routes and, with ready-made ids, through the direct atomics -- against the loop
    a user writes without the bank (one `CountMinSketch` per sketch, one `add_many` per segment) and against ONE `CountMinSketch.add_many` of
    all keys into a table of the same total size.
(b) random ids, n = 2^16 ... 2^`--log2-keys`: direct atomics (`psk_cms_bank_add`) against torch.sort + grouped build (`psk_cms_bank_build` with
    perm): this decides CMS_BANK_GROUP_MIN_KEYS (pyprobables_amd/cmsbank.py).
(c) keys per sketch 1 ... 1024, grouped: LDS image (route 1) against global atomics (route 2): the crossover in keys * depth / ints is the R of
    route 0 (kCmsBankRouteR, csrc/psk_cms_bank.hip).
(d) `check_many` under the three query types, and `reduce` of 512 groups of 8.

Every call is timed end to end as a user makes it, around a device synchronise; the bank is cleared between calls, outside the timing.  Warm-up
first, then the median of `--reps` (>= 7) runs.  The tables go to `--out`, one JSON line to stdout."""
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
from pyprobables_amd import cmsbank as bank_mod  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--sketches", type=int, default=4096)
ap.add_argument("--log2-keys", type=int, default=25)
ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "cms_bank_bench.txt")
args = ap.parse_args()
assert args.reps >= 7

WIDTH, DEPTH = 2048, 5
S, n = args.sketches, 1 << args.log2_keys
gen = torch.Generator(device="cuda").manual_seed(26)
keys = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device="cuda", generator=gen)
bank = pa.CountMinSketchBank(S, WIDTH, DEPTH)
ints = bank.row_bytes // 4
dev = torch.cuda.get_device_name(0)


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


def forced(policy, route, split=None):
    bank._add_policy, bank._route, bank._split = policy, route, split


result = {"bench": "cms_bank", "device": dev, "sketches": S, "width": WIDTH, "depth": DEPTH, "row_bytes": bank.row_bytes, "keys": n, "reps": args.reps}
lines = [f"CountMinSketchBank, {S} sketches of {WIDTH} x {DEPTH}: rows of {bank.row_bytes} bytes; {dev}; median of {args.reps} calls, end to end",
         f"constants in force: R = {bank_mod.CMS_BANK_ROUTE_R}, CMS_BANK_GROUP_MIN_KEYS = {bank_mod.CMS_BANK_GROUP_MIN_KEYS}, split = {bank.split_for()} "
         f"(1 unless sketches < 2 * CUs = {2 * bank._cus}, then ceil(2 * CUs / sketches))", ""]

# ---- (a)
per = n // S
offs = torch.arange(S + 1, device="cuda", dtype=torch.int64) * per
offs[-1] = n
lines.append(f"(a) grouped build of 2^{args.log2_keys} keys by offsets ({per} keys per sketch)")
ta = {}
for name, route in (("route 0 (auto)", 0), ("route 1 (LDS image)", 1), ("route 2 (global atomics)", 2)):
    forced("grouped", route)
    ta[name] = median_time(lambda: bank.add_many(keys, sketch_offsets=offs, validate=False), bank.clear)
    lines.append(f"    bank, {name:<26} {ta[name] * 1e3:>10.3f} ms {n / ta[name] / 1e9:>8.2f} G keys/s")
forced("direct", 0)
ids_a = torch.repeat_interleave(torch.arange(S, device="cuda"), offs[1:] - offs[:-1])  # ready-made ids: not part of the timed call
ta["direct"] = median_time(lambda: bank.add_many(keys, ids_a, validate=False), bank.clear)
del ids_a
lines.append(f"    bank, {'direct atomics (ids)':<26} {ta['direct'] * 1e3:>10.3f} ms {n / ta['direct'] / 1e9:>8.2f} G keys/s")
singles = [pa.CountMinSketch(width=WIDTH, depth=DEPTH) for _ in range(S)]
bounds = offs.cpu().tolist()
segs = [keys[bounds[s]:bounds[s + 1]] for s in range(S)]


def loop():
    for cms, seg in zip(singles, segs):
        cms.add_many(seg)


def clear_singles():
    for cms in singles:
        cms.clear()


ta["loop"] = median_time(loop, clear_singles)
lines.append(f"    loop over {S} CountMinSketch objects {'':<1} {ta['loop'] * 1e3:>10.3f} ms {n / ta['loop'] / 1e9:>8.2f} G keys/s")
forced("grouped", 0)
bank.clear()
bank.add_many(keys, sketch_offsets=offs, validate=False)
clear_singles()
loop()
same = all(torch.equal(bank.table_tensor[s], singles[s].table_tensor) for s in range(0, S, max(1, S // 64)))
assert same, "the bank's rows differ from the loop's sketches"
del singles, segs
one = pa.CountMinSketch(width=WIDTH * S, depth=DEPTH)
ta["one table"] = median_time(lambda: one.add_many(keys), one.clear)
lines.append(f"    ONE CountMinSketch of width {one.width:<11} {ta['one table'] * 1e3:>10.3f} ms {n / ta['one table'] / 1e9:>8.2f} G keys/s   (no per-sketch answer)")
best = min(("route 0 (auto)", "route 1 (LDS image)", "route 2 (global atomics)", "direct"), key=lambda k: ta[k])
lines.append(f"    bank (route 0) / loop = {ta['loop'] / ta['route 0 (auto)']:.1f} x faster; fastest bank route: {best}; rows compared with the loop's sketches: equal")
lines.append("")
result["a"] = ta
del one

# ---- (b)
lines.append("(b) random ids: direct atomics against torch.sort + grouped build (route 0)")
lines.append(f"    {'n':>10} {'direct ms':>10} {'grouped ms':>11} {'direct/grouped':>15}")
rows_b = []
for lg in range(16, args.log2_keys + 1):
    nn = 1 << lg
    ids = torch.randint(0, S, (nn,), dtype=torch.int64, device="cuda", generator=gen)
    kk = keys[:nn]
    t = {}
    for policy in ("direct", "grouped"):
        forced(policy, 0)
        t[policy] = median_time(lambda: bank.add_many(kk, ids, validate=False), bank.clear)
    rows_b.append({"n": nn, "direct_s": t["direct"], "grouped_s": t["grouped"]})
    lines.append(f"    {nn:>10} {t['direct'] * 1e3:>10.3f} {t['grouped'] * 1e3:>11.3f} {t['direct'] / t['grouped']:>15.2f}")
wins = [r["n"] for r in rows_b if r["grouped_s"] < r["direct_s"]]
lines.append(f"    sort + grouped is the faster path for n in {{{', '.join(map(str, wins))}}}" if wins else "    direct atomics are the faster path at every n measured")
lines.append("")
result["b"] = rows_b

# ---- (c)
lines.append(f"(c) grouped build, keys per sketch: LDS image (route 1) against global atomics (route 2); rows of {ints} ints, depth = {DEPTH}")
lines.append(f"    {'keys/sketch':>11} {'keys*d/ints':>12} {'image ms':>10} {'atomics ms':>11} {'atomics/image':>14}")
rows_c = []
for per_s in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024):
    if per_s * S > n:
        break
    o = torch.arange(S + 1, device="cuda", dtype=torch.int64) * per_s
    kk = keys[: per_s * S]
    t = {}
    for route in (1, 2):
        forced("grouped", route, 1)
        t[route] = median_time(lambda: bank.add_many(kk, sketch_offsets=o, validate=False), bank.clear)
    rows_c.append({"keys_per_sketch": per_s, "image_s": t[1], "atomics_s": t[2]})
    lines.append(f"    {per_s:>11} {per_s * DEPTH / ints:>12.4f} {t[1] * 1e3:>10.3f} {t[2] * 1e3:>11.3f} {t[2] / t[1]:>14.2f}")
cross = next((r["keys_per_sketch"] for r in rows_c if r["image_s"] < r["atomics_s"]), None)
lines.append(f"    the image wins from {cross} keys per sketch on: keys * depth / ints = {cross * DEPTH / ints:.4f}, i.e. R = ints / (keys * depth) = {ints / (cross * DEPTH):.1f}"
             if cross else "    global atomics win at every size measured")
lines.append("")
result["c"] = rows_c

# ---- (d)
forced("grouped", 0)
bank.clear()
bank.add_many(keys, sketch_offsets=offs, validate=False)
nc = min(n, 1 << 24)
ids_c = torch.repeat_interleave(torch.arange(S, device="cuda"), offs[1:] - offs[:-1])[:nc]
td = {}
for q in ("min", "mean", "mean-min"):
    bank.query_type = q
    td[q] = median_time(lambda: bank.check_many(keys[:nc], ids_c, validate=False))
    lines.append(f"(d) check_many of {nc} keys, query {q:<9} {td[q] * 1e3:>10.3f} ms {nc / td[q] / 1e9:>8.2f} G keys/s")
groups = (torch.randint(0, S, (512 * 8,), dtype=torch.int64, device="cuda", generator=gen), torch.arange(513, device="cuda", dtype=torch.int64) * 8)
td["reduce"] = median_time(lambda: bank.reduce(groups, validate=False))
lines.append(f"(d) reduce of 512 groups of 8 sketches {'':<14} {td['reduce'] * 1e3:>10.3f} ms   (the new bank's table allocated and zeroed inside)")
result["d"] = td

args.out.parent.mkdir(parents=True, exist_ok=True)
args.out.write_text("\n".join(lines) + "\n")
print("\n".join(lines), flush=True)
print(json.dumps(result))
