#!/usr/bin/env python3
"""BloomFilterBank against the loop over BloomFilter objects it replaces, and the measurements behind its constants.

(a) the grouped build: `--filters` filters of (10000, 0.01) (m = 95 851 bits, rows of 11 984 bytes) and 2^`--log2-keys` device keys grouped by
    offsets, through `BloomFilterBank.add_many(keys, filter_offsets=...)` under the build's three routes -- against the loop a user writes without
    the bank (one `BloomFilter` per filter, one `add_many` per segment) and against the ceiling (ONE `BloomFilter.add_many` of all keys into one
    table of the same total size).
(b) random ids, n = 2^14 ... 2^`--log2-keys`: direct atomics (`psk_bank_add`) against torch.sort + grouped build (`psk_bank_build` with perm): this
    decides BANK_GROUP_MIN_KEYS (pyprobables_amd/bank.py).
(c) `check_many` of present and of absent keys.
(d) keys per filter 1 ... 1024, grouped: LDS image (route 1) against global atomics (route 2): the crossover in keys * k / words is the R of
    route 0 (kBankRouteR, csrc/psk_bank.hip).

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
from pyprobables_amd import bank as bank_mod  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--filters", type=int, default=4096)
ap.add_argument("--log2-keys", type=int, default=25)
ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "bank_bench.txt")
args = ap.parse_args()
assert args.reps >= 7

EST, FPR = 10000, 0.01
F, n = args.filters, 1 << args.log2_keys
gen = torch.Generator(device="cuda").manual_seed(25)
keys = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device="cuda", generator=gen)
other = torch.randint(0, 256, (1 << min(args.log2_keys, 24), 16), dtype=torch.uint8, device="cuda", generator=gen)
bank = pa.BloomFilterBank(F, EST, FPR)
m, k, words = bank.number_bits, bank.number_hashes, bank.row_bytes // 4
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


result = {"bench": "bank", "device": dev, "filters": F, "m": m, "k": k, "row_bytes": bank.row_bytes, "keys": n, "reps": args.reps}
lines = [f"BloomFilterBank, {F} filters of ({EST}, {FPR}): m = {m}, k = {k}, rows of {bank.row_bytes} bytes; {dev}; median of {args.reps} calls, end to end",
         f"constants in force: R = {bank_mod.BANK_ROUTE_R}, BANK_GROUP_MIN_KEYS = {bank_mod.BANK_GROUP_MIN_KEYS}, split = {bank.split_for()} "
         f"(1 unless filters < 2 * CUs = {2 * bank._cus}, then ceil(2 * CUs / filters))", ""]

# ---- (a)
per = n // F
offs = torch.arange(F + 1, device="cuda", dtype=torch.int64) * per
offs[-1] = n
lines.append(f"(a) grouped build of 2^{args.log2_keys} keys by offsets ({per} keys per filter)")
ta = {}
for name, route in (("route 0 (auto)", 0), ("route 1 (LDS image)", 1), ("route 2 (global atomics)", 2)):
    forced("grouped", route)
    ta[name] = median_time(lambda: bank.add_many(keys, filter_offsets=offs, validate=False), bank.clear)
    lines.append(f"    bank, {name:<26} {ta[name] * 1e3:>10.3f} ms {n / ta[name] / 1e9:>8.2f} G keys/s")
forced("direct", 0)
ta["direct"] = median_time(lambda: bank.add_many(keys, filter_offsets=offs, validate=False), bank.clear)
lines.append(f"    bank, {'direct atomics (ids)':<26} {ta['direct'] * 1e3:>10.3f} ms {n / ta['direct'] / 1e9:>8.2f} G keys/s")
singles = [pa.BloomFilter(EST, FPR) for _ in range(F)]
bounds = offs.cpu().tolist()
segs = [keys[bounds[f]:bounds[f + 1]] for f in range(F)]


def loop():
    for blm, seg in zip(singles, segs):
        blm.add_many(seg)


ta["loop"] = median_time(loop)
lines.append(f"    loop over {F} BloomFilter objects {'':<4} {ta['loop'] * 1e3:>10.3f} ms {n / ta['loop'] / 1e9:>8.2f} G keys/s")
forced("grouped", 0)
bank.clear()
bank.add_many(keys, filter_offsets=offs, validate=False)
same = all(torch.equal(bank.table_tensor[f], singles[f]._tab.tensor) for f in range(0, F, max(1, F // 64)))
assert same, "the bank's rows differ from the loop's filters"
del singles, segs
one = pa.BloomFilter(EST * F, FPR)
ta["ceiling"] = median_time(lambda: one.add_many(keys))
lines.append(f"    ONE BloomFilter of m = {one.number_bits:<12} {ta['ceiling'] * 1e3:>10.3f} ms {n / ta['ceiling'] / 1e9:>8.2f} G keys/s   (the ceiling)")
lines.append(f"    bank (route 0) / loop = {ta['loop'] / ta['route 0 (auto)']:.1f} x faster; rows compared with the loop's filters: equal")
lines.append("")
result["a"] = ta
del one

# ---- (b)
lines.append("(b) random ids: direct atomics against torch.sort + grouped build (route 0)")
lines.append(f"    {'n':>10} {'direct ms':>10} {'grouped ms':>11} {'direct/grouped':>15}")
rows_b = []
for lg in range(14, args.log2_keys + 1):
    nn = 1 << lg
    ids = torch.randint(0, F, (nn,), dtype=torch.int64, device="cuda", generator=gen)
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
forced("grouped", 0)
bank.clear()
bank.add_many(keys, filter_offsets=offs, validate=False)
nc = other.shape[0]
ids_present = torch.repeat_interleave(torch.arange(F, device="cuda"), offs[1:] - offs[:-1])[:nc]
ids_absent = torch.randint(0, F, (nc,), dtype=torch.int64, device="cuda", generator=gen)
tc = {"present": median_time(lambda: bank.check_many(keys[:nc], ids_present, validate=False)),
      "absent": median_time(lambda: bank.check_many(other, ids_absent, validate=False))}
hits = (int(bank.check_many(keys[:nc], ids_present).sum().item()), int(bank.check_many(other, ids_absent).sum().item()))
assert hits[0] == nc
lines.append(f"(c) check_many of {nc} keys: present {tc['present'] * 1e3:.3f} ms ({nc / tc['present'] / 1e9:.2f} G keys/s), "
             f"absent {tc['absent'] * 1e3:.3f} ms ({nc / tc['absent'] / 1e9:.2f} G keys/s; {hits[1]} false positives)")
lines.append("")
result["c"] = tc

# ---- (d)
lines.append(f"(d) grouped build, keys per filter: LDS image (route 1) against global atomics (route 2); rows of {words} words, k = {k}")
lines.append(f"    {'keys/filter':>11} {'keys*k/words':>13} {'image ms':>10} {'atomics ms':>11} {'atomics/image':>14}")
rows_d = []
for per_f in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024):
    if per_f * F > n:
        break
    o = torch.arange(F + 1, device="cuda", dtype=torch.int64) * per_f
    kk = keys[: per_f * F]
    t = {}
    for route in (1, 2):
        forced("grouped", route, 1)
        t[route] = median_time(lambda: bank.add_many(kk, filter_offsets=o, validate=False), bank.clear)
    rows_d.append({"keys_per_filter": per_f, "image_s": t[1], "atomics_s": t[2]})
    lines.append(f"    {per_f:>11} {per_f * k / words:>13.3f} {t[1] * 1e3:>10.3f} {t[2] * 1e3:>11.3f} {t[2] / t[1]:>14.2f}")
cross = next((r["keys_per_filter"] for r in rows_d if r["image_s"] < r["atomics_s"]), None)
lines.append(f"    the image wins from {cross} keys per filter on: keys * k / words = {cross * k / words:.3f}, i.e. R = words / (keys * k) = {words / (cross * k):.1f}"
             if cross else "    global atomics win at every size measured")
result["d"] = rows_d

args.out.parent.mkdir(parents=True, exist_ok=True)
args.out.write_text("\n".join(lines) + "\n")
print("\n".join(lines), flush=True)
print(json.dumps(result))
