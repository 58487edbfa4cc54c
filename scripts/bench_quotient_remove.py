#!/usr/bin/env python3
"""Batch removal from a QuotientFilter at q = 24, load 0.8: `remove_alt_many` of m present hashes, m = 2^10 ... 2^22, under both forced
policies -- "local" (psk_qf_remove_alt: the hit clusters repaired in place) and "rebuild" (decode, sorted set difference, psk_qf_build) --
next to the only small update the table had before: `add_alt_many` of ONE new hash, a rebuild of all 2^q slots.

Every call is timed end to end as a user makes it (the batch's sort + unique, the kernels, the read-back of the removed count), around a
device synchronise; the table is put back from a copy between calls, outside the timing.  Warm-up first, then the median of `--reps` runs.
The table goes to `--out`, one JSON line to stdout.  profiles/quotient_remove_bench.txt holds the default run and one with
`--quotient 20 --max-log2 19`: the crossover of `_remove_policy = "auto"` (REMOVE_LOCAL_MAX_FRACTION) is read from the two."""
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
ap.add_argument("--quotient", type=int, default=24)
ap.add_argument("--load", type=float, default=0.8)
ap.add_argument("--min-log2", type=int, default=10)
ap.add_argument("--max-log2", type=int, default=22)
ap.add_argument("--verify", action="store_true", help="also compare the four arrays the two paths leave, at every m (untimed)")
ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "quotient_remove_bench.txt")
args = ap.parse_args()

q = args.quotient
gen = torch.Generator(device="cuda").manual_seed(24)
n = int(args.load * (1 << q))
hashes = torch.unique(torch.randint(-(2**31), 2**31, (n + n // 64,), dtype=torch.int64, device="cuda", generator=gen))
hashes = hashes[torch.randperm(hashes.numel(), device="cuda", generator=gen)][:n].to(torch.int32)  # int32 bit patterns of distinct 32-bit hashes

qf = pa.QuotientFilter(quotient=q, auto_expand=False)
qf.add_alt_many(hashes)
assert qf.elements_held == n
saved = tuple(t.clone() for t in (qf._filter, qf._occ, qf._cont, qf._sh))


def restore():
    for dst, src in zip((qf._filter, qf._occ, qf._cont, qf._sh), saved):
        dst.copy_(src)
    qf._held, qf._stale = n, 0


def median_time(fn, reps, warm=1):
    ts = []
    for r in range(warm + reps):
        restore()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warm:
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


absent = torch.tensor([12345], dtype=torch.int32, device="cuda")
assert not bool(qf.check_alt_many(absent)[0])
t_add = median_time(lambda: qf.add_alt_many(absent), args.reps)

rows = []
lines = [f"QuotientFilter.remove_alt_many, q = {q}, load {args.load} ({n} hashes held), {torch.cuda.get_device_name(0)}; median of {args.reps} calls, end to end",
         f"one-hash add_alt_many (decode + sort + rebuild of all 2^{q} slots): {t_add * 1e3:.3f} ms",
         f"{'m':>9} {'local ms':>10} {'rebuild ms':>11} {'rebuild/local':>14} {'local M hashes/s':>17}"]
for lg in range(args.min_log2, args.max_log2 + 1):
    m = 1 << lg
    batch = hashes[torch.randperm(n, device="cuda", generator=gen)[:m]].clone()
    t = {}
    for policy in ("local", "rebuild"):
        qf._remove_policy = policy

        def call():
            assert qf.remove_alt_many(batch) == m

        t[policy] = median_time(call, args.reps)
    if args.verify:  # faster and different is not faster: both paths must leave the same table
        left = {}
        for policy in ("local", "rebuild"):
            qf._remove_policy = policy
            restore()
            qf.remove_alt_many(batch)
            left[policy] = tuple(x.clone() for x in (qf._filter, qf._occ, qf._cont, qf._sh))
        assert all(torch.equal(a, b) for a, b in zip(left["local"], left["rebuild"])), f"the two paths differ at m = {m}"
    rows.append({"m": m, "local_s": t["local"], "rebuild_s": t["rebuild"]})
    lines.append(f"{m:>9} {t['local'] * 1e3:>10.3f} {t['rebuild'] * 1e3:>11.3f} {t['rebuild'] / t['local']:>14.2f} {m / t['local'] / 1e6:>17.1f}")
    print(lines[-1], flush=True)

wins = [r["m"] for r in rows if r["local_s"] < r["rebuild_s"]]
lines.append(f"local is the faster path for m in {{{', '.join(str(m) for m in wins)}}}" if wins else "rebuild is the faster path at every m measured")
args.out.parent.mkdir(parents=True, exist_ok=True)
args.out.write_text("\n".join(lines) + "\n")
print(json.dumps({"bench": "quotient_remove", "device": torch.cuda.get_device_name(0), "q": q, "load": args.load, "held": n, "reps": args.reps,
                  "one_hash_add_s": t_add, "rows": rows}))
