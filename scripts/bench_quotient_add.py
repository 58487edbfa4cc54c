#!/usr/bin/env python3
"""Batch insertion into a loaded QuotientFilter at q = 24, load about 0.8: `add_alt_many` of m NEW hashes, m = 2^10 ... 2^21, under both forced
policies -- "local" (psk_qf_add_alt: the touched regions rewritten in place) and "rebuild" (decode, concatenate, sort + unique, psk_qf_build:
the only path a loaded table had before, so that is the baseline).

Every call is timed end to end as a user makes it (the batch's sort + unique, the kernels, the read-back of
count and status), around a device synchronise; the table is put back from a copy between calls, outside the timing.  Warm-up first, then the median
of `--reps` runs.  The table goes to `--out` (appended with `--append`, so that one file holds the run at q = 24 and the ones with
`--quotient 22 --max-log2 19` and `--quotient 20 --max-log2 17`), one JSON line to stdout: the two constants of `_add_policy = "auto"`
(ADD_LOCAL_MAX_FRACTION, ADD_LOCAL_MIN_QUOTIENT) are read from them.  The largest batch must fit ABOVE the load: 0.8 * 2^q + m < 2^q, so m stops
at 2^21 for q = 24 (2^22 does not fit), 2^19 for q = 22 and 2^17 for q = 20."""
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
ap.add_argument("--load", type=float, default=0.8, help="load of the table BEHIND the largest batch is load + 2^max-log2 / 2^q: keep it under 1")
ap.add_argument("--min-log2", type=int, default=10)
ap.add_argument("--max-log2", type=int, default=21)
ap.add_argument("--verify", action="store_true", help="also compare the four arrays the two paths leave, at every m (untimed)")
ap.add_argument("--append", action="store_true")
ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "quotient_add_bench.txt")
args = ap.parse_args()

q = args.quotient
gen = torch.Generator(device="cuda").manual_seed(24)
n = int(args.load * (1 << q))
extra = 1 << args.max_log2
assert n + extra < (1 << q), "the largest batch must leave an empty slot"
hashes = torch.unique(torch.randint(-(2**31), 2**31, (n + extra + (n + extra) // 64,), dtype=torch.int64, device="cuda", generator=gen))
hashes = hashes[torch.randperm(hashes.numel(), device="cuda", generator=gen)][: n + extra].to(torch.int32)  # int32 bit patterns of distinct 32-bit hashes
held, fresh = hashes[:n], hashes[n:]

qf = pa.QuotientFilter(quotient=q, auto_expand=False)
qf.add_alt_many(held)
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


rows = []
lines = [f"QuotientFilter.add_alt_many, q = {q}, load {args.load} ({n} hashes held), {torch.cuda.get_device_name(0)}; median of {args.reps} calls, end to end",
         f"{'m':>9} {'m/held':>8} {'local ms':>10} {'rebuild ms':>11} {'rebuild/local':>14} {'local M hashes/s':>17}"]
for lg in range(args.min_log2, args.max_log2 + 1):
    m = 1 << lg
    batch = fresh[:m].clone()
    t = {}
    for policy in ("local", "rebuild"):
        qf._add_policy = policy

        def call():
            qf.add_alt_many(batch)
            assert qf.elements_held == n + m

        t[policy] = median_time(call, args.reps)
    if args.verify:  # faster and different is not faster: both paths must leave the same table
        left = {}
        for policy in ("local", "rebuild"):
            qf._add_policy = policy
            restore()
            qf.add_alt_many(batch)
            left[policy] = tuple(x.clone() for x in (qf._filter, qf._occ, qf._cont, qf._sh))
        assert all(torch.equal(a, b) for a, b in zip(left["local"], left["rebuild"])), f"the two paths differ at m = {m}"
    rows.append({"m": m, "local_s": t["local"], "rebuild_s": t["rebuild"]})
    lines.append(f"{m:>9} {m / n:>8.4f} {t['local'] * 1e3:>10.3f} {t['rebuild'] * 1e3:>11.3f} {t['rebuild'] / t['local']:>14.2f} {m / t['local'] / 1e6:>17.1f}")
    print(lines[-1], flush=True)

wins = [r["m"] for r in rows if r["local_s"] < r["rebuild_s"]]
lines.append(f"local is the faster path for m in {{{', '.join(str(m) for m in wins)}}}" if wins else "rebuild is the faster path at every m measured")
args.out.parent.mkdir(parents=True, exist_ok=True)
with args.out.open("a" if args.append else "w") as f:
    f.write("\n".join(lines) + "\n\n")
print(json.dumps({"bench": "quotient_add", "device": torch.cuda.get_device_name(0), "q": q, "load": args.load, "held": n, "reps": args.reps, "rows": rows}))
