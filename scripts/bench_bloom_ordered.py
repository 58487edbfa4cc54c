#!/usr/bin/env python3
"""Rate of the exact ordered BloomFilter batch (add_many_ordered -> psk_bloom_add_running) on 16-byte device keys into the README's
table (est_elements = 28 005 615, fpr 0.01 -> 2^28 bits, k = 7), for streams of 2^20 and 10^7 keys and three mixes:

  * all new       distinct keys into an empty table;
  * half repeats  the second half of the stream revisits the first, into an empty table;
  * all present   the table already holds every key of the stream.

The yardstick, in the same process on the same streams: ExpandingBloomFilter.add_many on a filter of the same geometry that does not
grow (est_elements exceeds the stream) -- the route that computed the same flags before (bit indices to memory, a Python chunk loop,
psk_idx_resolve_ordered_hashed + psk_idx_insert): the same table work, its flags thrown away.

One run = one call around a device synchronise; a deferred clear is made to land before the clock starts.  Median, min and max of
`--reps` runs after one warm-up; before anything is timed the two routes' tables are compared byte for byte.  The lines go to stdout
and to `--out` (default profiles/bloom_ordered_bench.txt), one JSON line at the end."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from _common import gen_keys  # noqa: E402
import torch  # noqa: E402

import pyprobables_amd as pa  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--sizes", type=int, nargs="*", default=[1 << 20, 10_000_000])
ap.add_argument("--out", default=str(ROOT / "profiles" / "bloom_ordered_bench.txt"))
args = ap.parse_args()

EST, FPR = 28_005_615, 0.01
lines = []
out = {"reps": args.reps, "device": torch.cuda.get_device_name(0)}


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(prepare, fn, reps):
    ts = []
    for r in range(1 + reps):
        prepare()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r:
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def report(label, n, t):
    med, lo, hi = t
    say(f"{label:62s} n={n:>9d}  {med * 1e3:9.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f})  {n / med / 1e6:9.2f} M keys/s")
    out[f"{label} n={n}"] = {"ms": med * 1e3, "min_ms": lo * 1e3, "max_ms": hi * 1e3, "mkeys": n / med / 1e6}
    return med


blm = pa.BloomFilter(EST, FPR, device=0)
ebf = pa.ExpandingBloomFilter(est_elements=EST, false_positive_rate=FPR, device=0)
say(f"# python scripts/bench_bloom_ordered.py   ({out['device']}; m = {blm.number_bits}, k = {blm.number_hashes}; one call per run, median of {args.reps} runs)")
one = gen_keys(1, start=1 << 40)


def empty_blm():
    blm.clear()
    blm.check_many(one)  # (the deferred clear lands here, not inside the clock)


def empty_ebf():
    assert ebf.expansions == 0, "the yardstick must not grow"
    ebf._blooms[0].clear()
    ebf._added_elements = 0
    ebf._blooms[0].check_many(one)


for n in args.sizes:
    distinct = gen_keys(n)
    half = torch.cat([distinct[: n // 2], distinct[: n - n // 2]])
    # the same table from both routes, and the flags of the half-repeats stream
    empty_blm()
    empty_ebf()
    seen = blm.add_many_ordered(half)
    ebf.add_many(half)
    same = bytes(blm)[:-20] == bytes(ebf._blooms[0])[:-20]
    repeats_seen = bool(seen[n // 2:].all().item())
    say(f"n = {n}: tables equal byte for byte: {same}; every revisit reported seen: {repeats_seen}; first halves reported new: {int((~seen[: n // 2]).sum().item())} of {n // 2}")
    out[f"n={n}: tables equal"] = same
    assert same and repeats_seen
    for mix, keys, prep_b, prep_e in (
        ("all new", distinct, empty_blm, empty_ebf),
        ("half repeats", half, empty_blm, empty_ebf),
        ("all present", distinct, None, None),
    ):
        if prep_b is None:  # the table holds the stream already and stays as it is: nothing to prepare between runs
            empty_blm()
            empty_ebf()
            blm.add_many(distinct)
            ebf.add_many(distinct)
            prep_b = prep_e = lambda: None
        t_new = report(f"add_many_ordered, {mix}", n, timed(prep_b, lambda: blm.add_many_ordered(keys), args.reps))
        t_old = report(f"ExpandingBloomFilter.add_many (yardstick), {mix}", n, timed(prep_e, lambda: ebf.add_many(keys), args.reps))
        say(f"    add_many_ordered takes {t_new / t_old:.3f} x the yardstick's time ({mix}, n = {n})")
        out[f"ratio new/yardstick, {mix}, n={n}"] = t_new / t_old
    del distinct, half
say(json.dumps(out))
Path(args.out).parent.mkdir(parents=True, exist_ok=True)
Path(args.out).write_text("\n".join(lines) + "\n")
