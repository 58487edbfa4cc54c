#!/usr/bin/env python3
"""Rate of the exact ordered CountMinSketch batch add (add_many_ordered -> psk_cms_add_running) on 16-byte keys into 2^20 x 5:

  * add_many_ordered, 2^20 and 10^7 keys (device batches, unit weights, distinct keys and the skewed stream);
  * update_ordered -- the sequential one-lane kernel that was the only exact per-op path before -- on the same 2^20 keys;
  * the unordered add_many, for context (it returns nothing);
  * StreamThreshold.add_many end to end, the host's dict work included, on the skewed stream.

Warm-up first, then the median of `--reps` runs, each timed around a device synchronise.  `--trace`: a few ordered adds only, for a
kernel-trace profiler run of its own.  One JSON line at the end.

`--signed`: the signed batches alone (update_many_ordered -> psk_cms_update_running), 2^20 ops into 2^20 x 5 with unit weights, half of
them removes, over uniform keys and over one hot key; add_many_ordered on the same keys beside them; update_ordered (the one-lane kernel)
over a prefix of 2^16 ops of the same signed streams, as a rate, and the ratio of the rates."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from _common import gen_keys  # noqa: E402
import torch  # noqa: E402

import pyprobables_amd as pa  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--trace", action="store_true")
ap.add_argument("--signed", action="store_true")
args = ap.parse_args()

WIDTH, DEPTH = 1 << 20, 5
SIZES = [1 << 20, 10_000_000]


def skewed(n, pool_keys):
    """x^3 / R^2 over a pool of R distinct keys: a few very hot keys, a long tail"""
    R = pool_keys.shape[0]
    g = torch.Generator(device=pool_keys.device)
    g.manual_seed(0x5EED)
    x = torch.randint(0, R, (n,), device=pool_keys.device, generator=g, dtype=torch.int64)
    return pool_keys[(x * x * x) // (R * R)]


def median_time(fn, reps, warm=2, before=None):
    ts = []
    for r in range(warm + reps):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warm:
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


distinct = gen_keys(SIZES[-1])
hot = skewed(SIZES[-1], gen_keys(1 << 18, start=1 << 30))
cms = pa.CountMinSketch(width=WIDTH, depth=DEPTH, device=0)

if args.trace:
    for n in SIZES:
        for _ in range(3):
            cms.clear()
            cms.add_many_ordered(distinct[:n])
    cms.add_many_ordered(hot)
    torch.cuda.synchronize()
    sys.exit(0)

out = {"width": WIDTH, "depth": DEPTH, "reps": args.reps, "device": torch.cuda.get_device_name(0)}


def report(label, n, t):
    med, lo, hi = t
    print(f"{label:46s} n={n:>9d}  {med * 1e3:10.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f})  {n / med / 1e6:10.1f} M ops/s", flush=True)
    out[f"{label} n={n}"] = {"ms": med * 1e3, "min_ms": lo * 1e3, "max_ms": hi * 1e3, "mops": n / med / 1e6}
    return med


if args.signed:
    n, prefix = SIZES[0], 1 << 16
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5EED)
    signs = torch.randint(0, 2, (n,), device="cuda", generator=g, dtype=torch.int32) * 2 - 1  # +1 / -1, half of each
    streams = (("uniform keys", distinct[:n]), ("one hot key", distinct[:1].expand(n, -1).contiguous()))
    for name, keys in streams:
        t_add = report(f"add_many_ordered, {name}", n, median_time(lambda: cms.add_many_ordered(keys), args.reps, before=cms.clear))
        t_upd = report(f"update_many_ordered, half removes, {name}", n, median_time(lambda: cms.update_many_ordered(keys, signs), args.reps, before=cms.clear))
        hk, hw = keys[:prefix].cpu().numpy(), signs[:prefix].cpu().numpy().astype("int64")
        cms.clear()
        cms.update_ordered(hk[:1000], hw[:1000])
        t_seq = report(f"update_ordered (one-lane kernel), {name}", prefix, median_time(lambda: cms.update_ordered(hk, hw), 2, warm=0, before=cms.clear))
        ratio = (n / t_upd) / (prefix / t_seq)
        out[f"ratio_update_many_ordered_over_update_ordered, {name}"] = ratio
        out[f"ratio_update_many_ordered_over_add_many_ordered, {name}"] = t_add / t_upd
        print(f"{name}: update_many_ordered runs {ratio:.1f} x the rate of update_ordered, {t_add / t_upd:.2f} x the rate of add_many_ordered", flush=True)
    print(json.dumps(out))
    sys.exit(0)

for n in SIZES:
    for label, keys in (("add_many_ordered distinct", distinct[:n]), ("add_many_ordered skewed", hot[:n])):
        t_ord = report(label, n, median_time(lambda: cms.add_many_ordered(keys), args.reps, before=cms.clear))
        if n == SIZES[0] and label.endswith("distinct"):
            t_fast = t_ord
    report("add_many (unordered, no results)", n, median_time(lambda: cms.add_many(distinct[:n]), args.reps, before=cms.clear))
    st = pa.StreamThreshold(threshold=1000, width=WIDTH, depth=DEPTH, device=0)
    report("StreamThreshold.add_many skewed, end to end", n, median_time(lambda: st.add_many(hot[:n]), args.reps, before=st.clear))
    out[f"meets_threshold n={n}"] = len(st.meets_threshold)

# the sequential kernel: host batches only, seconds per run -- one warm-up at a small size, then two timed runs
n = SIZES[0]
host = distinct[:n].cpu().numpy()
cms.clear()
cms.update_ordered(host[:1000], 1)
t_seq = report("update_ordered (sequential kernel)", n, median_time(lambda: cms.update_ordered(host, 1), 2, warm=0, before=cms.clear))
t_host = report("add_many_ordered distinct, host batch", n, median_time(lambda: cms.add_many_ordered(host), args.reps, before=cms.clear))
out["ratio_update_ordered_over_add_many_ordered_2^20"] = t_seq / t_fast
out["ratio_host_batches_2^20"] = t_seq / t_host
print(f"update_ordered / add_many_ordered at 2^20 keys: {t_seq / t_fast:.1f} x (device batch), {t_seq / t_host:.1f} x (host batch both)")
print(json.dumps(out))
