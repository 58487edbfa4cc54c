#!/usr/bin/env python3
"""Rate of the exact ordered CountingBloomFilter batches (add_many_ordered / update_many_ordered -> psk_cbf_add_running /
psk_cbf_update_running) on 16-byte keys, 2^20 ops per call, device batches, into

  * the README's geometry: est_elements = 28 005 615, fpr 0.01 -> 2^28 counters (1 GiB), k = 7;
  * a small table: est_elements = 100 000, fpr 0.01 -> ~10^6 counters, k = 7;

over distinct keys and over a skewed stream (a few very hot keys), beside update_ordered -- the one-lane kernel that was the only exact
per-op path before -- on a prefix of the same streams, as a rate per op.

The signed stream is well formed: its first half adds, its second half removes the same keys in the same order, so a call leaves the
table as it found it and the parallel passes serve every chunk (the script checks "cbf_running_replayed_chunks").  One window times
`--calls` calls around a device synchronise, after a warm-up of the same shape; the median of `--reps` windows is reported.  Before
anything is timed the two paths are compared value for value on the prefix.  One JSON line at the end."""
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
from pyprobables_amd import _native as N  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--calls", type=int, default=8)
ap.add_argument("--ops", type=int, default=1 << 20)
ap.add_argument("--prefix", type=int, default=1 << 15)
args = ap.parse_args()

n, half = args.ops, args.ops // 2
GEOMETRIES = (("2^28 counters (README)", 28_005_615), ("~10^6 counters", 100_000))


def skewed(count, pool_keys):
    """x^3 / R^2 over a pool of R distinct keys: a few very hot keys, a long tail"""
    R = pool_keys.shape[0]
    g = torch.Generator(device=pool_keys.device)
    g.manual_seed(0x5EED)
    x = torch.randint(0, R, (count,), device=pool_keys.device, generator=g, dtype=torch.int64)
    return pool_keys[(x * x * x) // (R * R)]


def window(fn, calls, reps, warm=1):
    ts = []
    for r in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        if r >= warm:
            ts.append((time.perf_counter() - t0) / calls)
    return statistics.median(ts), min(ts), max(ts)


out = {"ops": n, "calls_per_window": args.calls, "reps": args.reps, "device": torch.cuda.get_device_name(0)}


def report(label, count, t):
    med, lo, hi = t
    print(f"{label:74s} n={count:>8d}  {med * 1e3:10.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f})  {count / med / 1e6:10.3f} M ops/s", flush=True)
    out[f"{label} n={count}"] = {"ms": med * 1e3, "min_ms": lo * 1e3, "max_ms": hi * 1e3, "mops": count / med / 1e6}
    return count / med


distinct = gen_keys(half)
hot = skewed(half, gen_keys(1 << 18, start=1 << 30))
signs = torch.cat([torch.ones(half, dtype=torch.int32, device="cuda"), -torch.ones(n - half, dtype=torch.int32, device="cuda")])

for gname, est in GEOMETRIES:
    cbf = pa.CountingBloomFilter(est_elements=est, false_positive_rate=0.01, device=0)
    twin = pa.CountingBloomFilter(est_elements=est, false_positive_rate=0.01, device=0)
    print(f"--- {gname}: m = {cbf.number_bits}, k = {cbf.number_hashes}", flush=True)
    for sname, base in (("distinct keys", distinct), ("skewed keys", hot)):
        keys = torch.cat([base, base[: n - half]])  # the second half revisits the first: every remove finds its add
        # the same values on both paths, on the prefix (adds, then removes of the same keys)
        p = args.prefix
        pk = torch.cat([base[: p // 2], base[: p - p // 2]])
        pw = torch.cat([signs[: p // 2], signs[half: half + p - p // 2]])
        hk, hw = pk.cpu().numpy(), pw.cpu().numpy().astype("int64")
        cbf.clear()
        twin.clear()
        same = bool((cbf.update_many_ordered(pk, pw).cpu().numpy().view("uint32") == twin.update_ordered(hk, hw)).all())
        same = same and bool((cbf._tab.read() == twin._tab.read()).all())
        out[f"{gname}, {sname}: results and table equal on the prefix"] = same
        print(f"{sname}: update_many_ordered == update_ordered on {p} ops (results and table): {same}", flush=True)
        assert same
        cbf.clear()
        opts0 = [N.get_option(o) for o in ("cbf_running_fast_chunks", "cbf_running_replayed_chunks")]
        r_add = report(f"{gname}: add_many_ordered, {sname}", n, window(lambda: cbf.add_many_ordered(keys), args.calls, args.reps))
        cbf.clear()
        r_upd = report(f"{gname}: update_many_ordered, half removes, {sname}", n, window(lambda: cbf.update_many_ordered(keys, signs), args.calls, args.reps))
        fast, replayed = (N.get_option(o) - o0 for o, o0 in zip(("cbf_running_fast_chunks", "cbf_running_replayed_chunks"), opts0))
        print(f"    chunks served by the parallel passes: {fast}, replayed in order: {replayed}", flush=True)
        assert replayed == 0 and fast == 2 * (1 + args.reps) * args.calls
        twin.clear()
        twin.update_ordered(hk[:1000], hw[:1000])
        twin.clear()
        r_seq = report(f"{gname}: update_ordered (one-lane kernel), {sname}", p, window(lambda: twin.update_ordered(hk, hw), 1, 3, warm=1))
        out[f"{gname}, {sname}: update_many_ordered over update_ordered, per op"] = r_upd / r_seq
        out[f"{gname}, {sname}: add_many_ordered over update_ordered, per op"] = r_add / r_seq
        print(f"    per op, update_many_ordered runs {r_upd / r_seq:.1f} x and add_many_ordered {r_add / r_seq:.1f} x the rate of update_ordered", flush=True)
    del cbf, twin
print(json.dumps(out))
