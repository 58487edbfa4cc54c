#!/usr/bin/env python3
"""Rates of CuckooFilter on 16-byte device keys, one GPU, median of `--reps` runs, each timed around a device synchronise:

  * check_many with present / absent / mixed keys, and remove_many, on a table that fits the cache (2^16 x 4 slots, 1 MiB) and one that
    does not (2^25 x 4 slots, 512 MiB), both filled to `--fill` of their slots;
  * add_many of a fresh filter up to its first kick (the parallel placement alone: claims sort, sweeps, scatter);
  * add_many of a fresh filter through loads 0.5 and 0.9 (both insert paths taking turns), as keys/s and as kicked keys/s, and the
    sequential kernel alone on the same keys, whose time per step sizes SEQ_BUDGET.

One JSON line at the end."""
import argparse
import json
import random
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
ap.add_argument("--fill", type=float, default=0.25)
ap.add_argument("--probes", type=int, default=1 << 22)
ap.add_argument("--lookup-capacities", type=int, nargs="+", default=[1 << 16, 1 << 25])
ap.add_argument("--insert-capacity", type=int, default=1 << 17)
args = ap.parse_args()


def timed(fn, setup=None, reps=args.reps, warm=1):
    ts = []
    for r in range(warm + reps):
        state = setup() if setup else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(state)
        torch.cuda.synchronize()
        if r >= warm:
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


rows = []
for cap in args.lookup_capacities:
    n = int(args.fill * cap * 4)
    keys = gen_keys(n)
    cf = pa.CuckooFilter(capacity=cap, auto_expand=False)
    cf.add_many(keys)
    p = min(args.probes, n)
    present, absent = keys[:p], gen_keys(p, start=1 << 40)
    mixed = torch.cat([present[: p // 2], absent[: p - p // 2]])[torch.randperm(p, device=keys.device)]
    fst = cf.last_insert_stats
    row = {"what": "lookup", "capacity": cap, "bucket_size": 4, "table_MiB": cap * 16 / 2**20, "keys": n, "probes": p, "kicked_while_filling": fst.get("kicked_keys", 0),
           "fill_sequential_steps": fst.get("sequential_steps", 0), "fill_sequential_seconds": fst.get("sequential_seconds", 0.0)}
    if row["fill_sequential_steps"]:
        row["fill_ns_per_step"] = row["fill_sequential_seconds"] * 1e9 / row["fill_sequential_steps"]
        print(f"capacity {cap} x 4: filling ran {row['fill_sequential_steps']} sequential steps in {row['fill_sequential_seconds'] * 1e3:.1f} ms = "
              f"{row['fill_ns_per_step']:.0f} ns per step", flush=True)
    for name, batch in (("present", present), ("absent", absent), ("mixed", mixed)):
        row[f"check_{name}_per_s"] = p / timed(lambda _: cf.check_many(batch))
        row[f"hits_{name}"] = float(cf.check_many(batch).float().mean().item())
    saved = (cf.buckets_tensor.clone(), cf.fill_tensor.clone(), cf.elements_added)

    def restore():
        cf.buckets_tensor.copy_(saved[0])
        cf.fill_tensor.copy_(saved[1])
        cf._elements_added = saved[2]

    row["remove_per_s"] = p / timed(lambda _: cf.remove_many(present), setup=restore)
    rows.append(row)
    print(f"capacity {cap} x 4 ({row['table_MiB']:.0f} MiB), {n} keys: check present {row['check_present_per_s'] / 1e9:.2f} absent {row['check_absent_per_s'] / 1e9:.2f} "
          f"(hits {row['hits_absent']:.5f}) mixed {row['check_mixed_per_s'] / 1e9:.2f} G keys/s; remove {row['remove_per_s'] / 1e9:.3f} G keys/s", flush=True)
    del keys, present, absent, mixed, cf, saved
    torch.cuda.empty_cache()

cap = args.insert_capacity
slots = cap * 4
keys = gen_keys(slots)


def fresh():
    random.seed(1)
    return pa.CuckooFilter(capacity=cap, auto_expand=False)


probe = fresh()
probe._insert_policy = "parallel"
probe.add_many(keys[: slots // 2])
first_kick = probe.elements_added if not probe.last_insert_stats.get("kicked_keys") else None
if first_kick is None:  # the first parallel pass ends at the first kick: ask it alone
    probe = fresh()
    first_kick = probe._place(probe._triples(keys[: slots // 2]))
t = timed(lambda cf: cf.add_many(keys[:first_kick]), setup=fresh)
rows.append({"what": "add_to_first_kick", "capacity": cap, "bucket_size": 4, "keys": first_kick, "load": first_kick / slots, "keys_per_s": first_kick / t})
print(f"capacity {cap} x 4: add_many up to the first kick (key {first_kick}, load {first_kick / slots:.3f}): {first_kick / t / 1e6:.1f} M keys/s", flush=True)

for load in (0.5, 0.9):
    n = int(load * slots)
    for policy in ("auto", "sequential"):
        def setup():
            cf = fresh()
            cf._insert_policy = policy
            return cf

        holder = {}

        def run(cf):
            cf.add_many(keys[:n])
            holder["stats"] = dict(cf.last_insert_stats)

        t = timed(run, setup=setup)
        st = holder["stats"]
        rows.append({"what": "add_through_load", "policy": policy, "capacity": cap, "bucket_size": 4, "load": load, "keys": n, "seconds": t, "keys_per_s": n / t,
                     "kicked_keys": st.get("kicked_keys", 0), "kicked_keys_per_s": st.get("kicked_keys", 0) / t, "parallel_keys": st.get("parallel_keys", 0),
                     "sequential_keys": st.get("sequential_keys", 0), "sequential_steps": st.get("sequential_steps", 0),
                     "sequential_seconds": st.get("sequential_seconds", 0.0),
                     "ns_per_step": st.get("sequential_seconds", 0.0) * 1e9 / max(st.get("sequential_steps", 0), 1)})
        print(f"capacity {cap} x 4: add_many through load {load} ({policy}): {n} keys in {t * 1e3:.1f} ms = {n / t / 1e6:.2f} M keys/s; {st.get('kicked_keys', 0)} kicked "
              f"keys = {st.get('kicked_keys', 0) / t / 1e3:.1f} k kicked keys/s; parallel {st.get('parallel_keys', 0)}, sequential {st.get('sequential_keys', 0)}: {st.get('sequential_steps', 0)} steps of "
              f"{rows[-1]['ns_per_step']:.0f} ns in the sequential kernel", flush=True)

print(json.dumps({"bench": "cuckoo", "device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}))
