#!/usr/bin/env python3
"""Rates of CountingCuckooFilter on 16-byte device keys, bucket_size 4, one GPU, median of `--reps` runs, each timed around a device
synchronise:

  * check_many with present / absent / mixed keys on a table that fits the cache (2^16 x 4 slots, 2 MiB of pairs) and one that does not
    (2^25 x 4 slots, 1 GiB), both filled to `--fill` of their slots -- and CuckooFilter.check_many on the same keys and capacities in the
    same run, the yardstick: a row of pairs is twice as wide as a row of fingerprints;
  * remove_many of the present keys on both tables;
  * add_many of 2^22 keys over 2^16 distinct fingerprints that are all in the table: the sort plus the weighted add, no kicks;
  * add_many of a fresh filter through load 0.5.

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
ap.add_argument("--repeat-keys", type=int, default=1 << 22)
ap.add_argument("--repeat-distinct", type=int, default=1 << 16)
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
    p = min(args.probes, n)
    present, absent = keys[:p], gen_keys(p, start=1 << 40)
    mixed = torch.cat([present[: p // 2], absent[: p - p // 2]])[torch.randperm(p, device=keys.device)]
    row = {"what": "lookup", "capacity": cap, "bucket_size": 4, "keys": n, "probes": p}
    for label, cls, width in (("counting", pa.CountingCuckooFilter, 32), ("plain", pa.CuckooFilter, 16)):
        f = cls(capacity=cap, auto_expand=False)
        f.add_many(keys)
        row[f"{label}_table_MiB"] = cap * width / 2**20
        for name, batch in (("present", present), ("absent", absent), ("mixed", mixed)):
            row[f"{label}_check_{name}_per_s"] = p / timed(lambda _: f.check_many(batch))
        if label == "counting":
            row["hits_absent"] = float((f.check_many(absent) != 0).float().mean().item())
            saved = (f.bins_tensor.clone(), f.fill_tensor.clone(), f.elements_added, f.unique_elements)

            def restore():
                f.bins_tensor.copy_(saved[0])
                f.fill_tensor.copy_(saved[1])
                f._elements_added, f._unique_elements = saved[2], saved[3]

            row["remove_per_s"] = p / timed(lambda _: f.remove_many(present), setup=restore)
            del saved
        del f
        torch.cuda.empty_cache()
    row["present_vs_plain"] = row["counting_check_present_per_s"] / row["plain_check_present_per_s"]
    rows.append(row)
    print(f"capacity {cap} x 4, {n} keys, check_many G keys/s present / absent / mixed: counting ({row['counting_table_MiB']:.0f} MiB) "
          f"{row['counting_check_present_per_s'] / 1e9:.2f} / {row['counting_check_absent_per_s'] / 1e9:.2f} / {row['counting_check_mixed_per_s'] / 1e9:.2f}; "
          f"CuckooFilter ({row['plain_table_MiB']:.0f} MiB) {row['plain_check_present_per_s'] / 1e9:.2f} / {row['plain_check_absent_per_s'] / 1e9:.2f} / "
          f"{row['plain_check_mixed_per_s'] / 1e9:.2f}; present-key ratio {row['present_vs_plain']:.2f}; remove_many {row['remove_per_s'] / 1e9:.3f} G keys/s", flush=True)
    del keys, present, absent, mixed
    torch.cuda.empty_cache()

cap = args.insert_capacity
slots = cap * 4

# repeats only: every key of the batch is in the table already
distinct = gen_keys(args.repeat_distinct)
batch = distinct[torch.randint(0, args.repeat_distinct, (args.repeat_keys,), device=distinct.device)]
cf = pa.CountingCuckooFilter(capacity=cap, auto_expand=False)
cf.add_many(distinct)
t = timed(lambda _: cf.add_many(batch))
rows.append({"what": "add_repeats", "capacity": cap, "bucket_size": 4, "keys": args.repeat_keys, "distinct": args.repeat_distinct, "seconds": t,
             "keys_per_s": args.repeat_keys / t})
print(f"capacity {cap} x 4: add_many of {args.repeat_keys} keys over {args.repeat_distinct} fingerprints in the table: {t * 1e3:.2f} ms = "
      f"{args.repeat_keys / t / 1e9:.3f} G keys/s", flush=True)
del cf, batch, distinct

keys = gen_keys(slots // 2)


def fresh():
    random.seed(1)
    return pa.CountingCuckooFilter(capacity=cap, auto_expand=False)


holder = {}


def run(f):
    f.add_many(keys)
    holder["stats"] = dict(f.last_insert_stats)


t = timed(run, setup=fresh)
st = holder["stats"]
rows.append({"what": "add_through_load", "capacity": cap, "bucket_size": 4, "load": 0.5, "keys": slots // 2, "seconds": t, "keys_per_s": slots // 2 / t,
             "kicked_keys": st.get("kicked_keys", 0), "parallel_keys": st.get("parallel_keys", 0), "sequential_keys": st.get("sequential_keys", 0),
             "sequential_steps": st.get("sequential_steps", 0)})
print(f"capacity {cap} x 4: add_many of a fresh filter through load 0.5: {slots // 2} keys in {t * 1e3:.1f} ms = {slots // 2 / t / 1e6:.2f} M keys/s; "
      f"{st.get('kicked_keys', 0)} kicked keys, parallel {st.get('parallel_keys', 0)}, sequential {st.get('sequential_keys', 0)}", flush=True)

print(json.dumps({"bench": "counting_cuckoo", "device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}))
