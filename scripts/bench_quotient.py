#!/usr/bin/env python3
"""Build and lookup rates of QuotientFilter on 16-byte device keys, q = 24 and q = 28, loads 0.5 and 0.85:

  * build: add_many into an empty filter end to end (hash, sort + unique, place), and the placing alone (psk_qf_build on the sorted
    distinct hashes);
  * lookup: check_many of 2^24 keys that are all present, all absent (up to hash collisions: the hit fraction is printed), and half / half.

`load` is keys / slots; 32-bit hashes of that many keys collide, so the distinct count (printed) is a little lower.  Warm-up first, then
the median of `--reps` runs, each timed around a device synchronise.  One JSON line at the end."""
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
ap.add_argument("--quotients", type=int, nargs="+", default=[24, 28])
ap.add_argument("--loads", type=float, nargs="+", default=[0.5, 0.85])
ap.add_argument("--probes", type=int, default=1 << 24)
args = ap.parse_args()


def median_time(fn, reps, warm=1):
    ts = []
    for r in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warm:
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


rows = []
for q in args.quotients:
    for load in args.loads:
        n = int(load * (1 << q))
        keys = gen_keys(n)
        qf = pa.QuotientFilter(quotient=q, auto_expand=False)

        def build():
            qf._set_params(q)  # an empty table again
            qf.add_many(keys)

        t_build = median_time(build, args.reps)
        hs = qf._decode()[0]
        t_place = median_time(lambda: qf._build(hs), args.reps)
        p = min(args.probes, n)
        present = keys[:p]
        absent = gen_keys(p, start=1 << 40)
        mixed = torch.cat([present[: p // 2], absent[: p - p // 2]])[torch.randperm(p, device=keys.device)]
        row = {"q": q, "load": load, "keys": n, "distinct": qf.elements_added, "build_keys_per_s": n / t_build,
               "place_hashes_per_s": qf.elements_added / t_place, "probes": p}
        for name, batch in (("present", present), ("absent", absent), ("mixed", mixed)):
            t = median_time(lambda: qf.check_many(batch), args.reps)
            row[f"lookup_{name}_per_s"] = p / t
            row[f"hits_{name}"] = float(qf.check_many(batch).float().mean().item())
        assert row["hits_present"] == 1.0
        rows.append(row)
        print(f"q={q} load={load}: {n} keys, {qf.elements_added} distinct; build {n / t_build / 1e9:.2f} G keys/s (placing alone "
              f"{qf.elements_added / t_place / 1e9:.2f} G hashes/s); lookup present {row['lookup_present_per_s'] / 1e9:.2f}, absent "
              f"{row['lookup_absent_per_s'] / 1e9:.2f} (hits {row['hits_absent']:.4f}), mixed {row['lookup_mixed_per_s'] / 1e9:.2f} G keys/s", flush=True)
        del keys, present, absent, mixed, qf, hs
        torch.cuda.empty_cache()

print(json.dumps({"bench": "quotient", "device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}))
