#!/usr/bin/env python3
"""BloomFilterBank.score_many -- "how many of this query's keys may each filter hold?" -- against the only way the bank offered before
(the per-key mask of match_many, unpacked and segment-summed in torch) and against the floor (match_many's count form: the same gather, no
per-filter output).

The geometry of scripts/bench_bank_match.py: `--filters` filters of (10000, 0.01) (m = 95 851 bits, k = 7), each holding `--per-filter` keys,
16-byte device keys; 2^20 probe keys, each present in one filter.

(1) `score_many` of the 2^20 keys as 1024 queries of 1024, as 2^14 queries of 64 and as ONE query of 2^20 (the split path), and the threshold
    form at fraction 0.5 over the 1024 queries.
(2) baseline (i): `match_many(form="mask")` + unpack of the mask bits + per-query sum, in chunks of `--chunk-queries` queries of 1024 keys so
    that it fits memory; its peak device memory beyond the bank is reported.  The sums are compared with (1)'s.
(3) baseline (ii): `match_many(form="count")` of the same 2^20 keys.

Every call is timed end to end as a user makes it, around a device synchronise: warm-up, then the median of `--reps` (>= 7) calls.  Each part
runs in a child process of its own under a time limit (`--limit` seconds), and the first part that fails or runs out of time ends the script.
The tables go to `--out`, one JSON line to stdout."""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--filters", type=int, default=4096)
ap.add_argument("--per-filter", type=int, default=10000)
ap.add_argument("--chunk-queries", type=int, default=16)
ap.add_argument("--limit", type=int, default=240)
ap.add_argument("--part", choices=["score", "mask", "count"], default=None)
ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "bank_score_bench.txt")
args = ap.parse_args()
assert args.reps >= 7

EST, FPR, NQ = 10000, 0.01, 1 << 20
F, per = args.filters, args.per_filter


def part(name):
    """one measured part, in this (child) process -> a dict"""
    import torch

    import pyprobables_amd as pa

    gen = torch.Generator(device="cuda").manual_seed(31)
    keys = torch.randint(0, 256, (F * per, 16), dtype=torch.uint8, device="cuda", generator=gen)
    bank = pa.BloomFilterBank(F, EST, FPR)
    bank.add_many(keys, filter_offsets=torch.arange(F + 1, device="cuda", dtype=torch.int64) * per, validate=False)
    pick = (torch.arange(NQ, device="cuda") % F) * per + torch.randint(0, per, (NQ,), device="cuda", generator=gen)
    probes = keys[pick].contiguous()
    del keys
    bank.refresh_slices()
    torch.cuda.synchronize()

    def median_time(fn, warm=2):
        ts = []
        for r in range(warm + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warm:
                ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    def offsets(queries):
        return torch.arange(queries + 1, device="cuda", dtype=torch.int64) * (NQ // queries)

    res = {"device": torch.cuda.get_device_name(0), "m": bank.number_bits, "k": bank.number_hashes, "cus": bank._cus}
    if name == "score":
        for queries in (1024, 1 << 14, 1):
            o = offsets(queries)
            res[f"score_{queries}_s"] = median_time(lambda: bank.score_many(probes, o, validate=False))
            res[f"split_{queries}"] = bank.score_split_for(queries)
        o = offsets(1024)
        res["threshold_1024_s"] = median_time(lambda: bank.score_many(probes, o, threshold=0.5, validate=False))
        s = bank.score_many(probes, o, validate=False)
        res["selected_per_query"] = float((s >= 512).sum(dim=1).float().mean().item())
        res["checksum_1024"] = int(s.to(torch.int64).sum().item())
        res["checksum_1"] = int(bank.score_many(probes, offsets(1), validate=False).to(torch.int64).sum().item())
    elif name == "mask":
        cq = args.chunk_queries
        shifts = torch.arange(32, device="cuda", dtype=torch.int32)

        def baseline():
            out = torch.empty((1024, F), dtype=torch.int32, device="cuda")
            for q0 in range(0, 1024, cq):
                mask = bank.match_many(probes[q0 * 1024:(q0 + cq) * 1024])
                bits = ((mask.view(cq * 1024, -1, 1) >> shifts) & 1).view(cq * 1024, -1)[:, :F]
                out[q0:q0 + cq] = bits.view(cq, 1024, F).sum(dim=1, dtype=torch.int32)
            return out

        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res["checksum_1024"] = int(baseline().to(torch.int64).sum().item())
        res["peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
        res["mask_1024_s"] = median_time(baseline)
        res["chunk_queries"] = cq
    else:
        res["count_s"] = median_time(lambda: bank.match_many(probes, form="count"))
    return res


if args.part:
    print(json.dumps(part(args.part)), flush=True)
    sys.exit(0)

got = {}
for name in ("score", "mask", "count"):
    cmd = [sys.executable, __file__, "--part", name, "--reps", str(args.reps), "--filters", str(F), "--per-filter", str(per), "--chunk-queries", str(args.chunk_queries)]
    try:
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired:
        sys.exit(f"part {name} ran beyond {args.limit} s: stopping")
    if run.returncode != 0:
        sys.exit(f"part {name} failed with status {run.returncode}: stopping\n{run.stderr[-2000:]}")
    got[name] = json.loads(run.stdout.strip().splitlines()[-1])

sc, mk, ct = got["score"], got["mask"], got["count"]
assert sc["checksum_1024"] == mk["checksum_1024"] == sc["checksum_1"], "score_many and the mask baseline disagree"
t = sc["score_1024_s"]
lines = [f"BloomFilterBank.score_many, {F} filters of ({EST}, {FPR}) holding {per} keys each: m = {sc['m']}, k = {sc['k']}; 2^20 present 16-byte device keys; "
         f"{sc['device']} ({sc['cus']} CUs); median of {args.reps} calls, end to end", "",
         "(1) score_many, image current",
         f"    {'queries':>8} {'keys each':>10} {'split':>6} {'ms':>10} {'M keys/s':>10}"]
for queries in (1024, 1 << 14, 1):
    s = sc[f"score_{queries}_s"]
    lines.append(f"    {queries:>8} {NQ // queries:>10} {sc[f'split_{queries}']:>6} {s * 1e3:>10.3f} {NQ / s / 1e6:>10.2f}")
lines += [f"    threshold form, fraction 0.5, 1024 queries: {sc['threshold_1024_s'] * 1e3:.3f} ms ({sc['selected_per_query']:.2f} filters selected per query)", "",
          f"(2) baseline (i): match_many(form=\"mask\") + unpack + per-query sum, {mk['chunk_queries']} queries of 1024 keys a chunk, 1024 queries",
          f"    {mk['mask_1024_s'] * 1e3:>10.3f} ms   peak device memory beyond the bank and the probes {mk['peak_bytes'] / 1e6:.1f} MB   "
          f"= {mk['mask_1024_s'] / t:.2f} x score_many's time" + ("" if t < mk["mask_1024_s"] else "   (score_many does NOT beat this baseline)"),
          "    the sums of both ways compared: equal", "",
          "(3) baseline (ii), the floor: match_many(form=\"count\") of the same 2^20 keys",
          f"    {ct['count_s'] * 1e3:>10.3f} ms   score_many (1024 queries) takes {t / ct['count_s']:.2f} x that"]
args.out.parent.mkdir(parents=True, exist_ok=True)
args.out.write_text("\n".join(lines) + "\n")
print("\n".join(lines), flush=True)
print(json.dumps({"bench": "bank_score", "filters": F, "reps": args.reps, **got}))
