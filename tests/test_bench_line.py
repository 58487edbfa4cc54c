"""The driver reads bench.py's LAST stdout line out of an ~8 KB tail (BENCH_r05.json could not be parsed: the line had grown to 23 KB).
compact_line() must turn the full result object into a line well under that cap, with the contract's fields intact.  CPU only: the full
objects are the committed round-5 lines under profiles/."""

import json
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
            "roofline", "cpu_baseline")


@pytest.mark.parametrize("name,cfg", [("r05_bench_cfg2_default", "cfg2"), ("r05_bench_cfg2_forced_dist_1rank", "cfg2"), ("r05_bench_cfg3", "cfg3"),
                                      ("r05_bench_cfg4", "cfg4"), ("r05_bench_cfg5", "cfg5")])
def test_compact_line_fits_and_keeps_the_contract(name, cfg):
    import bench

    full = json.loads((ROOT / "profiles" / f"{name}.json").read_text().strip().splitlines()[-1])
    line = bench.compact_line(full, cfg, "gpurun_out/bench_detail.json")
    text = json.dumps(line, separators=(",", ":"))
    assert len(text) < bench.LINE_LIMIT < 8000
    back = json.loads(text)
    assert all(k in back for k in CONTRACT)
    assert back["value"] == pytest.approx(full["value"], rel=1e-5) and back["ms_per_step"] == pytest.approx(full["ms_per_step"], rel=1e-5)
    rf = back["roofline"]
    assert set(rf) >= {"bound", "kernel", "achieved", "peak", "unit", "frac", "traffic"} and len(rf["kernel"]) <= 80
    assert rf["frac"] == pytest.approx(full["roofline"]["frac"], rel=1e-5) and rf["frac"] == pytest.approx(rf["achieved"] / rf["peak"], rel=1e-4)
    assert "workload" in back["config"] and "model" not in back["config"]
    if full.get("cpu_baseline"):
        assert set(back["cpu_baseline"]) >= {"value", "unit", "cores", "kind", "sample"}
    if full.get("configs"):
        assert set(back["configs"]) == set(full["configs"])


def test_an_oversized_object_still_fits():
    import bench

    full = json.loads((ROOT / "profiles" / "r05_bench_cfg2_default.json").read_text().strip().splitlines()[-1])
    full["rooflines"] = {f"op{i}": dict(full["rooflines"]["cms_add"]) for i in range(200)}
    assert len(json.dumps(bench.compact_line(full, "cfg2", None), separators=(",", ":"))) < bench.LINE_LIMIT


def test_the_round_6_detail_object_keeps_the_per_key_latencies_on_the_line():
    """the FULL object of a default run (profiles/r06_bench_cfg2_default_detail.json, as bench.py wrote it on the GPU box) -> the compact line:
    the per-key call latencies travel on it, rounded, and it still fits"""
    import bench

    full = json.loads((ROOT / "profiles" / "r06_bench_cfg2_default_detail.json").read_text())
    line = bench.compact_line(full, "cfg2", "gpurun_out/bench_detail.json")
    text = json.dumps(line, separators=(",", ":"))
    assert len(text) < bench.LINE_LIMIT
    pk = json.loads(text)["detail"]["per_key_call_us"]
    assert set(pk) == {"bloom_check", "cms_add", "cms_check", "cbf_add", "cbf_check"} and all(0 < v < 100 for v in pk.values())


def test_a_plain_run_is_lean_by_default(monkeypatch):
    """without --full the run times exactly --steps steps once and measures nothing else; --full and --dump-outputs are options"""
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert args.steps == 7 and args.warmup == 2 and not args.full and args.dump_outputs is None and (args.repeats or 1) == 1
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    args = bench.parse()
    assert args.full and args.dump_outputs == "out"


def test_dump_outputs_writes_exact_seeded_samples(tmp_path):
    """--dump-outputs: float32 answers, float64 words (read unsigned or signed), a fixed sample of large outputs read across chunks"""
    torch = pytest.importorskip("torch")
    import numpy as np

    import bench

    g = torch.Generator().manual_seed(1)
    words = [torch.randint(-2**31, 2**31 - 1, (3 << 20,), dtype=torch.int32, generator=g), torch.arange(-5, 5, dtype=torch.int32)]
    hits = [torch.rand(1000, generator=g) > 0.5]
    got = bench.dump_outputs(torch, {"table": (words, "u32"), "check": (hits, "bool"), "small": (words[1:], "i32")}, tmp_path / "a")
    bench.dump_outputs(torch, {"table": (words, "u32")}, tmp_path / "b")
    table, check, small = (np.load(tmp_path / "a" / f"{k}.npy") for k in ("table", "check", "small"))
    assert table.dtype == np.float64 and check.dtype == np.float32 and small.dtype == np.float64
    pos = bench.sample_positions((3 << 20) + 10, "table")
    assert got["table"] == pos.size <= bench.DUMP_SAMPLE and np.all(np.diff(pos) > 0)
    flat = np.concatenate([w.numpy() for w in words]).view(np.uint32)
    assert np.array_equal(table, flat[pos].astype(np.float64)) and np.array_equal(table, np.load(tmp_path / "b" / "table.npy"))
    assert np.array_equal(check, hits[0].numpy().astype(np.float32)) and np.array_equal(small, np.arange(-5, 5, dtype=np.float64))
