"""A plain bench.py run (no --full) is the lean headline measurement: exactly --steps timed steps, no side measurements, no detail
file.  --dump-outputs writes what the last timed step computed; the same arguments give the same files, and they hold what the
plain-C oracle computes for the same seeded keys."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
HEAD = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _plain(args, tmp_path, tag):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    detail = tmp_path / f"detail_{tag}.json"
    env = dict(os.environ, PSK_BENCH_DETAIL=str(detail))
    env.pop("WORLD_SIZE", None)
    out = tmp_path / tag
    run = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args, "--dump-outputs", str(out)], capture_output=True, text=True,
                         timeout=600, env=env, cwd=str(ROOT))
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert not detail.exists()  # the detail file is a --full product
    return line, {f.stem: np.load(f) for f in sorted(out.glob("*.npy"))}


def test_plain_cfg2_run_dumps_the_oracles_answers(tmp_path):
    n = 1_000_000
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--spinup", "0", "--keys-per-rank", str(n)]
    line, out = _plain(args, tmp_path, "a")
    assert all(line[k] is not None for k in HEAD) and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["steps"] == 3 and line["warmup"] == 1 and line["repeats"] == 1 and line["rc"] == 0
    assert "configs" not in line and line["cpu_baseline"] is None and line["detail_file"] is None
    assert set(out) == {"check", "table"}
    assert out["check"].dtype == np.float32 and out["table"].dtype == np.float64
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    assert out["check"].size == n and (out["check"] == 1.0).all()  # every inserted key is found

    sys.path.insert(0, str(ROOT / "oracle"))
    import oracle

    import bench

    ob = oracle.OracleBloom(2**28, 7)
    ob.add_keys(oracle.gen_keys16(0, n))
    words = ob.bloom.view("<u4")
    pos = bench.sample_positions(words.size, "table")
    assert out["table"].size == pos.size and np.array_equal(out["table"], words[pos].astype(np.float64))

    line2, out2 = _plain(args, tmp_path, "b")  # same arguments, same outputs
    assert line2["steps"] == 3
    assert all(np.array_equal(out[k], out2[k]) for k in out)


@pytest.mark.parametrize("cfg,extra,kind", [("cfg3", ["--keys-per-rank", "1000000"], np.float64), ("cfg4", ["--batch", "200000", "--batches", "6"], np.float64)])
def test_plain_runs_of_the_other_configs_dump_their_tables(tmp_path, cfg, extra, kind):
    line, out = _plain(["--config", cfg, "--steps", "2", "--warmup", "1", "--spinup", "0", *extra], tmp_path, cfg)
    assert line["steps"] == 2 and line["repeats"] == 1 and line["value"] > 0 and "cpu_baseline" in line and line["cpu_baseline"] is None
    assert set(out) == {"table"} and out["table"].dtype == kind and out["table"].nbytes <= 64 << 20
    assert out["table"].min() >= 0 and out["table"].sum() > 0
