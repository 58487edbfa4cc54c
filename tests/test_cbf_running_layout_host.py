"""The chunk and scratch arithmetic of the ordered CountingBloomFilter batches (csrc/psk_cbf_running_layout.hpp) as host code of its own:
tests/host/cbf_running_layout_main.cpp is compiled with AddressSanitizer and UndefinedBehaviorSanitizer on the host side and run on the CPU
(k = 1 .. 64, n = 0, 1, 2^20 + 1 ..., every pass count).  No GPU, no Python under a sanitizer: the program has its own main."""

import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_layout_arithmetic_under_the_host_sanitizers(tmp_path):
    from pyprobables_amd import build as B

    exe = tmp_path / "cbf_running_layout_check"
    src = ROOT / "tests" / "host" / "cbf_running_layout_main.cpp"
    cmd = [B.hipcc(), "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           str(src), "-o", str(exe)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert run.stdout.strip().endswith("0 failures")
