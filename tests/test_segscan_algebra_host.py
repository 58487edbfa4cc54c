"""The scan values of the ordered batches (RunSeg, RunMap, RunSum, RunMap64 of csrc/psk_running.hpp, CbfMap of csrc/psk_cbf_running.hpp) as
host code: tests/host/segscan_algebra_main.cpp is compiled with AddressSanitizer and UndefinedBehaviorSanitizer on the host side and run on
the CPU.  It checks the laws the scan skeleton (csrc/psk_segscan.hpp) relies on -- identity, associativity, with the rails in the set -- and
runs the three levels of the scan in plain C++ against the reference's loop, one op after the other.  No GPU, no Python under a sanitizer:
the program has its own main."""

import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_scan_algebra_under_the_host_sanitizers(tmp_path):
    from pyprobables_amd import build as B

    exe = tmp_path / "segscan_algebra_check"
    src = ROOT / "tests" / "host" / "segscan_algebra_main.cpp"
    cmd = [B.hipcc(), "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           str(src), "-o", str(exe)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert run.stdout.strip().endswith("0 failures")
