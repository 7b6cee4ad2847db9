"""The batch descriptor of the output tail (csrc/ragged.hip.h) on the CPU: tools/ragged_hostcheck.hip compares Items::len_in / len_out /
from, n_out, marks_end and ResamplePlan::n_out with a 128-bit restatement over units x hop x rate x cap.  The functions are __host__
__device__, so the program needs no GPU; it is built here as a plain stand-alone program and run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_ragged_hostcheck(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "ragged_hostcheck")
    flags = ["-Wall", "-Werror", "-Wno-unused-function", "-Wno-unused-result", "-Wno-unused-value"]  # the library's own, and no warning passes
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", *flags, os.path.join(ROOT, "tools", "ragged_hostcheck.hip"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    last = run.stdout.strip().splitlines()[-1]
    assert last.startswith("ragged_hostcheck: ") and last.endswith(", 0 failed"), last
    assert int(last.split()[1]) > 1000  # (the grid was walked)
