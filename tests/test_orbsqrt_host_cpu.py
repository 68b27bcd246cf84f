"""CPU: the host code behind the nq_orb_sqrt_* entry points (argument checks, the iteration limits, the refusal of aliased arrays, the tile arithmetic that sizes the grids) under
AddressSanitizer and UndefinedBehaviorSanitizer.  A stand-alone program with its own ``main`` (tests/host/orbsqrt_host_check.hip) is compiled together with
csrc/orbsqrt.hip, the host side instrumented, and run as a child process: nothing is loaded into Python and no device is touched.  Sanitizer runs belong on
hosts without a GPU: skipped where a device is visible, like tests/test_orblowdin_host_cpu.py."""
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_code_of_the_square_root_entry_points_is_clean_under_the_sanitizers(tmp_path):
    if torch.cuda.is_available():
        pytest.skip("host-only check: a device is visible")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "orbsqrt_host_check")
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "host", "orbsqrt_host_check.hip"), os.path.join(ROOT, "nabladft_amd", "csrc", "orbsqrt.hip"),
           "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0 and "orbsqrt_host_check: ok" in run.stdout, run.stdout
