"""CPU: the host code behind the nq_orb_front_* entry points (argument checks, the limits of k_max and tol, the refusal of aliased arrays and of a second output
without its input, the arithmetic that sizes the grids) under AddressSanitizer and UndefinedBehaviorSanitizer.  A stand-alone program with its own ``main``
(tests/host/orbfrontier_host_check.hip) is compiled together with csrc/orbfrontier.hip, the host side instrumented, and run as a child process: nothing is
loaded into Python and no device is touched.  Sanitizer runs belong on hosts without a GPU: skipped where a device is visible, like
tests/test_orbpurify_host_cpu.py."""
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_code_of_the_frontier_entry_points_is_clean_under_the_sanitizers(tmp_path):
    if torch.cuda.is_available():
        pytest.skip("host-only check: a device is visible")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "orbfrontier_host_check")
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "host", "orbfrontier_host_check.hip"),
           os.path.join(ROOT, "nabladft_amd", "csrc", "orbfrontier.hip"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0 and "orbfrontier_host_check: ok" in run.stdout, run.stdout
