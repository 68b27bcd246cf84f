"""CPU: the host code behind the entry points of csrc/orbocc.hip (``nq_orb_occ_factor`` / ``nq_orb_occ_reduce`` / ``nq_orb_occ_back``: argument checks, the
refusal of aliased arrays and of reduced dimensions that do not fit the batch, the tile arithmetic that sizes the grids) under AddressSanitizer and
UndefinedBehaviorSanitizer, built the way tests/test_orb_host_cpu.py builds its siblings: the stand-alone program tests/host/orbocc_host_check.hip (its own
``main``, on the shared tests/host/host_check.h) is compiled together with the source, the host side instrumented, and run as a child process: nothing is
loaded into Python and no device is touched.  Sanitizer runs belong on hosts without a GPU: skipped where a device is visible."""
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_code_of_the_occupied_entry_points_is_clean_under_the_sanitizers(tmp_path):
    if torch.cuda.is_available():
        pytest.skip("host-only check: a device is visible")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "orbocc_host_check")
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "host", "orbocc_host_check.hip"), os.path.join(ROOT, "nabladft_amd", "csrc", "orbocc.hip"),
           "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0 and "orbocc_host_check: ok" in run.stdout, run.stdout
