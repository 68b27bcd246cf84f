"""CPU: the host code behind the entry points of the orbital family (argument checks, limits, the refusal of aliased arrays, the state layout, the tile
arithmetic that sizes the grids) under AddressSanitizer and UndefinedBehaviorSanitizer.  For each csrc/orb*.hip below a stand-alone program with its own
``main`` (tests/host/<name>_host_check.hip, on the shared tests/host/host_check.h) is compiled together with it, the host side instrumented, and run as a child
process: nothing is loaded into Python and no device is touched.  Sanitizer runs belong on hosts without a GPU: skipped where a device is visible.
csrc/orbsmear.hip has a module of its own (tests/test_orbsmear_host_cpu.py), which also reads the values its program prints."""
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["orbbond", "orbcomm", "orbdens", "orbfrontier", "orblowdin", "orbpurify", "orbsqrt"])
def test_host_code_of_the_entry_points_is_clean_under_the_sanitizers(name, tmp_path):
    if torch.cuda.is_available():
        pytest.skip("host-only check: a device is visible")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / f"{name}_host_check")
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "host", f"{name}_host_check.hip"), os.path.join(ROOT, "nabladft_amd", "csrc", f"{name}.hip"),
           "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0 and f"{name}_host_check: ok" in run.stdout, run.stdout
