"""The device primitives of DESIGN.md 4.18 (wavefront and workgroup scans, the multi-workgroup scan and its total, the radix sort, the
LDS bitonic network) against plain host code: tests/native/prims_harness.hip is compiled with the library's flags together with
locityper_amd/csrc/lcty_sort.hip into tests/native/_build/ and run once; it prints the first mismatch of every failing case."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "locityper_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter"]


def build_harness():
    out = os.path.join(ROOT, "tests", "native", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "prims_harness")
    srcs = [os.path.join(ROOT, "tests", "native", "prims_harness.hip"), os.path.join(CSRC, "lcty_sort.hip")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("lcty_scan.hpp", "lcty_sort.hpp", "lcty_bitonic.hpp", "lcty_common.hpp", "lcty_device.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        r = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["-I" + CSRC] + srcs + ["-o", exe, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
        assert r.returncode == 0 and "warning" not in r.stderr, r.stdout + r.stderr
    return exe


@pytest.mark.gpu
def test_device_primitives_match_host_code():
    r = subprocess.run([build_harness()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith(" 0 failed"), r.stdout
