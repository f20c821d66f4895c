"""The host-only plumbing of the C interface (locityper_amd/csrc/lcty_host.hpp: check_haps, split_names, sized, Handoff) without a
device: tests/native/host_harness.cpp is built by g++ with the address and undefined-behaviour sanitizers into tests/native/_build/ and
run as a program of its own. It ends with a non-zero status at the first expectation that does not hold and at any sanitizer report
(a leaked block, a double free, a read past a buffer)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_harness():
    out = os.path.join(ROOT, "tests", "native", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "host_harness")
    src = os.path.join(ROOT, "tests", "native", "host_harness.cpp")
    # the sanitizers' runtimes are linked into the program itself: it runs the same whatever else the process environment loads
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-Wall", "-Wextra", "-o", exe, src])
    r = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "checks passed" in r.stdout
