#!/usr/bin/env python3
"""Pruning (locityper prune) on the device, stage by stage:
   python3 scripts/prune_probe.py N [--families F] [--threshold 0.0002] [--repeats 2] [--no-host] [--out profiles/prune_probe_N.json]

Builds the triangle of N haplotypes from a synthetic family tree (F families; divergences grow with the depth of the last common
ancestor, a small distinct jitter on every pair), runs lcty_prune_cluster --repeats times and prints, for the last (warm) call, the
milliseconds of the matrix build, the merge loop and the representatives kernel (the stream is drained after each stage). Beside it the
same algorithm in ONE host thread (scripts/prune_probe_host.cpp: same tie rule, same caches), whose steps must equal the device's.
One JSON line; --out also writes it to a file."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from locityper_amd import api, cdefs  # noqa: E402


def family_triangle(n, families, seed=1):
    """dv-like values: haplotypes are leaves of a random binary-ish tree per family; a pair's divergence is 2e-5 per level up to the last
    common ancestor inside a family, about 2e-2 across families, times a distinct jitter"""
    rng = np.random.default_rng(seed)
    fam = rng.integers(0, families, n)
    depth = 12
    path = rng.integers(0, 2, (n, depth))
    i, j = np.triu_indices(n, 1)                     # rows i, then j > i: the order of the triangle
    same = fam[i] == fam[j]
    diff = path[i] != path[j]
    first = np.where(diff.any(axis=1), diff.argmax(axis=1), depth)
    tri = np.where(same, 2e-5 * (depth - first) + 1e-6, 2e-2)
    return tri * (1.0 + 1e-3 * rng.random(len(tri)))


def host_lib():
    here = os.path.dirname(os.path.abspath(__file__))
    out = os.path.join(tempfile.mkdtemp(prefix="prune_probe_"), "libprune_probe_host.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", os.path.join(here, "prune_probe_host.cpp"), "-o", out], check=True)
    L = C.CDLL(out)
    L.prune_probe_host.restype = C.c_double
    L.prune_probe_host.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    return L


def host_steps(n, tri, lib=None):
    """(steps, merge ms, build ms) of the one-thread form"""
    t = np.ascontiguousarray(tri, dtype=np.float64)
    steps = np.zeros(max(n - 1, 1), dtype=cdefs.PRUNE_STEP_DTYPE)
    build = C.c_double()
    ms = (lib or host_lib()).prune_probe_host(n, t.ctypes.data, steps.ctypes.data, C.byref(build))
    return steps[:n - 1], ms, build.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int)
    ap.add_argument("--families", type=int, default=0, help="0 = n / 16")
    ap.add_argument("--threshold", type=float, default=0.0002)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    tri = family_triangle(a.n, a.families or max(a.n // 16, 1))
    ctx = api.Context(0)
    prm = api.prune_params(threshold=a.threshold)
    for _ in range(max(a.repeats, 1)):
        res = api.prune_cluster(ctx, a.n, tri, None, prm)
    st = res["stats"]
    out = {"n": a.n, "pairs": len(tri), "kept": len(res["keep_ids"]), "threshold": a.threshold,
           "build_ms": st["build_ms"], "merge_ms": st["merge_ms"], "repr_ms": st["repr_ms"], "host_side_ms": st["host_ms"], "total_ms": st["total_ms"],
           "rescans": st["n_rescans"], "rep_pairs": st["n_rep_pairs"], "matrix_bytes": st["matrix_bytes"]}
    if not a.no_host:
        hs, ms, build = host_steps(a.n, tri)
        out["host_1_thread_build_ms"], out["host_1_thread_merge_ms"] = build, ms
        out["host_steps_equal_device"] = bool(hs.tobytes() == res["steps"].tobytes())
        out["merge_device_over_host"] = st["merge_ms"] / ms if ms > 0 else None
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
