#!/usr/bin/env python3
"""A locus from a pangenome VCF on the device, stage by stage:
   python3 scripts/panvcf_probe.py H V L [--rate 0.02] [--boundary 200000] [--repeats 2] [--no-host] [--out profiles/panvcf_probe_H_V_L.json]

Makes a seeded case of H haplotype columns, V records over a reference of L bases (tests/panvcf_cases.py), runs
lcty_panvcf_reconstruct --repeats times and prints, for the last (warm) call, the milliseconds of the row reduction, the chain, the
scans with the segment lists, the gather and the compaction (the stream is drained after each stage); then one lcty_db_find_boundary
over --boundary positions with a record every 300 bases. Beside them the same serial loops in ONE host thread
(scripts/panvcf_probe_host.cpp), whose outputs — every sequence, unknown_nts, the overlaps; every weight to the bit, the position —
must equal the device's. One JSON line; --out also writes it to a file."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from locityper_amd import api  # noqa: E402
from tests import panvcf_cases as PC  # noqa: E402


def host_lib():
    here = os.path.dirname(os.path.abspath(__file__))
    out = os.path.join(tempfile.mkdtemp(prefix="panvcf_probe_"), "libpanvcf_probe_host.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(here, "panvcf_probe_host.cpp"), "-o", out], check=True)
    L = C.CDLL(out)
    L.panvcf_probe_host_reconstruct.restype = C.c_double
    L.panvcf_probe_host_reconstruct.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] + [C.c_uint32] + [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_void_p,
                                                                                                                         C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.panvcf_probe_host_boundary.restype = C.c_double
    L.panvcf_probe_host_boundary.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                             C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("haplotypes", type=int)
    ap.add_argument("records", type=int)
    ap.add_argument("length", type=int)
    ap.add_argument("--rate", type=float, default=0.02)
    ap.add_argument("--boundary", type=int, default=200_000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    H, V, L = a.haplotypes, a.records, a.length
    s, e, ref, records, gt = PC.make_case(1, L, V, H, a.rate, missing_rate=0.001)
    flat = PC.flat(records)
    refa = np.frombuffer(ref, dtype=np.uint8)
    names = [f"h{c}" for c in range(H)]
    ctx = api.Context(0)
    for _ in range(max(a.repeats, 1)):
        t0 = time.perf_counter()
        res = api.panvcf_reconstruct(ctx, "chr1", s, e, refa, flat, gt, names, 1.0, True)
        wall = (time.perf_counter() - t0) * 1e3
    st = res["stats"]
    out = {"haplotypes": H, "records": V, "ref_len": L, "rate": a.rate, "kept_records": res["n_kept_records"], "segments": st["n_segments"],
           "out_bytes": st["out_bytes"], "overlaps": res["total_overlaps"], "upload_ms": st["upload_ms"], "rows_ms": st["rows_ms"], "chain_ms": st["chain_ms"],
           "scan_ms": st["scan_ms"], "gather_ms": st["gather_ms"], "compact_download_ms": st["compact_ms"], "total_ms": st["total_ms"], "python_call_ms": wall}
    lib = None if a.no_host else host_lib()
    if lib:
        cap = int(res["seq_off"][-1])
        seqs = np.zeros(max(cap, 1), dtype=np.uint8); off = np.zeros(H + 1, dtype=np.uint64); unk = np.zeros(H, dtype=np.uint32); ov = C.c_uint64()
        ms = lib.panvcf_probe_host_reconstruct(s, e, refa.ctypes.data, V, flat["pos"].ctypes.data, flat["ref_len"].ctypes.data, flat["rec_allele"].ctypes.data,
                                               flat["allele_off"].ctypes.data, flat["allele_bytes"].ctypes.data, H, gt.ctypes.data, seqs.ctypes.data, cap,
                                               off.ctypes.data, unk.ctypes.data, C.byref(ov))
        out["host_1_thread_walk_ms"] = ms
        out["host_equal_device"] = bool(ms >= 0 and np.array_equal(off, res["seq_off"]) and np.array_equal(seqs[:cap], res["seqs"])
                                        and np.array_equal(unk, res["col_unknown"]) and ov.value == res["total_overlaps"])
        out["device_stages_over_host"] = (st["rows_ms"] + st["chain_ms"] + st["scan_ms"] + st["gather_ms"]) / ms if ms > 0 else None
    # the boundary search
    n, k, mw = a.boundary, 25, 500
    rng = np.random.default_rng(2)
    counts = rng.choice(np.array([0, 1, 1, 2, 7], dtype=np.uint16), n + mw - k)
    pos = np.sort(rng.integers(1_000_000 - 10, 1_000_000 + n + 10, max(n // 300, 1))).astype(np.uint32)
    rlen = rng.integers(1, 40, len(pos)).astype(np.uint32)
    for left in (True, False):
        for _ in range(max(a.repeats, 1)):
            t0 = time.perf_counter()
            at, w = api.db_find_boundary(ctx, 1_000_000, 1_000_000 + n, pos, rlen, k, counts, n, mw, left)
            ms_dev = (time.perf_counter() - t0) * 1e3
        side = "left" if left else "right"
        out[f"boundary_{side}_call_ms"] = ms_dev
        if lib:
            hw = np.zeros(n, dtype=np.float64); found, hat = C.c_int32(), C.c_uint32()
            ms = lib.panvcf_probe_host_boundary(1_000_000, 1_000_000 + n, len(pos), pos.ctypes.data, rlen.ctypes.data, k, counts.ctypes.data, len(counts), n, mw,
                                                int(left), hw.ctypes.data, C.byref(found), C.byref(hat))
            out[f"boundary_{side}_host_1_thread_ms"] = ms
            out[f"boundary_{side}_host_equal_device"] = bool(hw.tobytes() == w.tobytes() and (at if at is not None else -1) == (hat.value if found.value else -1))
    out["boundary_positions"], out["boundary_records"] = n, len(pos)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
