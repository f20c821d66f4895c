"""Developer measurement: the locus-database build (lcty_db.hip) on synthetic alleles.
   python3 scripts/db_probe.py ALLELES LENGTH [--count-k 25] [--no-merge] [--chunk-cols N]
One JSON line: per-stage milliseconds of lcty_db_divergences (minimizers, LDS sort, host sort, column index, bit matrix + Gram
tiles, host) and of lcty_db_off_target as lcty_db_stats reports them (wall time per stage with the stream drained at its end), bytes
moved, and the reference's algorithm as the comparison point: the two-pointer merge of minim_div.rs:16-40 over all pairs in 16 host
threads (scripts/db_probe_merge.cpp, g++ -O3), whose result must equal the device's. Kernel times proper: run this under
`rocprofv3 --kernel-trace --stats -- python3 scripts/db_probe.py ...`."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def merge_lib():
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "db_probe_merge.cpp")
    out = os.path.join(tempfile.mkdtemp(prefix="db_probe_"), "libdb_probe_merge.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-pthread", src, "-o", out], check=True)
    L = C.CDLL(out)
    L.db_probe_merge.restype = C.c_double
    L.db_probe_merge.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("alleles", type=int)
    ap.add_argument("length", type=int)
    ap.add_argument("--count-k", type=int, default=25)
    ap.add_argument("--no-merge", action="store_true")
    ap.add_argument("--chunk-cols", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    from locityper_amd import api, synth
    L = synth.SynthLocus(a.alleles, 16, base_len=a.length, seed=5, k=a.count_k)
    ctx = api.Context(0)
    if a.chunk_cols:
        ctx.set_knob("db_chunk_cols", a.chunk_cols)
    out = {"alleles": a.alleles, "length": a.length, "div_k": 15, "div_w": 15, "count_k": a.count_k, "divergences": [], "off_target": []}
    for _ in range(a.repeats):                              # the first repeat carries module loading and the first allocations
        t0 = time.perf_counter()
        uniq, _, chk, st = api.db_divergences(ctx, L.seqs, L.seq_off, 15, 15, with_f64=False)
        st["wall_ms"] = 1e3 * (time.perf_counter() - t0)
        out["divergences"].append(st)
    out["check"] = chk
    ref = L.allele(0)
    rc = np.ones(len(ref) + 1 - a.count_k, dtype=np.uint16)
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        _, warn, st = api.db_off_target(ctx, L.seqs, L.seq_off, L.counts, L.cnt_off, a.count_k, 2, np.frombuffer(ref, dtype=np.uint8), rc)
        st["wall_ms"] = 1e3 * (time.perf_counter() - t0)
        out["off_target"].append({k: v for k, v in st.items() if k in ("offt_ms", "host_ms", "total_ms", "wall_ms", "bytes_h2d", "bytes_d2h")})
    if not a.no_merge:
        moff, hashes, _ = api.db_minimizers(ctx, L.seqs, L.seq_off, 15, 15)
        M = merge_lib()
        ref_uniq = np.zeros(len(uniq), dtype=np.uint32)
        ms = M.db_probe_merge(a.alleles, moff.ctypes.data, hashes.ctypes.data, 16, ref_uniq.ctypes.data)
        best = min(out["divergences"][1:] or out["divergences"], key=lambda s: s["total_ms"])
        dev = best["total_ms"]
        out["merge_16_threads_ms"] = ms
        out["merge_equals_device"] = bool(np.array_equal(ref_uniq, uniq))
        out["device_divergence_stage_ms"] = dev            # the whole call: upload, minimizers, sorts, index, tiles, download, host division
        out["device_over_merge"] = dev / ms
    print(json.dumps(out))


if __name__ == "__main__":
    main()
