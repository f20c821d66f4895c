"""Developer measurement: the basis step (lcty_basis.hip, lcty_basis_search.cpp) on synthetic alleles.
   python3 scripts/basis_probe.py ALLELES BASE_LEN [-x 0.01] [-w 250] [-s 0] [--repeats 2] [--no-walk] [--batch-words N]
One JSON line: per call of lcty_basis_build (the first carries module loading and the first allocations) the milliseconds of the
windows, dedup and subsume stages and of the host search as lcty_basis_stats reports them (wall time per stage with the stream drained
at its end), the rows raw -> unique -> minimal, the same with the presolve off (minimal = 0: the search on the unique rows), and the
reference's algorithm as the comparison point: the serial walk of cigar.rs:660-751 over the same entries in 16 host threads
(scripts/basis_probe_walk.cpp, g++ -O3), whose row table must equal the device's. Kernel times proper: run this under
`rocprofv3 --kernel-trace --stats -- python3 scripts/basis_probe.py ...`."""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def walk_lib():
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "basis_probe_walk.cpp")
    out = os.path.join(tempfile.mkdtemp(prefix="basis_probe_"), "libbasis_probe_walk.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-pthread", src, "-o", out], check=True)
    L = C.CDLL(out)
    L.basis_probe_walk.restype = C.c_double
    L.basis_probe_walk.argtypes = [C.c_uint64] + [C.c_void_p] * 8 + [C.c_uint32] * 4 + [C.c_double, C.c_uint32, C.c_void_p]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("alleles", type=int)
    ap.add_argument("base_len", type=int)
    ap.add_argument("-x", "--divergence", type=float, default=0.01)
    ap.add_argument("-w", "--window", type=int, default=250)
    ap.add_argument("-s", "--step", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--no-walk", action="store_true")
    ap.add_argument("--batch-words", type=int, default=0)
    ap.add_argument("--node-limit", type=int, default=2000000)
    a = ap.parse_args()
    from locityper_amd import api, synth
    t0 = time.perf_counter()
    L = synth.SynthLocus(a.alleles, 16, base_len=a.base_len)
    lens = np.diff(L.seq_off.astype(np.int64)).astype(np.uint32)
    ents = L.hap_alns()
    out = {"alleles": a.alleles, "base_len": a.base_len, "divergence": a.divergence, "window": a.window, "step": a.step,
           "entries": len(ents), "cigar_words": int(sum(len(e[2]) for e in ents)), "make_input_s": time.perf_counter() - t0,
           "build": [], "build_without_presolve": []}
    ctx = api.Context(0)
    if a.batch_words:
        ctx.set_knob("basis_batch_words", a.batch_words)
    for minimal, key in ((1, "build"), (0, "build_without_presolve")):
        p = api.basis_params(divergence=a.divergence, window=a.window, step=a.step, minimal=minimal, node_limit=a.node_limit)
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            ids, bound, optimal, st = api.basis_build(ctx, lens, ents, p)
            st.update(wall_ms=1e3 * (time.perf_counter() - t0), basis=len(ids), bound=bound, optimal=optimal)
            out[key].append(st)
    if not a.no_walk:
        p = api.basis_params(divergence=a.divergence, window=a.window, step=a.step)
        win_off, rows, st = api.basis_windows(ctx, lens, ents, p)
        n, id1, id2, nm, ln, off, words = api._basis_entries(ents)
        step = a.step or max(a.window >> 1, 1)
        nw = rows.shape[1]
        bits = np.zeros_like(rows)
        for c in range(a.alleles):
            bits[int(win_off[c]):int(win_off[c + 1]), c >> 5] = 1 << (c & 31)
        ms = walk_lib().basis_probe_walk(n, id1.ctypes.data, id2.ctypes.data, nm.ctypes.data, ln.ctypes.data, off.ctypes.data, words.ctypes.data,
                                         lens.ctypes.data, win_off.ctypes.data, nw, a.window, step, int(math.floor(a.window * a.divergence)),
                                         a.divergence, 16, bits.ctypes.data)
        out["walk_16_threads_ms"] = ms
        out["walk_equals_device"] = bool(np.array_equal(bits, rows))
        out["device_windows_call_ms"] = st["total_ms"]          # the whole call: upload, kernel, download of the row table
        out["device_windows_stage_ms"] = st["windows_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
