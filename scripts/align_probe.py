"""Developer measurement: the pairwise haplotype alignments (lcty_align.hip) on synthetic haplotypes.
   python3 scripts/align_probe.py ALLELES BASE_LEN [-D 0.01] [-k 25,51,101] [-g 10000] [--repeats 2] [--no-host] [--host-pairs N] [--batch-pairs N]
                                  [--tr-div 0.01 [--tr-anchor 101]] [--lib path]
One JSON line: per call of lcty_align_haplotypes over all pairs (the first call carries module loading and the first allocations) the
per-stage milliseconds of lcty_align_stats (wall time per stage with the stream drained at its end: divergences, k-mer index, matches,
chains, gap fill, best k + download), the counts of matches, chain points, stretches by route and DP cells, and as the comparison point
the same backbone route in 16 host threads (scripts/align_probe_host.cpp, g++ -O3; scores only) over the pairs the device aligned —
or over the first --host-pairs of them, the time then scaled to all — whose scores and best ks must equal the device's.
With --tr-div the calls are lcty_align_haplotypes_transitive (the stats gain rounds, accelerated pairs and the milliseconds of the plan,
walk, optimize and count stages) and the comparison point is the transitive route in host threads, round by round, whose scores, best
ks, routes, via and number of rounds must equal the device's.
Kernel times proper: run this under `rocprofv3 --kernel-trace --stats -- python3 scripts/align_probe.py ...`."""
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


def host_lib():
    here = os.path.dirname(os.path.abspath(__file__))
    src = os.path.join(here, "align_probe_host.cpp")
    out = os.path.join(tempfile.mkdtemp(prefix="align_probe_"), "libalign_probe_host.so")
    # lcty_gotoh.hpp, the library's own aligner primitives, compiled for the host
    subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-pthread", "-I", os.path.join(os.path.dirname(here), "locityper_amd", "csrc"), src,
                    "-o", out], check=True)
    L = C.CDLL(out)
    L.align_probe_host.restype = C.c_double
    L.align_probe_host.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                   C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    L.align_probe_host_transitive.restype = C.c_double
    L.align_probe_host_transitive.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                              C.c_double, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64),
                                              C.POINTER(C.c_double)]
    L.align_probe_stretch.restype = C.c_int32
    L.align_probe_stretch.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    return L


def host_stretch(ref, query, max_gap, lib=None):
    """(score, pushes as (operation code, length)) of smart_align on one stretch, walk back included: the host instantiation of lcty_gotoh.hpp"""
    r = np.frombuffer(bytes(ref), dtype=np.uint8); q = np.frombuffer(bytes(query), dtype=np.uint8)
    words = np.zeros(2 * (len(r) + len(q)) + 4, dtype=np.uint32)
    n = C.c_uint32(0)
    score = (lib or host_lib()).align_probe_stretch(r.ctypes.data, len(r), q.ctypes.data, len(q), max_gap, words.ctypes.data, len(words), C.byref(n))
    assert n.value <= len(words)
    return score, [(int(w) & 15, int(w) >> 4) for w in words[:n.value]]


def host_route(seqs, off, ref, query, ks, max_gap, threads=16):
    """(scores, best ks, ms of the pairs, ms of the k-mer lists) of the host-thread form"""
    seqs = np.ascontiguousarray(seqs, dtype=np.uint8); off = np.ascontiguousarray(off, dtype=np.uint64)
    ref = np.ascontiguousarray(ref, dtype=np.uint32); query = np.ascontiguousarray(query, dtype=np.uint32)
    kk = np.ascontiguousarray(ks, dtype=np.uint32)
    score = np.zeros(max(len(ref), 1), dtype=np.int32); best = np.zeros(max(len(ref), 1), dtype=np.uint32)
    index_ms = C.c_double(0)
    ms = host_lib().align_probe_host(len(off) - 1, seqs.ctypes.data, off.ctypes.data, len(ref), ref.ctypes.data, query.ctypes.data, len(kk), kk.ctypes.data,
                                     max_gap, threads, score.ctypes.data, best.ctypes.data, C.byref(index_ms))
    return score[:len(ref)], best[:len(ref)], ms, index_ms.value


def host_route_transitive(seqs, off, ref, query, aligned, ks, max_gap, tr_div, anchor, threads=16, lib=None):
    """the transitive route in host threads, round by round: dict of score, best_k, route, via, n_rounds, ms, index_ms. aligned: per
    pair 0 = skipped by its minimizer divergence (the host form does not compute divergences), or None"""
    seqs = np.ascontiguousarray(seqs, dtype=np.uint8); off = np.ascontiguousarray(off, dtype=np.uint64)
    ref = np.ascontiguousarray(ref, dtype=np.uint32); query = np.ascontiguousarray(query, dtype=np.uint32)
    ag = None if aligned is None else np.ascontiguousarray(aligned, dtype=np.uint8)
    kk = np.ascontiguousarray(ks, dtype=np.uint32)
    n = max(len(ref), 1)
    score = np.zeros(n, dtype=np.int32); best = np.zeros(n, dtype=np.uint32); route = np.zeros(n, dtype=np.uint8); via = np.zeros(n, dtype=np.uint32)
    rounds, index_ms = C.c_uint64(0), C.c_double(0)
    ms = (lib or host_lib()).align_probe_host_transitive(len(off) - 1, seqs.ctypes.data, off.ctypes.data, len(ref), ref.ctypes.data, query.ctypes.data,
                                                         None if ag is None else ag.ctypes.data, len(kk), kk.ctypes.data, max_gap, tr_div, anchor, threads,
                                                         score.ctypes.data, best.ctypes.data, route.ctypes.data, via.ctypes.data, C.byref(rounds),
                                                         C.byref(index_ms))
    m = len(ref)
    return {"score": score[:m], "best_k": best[:m], "route": route[:m], "via": via[:m], "n_rounds": rounds.value, "ms": ms, "index_ms": index_ms.value}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("alleles", type=int)
    ap.add_argument("base_len", type=int)
    ap.add_argument("-D", "--thresh-div", type=float, default=0.01)
    ap.add_argument("-k", "--backbone-ks", default="25,51,101")
    ap.add_argument("-g", "--max-gap", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-pairs", type=int, default=0)
    ap.add_argument("--batch-pairs", type=int, default=0)
    ap.add_argument("--tr-div", type=float, default=None, help="the transitive route (lcty_align_haplotypes_transitive) with this divergence")
    ap.add_argument("--tr-anchor", type=int, default=101)
    ap.add_argument("--lib", default=None, help="a library built by hand, such as the commit before a change, for a side-by-side run")
    a = ap.parse_args()
    from locityper_amd import _lib, api, synth
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    ks = [int(x) for x in a.backbone_ks.split(",")]
    t0 = time.perf_counter()
    L = synth.SynthLocus(a.alleles, 16, base_len=a.base_len)
    seqs, off = np.asarray(L.seqs, dtype=np.uint8), np.asarray(L.seq_off, dtype=np.uint64)
    ref, query = api.align_all_pairs(a.alleles)
    out = {"alleles": a.alleles, "base_len": a.base_len, "thresh_div": a.thresh_div, "backbone_ks": ks, "max_gap": a.max_gap, "pairs": len(ref),
           "make_input_s": time.perf_counter() - t0, "calls": []}
    ctx = api.Context(0)
    if a.batch_pairs:
        ctx.set_knob("align_batch_pairs", a.batch_pairs)
    p = api.align_params(thresh_div=a.thresh_div, backbone_ks=ks, max_gap=a.max_gap)
    res = None
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        if a.tr_div is None:
            res, st = api.align_haplotypes(ctx, seqs, off, ref, query, p)
        else:
            res, st = api.align_haplotypes_transitive(ctx, seqs, off, ref, query, p, api.align_tr_params(transitive_div=a.tr_div, transitive_anchor=a.tr_anchor))
        st["wall_ms"] = 1e3 * (time.perf_counter() - t0)
        out["calls"].append(st)
    out["cigar_words"] = int(len(res["cigar"]))
    if a.tr_div is not None:
        out["tr_div"], out["tr_anchor"] = a.tr_div, a.tr_anchor
        out["accelerated_share"] = out["calls"][-1]["n_accelerated"] / max(out["calls"][-1]["n_aligned"], 1)
    if not a.no_host and a.tr_div is not None:
        # the rounds depend on every pair before them: the host form runs all pairs (--host-pairs does not apply)
        h = host_route_transitive(seqs, off, ref, query, res["aligned"], ks, a.max_gap, a.tr_div, a.tr_anchor)
        out["host_16_threads_index_ms"], out["host_16_threads_ms"], out["host_rounds"] = h["index_ms"], h["ms"], h["n_rounds"]
        out["host_accelerated"] = int((h["route"] >= 2).sum())
        same = all(np.array_equal(h[k], res[k]) for k in ("score", "best_k", "route", "via")) and h["n_rounds"] == out["calls"][-1]["n_rounds"]
        out["host_scores_equal_device"] = bool(same)
        if not same:
            bad = np.flatnonzero((h["score"] != res["score"]) | (h["route"] != res["route"]) | (h["via"] != res["via"]) | (h["best_k"] != res["best_k"]))
            if len(bad):
                b = int(bad[0])
                out["first_difference"] = {"pair": [int(ref[b]), int(query[b])], "host": [int(h["score"][b]), int(h["route"][b]), int(h["via"][b])],
                                           "device": [int(res["score"][b]), int(res["route"][b]), int(res["via"][b])]}
    elif not a.no_host:
        took = np.flatnonzero(res["aligned"])
        n_all = len(took)
        if a.host_pairs and a.host_pairs < n_all:
            took = took[:a.host_pairs]
        score, best, ms, index_ms = host_route(seqs, off, ref[took], query[took], ks, a.max_gap)
        out["host_16_threads_pairs"] = int(len(took))
        out["host_16_threads_index_ms"] = index_ms
        out["host_16_threads_ms"] = ms
        out["host_16_threads_ms_scaled_to_all"] = ms * n_all / max(len(took), 1)
        out["host_scores_equal_device"] = bool(np.array_equal(score, res["score"][took]) and np.array_equal(best, res["best_k"][took]))
        if not out["host_scores_equal_device"]:
            bad = np.flatnonzero((score != res["score"][took]) | (best != res["best_k"][took]))
            out["first_difference"] = {"pair": [int(ref[took[bad[0]]]), int(query[took[bad[0]]])], "host": [int(score[bad[0]]), int(best[bad[0]])],
                                       "device": [int(res["score"][took[bad[0]]]), int(res["best_k"][took[bad[0]]])]}
    print(json.dumps(out))
    return 0 if out.get("host_scores_equal_device", True) else 1


if __name__ == "__main__":
    sys.exit(main())
