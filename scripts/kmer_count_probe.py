#!/usr/bin/env python3
"""Genome k-mer counts on the device, stage by stage:
   python3 scripts/kmer_count_probe.py GENOME_BASES QUERY_SEQS QUERY_LEN [-k 25] [--repeats 2] [--threads 16] [--no-host] [--diag [--form 1]]
                                       [--out profiles/kmer_count_probe_....json]

Makes a seeded synthetic genome of GENOME_BASES bases in contigs of 2^27 (scripts/kmer_count_probe_host.cpp: random bases, a planted
share of repeats — copies of one 4 kb unit and poly-A runs in 10 % of the 1 Mb blocks —, every fourth block soft-masked, 10 kb of N at
the start of every contig), loads it with lcty_genome_append (pack: the wall time of upload + pack kernel), cuts QUERY_SEQS sequences
of QUERY_LEN bases out of it (a part of them out of the repeats, so that many adds meet on few counters) and calls
lcty_genome_kmer_counts --repeats times. It prints, for the last (warm) call, the per-stage milliseconds of table / scan / gather from
the call's own events, genome positions per second of the scan, the hits, and the same loop in --threads host threads on the ASCII
genome; the two tables of values must be equal. --diag --form 1 takes the developer build and its scan without the merging of equal
consecutive hits. One JSON line with the hash of the library's sources; --out also writes it to a file."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from locityper_amd import _lib, api  # noqa: E402
from sources_sha import sources_sha16  # noqa: E402

CONTIG = 1 << 27


def host_lib():
    here = os.path.dirname(os.path.abspath(__file__))
    out = os.path.join(tempfile.mkdtemp(prefix="kmer_count_probe_"), "libkmer_count_probe_host.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-pthread", os.path.join(here, "kmer_count_probe_host.cpp"), "-o", out], check=True)
    L = C.CDLL(out)
    L.kmer_probe_make_genome.restype = None
    L.kmer_probe_make_genome.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]
    L.kmer_probe_host_counts.restype = C.c_int
    L.kmer_probe_host_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                         C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    return L


def cut_queries(genome, n_seqs, length, rng):
    """sequences of the genome itself (upper case, off the N runs), every fourth starting in a block of planted repeats if one is found"""
    out = []
    tries = 0
    while len(out) < n_seqs and tries < 100 * n_seqs + 1000:
        tries += 1
        at = int(rng.integers(0, len(genome) - length))
        s = genome[at:at + length]
        if len(out) % 4 == 3 and tries < 50 * n_seqs and not (s[:1024] == s[0]).all() and not np.array_equal(s[:2048], genome[at + 4096:at + 6144]):
            continue                                                      # wanted: a cut inside the repeats
        s = s & 0xDF
        if (s == ord("N")).any():
            continue
        out.append(s.tobytes())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("genome_bases", type=int)
    ap.add_argument("query_seqs", type=int)
    ap.add_argument("query_len", type=int)
    ap.add_argument("-k", type=int, default=25)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--diag", action="store_true")
    ap.add_argument("--form", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    threads = min(a.threads, 16)
    if a.diag:
        _lib.use_diag_build()
    H = host_lib()
    t0 = time.perf_counter()
    genome = np.empty(a.genome_bases, dtype=np.uint8)
    H.kmer_probe_make_genome(1, a.genome_bases, CONTIG, 10, threads, genome.ctypes.data)
    rng = np.random.default_rng(5)
    seqs = cut_queries(genome, a.query_seqs, a.query_len, rng)
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    flat = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    make_ms = (time.perf_counter() - t0) * 1e3

    ctx = api.Context(0)
    if a.diag:
        ctx.set_knob("genome_scan_form", a.form)
    contig_off = np.array(list(range(0, a.genome_bases, CONTIG)) + [a.genome_bases], dtype=np.uint64)
    t0 = time.perf_counter()
    g = api.Genome(ctx)
    for c in range(len(contig_off) - 1):
        g.append(f"contig{c}", genome[int(contig_off[c]):int(contig_off[c + 1])])
    pack_ms = (time.perf_counter() - t0) * 1e3
    for _ in range(max(a.repeats, 1)):
        counts, cnt_off, st = g.kmer_counts(flat, off, a.k, 2)
    res = {"probe": "kmer_count", "genome_bases": a.genome_bases, "contigs": len(contig_off) - 1, "query_seqs": len(seqs), "query_len": a.query_len,
           "k": a.k, "build": "diag" if a.diag else "product", "scan_form": a.form if a.diag else 0, "make_ms": round(make_ms, 1),
           "device": {"pack_ms": round(pack_ms, 1), **{n: (round(v, 3) if isinstance(v, float) else v) for n, v in st.items()},
                      "positions_per_s": round(st["n_scanned"] / (st["scan_ms"] * 1e-3)) if st["scan_ms"] > 0 else None}}
    if not a.no_host:
        hc = np.zeros(max(len(counts), 1), dtype=np.uint16)
        ms = np.zeros(3, dtype=np.float64)
        nd, nh = C.c_uint64(), C.c_uint64()
        H.kmer_probe_host_counts(genome.ctypes.data, contig_off.ctypes.data, len(contig_off) - 1, a.k, flat.ctypes.data, off.ctypes.data, len(seqs), threads,
                                 hc.ctypes.data, ms.ctypes.data, C.byref(nd), C.byref(nh))
        equal = bool(np.array_equal(hc[:len(counts)], counts)) and nd.value == st["n_distinct"] and nh.value == st["n_hits"]
        res["host"] = {"threads": threads, "table_ms": round(float(ms[0]), 3), "scan_ms": round(float(ms[1]), 3), "gather_ms": round(float(ms[2]), 3),
                       "n_distinct": nd.value, "n_hits": nh.value, "positions_per_s": round(a.genome_bases / (ms[1] * 1e-3)) if ms[1] > 0 else None}
        res["tables_equal"] = equal
        res["max_value_seen"] = int(counts.max()) if len(counts) else 0
    res["sources_sha16"] = sources_sha16(ROOT)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not a.no_host and not res["tables_equal"]:
        sys.exit("the device's and the host's tables differ")


if __name__ == "__main__":
    main()
