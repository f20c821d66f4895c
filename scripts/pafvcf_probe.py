#!/usr/bin/env python3
"""A locus's haplotypes as a VCF on the device, stage by stage:
   python3 scripts/pafvcf_probe.py N_HAPS LEN [--items 401] [--runs 0.2] [--repeats 2] [--no-host] [--out profiles/pafvcf_probe_N_LEN.json]

Makes a seeded case of N_HAPS haplotypes planted into a reference of LEN bases with --items CIGAR items each (tests/pafvcf_cases.py: the
true CIGARs, every haplotype one entry against the reference), runs lcty_paf_to_vcf --repeats times for the merged file and prints, for the
last (warm) call, the milliseconds of the variants (entries, walk, shift), the ranges (sort, unique, merge), the table and the text with its
download (the stream is drained after each stage). Beside them the same stages as serial loops in ONE host thread
(scripts/pafvcf_probe_host.cpp) — the execution model of the reference, which has no threads here — whose body must equal the device's.
The variants stage is not like for like: the device also compares every '=' run with the bases it covers, the host twin (as the
reference) trusts them. The case generator is the tests' (tests/pafvcf_cases.py), so the probe runs from a checkout with its test tree.
One JSON line with the hash of the library's sources; --out also writes it to a file."""
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
from locityper_amd import api, cdefs  # noqa: E402
from sources_sha import sources_sha16  # noqa: E402
from tests import pafvcf_cases as PC  # noqa: E402


def host_lib():
    here = os.path.dirname(os.path.abspath(__file__))
    out = os.path.join(tempfile.mkdtemp(prefix="pafvcf_probe_"), "libpafvcf_probe_host.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", os.path.join(here, "pafvcf_probe_host.cpp"), "-o", out], check=True)
    L = C.CDLL(out)
    L.pafvcf_probe_host.restype = C.c_int
    L.pafvcf_probe_host.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                    C.c_char_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.pafvcf_probe_host_free.argtypes = [C.c_void_p]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("haplotypes", type=int)
    ap.add_argument("length", type=int)
    ap.add_argument("--items", type=int, default=401)
    ap.add_argument("--runs", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    t0 = time.perf_counter()
    names, seqs, entries, ref_hap = PC.make_case(1, a.haplotypes, a.length, [a.items], run_rate=a.runs, indel_at_0_rate=0.05, as_query_rate=0.0, dup_rate=0.0,
                                                 round_trip=True)
    flat, off = PC.flat(seqs)
    ent = PC.api_entries(entries)
    make_ms = (time.perf_counter() - t0) * 1e3
    ctx = api.Context(0)
    for _ in range(max(a.repeats, 1)):
        t0 = time.perf_counter()
        merged, _, st = api.paf_to_vcf(ctx, names, flat, off, ent, ref_hap, with_separate=False)
        wall = (time.perf_counter() - t0) * 1e3
    header_len = merged.index(b"\n#CHROM") + 1
    header_len = merged.index(b"\n", header_len) + 1
    out = {"haplotypes": a.haplotypes, "ref_len": a.length, "items": a.items, "runs": a.runs, "sources_sha16": sources_sha16(ROOT), "make_case_ms": make_ms,
           "variants": st["n_variants"], "shifted": st["n_shifted"], "unique": st["n_unique"], "merged": st["n_merged"], "lines": st["n_lines_merged"],
           "text_bytes": len(merged), "cells": st["n_merged"] * (a.haplotypes + 1),
           "upload_ms": st["upload_ms"], "variants_ms": st["variants_ms"], "ranges_ms": st["ranges_ms"], "table_ms": st["table_ms"], "text_ms": st["text_ms"],
           "total_ms": st["total_ms"], "python_call_ms": wall}
    if not a.no_host:
        lib = host_lib()
        groups, ref_id, _ = api.pafvcf_samples(names, ref_hap)
        slot_hap = np.array([cdefs.NONE_U32 if h is None else h for g in groups for h in g[1]], dtype=np.uint32)
        slot_first = np.array([i == 0 for g in groups for i in range(len(g[1]))], dtype=np.uint8)
        id1 = np.array([e[0] for e in ent], dtype=np.uint32)
        coff = np.zeros(len(ent) + 1, dtype=np.uint64)
        np.cumsum([len(e[2]) for e in ent], out=coff[1:])
        words = np.concatenate([e[2] for e in ent] + [np.zeros(1, dtype=np.uint32)])
        ms = np.zeros(4, dtype=np.float64)
        nv, nm, text, tl = C.c_uint64(), C.c_uint64(), C.c_void_p(), C.c_uint64()
        rc = lib.pafvcf_probe_host(len(seqs), flat.ctypes.data, off.ctypes.data, ref_id, len(ent), id1.ctypes.data, coff.ctypes.data, words.ctypes.data, len(slot_hap),
                                   slot_hap.ctypes.data, slot_first.ctypes.data, ref_hap, 0, ms.ctypes.data, C.byref(nv), C.byref(nm), C.byref(text), C.byref(tl))
        body = C.string_at(text, tl.value) if rc == 0 else b""
        if rc == 0:
            lib.pafvcf_probe_host_free(text)
        out.update(host_1_thread_variants_ms=ms[0], host_1_thread_ranges_ms=ms[1], host_1_thread_table_ms=ms[2], host_1_thread_text_ms=ms[3],
                   host_1_thread_total_ms=float(ms.sum()),
                   host_equal_device=bool(rc == 0 and body == merged[header_len:] and nv.value == st["n_variants"] and nm.value == st["n_merged"]))
        for k in ("variants", "ranges", "table", "text"):
            out[f"host_over_device_{k}"] = out[f"host_1_thread_{k}_ms"] / st[f"{k}_ms"] if st[f"{k}_ms"] > 0 else None
        out["host_over_device_total"] = out["host_1_thread_total_ms"] / st["total_ms"] if st["total_ms"] > 0 else None
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
