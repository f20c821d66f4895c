#!/usr/bin/env python3
"""A cohort's genotypes as a phased VCF on the device, stage by stage:
   python3 scripts/gtvcf_probe.py [--samples 3202 --records 2000 --loci 8] [--repeats 2] [--no-host] [--out profiles/gtvcf_probe.json]

Makes a seeded synthetic cohort: --samples diploid samples whose predicted haplotypes are columns of a phased variants window, --loci loci
of --records records each on one contig, every locus overlapping the next by a quarter so that the merge has records to join; a twentieth
of the samples has no prediction in a locus and a tenth carries a warning text. Runs lcty_gtvcf_add_locus for every locus, lcty_bgzf_deflate
over every file and lcty_gtvcf_merge, --repeats times, and prints for the last (warm) run the summed milliseconds of upload, cells, widths,
write, download (lcty_gtvcf_stats, the stream drained after each stage), merge (merge_ms) and deflate (the total of lcty_bgzf_deflate's own
stats: its upload, kernel and download). Beside them the same stages as serial loops in ONE host thread (scripts/gtvcf_probe_host.cpp with
-DGTVCF_PROBE_SERIAL) — the execution model of extra/into_vcf.py — whose files must equal the device's byte for byte; its deflate is zlib at
level 6 per 0xff00-byte block, so the deflated sizes differ while the inflated bytes do not. The host twin has no upload or download.
One JSON line with the hash of the library's sources; --out appends it to a file."""
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
from locityper_amd import api, cdefs, io  # noqa: E402
from locityper_amd._lib import lib, check  # noqa: E402
from sources_sha import sources_sha16  # noqa: E402

STAGES = ("upload", "cells", "widths", "write", "download", "merge", "deflate")


def host_lib():
    here = os.path.dirname(os.path.abspath(__file__))
    out = os.path.join(tempfile.mkdtemp(prefix="gtvcf_probe_"), "libgtvcf_probe_host.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-DGTVCF_PROBE_SERIAL", "-I" + os.path.join(ROOT, "locityper_amd", "csrc"),
                    os.path.join(here, "gtvcf_probe_host.cpp"), "-o", out, "-lz"], check=True)
    L = C.CDLL(out)
    L.gtvcf_probe_serial.restype = C.c_int
    L.gtvcf_probe_serial.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p,
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.gtvcf_probe_serial_free.argtypes = [C.c_void_p]
    return L


def make_cohort(n_samples, n_records, n_loci, seed=1):
    """-> (sample names, an array of cdefs.GtvcfLocusIn, what keeps their arrays alive)"""
    rng = np.random.default_rng(seed)
    step = max(n_records * 3 // 4, 1)
    total = n_records + (n_loci - 1) * step
    n_haps = 2 * n_samples
    n_alt = rng.integers(1, 4, total)
    lens = []
    for r in range(total):
        lens.append(int(rng.integers(1, 5)))
        lens += [int(x) for x in rng.integers(1, 6, n_alt[r])]
    rec_allele = np.zeros(total + 1, dtype=np.uint32)
    np.cumsum(n_alt + 1, out=rec_allele[1:])
    allele_off = np.zeros(len(lens) + 1, dtype=np.uint64)
    np.cumsum(lens, out=allele_off[1:])
    allele_bytes = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(allele_off[-1]))].copy()
    pos = (1000 + 50 * np.arange(total)).astype(np.uint32)
    ref_len = (allele_off[rec_allele[:-1] + 1] - allele_off[rec_allele[:-1]]).astype(np.uint32)
    gt = (rng.integers(0, 4, (total, n_haps)) % (n_alt[:, None] + 1)).astype(np.int16)
    gt[rng.random((total, n_haps)) < 0.02] = -1
    samples = ["s%05d" % i for i in range(n_samples)]
    arr = (cdefs.GtvcfLocusIn * n_loci)()
    keep = []

    def ptr(a):
        keep.append(a)
        return a.ctypes.data
    for l in range(n_loci):
        r0, r1 = l * step, l * step + n_records
        a0, a1 = int(rec_allele[r0]), int(rec_allele[r1])
        predicted = rng.random(n_samples) >= 0.05
        pred_off = np.zeros(n_samples + 1, dtype=np.uint32)
        np.cumsum(2 * predicted, out=pred_off[1:])
        pred_col = rng.integers(0, n_haps, int(pred_off[-1])).astype(np.uint32)
        pred_col[rng.random(len(pred_col)) < 0.01] = cdefs.GTVCF_REF
        warns = [b"FewReads(%d)" % (l + s) if s % 10 == 0 else b"" for s in range(n_samples)]
        warn_off = np.zeros(n_samples + 1, dtype=np.uint64)
        np.cumsum([len(w) for w in warns], out=warn_off[1:])
        i = arr[l]
        names = (b"locus%d" % l, b"chr1")
        keep.append(names)
        i.locus, i.chrom, i.contig_len, i.contig_ix, i.start, i.end = names[0], names[1], 248956422, 0, int(pos[r0]), int(pos[r1 - 1]) + 1
        i.n_recs, i.n_haps = n_records, n_haps
        i.pos, i.ref_len = ptr(pos[r0:r1].copy()), ptr(ref_len[r0:r1].copy())
        i.rec_allele = ptr((rec_allele[r0:r1 + 1] - rec_allele[r0]).astype(np.uint32))
        i.allele_off = ptr((allele_off[a0:a1 + 1] - allele_off[a0]).astype(np.uint64))
        i.allele_bytes = ptr(allele_bytes[int(allele_off[a0]):int(allele_off[a1])].copy())
        i.gt = ptr(np.ascontiguousarray(gt[r0:r1]))
        i.pred_off, i.pred_col = ptr(pred_off), ptr(np.concatenate([pred_col, np.zeros(1, np.uint32)]))
        i.qual10, i.reads = ptr(rng.integers(0, 2000, n_samples).astype(np.int64)), ptr(rng.integers(0, 50000, n_samples).astype(np.int64))
        i.unexpl, i.wdist5 = ptr(rng.integers(0, 900, n_samples).astype(np.int64)), ptr(rng.integers(0, 3000000, n_samples).astype(np.int64))
        i.warn_off, i.warn = ptr(warn_off), ptr(np.frombuffer(b"".join(warns) + b"\0", dtype=np.uint8).copy())
    return samples, arr, keep


def device_run(ctx, samples, arr, mask):
    """-> (the loci's texts, the merged text, stage -> ms, counts)"""
    ms = {k: 0.0 for k in STAGES}
    gv = api.GenotypeVcf(ctx, samples, mask)
    texts, deflated = [], 0

    def book(st, text):
        nonlocal deflated
        for k in ("upload", "cells", "widths", "write", "download", "merge"):
            ms[k] += st[k + "_ms"]
        data, _, ds = io.bgzf_deflate(ctx, text)
        ms["deflate"] += ds["ms_total"]
        deflated += len(data)
    try:
        for i in arr:
            o = cdefs.GtvcfOut()
            check(lib().lcty_gtvcf_add_locus(gv._h, C.byref(i), C.byref(o)))
            texts.append(C.string_at(o.text, o.text_len))
            st = o.stats.as_dict()
            lib().lcty_gtvcf_out_free(C.byref(o))
            book(st, texts[-1])
        m = gv.merge()
        book(m["stats"], m["text"])
    finally:
        gv.close()
    return texts, m["text"], ms, dict(joined=m["n_joined"], merged_records=len(m["line_pos"]), deflated_bytes=deflated)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3202)
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--loci", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    t0 = time.perf_counter()
    samples, arr, keep = make_cohort(a.samples, a.records, a.loci)
    make_ms = (time.perf_counter() - t0) * 1e3
    mask = cdefs.GTVCF_ALL
    ctx = api.Context(0)
    for _ in range(max(a.repeats, 1)):
        t0 = time.perf_counter()
        texts, merged, ms, counts = device_run(ctx, samples, arr, mask)
        wall = (time.perf_counter() - t0) * 1e3
    out = {"samples": a.samples, "records": a.records, "loci": a.loci, "runs": max(a.repeats, 1), "sources_sha16": sources_sha16(ROOT), "make_cohort_ms": make_ms,
           "cells": a.samples * a.records * a.loci, "text_bytes": sum(len(t) for t in texts) + len(merged), "python_wall_ms": wall, **counts}
    out.update({k + "_ms": ms[k] for k in STAGES})
    out["total_ms"] = sum(ms.values())
    if not a.no_host:
        L = host_lib()
        hms = np.zeros(5, dtype=np.float64)
        text_len = np.zeros(a.loci, dtype=np.uint64)
        p, merged_len, joined, deflated = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        blob = b"".join(s.encode() + b"\0" for s in samples)
        rc = L.gtvcf_probe_serial(a.loci, C.cast(arr, C.c_void_p), a.samples, blob, mask, hms.ctypes.data, C.byref(p), text_len.ctypes.data, C.byref(merged_len),
                                  C.byref(joined), C.byref(deflated))
        equal = rc == 0 and joined.value == counts["joined"]
        if rc == 0:
            at = 0
            for n, t in zip(list(text_len) + [merged_len.value], texts + [merged]):
                equal = equal and C.string_at(p.value + at, int(n)) == t
                at += int(n)
            L.gtvcf_probe_serial_free(p)
        for k, v in zip(("cells", "widths", "write", "merge", "deflate"), hms):
            out[f"host_1_thread_{k}_ms"] = float(v)
            out[f"host_over_device_{k}"] = float(v) / ms[k] if ms[k] > 0 else None
        out["host_1_thread_total_ms"] = float(hms.sum())
        out["host_over_device_total"] = float(hms.sum()) / out["total_ms"] if out["total_ms"] > 0 else None
        out["host_1_thread_deflated_bytes"] = int(deflated.value)
        out["host_equal_device"] = bool(equal)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    ctx.close()
    del keep
    if not a.no_host and not out["host_equal_device"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
