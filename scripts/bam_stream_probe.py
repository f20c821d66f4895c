"""Developer measurement: whole BAM files without an index streamed through the device (lcty_bam_stream_*) against the
FASTQ device route over the same reads, at the shape of `locityper genotype -a reads.bam --no-index -^`:
   fastq    lcty_fastx_device_next (one interleaved FASTQ file) + lcty_fastx_device_recruit      the yardstick
   bam      lcty_bam_stream_next (--files name-grouped BAM files) + lcty_sample_reads_recruit
   python3 scripts/bam_stream_probe.py [--pairs 1000000] [--len 150] [--files 1] [--inflate host|device] [--runs 1]
One synthetic sample is made: `--pairs` pairs of `--len` bases, one pair in eight drawn from the alleles of the one locus the targets
hold, the rest random; as one interleaved FASTQ file and as `--files` BAM files of the same records, mates side by side (deflated on the
device). Each route runs once to warm up (allocations, the page cache), then alternately `--runs` times; before any time is printed
the answers of the two routes must be equal, read for read. The stage times are printed and appended to profiles/bam_stream_probe.json
(--out), stamped with scripts/sources_sha.py. --inflate: knob "sample_bam_inflate" of the BAM route's BGZF blocks."""
import argparse
import json
import os
import statistics
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from locityper_amd import api, io as lio  # noqa: E402
from fastx_probe import MAX_OUT, digest_of, make_text  # noqa: E402
from sources_sha import sources_sha16  # noqa: E402
import hashlib  # noqa: E402

BAM_HEADER = b"BAM\1" + struct.pack("<I", 0) + struct.pack("<I", 0)          # no text, no contigs: an unaligned BAM


def bam_records(text, n, length, flag):
    """the fixed-width FASTQ records of fastx_probe.make_text as unaligned BAM records, [n, width] bytes"""
    width_fq = 14 + length + 3 + length + 1
    fq = np.frombuffer(text, dtype=np.uint8).reshape(n, width_fq)
    half = (length + 1) // 2
    body = 32 + 13 + half + length
    rec = np.zeros((n, 4 + body), dtype=np.uint8)
    head = struct.pack("<IiiBBHHHIiii", body, -1, -1, 13, 0, 4680, 0, flag, length, -1, -1, 0)
    rec[:, :36] = np.frombuffer(head, dtype=np.uint8)
    rec[:, 36:48] = fq[:, 1:13]                                              # p<9 digits>/<mate>, then the NUL
    code = np.zeros(256, dtype=np.uint8)
    code[list(b"ACGT")] = [1, 2, 4, 8]
    nib = np.zeros((n, 2 * half), dtype=np.uint8)
    nib[:, :length] = code[fq[:, 14:14 + length]]
    rec[:, 49:49 + half] = (nib[:, 0::2] << 4) | nib[:, 1::2]
    rec[:, 49 + half:] = fq[:, 17 + length:17 + 2 * length] - 33
    return rec


def make_files(d, ctx, pairs, length, n_files, alleles):
    """-> (the interleaved FASTQ, the BAM files, bytes of FASTQ text, inflated bytes of the BAM files)"""
    il = os.path.join(d, "reads.fq")
    bams = [os.path.join(d, f"reads.{k}.bam") for k in range(n_files)]
    per_file = (pairs + n_files - 1) // n_files
    rngs = [np.random.default_rng(101), np.random.default_rng(102)]
    text_bytes = bam_bytes = 0
    with open(il, "wb") as out:
        for k, path in enumerate(bams):
            lo, hi = k * per_file, min(pairs, (k + 1) * per_file)
            data = [BAM_HEADER]
            for f in range(lo, hi, 250_000):
                n = min(250_000, hi - f)
                t = [make_text(rngs[m], alleles, f, n, length, m + 1) for m in (0, 1)]
                width = len(t[0]) // n
                both = np.stack([np.frombuffer(x, dtype=np.uint8).reshape(n, width) for x in t], axis=1)
                out.write(both.tobytes()); text_bytes += both.size
                r = np.stack([bam_records(t[0], n, length, 0x4D), bam_records(t[1], n, length, 0x8D)], axis=1)
                data.append(r.tobytes())
            blob = b"".join(data)
            bam_bytes += len(blob)
            lio.write_bgzf_device(ctx, path, blob)
    return il, bams, text_bytes, bam_bytes


def run_fastq(ctx, gt, il, chunk):
    t = dict(ms_recruit=0.0)
    h, n, rec = (hashlib.sha1(), hashlib.sha1()), 0, 0
    t_all = time.perf_counter()
    f = lio.FastxDevice(ctx, il, interleaved=True)
    while f.next(chunk):
        t0 = time.perf_counter()
        cnt, loci = f.recruit(gt, max_out=MAX_OUT)
        t["ms_recruit"] += (time.perf_counter() - t0) * 1e3
        n += f.n; rec += digest_of(h, cnt, loci)
    t.update(f.stats)
    f.close()
    t["ms_wall"] = (time.perf_counter() - t_all) * 1e3
    return t, n, rec, h[0].hexdigest() + h[1].hexdigest()


def run_bam(ctx, gt, bams):
    t = dict(ms_recruit=0.0)
    h, n, rec = (hashlib.sha1(), hashlib.sha1()), 0, 0
    t_all = time.perf_counter()
    st = lio.BamStream(ctx, bams, interleaved=True)
    while True:
        reads, stats = st.next()
        k = reads.stats["n_pairs"]
        if not k:
            break
        t0 = time.perf_counter()
        cnt, loci = reads.recruit(gt, max_out=MAX_OUT)
        t["ms_recruit"] += (time.perf_counter() - t0) * 1e3
        n += k; rec += digest_of(h, cnt, loci)
    t.update(st.stats)
    st.close()
    t["ms_wall"] = (time.perf_counter() - t_all) * 1e3
    return t, n, rec, h[0].hexdigest() + h[1].hexdigest()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--files", type=int, default=1)
    ap.add_argument("--inflate", choices=("host", "device"), default="host")
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=1 << 20, help="read pairs a call of the FASTQ route")
    ap.add_argument("--window", type=int, default=-1, help='knob "bam_stream_window_bytes" (default 2^28)')
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_stream_probe.json"))
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary directory)")
    a = ap.parse_args()
    if not 20 <= a.len <= 256:
        raise SystemExit("--len: 20 .. 256 (the pair kernel of recruitment takes mates of up to 256 bases)")
    if not 1 <= a.files <= a.pairs:
        raise SystemExit("--files: 1 .. --pairs")
    ctx = api.Context(0)
    ctx.set_knob("sample_bam_inflate", 1 if a.inflate == "device" else 0)
    ctx.set_knob("bam_stream_window_bytes", a.window)
    rng = np.random.default_rng(1)
    alleles = [rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 20_000) for _ in range(4)]
    gt = api.Targets(ctx, api.recruit_params(paired=True))
    counts = [np.zeros(len(x) - 24, dtype=np.uint16) for x in alleles]
    gt.add_locus(np.concatenate(alleles), np.cumsum([0] + [len(x) for x in alleles]).astype(np.uint64), np.concatenate(counts),
                 np.cumsum([0] + [len(c) for c in counts]).astype(np.uint64), 25)
    gt.finalize()
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        t0 = time.perf_counter()
        il, bams, text_bytes, bam_bytes = make_files(d, ctx, a.pairs, a.len, a.files, alleles)
        file_bytes = sum(os.path.getsize(p) for p in bams)
        print(json.dumps(dict(made=[il] + bams, text_bytes=text_bytes, bam_bytes=bam_bytes, file_bytes=file_bytes, ms_make=round((time.perf_counter() - t0) * 1e3))), flush=True)
        rows = {"fastq": [], "bam": []}
        for r in range(a.runs + 1):                                          # round 0 warms both routes up
            tf, nf, rf, df = run_fastq(ctx, gt, il, a.chunk)
            tb, nb, rb, db = run_bam(ctx, gt, bams)
            if (nf, rf, df) != (nb, rb, db) or nf != a.pairs:
                raise SystemExit(f"the routes differ: fastq {nf} pairs, {rf} recruited, {df}; bam {nb} pairs, {rb} recruited, {db}")
            if r:
                rows["fastq"].append(tf); rows["bam"].append(tb)
    med = {k: {f: (round(statistics.median(x[f] for x in v), 3) if f.startswith("ms_") else v[-1][f]) for f in v[0]} for k, v in rows.items()}
    b = med["bam"]
    windows = max(b["windows"], 1)
    front = b["ms_read"] + b["ms_inflate"]
    line = {"sources_sha": sources_sha16(ROOT), "pairs": a.pairs, "len": a.len, "files": a.files, "inflate": a.inflate, "runs": a.runs, "chunk": a.chunk,
            "window": a.window, "text_bytes": text_bytes, "bam_bytes": bam_bytes, "file_bytes": file_bytes, "recruited": rb, "answers_equal": True,
            "fastq": med["fastq"], "bam": b,
            "bam_ms_per_window": {f: round(b[f] / windows, 3) for f in ("ms_read", "ms_inflate", "ms_walk", "ms_upload", "ms_record", "ms_pair", "ms_unpack", "ms_total")},
            "bam_inflated_gb_per_s": round(b["bytes_inflated"] / (b["ms_total"] * 1e-3) / 1e9, 3),
            "bam_host_front_share": round(front / b["ms_total"], 3),          # what overlapping the next window's read + inflate would hide
            "pairs_per_s": {k: round(a.pairs / (med[k]["ms_wall"] * 1e-3)) for k in med}}
    print(json.dumps(line, indent=1))
    hist = json.load(open(a.out)) if os.path.exists(a.out) else []
    hist.append(line)
    with open(a.out, "w") as f:
        json.dump(hist, f, indent=1)
        f.write("\n")
