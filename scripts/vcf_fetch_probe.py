#!/usr/bin/env python3
"""Times the two readers of a pangenome VCF on one window:
  whole    lcty_vcf_open (the whole file read, inflated and walked on one host thread) + lcty_vcf_region (the window's records parsed
           on one host thread)
  indexed  lcty_vcf_indexed_open (the index and the head of the file) + lcty_vcf_indexed_fetch (the window's chunks read and inflated,
           the text parsed on the device), with knob "sample_bam_inflate" 0 (host zlib pool) and 1 (device)
The file is synthetic: `--records` records over ten contigs, `--samples` diploid samples with phased calls, BGZF with a tabix index,
both written here (this script has its own writers). The window holds `--window` records of a contig in the middle of the file. The
fetches are alternated, `--runs` times each; before any time is printed every array of the three routes must be equal. The stage
times, the bytes read and the bytes inflated are printed and appended to profiles/vcf_fetch_probe.json (--out), stamped with
scripts/sources_sha.py."""
import argparse
import json
import os
import statistics
import struct
import sys
import tempfile
import time
import zlib
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from locityper_amd import api, io as lio  # noqa: E402
from sources_sha import sources_sha16  # noqa: E402

BLOCK = 0xff00
STEP = 100                                                   # bases between two records
N_CONTIGS = 10
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_block(chunk):
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    comp = c.compress(chunk) + c.flush()
    return struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk))


def contig_text(name, n, n_samples, rng):
    """n records of fixed width: name, POS (zero-padded), '.', REF, ALT, three dots, GT, n_samples fields 'a|b'."""
    head = (name + "\t%09d\t.\tA\tC\t.\t.\t.\tGT\t").encode()
    w_head = len(head % 0)
    m = np.empty((n, w_head + 4 * n_samples), dtype=np.uint8)
    m[:, :w_head] = np.frombuffer(b"".join(head % (1 + STEP * i) for i in range(n)), dtype=np.uint8).reshape(n, w_head)
    calls = m[:, w_head:].reshape(n, n_samples, 4)
    calls[:, :, 0] = 48 + (rng.random((n, n_samples)) < 0.1)
    calls[:, :, 1] = ord("|")
    calls[:, :, 2] = 48 + (rng.random((n, n_samples)) < 0.1)
    calls[:, :, 3] = 9
    m[:, -1] = 10
    return m


def write_file(path, n_records, n_samples):
    """-> (the contigs' names, records per contig, the bytes of the text). Writes path and path + '.tbi'."""
    rng = np.random.default_rng(1)
    names = [f"chr{c + 1}" for c in range(N_CONTIGS)]
    per = n_records // N_CONTIGS
    header = ("##fileformat=VCFv4.2\n" + "".join(f"##contig=<ID={c}>\n" for c in names) + '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n' +
              "\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + [f"S{i}" for i in range(n_samples)]) + "\n").encode()
    # the text goes through the compressor in pieces of whole blocks; what is left of a contig is carried to the next
    line_at, csizes, carry, u = [], [], header, len(header)
    with open(path, "wb") as f, Pool(min(16, os.cpu_count() or 1)) as pool:
        def flush(data, last):
            n_full = len(data) // BLOCK * BLOCK if not last else len(data)
            chunks = [bytes(data[i:i + BLOCK]) for i in range(0, n_full, BLOCK)]
            for b in pool.map(bgzf_block, chunks, chunksize=8):
                csizes.append(len(b)); f.write(b)
            return data[n_full:]
        for c in range(N_CONTIGS):
            m = contig_text(names[c], per, n_samples, rng)
            line_at.append(u + m.shape[1] * np.arange(per, dtype=np.int64))
            u += m.size
            carry = flush(bytes(carry) + m.tobytes(), c + 1 == N_CONTIGS)
        f.write(EOF_BLOCK)
    cstart = np.concatenate([[0], np.cumsum(np.array(csizes, dtype=np.int64))])

    def voff(at):
        return (cstart[at // BLOCK] << 16) | (at % BLOCK)
    # ---- the tabix index: every record is one base long, so its bin is the 16 kb bin of its position; records of a bin are adjacent
    out = b"TBI\1" + struct.pack("<8i", N_CONTIGS, 2, 1, 2, 0, ord("#"), 0, sum(len(c) + 1 for c in names)) + b"".join(c.encode() + b"\0" for c in names)
    pos = STEP * np.arange(per, dtype=np.int64)
    win = pos >> 14
    first = np.flatnonzero(np.concatenate([[True], win[1:] != win[:-1]]))
    last = np.concatenate([first[1:], [per]])
    for c in range(N_CONTIGS):
        at = line_at[c]
        end_of = np.concatenate([at[1:], [at[-1] + (at[1] - at[0])]])
        out += struct.pack("<i", len(first) + 1)
        for a, b in zip(first, last):
            out += struct.pack("<IiQQ", 4681 + int(win[a]), 1, int(voff(at[a])), int(voff(end_of[b - 1])))
        out += struct.pack("<IiQQQQ", 37450, 2, int(voff(at[0])), int(voff(end_of[-1])), per, 0)
        out += struct.pack("<i", int(win[-1]) + 1)
        lin = np.zeros(int(win[-1]) + 1, dtype=np.int64)
        lin[win[first]] = voff(at[first])
        out += lin.astype("<u8").tobytes()
    out += struct.pack("<Q", 0)
    with open(path + ".tbi", "wb") as f:
        for i in range(0, len(out), BLOCK):
            f.write(bgzf_block(out[i:i + BLOCK]))
        f.write(EOF_BLOCK)
    return names, per, u


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=45, help="diploid samples (45: 90 haplotypes)")
    ap.add_argument("--records", type=int, default=200_000, help="records of the file")
    ap.add_argument("--window", type=int, default=20_000, help="records of the window")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcf_fetch_probe.json"))
    ap.add_argument("--dir", default=None, help="where the file is written (default: a temporary directory)")
    a = ap.parse_args()
    if a.window > a.records // N_CONTIGS:
        sys.exit("--window must fit into one of the ten contigs")
    tmp = tempfile.TemporaryDirectory(dir=a.dir)
    path = os.path.join(tmp.name, "probe.vcf.gz")
    t0 = time.perf_counter()
    names, per, text_bytes = write_file(path, a.records, a.samples)
    print(f"file: {a.records} records x {2 * a.samples} haplotypes, {text_bytes} bytes of text, {os.path.getsize(path)} in the file ({time.perf_counter() - t0:.1f} s)", flush=True)
    contig = names[N_CONTIGS // 2]
    i0 = (per - a.window) // 2
    region = (contig, STEP * i0, STEP * (i0 + a.window - 1) + 1)

    ctx = api.Context(0)
    t0 = time.perf_counter()
    whole = lio.Vcf(path)
    ms_open = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    indexed = lio.VcfIndexed(path, ctx=ctx)
    ms_iopen = 1e3 * (time.perf_counter() - t0)
    assert indexed.samples == whole.samples and indexed.ploidy.tolist() == whole.ploidy.tolist()
    routes = {"whole": [], "indexed_i0": [], "indexed_i1": []}
    stages = {"indexed_i0": [], "indexed_i1": []}
    want = None
    for _ in range(a.runs + 1):                                           # the first turn warms up and is compared
        t0 = time.perf_counter()
        r = whole.region(*region)
        routes["whole"].append(1e3 * (time.perf_counter() - t0))
        if want is None:
            want = r
            assert len(want["pos"]) == a.window
        for inflate in (0, 1):
            ctx.set_knob("sample_bam_inflate", inflate)
            t0 = time.perf_counter()
            g = indexed.region(*region)
            routes[f"indexed_i{inflate}"].append(1e3 * (time.perf_counter() - t0))
            stages[f"indexed_i{inflate}"].append(indexed.stats)
            for key in want:
                assert np.array_equal(g[key], want[key]) and g[key].dtype == want[key].dtype, key
    ctx.set_knob("sample_bam_inflate", -1)
    line = {"sources_sha": sources_sha16(ROOT), "samples": a.samples, "haplotypes": 2 * a.samples, "records": a.records, "window": a.window, "runs": a.runs,
            "text_bytes": text_bytes, "file_bytes": os.path.getsize(path), "ms_open_whole": ms_open, "ms_open_indexed": ms_iopen, "routes": {}}
    for name, ms in routes.items():
        line["routes"][name] = {"ms_call_median": statistics.median(ms[1:]), "ms_call": ms[1:]}
        if name in stages:
            st = stages[name][1:]
            line["routes"][name]["stats_median"] = {k: statistics.median(s[k] for s in st) for k in st[0]}
    print(json.dumps(line, indent=1))
    hist = json.load(open(a.out)) if os.path.exists(a.out) else []
    hist.append(line)
    with open(a.out, "w") as f:
        json.dump(hist, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
