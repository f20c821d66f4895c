#!/usr/bin/env python3
"""Times the two routes of a locus's aln.bam into a batch on one file:
  host     lcty_bam_read (inflate, one host thread over the records) + lcty_reads_append (host validation, upload)
  device   lcty_bam_read_device (host: read, inflate, header, walk; device: everything else) + lcty_reads_append_bam (device to device),
           with host_copy 0 and 1, and with knob "sample_bam_inflate" 0 and 1
The file is name-grouped as the mapper writes it: per read end a primary record (SEQ, qualities) and one secondary record per other
allele, `--pairs` x `--alleles` (default: the chunk of bench.py --format records, 32 768 x 256 — 16.8 M records). The routes are
alternated, `--runs` times each (the library calls alone are timed, not the copies into numpy arrays); before any time is printed the records of the two batches (lcty_reads_get_records) must be equal.
Medians and the stage times of the device route are printed and appended to profiles/aln_bam_probe.json (--out)."""
import argparse
import json
import os
import statistics
import struct
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from locityper_amd import api, io as lio, synth  # noqa: E402

READ_LEN = 150


def write_aln_bam(path, names, lens, n_pairs, level=1):
    """The file, built with numpy: every read end is a primary on allele (end + pair) % A and a secondary on every other allele."""
    A = len(names)
    head = b"BAM\1" + struct.pack("<I", 0) + struct.pack("<I", A)
    for nm, ln in zip(names, lens):
        head += struct.pack("<I", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<I", ln)
    l_name = 10                                             # "r%08d" + NUL
    prim_len = 36 + l_name + 4 + (READ_LEN + 1) // 2 + READ_LEN
    sec_len = 36 + l_name + 4
    n_ends = 2 * n_pairs
    rng = np.random.default_rng(11)
    end_bytes = prim_len + (A - 1) * sec_len
    out = np.zeros((n_ends, end_bytes), dtype=np.uint8)
    ends = np.arange(n_ends)
    name = np.frombuffer(b"".join(b"r%08d\0" % (e // 2) for e in range(n_ends)), dtype=np.uint8).reshape(n_ends, l_name)
    pos = rng.integers(0, min(lens) - READ_LEN - 1, size=(n_ends, A), dtype=np.int64).astype("<i4")

    def put(block, at, value, dt):
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(value), (n_ends,)).astype(dt))
        block[:, at:at + v.dtype.itemsize] = v.view(np.uint8).reshape(n_ends, -1)
    first = (ends + ends // 2) % A
    for k in range(A):                                      # record k of every end
        tid = (first + k) % A
        at0 = 0 if k == 0 else prim_len + (k - 1) * sec_len
        n = prim_len if k == 0 else sec_len
        blk = out[:, at0:at0 + n]
        flag = np.where(ends % 2 == 1, 0x80, 0) | (0 if k == 0 else 0x100) | np.where((ends + k) % 3 == 0, 0x10, 0)
        put(blk, 0, n - 4, "<u4"); put(blk, 4, tid, "<i4"); put(blk, 8, pos[ends, tid], "<i4")
        put(blk, 12, l_name | (((ends + k) % 61) << 8) | (4680 << 16), "<u4")
        put(blk, 16, 1 | (flag << 16), "<u4"); put(blk, 20, READ_LEN if k == 0 else 0, "<u4")
        put(blk, 24, -1, "<i4"); put(blk, 28, -1, "<i4"); put(blk, 32, 0, "<i4")
        blk[:, 36:36 + l_name] = name
        put(blk, 36 + l_name, (READ_LEN << 4) | 0, "<u4")
        if k == 0:
            codes = np.array([1, 2, 4, 8], dtype=np.uint8)[rng.integers(0, 4, size=(n_ends, 2 * ((READ_LEN + 1) // 2)))]
            blk[:, 36 + l_name + 4:36 + l_name + 4 + (READ_LEN + 1) // 2] = (codes[:, 0::2] << 4) | codes[:, 1::2]
            blk[:, 36 + l_name + 4 + (READ_LEN + 1) // 2:] = rng.integers(2, 41, size=(n_ends, READ_LEN), dtype=np.uint8)
    data = head + out.tobytes()
    del out
    with open(path, "wb") as f:
        for i in range(0, len(data), 0xff00):
            chunk = data[i:i + 0xff00]
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            comp = c.compress(chunk) + c.flush()
            f.write(struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(comp) + 25) + comp +
                    struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)))
        f.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    return len(data), n_ends * A


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=32768)
    ap.add_argument("--alleles", type=int, default=256)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aln_bam_probe.json"))
    ap.add_argument("--keep", help="write the file here instead of a temporary directory")
    a = ap.parse_args()

    t0 = time.perf_counter()
    L = synth.SynthLocus(a.alleles, 64, base_len=10_000)
    names = [f"a{i}" for i in range(a.alleles)]
    lens = [int(L.seq_off[i + 1] - L.seq_off[i]) for i in range(a.alleles)]
    tmp = tempfile.TemporaryDirectory()
    path = a.keep or os.path.join(tmp.name, "aln.bam")
    n_bytes, n_recs = write_aln_bam(path, names, lens, a.pairs)
    t_gen = time.perf_counter() - t0
    print(f"aln.bam: {a.pairs} pairs x {a.alleles} alleles, {n_recs} records, {n_bytes} bytes inflated, {os.path.getsize(path)} on disk, "
          f"written in {t_gen:.1f} s", flush=True)

    ctx = api.Context(0)
    loc = api.Locus(ctx, L.seqs, L.seq_off, L.counts, L.cnt_off, L.k, L.bg, api.resolve_params(api.default_params(), L.bg))

    def host_route():
        T = lio.BamTable(path, names, paired=True)
        t_read = 1e-3 * T.ms_native
        aa = api.AllAlignments(loc, *T.sizes()[:4])
        t = time.perf_counter()
        aa.append(T.chunk)
        return aa, dict(ms_read=1e3 * t_read, ms_append=1e3 * (time.perf_counter() - t))

    def device_route(host_copy):
        T = lio.BamTable(path, names, paired=True, ctx=ctx, host_copy=host_copy)
        t_read = 1e-3 * T.ms_native
        aa = api.AllAlignments(loc, *T.sizes()[:4])
        t = time.perf_counter()
        aa.append_bam(T)
        return aa, dict(ms_read=1e3 * t_read, ms_append=1e3 * (time.perf_counter() - t), stages=T.stats)

    # the two batches hold the same records before any time counts
    ah, _ = host_route()
    want = ah.records()
    del ah
    for inflate in (0, 1):
        ctx.set_knob("sample_bam_inflate", inflate)
        for hc in (False, True):
            ad, _ = device_route(hc)
            got = ad.records()
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want)), f"records differ (inflate {inflate}, host_copy {hc})"
            del ad, got
    del want
    print("records of the two batches are equal (inflate 0 / 1, host_copy 0 / 1)", flush=True)

    runs = {}
    for _ in range(a.runs):                                 # alternated
        for key, fn in (("host", host_route), ("device_i0_hc0", lambda: device_route(False)), ("device_i0_hc1", lambda: device_route(True)),
                        ("device_i1_hc0", lambda: device_route(False)), ("device_i1_hc1", lambda: device_route(True))):
            ctx.set_knob("sample_bam_inflate", 1 if "_i1_" in key else 0)
            aa, t = fn()
            del aa
            runs.setdefault(key, []).append(t)
    ctx.set_knob("sample_bam_inflate", -1)
    result = dict(pairs=a.pairs, alleles=a.alleles, records=n_recs, bytes_inflated=n_bytes, bytes_file=os.path.getsize(path), runs=a.runs, routes={})
    for key, ts in runs.items():
        total = [t["ms_read"] + t["ms_append"] for t in ts]
        r = dict(ms_total_median=statistics.median(total), ms_total=total, ms_read_median=statistics.median(t["ms_read"] for t in ts),
                 ms_append_median=statistics.median(t["ms_append"] for t in ts))
        if "stages" in ts[0]:
            r["stages_median"] = {k: statistics.median(t["stages"][k] for t in ts) for k in ts[0]["stages"] if k.startswith("ms_")}
        result["routes"][key] = r
        print(f"{key:>14}: read {r['ms_read_median']:9.1f} ms  append {r['ms_append_median']:8.1f} ms  total {r['ms_total_median']:9.1f} ms"
              + ("  " + " ".join(f"{k[3:]} {v:.1f}" for k, v in r["stages_median"].items()) if "stages_median" in r else ""), flush=True)
    prev = []
    if os.path.exists(a.out):
        prev = json.load(open(a.out))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(prev + [result], open(a.out, "w"), indent=1)
    print("appended to", a.out)


if __name__ == "__main__":
    main()
