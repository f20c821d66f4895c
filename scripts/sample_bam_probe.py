"""Developer measurement: lcty_sample_bam_fetch + lcty_sample_reads_recruit at the shape of `locityper genotype -a`: a coordinate-sorted,
indexed BAM file, a few hundred fetch regions with 30x of 100-base pairs inside them, foreign records between the regions that the index
must skip, a share of pairs without coordinate. Synthetic, written with tests/pyref_sample_bam.
   python3 scripts/sample_bam_probe.py --make DIR [--regions 200] [--region-len 4000] [--unmapped 0.05] [--foreign 0.5]     (CPU only)
   python3 scripts/sample_bam_probe.py DIR [--calls 5] [--inflate host|device]
--inflate: knob "sample_bam_inflate" (host: zlib on at most 16 threads; device: bgzf_inflate_kernel).
measure: the first call pays the allocations; one JSON line with the medians of the calls after it per stage (file read, inflate, walk,
upload, record / pair / unpack stages, recruitment), and the same stages as serial loops in one host thread (numpy for the per-record
tests, a dict for the pairing, one zlib stream), whose stream, pairs and discarded count must equal the library's."""
import argparse
import json
import os
import pickle
import struct
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def make(d, n_regions, region_len, unmapped, foreign, seed=5):
    from tests import pyref_sample_bam as P
    rng = np.random.default_rng(seed)
    os.makedirs(d, exist_ok=True)
    n_contigs = 8
    refs = [(f"chr{c + 1}", 60_000_000) for c in range(n_contigs)]
    # regions spread over the contigs, 200 kb apart; foreign records in the gaps
    regions, spans = [], []
    for i in range(n_regions):
        t, s = i % n_contigs, 1_000_000 + (i // n_contigs) * 200_000
        regions.append((t, s, s + region_len))
        spans.append((t, s - 500, s + region_len + 500, int(30 * (region_len + 1000) / 200)))
        spans.append((t, s + 60_000, s + 60_000 + region_len, int(foreign * 30 * region_len / 200)))
    regions.sort()
    recs = []
    codes = np.array([0x1, 0x2, 0x4, 0x8], dtype=np.uint8)
    qual = bytes([30]) * 100

    def seq_bytes():
        c = codes[rng.integers(0, 4, 100)]
        return bytes((c[0::2] << 4) | c[1::2])
    pid = 0
    for t, lo, hi, n in spans:
        p1s = rng.integers(lo, hi, n)
        ins = rng.integers(250, 450, n)
        for p1, i in zip(p1s.tolist(), ins.tolist()):
            p2 = p1 + i - 100
            rev = pid & 1
            nm = f"q{pid}".encode() + b"\0"
            recs.append((t, p1, nm, 0x41 | (0x10 if rev else 0x20), t, p2))
            recs.append((t, p2, nm, 0x81 | (0x20 if rev else 0x10), t, p1))
            pid += 1
    recs.sort(key=lambda r: (r[0], r[1]))
    n_tail = int(unmapped * pid)
    for i in range(n_tail):
        nm = f"u{i}".encode() + b"\0"
        recs.append((-1, -1, nm, 0x4d, -1, -1))
        recs.append((-1, -1, nm, 0x8d, -1, -1))
    blobs, light = [], []
    for t, p, nm, fl, mt, mp in recs:
        placed = t >= 0
        cig = struct.pack("<I", (100 << 4)) if placed else b""
        b = P.reg2bin(p, p + 100) if placed else 4680
        body = struct.pack("<iiBBHHHIiii", t, p, len(nm), 60, b, 1 if placed else 0, fl, 100, mt, mp, 0) + nm + cig + seq_bytes() + qual
        blobs.append(struct.pack("<I", len(body)) + body)
        light.append(dict(tid=t, pos=p, flag=fl, cigar=[("M", 100)] if placed else []))
    P.write_bam(os.path.join(d, "sample.bam"), refs, light, raw_records=blobs)
    with open(os.path.join(d, "sample.pkl"), "wb") as f:
        pickle.dump(dict(regions=regions, n_records=len(recs)), f)
    print(json.dumps(dict(records=len(recs), regions=len(regions), bytes=os.path.getsize(os.path.join(d, "sample.bam")))))


def host_serial(path, regions):
    """The stages in one host thread, on the whole file: inflate, walk, per-record tests, pairing. -> (times, stream ordinals of the mates, discarded)"""
    t = {}
    t0 = time.perf_counter()
    raw = open(path, "rb").read()
    t["ms_read"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    out, at = [], 0
    while at < len(raw):
        bsize = struct.unpack_from("<H", raw, at + 16)[0] + 1
        out.append(zlib.decompress(raw[at + 18:at + bsize - 8], -15))
        at += bsize
    data = b"".join(out)
    t["ms_inflate"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    l_text = struct.unpack_from("<I", data, 4)[0]
    at = 8 + l_text
    n_ref = struct.unpack_from("<I", data, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<I", data, at)[0]
    offs = []
    while at < len(data):
        offs.append(at)
        at += 4 + struct.unpack_from("<I", data, at)[0]
    offs = np.array(offs, dtype=np.int64)
    t["ms_walk"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    buf = np.frombuffer(data, dtype=np.uint8)
    def field(o, dt):
        n = np.dtype(dt).itemsize
        return np.ascontiguousarray(buf[(offs + o)[:, None] + np.arange(n)]).view(dt)[:, 0]
    tid, pos, flag = field(4, "<i4").astype(np.int64), field(8, "<i4").astype(np.int64), field(18, "<u2").astype(np.int64)
    mtid, mpos, n_cig = field(24, "<i4").astype(np.int64), field(28, "<i4").astype(np.int64), field(16, "<u2")
    assert int(n_cig.max()) <= 1                                         # the probe's records: one M operation, or none
    l_name = buf[offs + 12].astype(np.int64)
    rlen = np.where((n_cig == 1) & ((flag & 4) == 0), 100, 0)
    end = pos + np.maximum(rlen, 1)
    reg = np.array(regions, dtype=np.int64)
    key = tid * (1 << 32) + pos
    i = np.searchsorted(reg[:, 0] * (1 << 32) + reg[:, 2], key, side="right")          # the first region that ends behind pos
    i = np.minimum(i, len(reg) - 1)
    placed = tid >= 0
    kept = ((flag & 0x900) == 0) & np.where(placed, (reg[i, 0] == tid) & (reg[i, 2] > pos) & (reg[i, 1] < end), True)
    stream = np.flatnonzero(kept)
    t["ms_record"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    waiting, pairs, discarded = {}, [], 0
    u = lambda a, bits: a & ((1 << bits) - 1)
    for s, r in enumerate(stream.tolist()):
        o = int(offs[r])
        name = data[o + 36:o + 36 + int(l_name[r])]
        m = waiting.pop(name, None)
        if m is not None:
            pairs.append((s, m) if flag[r] & 0x40 else (m, s))
        elif (u(int(tid[r]), 32), u(int(pos[r]), 64)) <= (u(int(mtid[r]), 32), u(int(mpos[r]), 64)):
            waiting[name] = s
        else:
            discarded += 1
    t["ms_pair"] = (time.perf_counter() - t0) * 1e3
    return t, np.array(pairs, dtype=np.uint32).reshape(-1), discarded + len(waiting), len(stream)


def measure(d, calls, inflate):
    from locityper_amd import api, io as lio
    with open(os.path.join(d, "sample.pkl"), "rb") as f:
        meta = pickle.load(f)
    regions = meta["regions"]
    path = os.path.join(d, "sample.bam")
    ctx = api.Context(0)
    ctx.set_knob("sample_bam_inflate", 1 if inflate == "device" else 0)
    rng = np.random.default_rng(1)
    gt = api.Targets(ctx, api.recruit_params(paired=True))
    alleles = [bytes(rng.choice(list(b"ACGT"), 20_000).astype(np.uint8)) for _ in range(4)]
    counts = [np.zeros(len(a) - 24, dtype=np.uint16) for a in alleles]
    gt.add_locus(np.frombuffer(b"".join(alleles), dtype=np.uint8), np.cumsum([0] + [len(a) for a in alleles]).astype(np.uint64),
                 np.concatenate(counts), np.cumsum([0] + [len(c) for c in counts]).astype(np.uint64), 25)
    gt.finalize()
    bam = lio.SampleBam(path)
    rows, src = [], None
    for c in range(calls + 1):
        t0 = time.perf_counter()
        reads = bam.fetch(ctx, regions, with_unmapped=True)
        st = dict(reads.stats)
        st["ms_fetch_wall"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        reads.recruit(gt)
        st["ms_recruit"] = (time.perf_counter() - t0) * 1e3
        if c == calls:
            src = reads.view()[1]
        reads.close()
        if c:
            rows.append(st)
    med = {k: (round(float(np.median([r[k] for r in rows])), 3) if k.startswith("ms_") else rows[-1][k]) for k in rows[0]}
    host_t, host_src, host_discarded, host_kept = host_serial(path, regions)
    equal = bool(np.array_equal(host_src, src)) and host_discarded == med["n_discarded"] and host_kept == med["records_kept"]
    print(json.dumps(dict(records_in_file=meta["n_records"], calls=calls, inflate=inflate, device=med, host_one_thread={k: round(v, 3) for k, v in host_t.items()},
                          host_equals_device=equal)))
    if not equal:
        raise SystemExit("the host's stream or pairs differ from the library's")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--make", action="store_true")
    ap.add_argument("--regions", type=int, default=200)
    ap.add_argument("--region-len", type=int, default=4000)
    ap.add_argument("--unmapped", type=float, default=0.05)
    ap.add_argument("--foreign", type=float, default=0.5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--inflate", choices=("host", "device"), default="host")
    a = ap.parse_args()
    if a.make:
        make(a.dir, a.regions, a.region_len, a.unmapped, a.foreign)
    else:
        measure(a.dir, a.calls, a.inflate)
