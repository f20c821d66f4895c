"""Developer measurement: lcty_bg_estimate at the full size of `locityper preproc` — the default 4.5 Mb background region
(preproc.rs:599-603) at 30x 150 bp paired-end Illumina (~450 k pairs) and 30x 10 kb ONT (~13.5 k reads) — synthetic, from tests/bg_synth.
   python3 scripts/bg_probe.py --make DIR [illumina|ont]
                                              write the samples under DIR (CPU only): the region's records as NAME.bam, the same
                                              records followed by as many bytes of foreign ones (behind the padded region and on a
                                              second contig) as the indexed NAME.whole.bam + .bai, the padded sequence, the k-mer counts
   python3 scripts/bg_probe.py DIR            measure: one JSON line with the host BAM decode, the device time of each kernel (events
                                              around synchronised work), the host fits and the whole call, per sample
   python3 scripts/bg_probe.py DIR --fetch [--out FILE]
                                              the two routes side by side, per sample: lcty_bg_reads_load on NAME.bam, and
                                              lcty_bg_reads_fetch on NAME.whole.bam with the host and with the device inflate (one call
                                              after a warm-up call each): the stage times, bytes_read against file_bytes, then the
                                              estimate; the JSON line is also appended to FILE (profiles/bg_fetch_probe.json)"""
import json
import os
import pickle
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

REGION = 4_500_000


def refs_of(s):
    return [(s.contig, s.padded_start + len(s.padded_seq) + 50_000_000), ("chrO", 200_000_000)]


def foreign(s, n_bytes):
    """(records for the index, their bytes): 150-base records 300 kb behind the padded region and on the second contig, n_bytes in all;
    a few thousand records are encoded, and contig, position and name patched into copies of them"""
    import struct
    from tests import pyref_sample_bam as SB
    fl = (0x1 | 0x2 | 0x40) if s.paired else 0
    rng = np.random.default_rng(5)                                  # 4 096 sequences in turn: none comes back inside a DEFLATE window
    tmpls = [bytearray(SB.record_bytes(SB.rec(0, 0, "f" + "0" * 9, fl, [("M", 150)], "".join(rng.choice(list("ACGT"), 150)))))
             for _ in range(4096)]
    n = n_bytes // len(tmpls[0]) + 1
    recs, blobs = [], []
    at = s.padded_start + len(s.padded_seq) + 300_000
    for half, (tid, first) in enumerate(((0, at), (1, 10_000))):
        for i in range(n // 2 + 1):
            pos = first + 10 * i
            b = bytearray(tmpls[i % 4096])
            struct.pack_into("<ii", b, 4, tid, pos)
            struct.pack_into("<H", b, 14, SB.reg2bin(pos, pos + 150))
            b[36:46] = b"f%d%08d" % (half, i)
            blobs.append(bytes(b))
            recs.append(dict(tid=tid, pos=pos, flag=fl, cigar=[("M", 150)]))
    return recs, blobs


def make(d, only=None):
    from tests import bg_fetch_cases, bg_synth, pyref_sample_bam as SB
    os.makedirs(d, exist_ok=True)
    for name in ("illumina", "ont"):
        if only and name != only:
            continue
        s = bg_synth.Sample(seed=21, region_len=REGION) if name == "illumina" else bg_synth.ont_sample(seed=22, region_len=REGION)
        bg_synth.write_bam(os.path.join(d, name + ".bam"), refs_of(s), s.records)
        own = [bg_fetch_cases.to_rec(t) for t in s.records]
        own_blobs = [SB.record_bytes(r) for r in own]
        f_recs, f_blobs = foreign(s, sum(len(b) for b in own_blobs))
        last_own = max(i for i, r in enumerate(own) if r["tid"] == 0) + 1            # the sample's records of the second contig go behind
        n_f0 = sum(1 for r in f_recs if r["tid"] == 0)
        recs = own[:last_own] + f_recs[:n_f0] + own[last_own:] + f_recs[n_f0:]
        blobs = own_blobs[:last_own] + f_blobs[:n_f0] + own_blobs[last_own:] + f_blobs[n_f0:]
        SB.write_bam(os.path.join(d, name + ".whole.bam"), refs_of(s), recs, raw_records=blobs)
        meta = dict(contig=s.contig, start=s.start, end=s.end, padded_start=s.padded_start, k=s.k, seq=s.padded_seq,
                    records_region=len(own), records_whole=len(recs))
        with open(os.path.join(d, name + ".pkl"), "wb") as f:
            pickle.dump(meta, f)
        s.kmer_counts.tofile(os.path.join(d, name + ".u16"))


def measure(d):
    from locityper_amd import api, cdefs
    ctx = api.Context(0)
    out = {"region_bp": REGION}
    for name, tech in (("illumina", cdefs.TECH_ILLUMINA), ("ont", cdefs.TECH_NANOPORE)):
        with open(os.path.join(d, name + ".pkl"), "rb") as f:
            m = pickle.load(f)
        counts = np.fromfile(os.path.join(d, name + ".u16"), dtype=np.uint16)
        prm = api.bg_params(tech)
        t0 = time.perf_counter()
        reads = api.read_bg_bam(os.path.join(d, name + ".bam"), m["contig"], m["start"], m["end"], m["padded_start"], len(m["seq"]), prm)
        t_read = (time.perf_counter() - t0) * 1e3
        res = None
        for _ in range(2):                                   # the first call pays for module load and allocation
            t0 = time.perf_counter()
            bg, rl, dg = api.estimate_bg(ctx, reads, m["seq"], m["padded_start"], counts, m["k"], m["start"], m["end"], prm)
            res = (time.perf_counter() - t0) * 1e3, dg
        wall, dg = res
        out[name] = dict(records=reads.n_records, pairs=int(dg["n_stage"][1]), windows=int(len(dg["win_start"])),
                         bam_decode_ms=round(t_read, 1), kernel_ms=dict(zip(("windows", "counts", "pairs", "depth"),
                                                                            [round(float(x), 3) for x in dg["kernel_ms"]])),
                         fit_ms=round(float(dg["fit_ms"]), 1), call_ms=round(float(dg["total_ms"]), 1), call_wall_ms=round(wall, 1))
    print(json.dumps(out))


def measure_fetch(d, out_path):
    from locityper_amd import api, cdefs, io
    ctx = api.Context(0)
    out = {"region_bp": REGION}
    stages = ("ms_read", "ms_inflate", "ms_walk", "ms_upload", "ms_record", "ms_pair", "ms_unpack", "ms_total")
    for name, tech in (("illumina", cdefs.TECH_ILLUMINA), ("ont", cdefs.TECH_NANOPORE)):
        with open(os.path.join(d, name + ".pkl"), "rb") as f:
            m = pickle.load(f)
        counts = np.fromfile(os.path.join(d, name + ".u16"), dtype=np.uint16)
        prm = api.bg_params(tech)
        args = (m["contig"], m["start"], m["end"], m["padded_start"], len(m["seq"]), prm)

        def estimate(reads):
            res = None
            for _ in range(2):                               # the first call pays for module load and allocation
                t0 = time.perf_counter()
                bg, rl, dg = api.estimate_bg(ctx, reads, m["seq"], m["padded_start"], counts, m["k"], m["start"], m["end"], prm)
                res = dict(call_wall_ms=round((time.perf_counter() - t0) * 1e3, 1), call_ms=round(float(dg["total_ms"]), 1),
                           fit_ms=round(float(dg["fit_ms"]), 1), kernels_ms=round(float(sum(dg["kernel_ms"])), 3))
            return res, bytes(bg)
        row = {}
        loaded = api.read_bg_bam(os.path.join(d, name + ".bam"), *args)
        est, bg_load = estimate(loaded)
        row["load"] = dict(file_bytes=os.path.getsize(os.path.join(d, name + ".bam")), records=loaded.n_records, estimate=est)
        row["load"]["decode_ms"] = None
        for _ in range(2):
            t0 = time.perf_counter()
            again = api.read_bg_bam(os.path.join(d, name + ".bam"), *args)
            row["load"]["decode_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            again.close()
        whole = io.SampleBam(os.path.join(d, name + ".whole.bam"))
        for route, knob in (("fetch", 0), ("fetch_device_inflate", 1)):
            ctx.set_knob("sample_bam_inflate", knob)
            reads = None
            for _ in range(2):
                if reads is not None:
                    reads.close()
                t0 = time.perf_counter()
                reads = api.BgReads.fetch(ctx, whole, *args)
                wall = (time.perf_counter() - t0) * 1e3
            st = reads.stats
            est, bg_fetch = estimate(reads)
            same = bg_fetch == bg_load and all(np.array_equal(getattr(reads, f), getattr(loaded, f)) for f in
                                               ("pos", "end", "qlen", "flags", "mate", "cigar_off", "cigar", "seq_off", "bases2", "nmask"))
            row[route] = dict(file_bytes=int(st["file_bytes"]), bytes_read=int(st["bytes_read"]), bytes_inflated=int(st["bytes_inflated"]),
                              n_chunks=int(st["n_chunks"]), records_walked=int(st["records_walked"]), records=reads.n_records,
                              records_in_file=m.get("records_whole"), call_wall_ms=round(wall, 1), equals_load=bool(same), estimate=est,
                              **{k: round(float(st[k]), 2) for k in stages})
            reads.close()
        ctx.set_knob("sample_bam_inflate", -1)
        whole.close()
        loaded.close()
        out[name] = row
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    a = sys.argv[1:]
    if len(a) in (2, 3) and a[0] == "--make":
        make(a[1], a[2] if len(a) == 3 else None)
    elif len(a) == 1:
        measure(a[0])
    elif len(a) >= 2 and a[1] == "--fetch" and (len(a) == 2 or (len(a) == 4 and a[2] == "--out")):
        measure_fetch(a[0], a[3] if len(a) == 4 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bg_fetch_probe.json"))
    else:
        sys.exit(__doc__)
