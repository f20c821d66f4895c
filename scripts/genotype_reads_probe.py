"""Developer measurement: one synthetic sample from its FASTQ files to mapped batches of every locus, on two routes:
   staged    lcty_fastx_device_recruit, lcty_fastx_device_write_recruited to LOCUS/reads.fq, lcty_fastx_open / lcty_fastx_next on that file
             again, lcty_reads_map_append of the host chunk — the seam of reads.fq between recruitment and the mapper;
   resident  lcty_fastx_device_recruit, lcty_recruited_add_fastx, lcty_reads_map_append_recruited — the reads stay on the device.
   python3 scripts/genotype_reads_probe.py [--pairs 20000] [--loci 8] [--calls 3] [--dir DIR]
The sample: --loci loci of three alleles of 5 000 bases, --pairs pairs of 150-base mates, three quarters of them drawn from the loci, in
two plain FASTQ files. After one warm call of each route the two are alternated --calls times; the records of every locus's batch
(lcty_reads_get_records) must be equal on both routes, or the script fails. One JSON line: the medians of the stage times in ms; it is
appended to profiles/genotype_reads_probe.json. No threshold is set on any of them."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def make_sample(d, n_pairs, n_loci, seed=11):
    rng = np.random.default_rng(seed)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    loci = []
    for _ in range(n_loci):
        base = rng.choice(list(b"ACGT"), 5000).astype(np.uint8)
        alleles = []
        for _ in range(3):
            s = base.copy(); m = rng.random(5000) < 0.01
            s[m] = rng.choice(list(b"ACGT"), int(m.sum()))
            alleles.append(bytes(s))
        loci.append(alleles)
    r1, r2 = os.path.join(d, "r1.fq"), os.path.join(d, "r2.fq")
    with open(r1, "wb") as a, open(r2, "wb") as b:
        for i in range(n_pairs):
            if i % 4 == 3:
                s1, s2 = (bytes(rng.choice(list(b"ACGT"), 150).astype(np.uint8)) for _ in range(2))
            else:
                al = loci[int(rng.integers(0, n_loci))][int(rng.integers(0, 3))]
                p = int(rng.integers(0, len(al) - 450))
                s1, s2 = al[p:p + 150], al[p + 300:p + 450].translate(comp)[::-1]
            a.write(b"@p%d\n%s\n+\n%s\n" % (i, s1, b"I" * 150))
            b.write(b"@p%d\n%s\n+\n%s\n" % (i, s2, b"I" * 150))
    return loci, r1, r2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20000)
    ap.add_argument("--loci", type=int, default=8)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    from locityper_amd import api, cdefs, io as lio
    d = a.dir or tempfile.mkdtemp(prefix="genotype_reads_probe_")
    os.makedirs(d, exist_ok=True)
    loci, r1, r2 = make_sample(d, a.pairs, a.loci)

    ctx = api.Context(0)
    bg = cdefs.Bg()
    import math
    for i, v in enumerate([math.log(0.995), math.log(0.003), math.log(0.001), math.log(0.001), math.log(0.003)]):
        bg.op_lnprobs[i] = v
    bg.edit_alpha, bg.edit_beta, bg.is_paired = 0.6, 90.0, 1
    bg.ins_n, bg.ins_p = 450.0 * 450.0 / (6400.0 - 450.0), 450.0 / 6400.0
    for i in range(cdefs.GC_BINS):
        bg.depth_n[i], bg.depth_p[i] = 20.0, 2.0 / 3.0
    bg.window, bg.neighb, bg.technology = 100, 300, cdefs.TECH_ILLUMINA
    bg.edit_kind, bg.edit_p1, bg.edit_p2 = cdefs.EDIT_FRACTION, 0.03, 0.06
    prm = api.resolve_params(api.default_params(), bg)
    targets = api.Targets(ctx, api.recruit_params(paired=True))
    locs = []
    mp = api.map_params()
    for alleles in loci:
        seqs = np.frombuffer(b"".join(alleles), dtype=np.uint8)
        seq_off = np.cumsum([0] + [len(x) for x in alleles]).astype(np.uint64)
        counts = np.zeros(sum(len(x) - 24 for x in alleles), dtype=np.uint16)
        cnt_off = np.cumsum([0] + [len(x) - 24 for x in alleles]).astype(np.uint64)
        targets.add_locus(seqs, seq_off, counts, cnt_off, 25)
        loc = api.Locus(ctx, seqs, seq_off, counts, cnt_off, 25, bg, prm)
        api.build_map_index(loc, [0, 1, 2], k=mp.k)
        locs.append(loc)
    targets.finalize()
    ms = lambda t0: (time.perf_counter() - t0) * 1e3

    def batch(l, n_pairs, n_bases):
        # room for the records of a locus: twelve per pair covers three alleles on both strands with their secondary records
        return api.AllAlignments(locs[l], max(n_pairs, 1), max(n_bases, 32), 12 * n_pairs + 64, 256 * n_pairs + 1024)

    def staged():
        t = dict(parse=0.0, recruit=0.0, write=0.0, reread=0.0, map=0.0)
        paths = [os.path.join(d, f"L{l}.reads.fq") for l in range(len(locs))]
        w = lio.FastxWriters(paths)
        dev = lio.FastxDevice(ctx, r1, r2)
        while True:
            t0 = time.perf_counter()
            n = dev.next(a.chunk)
            t["parse"] += ms(t0)
            if not n:
                break
            t0 = time.perf_counter()
            cnt, lc = dev.recruit(targets)
            t["recruit"] += ms(t0); t0 = time.perf_counter()
            dev.write_recruited(w, cnt, lc)
            t["write"] += ms(t0)
        t0 = time.perf_counter()
        w.close()
        t["write"] += ms(t0)
        dev.close()
        out = []
        for l, p in enumerate(paths):
            t0 = time.perf_counter()
            f = lio.Fastx(p, interleaved=True)
            chunk = f.next(1 << 40)
            t["reread"] += ms(t0); t0 = time.perf_counter()
            aa = batch(l, chunk.n_pairs if chunk else 0, chunk.n_bases if chunk else 0)
            if chunk is not None:
                api.map_append(aa, chunk, mp)
            t["map"] += ms(t0)
            out.append(aa.records())
            aa.close(); f.close()
        return t, out

    def resident():
        t = dict(parse=0.0, recruit=0.0, scatter=0.0, map=0.0)
        rset = api.Recruited(targets)
        dev = lio.FastxDevice(ctx, r1, r2)
        while True:
            t0 = time.perf_counter()
            n = dev.next(a.chunk)
            t["parse"] += ms(t0)
            if not n:
                break
            t0 = time.perf_counter()
            cnt, lc = dev.recruit(targets)
            t["recruit"] += ms(t0); t0 = time.perf_counter()
            dev.add_recruited(rset, cnt, lc)
            t["scatter"] += ms(t0)
        dev.close()
        out, recruited, resident_bytes = [], [], 0
        for l in range(len(locs)):
            n_pairs, n_bases = rset.sizes(l)
            recruited.append(n_pairs)
            resident_bytes += n_bases // 32 * cdefs.RECRUITED_UNIT_BYTES + n_pairs * cdefs.RECRUITED_PAIR_BYTES
            t0 = time.perf_counter()
            aa = batch(l, n_pairs, n_bases)
            api.map_append_recruited(aa, rset, l, mp)
            t["map"] += ms(t0)
            out.append(aa.records())
            aa.close()
        rset.close()
        return t, out, recruited, resident_bytes

    staged(); resident()                                                     # the warm call of each: allocations, code objects
    rows_s, rows_r = [], []
    for _ in range(a.calls):
        ts, recs_s = staged()
        tr, recs_r, recruited, resident_bytes = resident()
        for l, (x, y) in enumerate(zip(recs_s, recs_r)):
            if not all(np.array_equal(p, q) for p, q in zip(x, y)):
                raise SystemExit(f"locus {l}: the batches of the two routes differ")
        rows_s.append(ts); rows_r.append(tr)
    med = lambda rows: {k: round(float(np.median([r[k] for r in rows])), 3) for k in rows[0]}
    line = dict(pairs=a.pairs, loci=a.loci, chunk=min(a.chunk, a.pairs), calls=a.calls, recruited=recruited, bytes_resident=resident_bytes,
                staged_ms=med(rows_s), resident_ms=med(rows_r), batches_equal=True)
    line["staged_ms"]["seam"] = round(line["staged_ms"]["write"] + line["staged_ms"]["reread"], 3)
    print(json.dumps(line))
    with open(os.path.join(ROOT, "profiles", "genotype_reads_probe.json"), "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
