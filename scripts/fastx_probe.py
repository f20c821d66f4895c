"""Developer measurement: the two routes from FASTQ files to recruited reads at the shape of `locityper genotype -i R1 R2`:
   host     lcty_fastx_next (one thread: lines, records, pack) + lcty_recruit (upload, kernel)
   device   lcty_fastx_device_next (windows of text, lines / records / pack kernels) + lcty_fastx_device_recruit (the kernel, in place)
   python3 scripts/fastx_probe.py [--pairs 4000000] [--len 150] [--container plain|gz|bgzf] [--inflate host|device] [--runs 1]
One synthetic paired FASTQ is made: two files of `--pairs` records of `--len` bases, one pair in eight drawn from the alleles of the one
locus the targets hold, the rest random. Both routes run once to warm up (allocations, the page cache), then alternately `--runs`
times; before any time is printed the answers of the two routes must be equal, read for read. The stage times are printed and
appended to profiles/fastx_probe.json (--out), stamped with scripts/sources_sha.py. --inflate: knob "sample_bam_inflate" of the device
route (BGZF blocks: host zlib pool or the device's inflate kernel)."""
import argparse
import gzip
import hashlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from locityper_amd import api, io as lio  # noqa: E402
from sources_sha import sources_sha16  # noqa: E402

MAX_OUT = 8


def make_text(rng, alleles, first, n, length, mate):
    """records first .. first + n of one mate's file as bytes: @p<9 digits>/<mate>, bases, +, qualities; fixed width, so one array"""
    width = 14 + length + 3 + length + 1
    rec = np.empty((n, width), dtype=np.uint8)
    rec[:, 0] = ord("@"); rec[:, 1] = ord("p")
    ids = first + np.arange(n, dtype=np.int64)
    for d in range(9):
        rec[:, 2 + d] = ord("0") + (ids // 10 ** (8 - d)) % 10
    rec[:, 11] = ord("/"); rec[:, 12] = ord("0") + mate
    rec[:, 13] = ord("\n")
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, length))]
    drawn = np.flatnonzero(ids % 8 == 0)                                     # one pair in eight comes from an allele: forward and reverse mate, 300 apart
    al = alleles[0]
    start = np.random.default_rng(first).integers(0, len(al) - length - 400, len(drawn))
    if mate == 1:
        bases[drawn] = al[start[:, None] + np.arange(length)]
    else:
        comp = np.zeros(256, dtype=np.uint8)
        comp[list(b"ACGT")] = list(b"TGCA")
        bases[drawn] = comp[al[start[:, None] + 300 + np.arange(length)]][:, ::-1]
    rec[:, 14:14 + length] = bases
    rec[:, 14 + length] = ord("\n"); rec[:, 15 + length] = ord("+"); rec[:, 16 + length] = ord("\n")
    rec[:, 17 + length:17 + 2 * length] = rng.integers(35, 74, (n, length), dtype=np.uint8)
    rec[:, width - 1] = ord("\n")
    return rec.tobytes()


def make_files(d, ctx, pairs, length, container, alleles):
    paths = [os.path.join(d, f"r{m}.fq" + {"plain": "", "gz": ".gz", "bgzf": ".bgzf.gz"}[container]) for m in (1, 2)]
    t0 = time.perf_counter()
    size = 0
    for m, path in zip((1, 2), paths):
        rng = np.random.default_rng(100 + m)
        if container == "bgzf":                                              # whole file, deflated on the device
            text = b"".join(make_text(rng, alleles, f, min(500_000, pairs - f), length, m) for f in range(0, pairs, 500_000))
            lio.write_bgzf_device(ctx, path, text)
            size += len(text)
            continue
        with (gzip.open(path, "wb", compresslevel=1) if container == "gz" else open(path, "wb")) as out:
            for f in range(0, pairs, 500_000):
                text = make_text(rng, alleles, f, min(500_000, pairs - f), length, m)
                out.write(text); size += len(text)
    return paths, size, (time.perf_counter() - t0) * 1e3


def digest_of(h, cnt, loci):
    keep = np.arange(MAX_OUT)[None, :] < cnt[:, None]
    h[0].update(cnt.tobytes()); h[1].update(np.where(keep, loci, 0).astype(np.uint32).tobytes())     # two streams: the routes cut their chunks differently
    return int(cnt.astype(bool).sum())


def run_host(gt, paths, chunk):
    t = dict(ms_parse=0.0, ms_recruit=0.0)
    h, n, rec = (hashlib.sha1(), hashlib.sha1()), 0, 0
    t_all = time.perf_counter()
    f = lio.Fastx(paths[0], paths[1])
    while True:
        t0 = time.perf_counter()
        ch = f.next(chunk)
        t["ms_parse"] += (time.perf_counter() - t0) * 1e3
        if ch is None:
            break
        t0 = time.perf_counter()
        cnt, loci = gt.recruit(ch, paired=True, max_out=MAX_OUT)
        t["ms_recruit"] += (time.perf_counter() - t0) * 1e3
        n += ch.n_pairs; rec += digest_of(h, cnt, loci)
    f.close()
    t["ms_wall"] = (time.perf_counter() - t_all) * 1e3
    return t, n, rec, h[0].hexdigest() + h[1].hexdigest()


def run_device(ctx, gt, paths, chunk):
    t = dict(ms_recruit=0.0)
    h, n, rec = (hashlib.sha1(), hashlib.sha1()), 0, 0
    t_all = time.perf_counter()
    f = lio.FastxDevice(ctx, paths[0], paths[1])
    while f.next(chunk):
        t0 = time.perf_counter()
        cnt, loci = f.recruit(gt, max_out=MAX_OUT)
        t["ms_recruit"] += (time.perf_counter() - t0) * 1e3
        n += f.n; rec += digest_of(h, cnt, loci)
    t.update(f.stats)
    f.close()
    t["ms_wall"] = (time.perf_counter() - t_all) * 1e3
    return t, n, rec, h[0].hexdigest() + h[1].hexdigest()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--container", choices=("plain", "gz", "bgzf"), default="plain")
    ap.add_argument("--inflate", choices=("host", "device"), default="host")
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=1 << 20, help="read pairs a call")
    ap.add_argument("--window", type=int, default=-1, help='knob "fastx_window_bytes" (default 2^28)')
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastx_probe.json"))
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary directory)")
    a = ap.parse_args()
    if not 20 <= a.len <= 256:
        raise SystemExit("--len: 20 .. 256 (the pair kernel of recruitment takes mates of up to 256 bases)")
    ctx = api.Context(0)
    ctx.set_knob("sample_bam_inflate", 1 if a.inflate == "device" else 0)
    ctx.set_knob("fastx_window_bytes", a.window)
    rng = np.random.default_rng(1)
    alleles = [rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 20_000) for _ in range(4)]
    gt = api.Targets(ctx, api.recruit_params(paired=True))
    counts = [np.zeros(len(x) - 24, dtype=np.uint16) for x in alleles]
    gt.add_locus(np.concatenate(alleles), np.cumsum([0] + [len(x) for x in alleles]).astype(np.uint64), np.concatenate(counts),
                 np.cumsum([0] + [len(c) for c in counts]).astype(np.uint64), 25)
    gt.finalize()
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        paths, text_bytes, ms_make = make_files(d, ctx, a.pairs, a.len, a.container, alleles)
        file_bytes = sum(os.path.getsize(p) for p in paths)
        print(json.dumps(dict(made=paths, text_bytes=text_bytes, file_bytes=file_bytes, ms_make=round(ms_make))), flush=True)
        rows = {"host": [], "device": []}
        for r in range(a.runs + 1):                                          # round 0 warms both routes up
            th, nh, rh, dh = run_host(gt, paths, a.chunk)
            td, nd, rd, dd = run_device(ctx, gt, paths, a.chunk)
            if (nh, rh, dh) != (nd, rd, dd) or nh != a.pairs:
                raise SystemExit(f"the routes differ: host {nh} pairs, {rh} recruited, {dh}; device {nd} pairs, {rd} recruited, {dd}")
            if r:
                rows["host"].append(th); rows["device"].append(td)
    med = {k: {f: (round(statistics.median(x[f] for x in v), 3) if f.startswith("ms_") else v[-1][f]) for f in v[0]} for k, v in rows.items()}
    line = {"sources_sha": sources_sha16(ROOT), "pairs": a.pairs, "len": a.len, "container": a.container, "inflate": a.inflate, "runs": a.runs,
            "chunk": a.chunk, "window": a.window, "text_bytes": text_bytes, "file_bytes": file_bytes, "recruited": rh, "answers_equal": True,
            "host": med["host"], "device": med["device"],
            "pairs_per_s": {k: round(a.pairs / (med[k]["ms_wall"] * 1e-3)) for k in med}}
    print(json.dumps(line, indent=1))
    hist = json.load(open(a.out)) if os.path.exists(a.out) else []
    hist.append(line)
    with open(a.out, "w") as f:
        json.dump(hist, f, indent=1)
        f.write("\n")
