"""examples/recruit_bam.cpp: a sample's BAM + BAI and two locus directories in, per-locus read files out — the same bytes the Python
binding of the same entry points writes, and files lcty_fastx_open reads back."""
import gzip
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from locityper_amd import api, io as lio
from tests import pyref_sample_bam as P
from tests import sample_bam_cases as S
from tests.test_gpu_example import build_example
from tests.test_gpu_sample_bam import _two_loci

pytestmark = pytest.mark.gpu


def _varint(v):
    out = bytearray()
    while True:
        b = v & 0x7F; v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def _locus_dir(path, alleles, bed_line, k=25):
    """haplotypes.fa.gz, kmers.bin.lz4 (one KmerCounts block of zeros in a stored LZ4 frame, seq/counts.rs:108-150) and ref.bed"""
    os.makedirs(path)
    with gzip.open(os.path.join(path, "haplotypes.fa.gz"), "wt") as f:
        for i, a in enumerate(alleles):
            f.write(f">a{i}\n{a.decode()}\n")
    block = bytes([k, 2]) + _varint(len(alleles)) + b"".join(_varint(len(a) - k + 1) + b"\0" * (len(a) - k + 1) for a in alleles)
    frame = struct.pack("<I", 0x184D2204) + bytes([0x60, 0x70, 0x73]) + struct.pack("<I", len(block) | 0x80000000) + block + struct.pack("<I", 0)
    open(os.path.join(path, "kmers.bin.lz4"), "wb").write(frame)
    open(os.path.join(path, "ref.bed"), "w").write(bed_line)


def test_recruit_bam_example(tmp_path):
    exe = str(tmp_path / "recruit_bam")
    build_example(exe, "recruit_bam.cpp")
    loci = _two_loci()
    recs = S.seeded_records(loci=loci)
    bam_path = str(tmp_path / "sample.bam")
    P.write_bam(bam_path, S.SEEDED_REFS, recs, block_size=2048)
    # the loci "lie" in the first and the fourth region of the seeded file; padding 0 and merge distance 1000 give these regions back
    dirs = [str(tmp_path / "DB" / "loci" / name) for name in ("LA", "LB")]
    _locus_dir(dirs[0], loci[0], "c0\t10000\t18000\tLA\n")
    _locus_dir(dirs[1], loci[1], "c1\t20000\t26000\tLB\n")
    out = str(tmp_path / "out")
    r = subprocess.run([exe, "-a", bam_path, "-d", dirs[0], "-d", dirs[1] + "/", "--padding", "0", "--alt-contig", "5000", "-o", out],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    stats = json.loads(r.stdout.strip().splitlines()[-1])
    regions = P.postprocess_targets([(0, 10_000, 18_000), (1, 20_000, 26_000)], [ln for _, ln in S.SEEDED_REFS], 0, 5000, 1000)
    assert regions == [(0, 10_000, 18_000), (1, 20_000, 26_000), (2, 0, 3_000)]
    src, mates, n_kept, n_discarded = S.expected(recs, regions, True, True)
    assert stats["paired"] == 1 and stats["regions"] == 3 and stats["pairs"] == len(mates) and stats["records_kept"] == n_kept and stats["discarded"] == n_discarded
    # the same through the binding
    ctx = api.Context(0)
    gt = api.Targets(ctx, api.recruit_params(paired=True))
    for alleles in loci:
        counts = [np.zeros(len(a) - 24, dtype=np.uint16) for a in alleles]
        gt.add_locus(np.frombuffer(b"".join(alleles), dtype=np.uint8), np.cumsum([0] + [len(a) for a in alleles]).astype(np.uint64),
                     np.concatenate(counts), np.cumsum([0] + [len(c) for c in counts]).astype(np.uint64), 25)
    gt.finalize()
    reads = lio.SampleBam(bam_path).fetch(ctx, regions, with_unmapped=True)
    cnt, out_loci = reads.recruit(gt)
    paths = [str(tmp_path / f"api{k}.fq") for k in range(2)]
    w = lio.FastxWriters(paths)
    n = reads.write_recruited(w, cnt, out_loci)
    w.close()
    assert stats["recruited"] == n > 50
    for k, name in enumerate(("LA", "LB")):
        got = open(os.path.join(out, name, "reads.fq"), "rb").read()
        assert got == open(paths[k], "rb").read() and len(got) > 1000
        fx = lio.Fastx(os.path.join(out, name, "reads.fq"), interleaved=True)          # the chunk is a view into the handle
        back = fx.next(1 << 20)
        sel = [i for i in range(len(mates)) if k in out_loci[i, :cnt[i]].tolist()]
        ml, _, b2, nm = P.packed([mates[i] for i in sel])
        assert back.mate_len.tolist() == ml.tolist() and np.array_equal(back.bases2[:len(b2)], b2) and np.array_equal(back.nmask[:len(nm)], nm)
