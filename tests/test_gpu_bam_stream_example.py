"""The examples on whole BAM files without an index: examples/recruit_bam.cpp --no-index -^ over two files writes the
reads.fq that examples/recruit_reads.cpp --interleaved writes for the FASTQ of the same reads, and examples/genotype_reads.cpp
-a ... --no-index -^ writes the res.json.gz that it writes for -i ... --interleaved with the same seed."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from locityper_amd import io as lio
from tests import bam_stream_cases as BC
from tests import pyref_sample_bam as SB
from tests.helpers import make_bg, random_alleles
from tests.test_gpu_example import build_example
from tests.test_gpu_sample_bam_example import _locus_dir
from tests.test_oracle_recruit import revcomp

pytestmark = pytest.mark.gpu


def _sample(tmp_path, loci, truth, n_pairs):
    """n_pairs pairs drawn from the loci's genotypes (every fourth one foreign) as one interleaved FASTQ file and as two name-grouped BAM
    files: a.bam ends with a first mate and a supplementary record, b.bam begins with its second mate"""
    rng = np.random.default_rng(12)
    recs, fq = [], []
    for i in range(n_pairs):
        if i % 4 == 3:
            s1, s2 = BC.seq_of(rng, 150), BC.seq_of(rng, 150)
        else:
            al = loci[i % len(loci)][truth[i % len(loci)][(i // 2) % 2]]
            p = int(rng.integers(0, len(al) - 450))
            s1, s2 = al[p:p + 150].decode(), revcomp(al[p + 300:p + 450]).decode()
        q1, q2 = bytes(int(q) for q in rng.integers(2, 40, 150)), bytes(int(q) for q in rng.integers(2, 40, 150))
        rev = i % 3 == 0                                                       # mate 2 as an aligner left it: reverse-complemented, flag 0x10
        recs.append(SB.rec(-1, -1, f"pair{i}/1", 0x4D, [], s1, q1))
        if i % 9 == 0 or i == n_pairs // 2:
            recs.append(SB.rec(-1, -1, f"pair{i}/1", 0x804, [], s1[:40], q1[:40]))
        recs.append(SB.rec(-1, -1, f"pair{i}/2", 0x8D | (0x10 if rev else 0), [], revcomp(s2.encode()).decode() if rev else s2, q2[::-1] if rev else q2))
        fq.append(f"@pair{i}/1\n{s1}\n+\n{''.join(chr(q + 33) for q in q1)}\n@pair{i}/2\n{s2}\n+\n{''.join(chr(q + 33) for q in q2)}\n")
    cut = next(k for k, r in enumerate(recs) if r["name"] == f"pair{n_pairs // 2}/2")
    assert recs[cut - 1]["flag"] & 0x800 and recs[cut - 2]["name"] == f"pair{n_pairs // 2}/1"
    a, b, il = str(tmp_path / "a.bam"), str(tmp_path / "b.bam"), str(tmp_path / "il.fq")
    SB.write_bam(a, BC.REFS, recs[:cut], block_size=3000, index=False)
    SB.write_bam(b, BC.REFS, recs[cut:], block_size=0xff00, index=False)
    open(il, "w").write("".join(fq))
    return a, b, il


def test_recruit_bam_no_index_writes_what_recruit_reads_writes(tmp_path):
    bam_exe, fq_exe = str(tmp_path / "recruit_bam"), str(tmp_path / "recruit_reads")
    build_example(bam_exe, "recruit_bam.cpp")
    build_example(fq_exe, "recruit_reads.cpp")
    loci = [random_alleles(3, 3000, seed=41), random_alleles(3, 3000, seed=42)]
    dirs = [str(tmp_path / "DB" / "loci" / name) for name in ("LA", "LB")]
    _locus_dir(dirs[0], loci[0], "chr1\t10000\t13000\tLA\n")
    _locus_dir(dirs[1], loci[1], "chr1\t20000\t23000\tLB\n")
    a, b, il = _sample(tmp_path, loci, [(0, 2), (1, 1)], 300)
    out_fq, out_bam = str(tmp_path / "out_fq"), str(tmp_path / "out_bam")
    r = subprocess.run([fq_exe, "-i", il, "--interleaved", "-d", dirs[0], "-d", dirs[1], "--parse", "device", "-o", out_fq], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    want = [open(os.path.join(out_fq, name, "reads.fq"), "rb").read() for name in ("LA", "LB")]
    assert all(len(t) > 10_000 for t in want)
    for inflate in ("host", "device"):
        r = subprocess.run([bam_exe, "--no-index", "-^", "-a", a, "-a", b, "-d", dirs[0], "-d", dirs[1], "--inflate", inflate, "-o", out_bam],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        stats = json.loads(r.stdout.strip().splitlines()[-1])
        assert stats["interleaved"] == 1 and stats["files"] == 2 and stats["reads"] == 300 and stats["records_kept"] == 600 and stats["recruited"] >= 200
        assert stats["bytes_carried"] > 0 and stats["file_bytes"] == os.path.getsize(a) + os.path.getsize(b)
        assert [open(os.path.join(out_bam, name, "reads.fq"), "rb").read() for name in ("LA", "LB")] == want
    # without -^ every kept record is a read of its own; several files without --no-index are refused
    r = subprocess.run([bam_exe, "--no-index", "-a", a, "-a", b, "-d", dirs[0], "-o", str(tmp_path / "out_single")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and json.loads(r.stdout.strip().splitlines()[-1])["reads"] == 600, r.stdout + r.stderr
    r = subprocess.run([bam_exe, "-a", a, "-a", b, "-d", dirs[0], "-o", str(tmp_path / "out_none")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2


def test_genotype_reads_no_index_writes_the_same_result(tmp_path):
    exe = str(tmp_path / "genotype_reads")
    build_example(exe, "genotype_reads.cpp")
    loci = [random_alleles(3, 3000, seed=31)]
    d = str(tmp_path / "DB" / "loci" / "LA")
    _locus_dir(d, loci[0], "chr1\t0\t9000\tLA\n")
    os.makedirs(tmp_path / "PREPROC")
    distr = str(tmp_path / "PREPROC" / "distr.gz")
    with gzip.open(distr, "wt") as f:
        f.write(lio.bg_to_json(make_bg(), 150.0))
    a, b, il = _sample(tmp_path, loci, [(0, 2)], 300)
    texts = []
    for k, inputs in enumerate((["-i", il, "--interleaved"], ["-a", a, "-a", b, "--no-index", "-^"])):
        out = str(tmp_path / f"out{k}")
        r = subprocess.run([exe] + inputs + ["-p", distr, "-d", d, "--seed", "5", "-o", out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        stats = json.loads(r.stdout.strip().splitlines()[-1])
        assert stats["reads"] == 300 and stats["recruited"][0] >= 200
        texts.append(gzip.open(os.path.join(out, "loci", "LA", "res.json.gz"), "rt").read())
    assert texts[0] == texts[1] and json.loads(texts[0])["genotype"] == "a0,a2"
    # -^ must agree with the pairedness distr.gz was made from
    r = subprocess.run([exe, "-a", a, "--no-index", "-p", distr, "-d", d, "-o", str(tmp_path / "out_refused")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "distr.gz" in r.stderr
