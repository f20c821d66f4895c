"""examples/build_locus_from_vcf.cpp with --index: the three diploid samples of tests/test_gpu_panvcf_example.py (part 2: quiet flanks,
-e 300,1000), their VCF embedded between two other contigs and written as BGZF with a tabix index. The run through the index
(lcty_vcf_indexed_open, lcty_vcf_indexed_fetch) must write what the run that reads the whole file writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from locityper_amd import io
from tests import panvcf_cases as PC
from tests import pyref_db as RD
from tests import vcf_index_cases as VC
from tests.test_gpu_db_example import K
from tests.test_gpu_example import build_example, ROOT
from tests.test_gpu_panvcf_example import vcf_of


def test_the_example_with_the_index_option_compiles_against_the_header(tmp_path):
    build_example(str(tmp_path / "build_locus_from_vcf"), "build_locus_from_vcf.cpp")
    src = open(os.path.join(ROOT, "examples", "build_locus_from_vcf.cpp")).read()
    assert "--index" in src and "lcty_vcf_indexed_fetch" in src


@pytest.mark.gpu
def test_the_index_route_writes_what_the_whole_file_route_writes(tmp_path):
    root = str(tmp_path / "lcty")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "make_locityper_dir.py"), root, "--alleles", "6", "--pairs", "200", "--base-len", "20000"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    names, seqs, off = io.fasta_read(os.path.join(root, "DB", "loci", "L1", "haplotypes.fa.gz"))
    haps = [bytes(seqs[int(off[i]):int(off[i + 1])]) for i in range(6)]
    exe = str(tmp_path / "build_locus_from_vcf")
    build_example(exe, "build_locus_from_vcf.cpp")
    src = tmp_path / "in"
    os.makedirs(src)
    rng = np.random.default_rng(31)
    flank, ref = 1500, haps[0]
    contig = PC.random_seq(rng, flank) + ref + PC.random_seq(rng, flank)
    samples, ploidy = ["S1", "S2", "S3"], [2, 2, 2]
    text, n_rows = vcf_of("chr1", ref, haps, flank, samples, ploidy)
    body = [l for l in text.split(b"\n") if l and not l.startswith(b"#")]
    assert n_rows == len(body) > 50

    # the locus's contig between two others: chr0 in front, chr10 behind, at the same positions
    def other(name, n):
        return [VC.rec(name, 100 + 40 * i, VC.seq(rng, 1 + i % 5), [VC.seq(rng, 1 + i % 3)], VC.random_calls(rng, ploidy, 1)) for i in range(n)]
    front, behind = other("chr0", 400), other("chr10", 400)
    mine = [VC.rec("chr1", int(l.split(b"\t")[1]) - 1, l.split(b"\t")[3], [l.split(b"\t")[4]], []) for l in body]
    vcf = str(src / "d.vcf.gz")
    info = VC.write_indexed(vcf, samples, front + mine + behind, block=4096, raw_lines={len(front) + i: l for i, l in enumerate(body)})
    assert len(VC.plan(info["tbi"], "chr1", 0, len(contig))) >= 1
    (src / "contig.fa").write_bytes(RD.multiline_fasta(["chr1"], [contig]))
    counts = rng.choice(np.array([0, 1, 1, 1, 3], dtype=np.uint16), len(contig) + 1 - K)
    (src / "contig.counts").write_bytes(RD.kmer_counts_save(K, 2, [counts]))

    runs = []
    for tag, extra in (("whole", []), ("index", ["--index"]), ("index_dev", ["--index", vcf + ".tbi", "--device-inflate"])):
        out = tmp_path / tag
        r = subprocess.run([exe, str(src / "contig.fa"), vcf, str(src / "contig.counts"), "chr1", str(flank), str(flank + len(ref)), "L2", str(out),
                            "--only-seqs", "-e", "300,1000", "--leave-out", "GRCh38"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        stats = json.loads(r.stdout.strip().split("\n")[-1])
        runs.append((stats, io.read_file(out / "loci" / "L2" / "haplotypes.fa.gz"), open(out / "loci" / "L2" / "ref.bed").read()))
    whole = runs[0]
    assert "fetch" not in whole[0] and whole[0]["haplotypes"] == 6 and whole[0]["kept_records"] > 50
    s, e = whole[0]["start"], whole[0]["end"]
    assert whole[1] == RD.multiline_fasta(["S1.1", "S1.2", "S2.1", "S2.2", "S3.1", "S3.2"], [contig[s:flank] + h + contig[flank + len(ref):e] for h in haps])
    for stats, fasta, bed in runs[1:]:
        assert fasta == whole[1] and bed == whole[2]
        for key in ("start", "end", "attempt", "haplotypes", "kept_records", "overlaps"):
            assert stats[key] == whole[0][key], key
        f = stats["fetch"]
        assert f["chunks"] >= 1 and f["records_kept"] == whole[0]["records"] and 0 < f["bytes_inflated"] < len(info["text"]) and f["file_bytes"] == info["file_bytes"]
