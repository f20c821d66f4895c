"""examples/build_locus_from_vcf.cpp from compiled code: a reference window, a phased VCF and k-mer counts in, DB/loci/<locus>/ with
ref.bed out. The VCF is derived inside the test from the alleles of a make_locityper_dir.py locus by a planted list of replacements
against allele 0 (no aligner: the truth is the alleles themselves); the directory written must carry a genotype_dir run to the true
genotype."""
import gzip
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from locityper_amd import io
from tests import panvcf_cases as PC
from tests import pyref_db as RD
from tests.test_gpu_db_example import _genome_counts, K
from tests.test_gpu_example import build_example, ROOT


def test_build_locus_from_vcf_example_compiles_against_the_header(tmp_path):
    build_example(str(tmp_path / "build_locus_from_vcf"), "build_locus_from_vcf.cpp")


def planted_records(ref, allele, shift, step=500, anchor=24):
    """Replacements that turn `ref` into `allele`: the two are cut where a 24-mer of `ref` on a 500-base grid occurs once in both, and
    every piece that differs is one record (pos + shift, [REF piece, ALT piece]). Their concatenation is the allele by construction."""
    cuts = [(0, 0)]
    for c in range(step, len(ref) - anchor, step):
        a = ref[c:c + anchor]
        j = allele.find(a, cuts[-1][1])
        if j >= 0 and ref.count(a) == 1 and allele.count(a) == 1:
            cuts.append((c, j))
    cuts.append((len(ref), len(allele)))
    recs = []
    for (c0, j0), (c1, j1) in zip(cuts, cuts[1:]):
        if ref[c0:c1] != allele[j0:j1]:
            assert j1 > j0
            recs.append((c0 + shift, [ref[c0:c1], allele[j0:j1]]))
    assert b"".join(allele[j0:j1] for (_, j0), (_, j1) in zip(cuts, cuts[1:])) == allele
    return recs


def vcf_of(contig, ref, alleles, shift, samples, ploidy):
    """One record per (allele, piece); gt column c carries the records of alleles[c]."""
    rows = []
    for c, al in enumerate(alleles):
        rows += [(rec, c) for rec in planted_records(ref, al, shift)]
    rows.sort(key=lambda x: (x[0][0], x[1]))
    gt = np.zeros((len(rows), len(alleles)), dtype=np.int16)
    for i, (_, c) in enumerate(rows):
        gt[i, c] = 1
    return PC.vcf_text(contig, [r for r, _ in rows], samples, ploidy, gt), len(rows)


@pytest.mark.gpu
def test_build_locus_from_vcf_example_writes_a_directory_that_genotyping_accepts(tmp_path):
    root = str(tmp_path / "lcty")
    n_alleles = 6
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "make_locityper_dir.py"), root, "--alleles", str(n_alleles), "--pairs", "5000",
                        "--base-len", "20000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    db = os.path.join(root, "DB", "loci", "L1")
    names, seqs, off = io.fasta_read(os.path.join(db, "haplotypes.fa.gz"))
    haps = [bytes(seqs[int(off[i]):int(off[i + 1])]) for i in range(n_alleles)]
    assert names == [f"a{i}" for i in range(n_alleles)] and len(set(haps)) == n_alleles
    exe = str(tmp_path / "build_locus_from_vcf")
    build_example(exe, "build_locus_from_vcf.cpp")
    src = tmp_path / "in"
    os.makedirs(src)

    # 1. the names of aln.bam: the reference is a0 (-g a0), a1 .. a5 are haploid samples; the locus is the whole of a0, no expansion (-e 0)
    ref = haps[0]
    text, n_rows = vcf_of("chr1", ref, haps[1:], 0, names[1:], [1] * 5)
    assert n_rows > 50
    (src / "a.vcf.gz").write_bytes(PC.bgzf(text))
    (src / "ref.fa").write_bytes(RD.multiline_fasta(["chr1"], [ref]))
    tables, _, _ = _genome_counts(haps, ref)
    (src / "haps.counts").write_bytes(RD.kmer_counts_save(K, 2, tables))
    out = tmp_path / "DB2"
    r = subprocess.run([exe, str(src / "ref.fa"), str(src / "a.vcf.gz"), "-", "chr1", "0", str(len(ref)), "L1", str(out), "--hap-counts", str(src / "haps.counts"),
                        "-e", "0", "-g", "a0", "--calc-div"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    stats = json.loads(r.stdout.strip().split("\n")[-1])
    built = out / "loci" / "L1"
    want = RD.build_locus(names, haps, ref, tables, K, 2, 15, 15, True)
    assert io.read_file(built / "haplotypes.fa.gz") == want["fasta"]                 # sequence for sequence the planted alleles, under their names
    assert io.read_file(built / "kmers.bin.br") == want["kmers"] and open(built / "distances.bin", "rb").read() == want["distances"]
    assert open(built / "ref.bed").read() == f"chr1\t0\t{len(ref)}\tL1\n"
    assert (stats["start"], stats["end"], stats["haplotypes"], stats["written"], stats["kept_records"], stats["overlaps"]) == (0, len(ref), 6, 6, n_rows, 0)
    os.remove(os.path.join(db, "kmers.bin.lz4"))                                     # genotype_dir prefers .lz4 over .br
    for f in ("haplotypes.fa.gz", "kmers.bin.br", "distances.bin"):
        shutil.copy(built / f, os.path.join(db, f))
    gexe = str(tmp_path / "genotype_dir")
    build_example(gexe, "genotype_dir.cpp")
    r = subprocess.run([gexe, root, "L1", "5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    truth = json.load(open(os.path.join(root, "truth.json")))
    res = json.load(gzip.open(os.path.join(root, "OUT", "loci", "L1", "res.json.gz"), "rt"))
    assert res["genotype"] == ",".join(truth["genotype"])

    # 2. the six alleles as three diploid samples on a contig with quiet flanks: the reference is left out, the locus may expand
    rng = np.random.default_rng(31)
    flank = 1500
    contig = PC.random_seq(rng, flank) + ref + PC.random_seq(rng, flank)
    text, _ = vcf_of("chr1", ref, haps, flank, ["S1", "S2", "S3"], [2, 2, 2])
    (src / "d.vcf").write_bytes(text)
    (src / "contig.fa").write_bytes(RD.multiline_fasta(["chr1"], [contig]))
    counts = rng.choice(np.array([0, 1, 1, 1, 3], dtype=np.uint16), len(contig) + 1 - K)
    (src / "contig.counts").write_bytes(RD.kmer_counts_save(K, 2, [counts]))
    out = tmp_path / "DB3"
    r = subprocess.run([exe, str(src / "contig.fa"), str(src / "d.vcf"), str(src / "contig.counts"), "chr1", str(flank), str(flank + len(ref)), "L2", str(out),
                        "--only-seqs", "-e", "300,1000", "--leave-out", "GRCh38"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    stats = json.loads(r.stdout.strip().split("\n")[-1])
    s, e = stats["start"], stats["end"]
    assert flank - 300 <= s <= flank and flank + len(ref) <= e <= flank + len(ref) + 300 and stats["attempt"] == 0 and stats["left_out"] == 1
    hnames = ["S1.1", "S1.2", "S2.1", "S2.2", "S3.1", "S3.2"]
    assert io.read_file(out / "loci" / "L2" / "haplotypes.fa.gz") == RD.multiline_fasta(hnames, [contig[s:flank] + h + contig[flank + len(ref):e] for h in haps])
    assert open(out / "loci" / "L2" / "ref.bed").read() == f"chr1\t{s}\t{e}\tL2\n"
    assert not os.path.exists(out / "loci" / "L2" / "kmers.bin.br")
