"""examples/paf_to_vcf.cpp from compiled code, and the chain locus -> PAF -> VCF -> locus through compiled programs only: align_locus writes
the alignments of a make_locityper_dir.py locus, paf_to_vcf turns them into haplotypes.vcf.gz, build_locus_from_vcf rebuilds the haplotypes
from that file."""
import json
import os
import struct
import subprocess
import sys

import pytest

from locityper_amd import io
from tests import pyref_db as RD
from tests.test_gpu_example import build_example, ROOT


def test_paf_to_vcf_example_compiles_against_the_header(tmp_path):
    build_example(str(tmp_path / "paf_to_vcf"), "paf_to_vcf.cpp")


def run(cmd, timeout=300):
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


@pytest.mark.gpu
def test_locus_to_paf_to_vcf_and_back_to_the_locus(tmp_path):
    root = str(tmp_path / "lcty")
    n_alleles = 6
    run([sys.executable, os.path.join(ROOT, "scripts", "make_locityper_dir.py"), root, "--alleles", n_alleles, "--pairs", 200, "--base-len", 8000])
    db = os.path.join(root, "DB", "loci", "L1")
    names, seqs, off = io.fasta_read(os.path.join(db, "haplotypes.fa.gz"))
    haps = [bytes(seqs[int(off[i]):int(off[i + 1])]) for i in range(n_alleles)]
    assert names == [f"a{i}" for i in range(n_alleles)]
    for exe in ("align_locus", "paf_to_vcf", "build_locus_from_vcf"):
        build_example(str(tmp_path / exe), exe + ".cpp")
    for old in ("haplotypes.paf", "haplotypes.paf.gz", "haplotypes.paf.br", "discarded_haplotypes.txt", "ref.bed"):
        if os.path.exists(os.path.join(db, old)):
            os.remove(os.path.join(db, old))

    # 1. the alignments of all pairs, then the VCF with the defaults of -i: DIR/haplotypes.vcf.gz, a BGZF file
    run([tmp_path / "align_locus", os.path.join(db, "haplotypes.fa.gz"), os.path.join(db, "haplotypes.paf.gz"), "--all"])
    r = run([tmp_path / "paf_to_vcf", "-i", db, "-r", "a0"])
    stats = json.loads(r.stdout.strip().splitlines()[-1])
    assert (stats["haplotypes"], stats["samples"], stats["missing"], stats["bad_len"]) == (n_alleles, n_alleles - 1, 0, 0)
    assert stats["entries"] == n_alleles * (n_alleles - 1) // 2 and stats["variants"] > 0 and 0 < stats["lines_merged"] <= stats["merged"]
    vcf = os.path.join(db, "haplotypes.vcf.gz")
    raw = open(vcf, "rb").read()
    assert raw[:4] == b"\x1f\x8b\x08\x04" and raw[12:14] == b"BC" and struct.unpack_from("<H", raw, 16)[0] + 1 <= len(raw)
    assert raw.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    text = io.read_file(vcf)
    assert text.startswith(b"##fileformat=VCFv4.2\n") and b"\tFORMAT\ta1\ta2\ta3\ta4\ta5\n" in text and text.count(b"\n") == 3 + stats["lines_merged"]
    assert stats["merged_bytes"] == len(text) and not [f for f in os.listdir(db) if f.endswith(".tmp")]

    # 2. back: the reference haplotype a0 as the contig, every other haplotype a haploid sample of the VCF
    src = tmp_path / "in"
    os.makedirs(src)
    (src / "ref.fa").write_bytes(RD.multiline_fasta(["a0"], [haps[0]]))
    out = tmp_path / "DB2"
    run([tmp_path / "build_locus_from_vcf", src / "ref.fa", vcf, "-", "a0", "0", len(haps[0]), "L1", out, "--only-seqs", "-e", "0", "-g", "a0"])
    names2, seqs2, off2 = io.fasta_read(out / "loci" / "L1" / "haplotypes.fa.gz")
    assert names2 == names and [bytes(seqs2[int(off2[i]):int(off2[i + 1])]) for i in range(n_alleles)] == haps

    # 3. the lookup order of -i (.br before .gz), ref.bed as the region (-R auto), a plain and a separate output
    io.write_br(os.path.join(db, "haplotypes.paf.br"), io.read_file(os.path.join(db, "haplotypes.paf.gz")))
    io.write_gz(os.path.join(db, "haplotypes.paf.gz"), b"not a PAF line\n")                 # must not be looked at
    open(os.path.join(db, "ref.bed"), "w").write(f"chr3\t1000\t{1000 + len(haps[0])}\tL1\n")
    m, s = tmp_path / "m.vcf", tmp_path / "s.vcf.gz"
    r = run([tmp_path / "paf_to_vcf", "-i", db, "-r", "a0", "-d", "none", "-o", m, s])
    js = json.loads(r.stdout.strip().splitlines()[-1])
    body = [line for line in text.split(b"\n") if line and not line.startswith(b"#")]
    plain = [line for line in m.read_bytes().split(b"\n") if line and not line.startswith(b"#")]
    assert len(plain) == len(body) and js["lines_separate"] >= js["lines_merged"] and io.read_file(s).count(b"\n") == 3 + js["lines_separate"]
    for a, b in zip(body, plain):
        fa, fb = a.split(b"\t"), b.split(b"\t")
        assert fb[0] == b"chr3" and int(fb[1]) == int(fa[1]) + 1000 and fa[2:] == fb[2:]
    # the same region spelled out; chrom:start alone is an input error
    m2 = tmp_path / "m2.vcf"
    run([tmp_path / "paf_to_vcf", "-p", os.path.join(db, "haplotypes.paf.br"), "-f", os.path.join(db, "haplotypes.fa.gz"), "-r", "a0", "-o", m2,
         "-R", f"chr3:1,001-{1000 + len(haps[0])}"])
    assert m2.read_bytes() == m.read_bytes()
    bad = subprocess.run([str(tmp_path / "paf_to_vcf"), "-i", db, "-r", "a0", "-R", "chr3:1001"], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "chrom:start-end" in bad.stderr
