"""examples/estimate_bg.cpp from compiled code: a BAM, a FASTA and a k-mer count file in, PREPROC/distr.gz out; the file must read back
as what the Python API estimates and carry a genotyping run of examples/genotype_dir.cpp."""
import gzip
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from locityper_amd import api, io
from tests import bg_synth
from tests.test_gpu_example import build_example, ROOT


def test_estimate_bg_example_compiles_against_the_header(tmp_path):
    build_example(str(tmp_path / "estimate_bg"), "estimate_bg.cpp")


@pytest.mark.gpu
def test_estimate_bg_example_writes_a_distr_that_genotyping_accepts(tmp_path):
    s = bg_synth.Sample()
    bam = s.write(tmp_path / "bg.bam")
    fa = tmp_path / "padded.fa"
    with open(fa, "w") as f:
        f.write(f">{s.contig}:{s.padded_start + 1}-{s.padded_start + s.padded_len()}\n")
        seq = s.padded_seq.decode()
        for i in range(0, len(seq), 80):
            f.write(seq[i:i + 80] + "\n")
    cnt = tmp_path / "padded.u16"
    s.kmer_counts.astype("<u2").tofile(cnt)
    exe = str(tmp_path / "estimate_bg")
    build_example(exe, "estimate_bg.cpp")
    out = tmp_path / "PREPROC"
    r = subprocess.run([exe, str(bam), str(fa), str(cnt), f"{s.contig}:{s.start + 1}-{s.end}", "illumina", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    text = gzip.open(out / "distr.gz", "rt").read()
    bg, rl = io.bg_from_json(text)
    reads = api.read_bg_bam(bam, s.contig, s.start, s.end, s.padded_start, s.padded_len(), api.bg_params())
    bg2, rl2, _ = api.estimate_bg(api.Context(0), reads, s.padded_seq, s.padded_start, s.kmer_counts, s.k, s.start, s.end, api.bg_params(),
                                  with_diag=False)
    assert bytes(bg) == bytes(bg2) and rl == rl2

    root = str(tmp_path / "lcty")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "make_locityper_dir.py"), root, "--alleles", "8", "--pairs", "6000",
                        "--base-len", "30000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    shutil.copy(out / "distr.gz", os.path.join(root, "PREPROC", "distr.gz"))
    gexe = str(tmp_path / "genotype_dir")
    build_example(gexe, "genotype_dir.cpp")
    r = subprocess.run([gexe, root, "L1", "5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    res = os.path.join(root, "OUT", "loci", "L1", "res.json.gz")
    assert os.path.getsize(res) > 0 and r.stdout.startswith("genotype ")
