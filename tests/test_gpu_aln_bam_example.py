"""examples/genotype_dir.cpp --bam device: the locus's aln.bam read on the device and appended from there must end in the files the
host reader's route writes, byte for byte."""
import os
import subprocess
import sys

import pytest

from tests.test_gpu_example import ROOT, build_example


@pytest.mark.gpu
def test_genotype_dir_reads_aln_bam_on_the_device(tmp_path):
    root = str(tmp_path / "lcty")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "make_locityper_dir.py"), root, "--alleles", "6", "--pairs", "2000",
                        "--base-len", "20000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = str(tmp_path / "genotype_dir")
    build_example(exe, "genotype_dir.cpp")
    outd = os.path.join(root, "OUT", "loci", "L1")
    got = {}
    for how in ("host", "device"):
        r = subprocess.run([exe, root, "L1", "5", "--bam", how], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        got[how] = (r.stdout, open(os.path.join(outd, "res.json.gz"), "rb").read(), open(os.path.join(outd, "alns", "00.bam"), "rb").read(),
                    open(os.path.join(outd, "alns", "00.bam.bai"), "rb").read())
        for f in ("res.json.gz", "alns/00.bam", "alns/00.bam.bai"):
            os.remove(os.path.join(outd, f))
    assert got["host"] == got["device"] and got["host"][0].startswith("genotype ") and len(got["host"][2]) > 1000
    # without the output BAM nothing of the table is downloaded but its per-pair arrays: the call is the same
    r = subprocess.run([exe, root, "L1", "5", "--bam", "device", "--no-out-bam"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(os.path.join(outd, "res.json.gz"), "rb").read() == got["host"][1] and not os.path.exists(os.path.join(outd, "alns", "00.bam"))
    r = subprocess.run([exe, root, "L1", "5", "--bam", "neither"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
