"""examples/align_locus.cpp with --tr-div: haplotypes.fa.gz in, haplotypes.paf.gz out, line for line the PAF of the transliteration
tests/pyref_transitive.py, and `accelerated` / `rounds` in the JSON line."""
import gzip
import json
import subprocess

import pytest

from locityper_amd import io
from tests import pyref_align as R
from tests import transitive_cases as TC
from tests.test_gpu_example import build_example


@pytest.mark.gpu
def test_align_locus_tr_div_writes_the_paf_of_the_transliteration(gpu_ctx, tmp_path):
    c, want = TC.by_name("tree"), TC.expected("tree")
    seqs, off = c.arrays()
    fa = tmp_path / "haplotypes.fa.gz"
    io.write_gz(fa, io.fasta_text(c.names, seqs, off))
    exe = str(tmp_path / "align_locus")
    build_example(exe, "align_locus.cpp")
    out = tmp_path / "haplotypes.paf.gz"
    r = subprocess.run([exe, str(fa), str(out), "--all", "--tr-div", str(c.tr_div), "--tr-anchor", str(c.anchor), "-k", ",".join(map(str, c.ks))],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    lines = gzip.open(out, "rt").read().split("\n")
    assert lines[0] + "\n" == R.paf_header(ks=c.ks) and lines[-1] == "" and len(lines) == len(c.pairs) + 2
    for x, (ref, q) in enumerate(c.pairs):
        assert lines[x + 1] + "\n" == R.paf_line(c.names[q], len(c.seqs[q]), c.names[ref], len(c.seqs[ref]), (want["items"][x], want["score"][x]), want["div"][x])
    assert js["accelerated"] == sum(rt >= 2 for rt in want["route"]) > 0 and js["rounds"] == len(want["rounds"]) and js["pairs"] == len(c.pairs)
