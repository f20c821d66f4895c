"""examples/align_locus.cpp from compiled code: haplotypes.fa.gz in, haplotypes.paf.gz and one JSON line out; the file must be exactly
io.paf_write of api.align_haplotypes."""
import json
import subprocess

import numpy as np
import pytest

from locityper_amd import api, io
from tests import align_cases as AC
from tests.test_gpu_example import build_example


def test_align_locus_example_compiles_against_the_header(tmp_path):
    build_example(str(tmp_path / "align_locus"), "align_locus.cpp")


@pytest.mark.gpu
def test_align_locus_example_writes_the_paf_of_the_api(gpu_ctx, tmp_path):
    c = AC.by_name("subs")
    seqs, off = c.arrays()
    fa = tmp_path / "haplotypes.fa.gz"
    io.write_gz(fa, io.fasta_text(c.names, seqs, off))
    exe = str(tmp_path / "align_locus")
    build_example(exe, "align_locus.cpp")
    out = tmp_path / "haplotypes.paf.gz"
    r = subprocess.run([exe, str(fa), str(out), "--all"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    ref, query = api.align_all_pairs(len(c.seqs))
    res, st = api.align_haplotypes(gpu_ctx, seqs, off, ref, query)
    assert io.read_file(out) == io.paf_write(c.names, off, ref, query, res)
    assert js["pairs"] == 6 and js["aligned"] == st["n_aligned"] == 6 and js["kmer_matches"] == st["n_kmer_matches"] and js["ms"]["total"] > 0
    assert len(io.paf_read(out, c.names)) == 6

    # --pairs-file (`query ref`, duplicates dropped whatever their order) and --against
    pf = tmp_path / "pairs.txt"
    pf.write_text(f"# query ref\n{c.names[2]} {c.names[0]}\n{c.names[0]} {c.names[2]}\n{c.names[3]}\t{c.names[1]}\n")
    out2 = tmp_path / "some.paf.gz"
    r = subprocess.run([exe, str(fa), str(out2), "--pairs-file", str(pf), "--against", c.names[3], "-k", "25,51"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    ref2, query2 = np.array([0, 1, 3, 3], dtype=np.uint32), np.array([2, 3, 0, 2], dtype=np.uint32)
    p = api.align_params(backbone_ks=[25, 51])
    against = np.array([0, 0, 0, 1], dtype=np.uint8)
    res2, _ = api.align_haplotypes(gpu_ctx, seqs, off, ref2, query2, p, against=against)
    assert io.read_file(out2) == io.paf_write(c.names, off, ref2, query2, res2, p)
