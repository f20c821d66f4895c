"""examples/build_basis.cpp from compiled code: a locus directory with haplotypes.fa.gz and haplotypes.paf.gz in,
haplotypes-basis.<tag>.fa.gz (and the default symlink) out; the file must hold exactly the API's basis."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from locityper_amd import api, io, synth
from tests.test_gpu_example import build_example, ROOT

# 12 alleles of 6 000 bases; divergence 0.004 over windows of 250 (at most one edit): a basis of several, not all, haplotypes
N_ALLELES, BASE_LEN, DIV, WINDOW = 12, 6000, 0.004, 250


def test_build_basis_example_compiles_against_the_header(tmp_path):
    build_example(str(tmp_path / "build_basis"), "build_basis.cpp")


@pytest.mark.gpu
def test_build_basis_example_writes_the_basis_of_the_api(tmp_path):
    root = str(tmp_path / "lcty")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "make_locityper_dir.py"), root, "--alleles", str(N_ALLELES), "--pairs", "2000",
                        "--base-len", str(BASE_LEN), "--paf"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    db = os.path.join(root, "DB", "loci", "L1")
    names, seqs, off = io.fasta_read(os.path.join(db, "haplotypes.fa.gz"))
    lens = np.diff(off.astype(np.int64))
    ents = io.paf_read(os.path.join(db, "haplotypes.paf.gz"), names)
    assert len(ents) == N_ALLELES * (N_ALLELES - 1) // 2
    ctx = api.Context(0)
    p = api.basis_params(divergence=DIV, window=WINDOW)
    ids, bound, optimal, st = api.basis_build(ctx, lens, ents, p)
    assert 1 < len(ids) < N_ALLELES and optimal and st["n_rows_unique"] > N_ALLELES

    exe = str(tmp_path / "build_basis")
    build_example(exe, "build_basis.cpp")
    r = subprocess.run([exe, db, "-x", str(DIV), "-w", str(WINDOW), "--default"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    tag = api.basis_tag(p)
    assert tag == "x0.004-w250" and out["tag"] == tag
    assert out["basis"] == [int(i) for i in ids] and out["names"] == [names[i] for i in ids]
    assert out["bound"] == bound and out["optimal"] is True
    path = os.path.join(db, f"haplotypes-basis.{tag}.fa.gz")
    n2, s2, o2 = io.fasta_read(path)
    assert n2 == [names[i] for i in ids]                                          # ascending id order
    for t, i in enumerate(ids):
        assert np.array_equal(s2[int(o2[t]):int(o2[t + 1])], seqs[int(off[i]):int(off[i + 1])])
    assert io.read_file(path) == api.basis_fasta(names, seqs, off, ids)
    link = os.path.join(db, "haplotypes-basis.fa.gz")
    assert os.path.islink(link) and os.readlink(link) == f"haplotypes-basis.{tag}.fa.gz"
    assert io.fasta_read(link)[0] == n2                                           # the symlink resolves

    # --basis-lo: the named haplotype is not in the basis, the ids are those of the full set, the tag says so
    r = subprocess.run([exe, db, "-x", str(DIV), "-w", str(WINDOW), "--basis-lo", names[int(ids[0])]], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    out_lo = json.loads(r.stdout.strip().splitlines()[-1])
    ids_lo = api.basis_build(ctx, lens, ents, p, leave_out=[int(ids[0])])[0]
    assert out_lo["basis"] == [int(i) for i in ids_lo] and int(ids[0]) not in out_lo["basis"]
    assert out_lo["tag"] == f"{tag}-lo{names[int(ids[0])]}" and os.path.exists(os.path.join(db, f"haplotypes-basis.{out_lo['tag']}.fa.gz"))

    # the ids are what candidate generation takes as its basis
    L = synth.SynthLocus(N_ALLELES, 2000, base_len=BASE_LEN)
    assert np.array_equal(L.seqs, seqs)
    prm = api.resolve_params(api.default_params(), L.bg)
    loc = api.Locus(ctx, L.seqs, L.seq_off, L.counts, L.cnt_off, L.k, L.bg, prm)
    api.build_map_index(loc, ids)
