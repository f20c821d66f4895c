"""examples/genotype_reads.cpp: a sample's reads in (two FASTQ files, or the indexed BAM of the same reads), res.json.gz of every locus out,
with the recruited reads resident on the device between recruitment and the mapper. For both inputs the file of each
locus must be, byte for byte, what the binding gives on the staged route with the same seed — recruit, select on the host
(tests/pyref_recruited.py), map_append, score, solve, lcty_res_to_json —, the call must be the genotype the reads were drawn from, and
alns/00.bam must hold exactly the names of the locus's recruited reads that lcty_write_bam writes: the used pairs (status GOOD) and those
with few unique k-mers (model/bam.rs:268-298) — most of the recruited pairs; one whose alignment leaves the inner part of the alleles has
no record there, as in the reference."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from locityper_amd import api, cdefs, io as lio
from tests import pyref_recruited as PR
from tests import pyref_sample_bam as PB
from tests import sample_bam_cases as SC
from tests.helpers import locus_arrays, make_bg, random_alleles
from tests.test_gpu_example import build_example
from tests.test_gpu_map_recruited import host_chunk
from tests.test_gpu_sample_bam_example import _locus_dir
from tests.test_oracle_recruit import revcomp

pytestmark = pytest.mark.gpu

SEED = 5
TRUTH = [(0, 2), (1, 1)]


def make_sample(tmp_path):
    """two locus directories, PREPROC/distr.gz, and the sample's reads as two FASTQ files and as an indexed BAM"""
    rng = np.random.default_rng(8)
    loci = [random_alleles(3, 3000, seed=31), random_alleles(3, 3000, seed=32)]
    dirs = [str(tmp_path / "DB" / "loci" / name) for name in ("LA", "LB")]
    _locus_dir(dirs[0], loci[0], "chrA\t0\t9000\tLA\n")
    _locus_dir(dirs[1], loci[1], "chrA\t0\t9000\tLB\n")
    bg = make_bg()
    os.makedirs(tmp_path / "PREPROC")
    distr = str(tmp_path / "PREPROC" / "distr.gz")
    with gzip.open(distr, "wt") as f:
        f.write(lio.bg_to_json(bg, 150.0))
    # 150 pairs from each haplotype of each locus's genotype, the loci alternating
    pairs = []
    for i in range(600):
        al = loci[i % 2][TRUTH[i % 2][(i // 2) % 2]]
        p = int(rng.integers(0, len(al) - 450))
        pairs.append((al[p:p + 150], revcomp(al[p + 300:p + 450])))
    names = [f"pair{i}" for i in range(len(pairs))]
    r1, r2, bam = str(tmp_path / "r1.fq"), str(tmp_path / "r2.fq.gz"), str(tmp_path / "sample.bam")
    with open(r1, "w") as a, gzip.open(r2, "wt") as b:
        for (s1, s2), nm in zip(pairs, names):
            a.write(f"@{nm} first mate\n{s1.decode()}\n+\n{'I' * 150}\n")
            b.write(f"@{nm}\n{s2.decode()}\n+\n{'5' * 150}\n")
    recs = [PB.rec(0, 100 + k, nm, 0x41, [("M", 150)], s1.decode(), bytes([40]) * 150, 0, 5000 + k) for k, ((s1, s2), nm) in enumerate(zip(pairs, names))]
    recs += [PB.rec(0, 5000 + k, nm, 0x81, [("M", 150)], s2.decode(), bytes([20]) * 150, 0, 100 + k) for k, ((s1, s2), nm) in enumerate(zip(pairs, names))]
    PB.write_bam(bam, SC.HAND_REFS, recs, block_size=4000)
    return loci, dirs, distr, pairs, names, r1, r2, bam


def test_genotype_reads_example_equals_the_staged_route(gpu_ctx, tmp_path):
    exe = str(tmp_path / "genotype_reads")
    build_example(exe, "genotype_reads.cpp")
    loci, dirs, distr, pairs, names, r1, r2, bam = make_sample(tmp_path)

    # ---- the staged route through the binding
    ctx = gpu_ctx
    bg_read, _ = lio.bg_from_json(gzip.open(distr, "rt").read())
    prm = api.resolve_params(api.default_params(), bg_read)
    targets = api.Targets(ctx, api.recruit_params(paired=True))
    arrays = [locus_arrays(alleles, 25) for alleles in loci]
    for seqs, seq_off, cflat, cnt_off, _ in arrays:
        targets.add_locus(seqs, seq_off, cflat, cnt_off, 25)
    targets.finalize()
    host = lio.Fastx(r1, r2)
    chunk = host.next(10_000)                                                # views into the reader: it is not asked again while they are in use
    assert chunk.n_pairs == len(pairs)
    cnt, out_loci = targets.recruit(chunk)
    E = PR.Expected(2)
    E.add(chunk, cnt, out_loci)
    mp = api.map_params()
    want_json, want_names, want_written = [], [], []
    for l, (seqs, seq_off, cflat, cnt_off, _) in enumerate(arrays):
        loc = api.Locus(ctx, seqs, seq_off, cflat, cnt_off, 25, bg_read, prm)
        api.build_map_index(loc, [0, 1, 2], k=mp.k)
        hc = host_chunk(E, l)
        assert hc.n_pairs >= 280
        sized = api.map_reads(loc, hc, mp)
        aa = api.AllAlignments(loc, hc.n_pairs, hc.n_bases, len(sized.recs), len(sized.cigar))
        api.map_append(aa, hc, mp)
        aa.score()
        call, mean, var, _ = api.solve_locus(aa, master_seed=SEED)
        ixs = [int(call.ixs[t]) for t in range(int(call.n_out))]
        gts = api.generate_genotypes(3, 2)
        want_json.append(lio.res_to_json(call, gts[ixs], [f"a{i}" for i in range(3)], mean[ixs], var[ixs]))
        assert tuple(int(x) for x in gts[ixs[0]]) == TRUTH[l]
        status = aa.status()[0]
        print(f"staged route, locus {l}: {hc.n_pairs} pairs, {int(call.n_good)} used, quality {call.quality:.3f}, status counts {np.bincount(status, minlength=4).tolist()}")
        recruited = [names[i] for i in range(len(pairs)) if l in out_loci[i, :cnt[i]]]
        written = [nm for nm, st in zip(recruited, status) if st in (cdefs.READ_GOOD, cdefs.READ_FEW_KMERS)]
        assert 0.7 * len(recruited) <= len(written) <= len(recruited)
        want_names.append(recruited)
        want_written.append(written)
        aa.close(); loc.close()
    targets.close(); host.close()

    # ---- the example, on the FASTQ files and on the BAM
    for k, inputs in enumerate((["-i", r1, r2], ["-a", bam, "--padding", "0", "--alt-contig", "5000"])):
        out = str(tmp_path / f"out{k}")
        r = subprocess.run([exe] + inputs + ["-p", distr, "-d", dirs[0], "-d", dirs[1] + "/", "--chunk", "128", "--map-chunk", "100", "--seed", str(SEED),
                                             "--out-bam", "-o", out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        stats = json.loads(r.stdout.strip().splitlines()[-1])
        print("example", inputs[0], stats)
        assert stats["reads"] == len(pairs) and stats["recruited"] == [len(n) for n in want_names]
        assert stats["bytes_resident"] == sum(len(n) for n in want_names) * (10 * PR.UNIT_BYTES + PR.PAIR_BYTES)
        for key in ("ms_parse", "ms_recruit", "ms_scatter", "ms_map", "ms_score", "ms_solve"):
            assert stats[key] >= 0
        for l, name in enumerate(("LA", "LB")):
            text = gzip.open(os.path.join(out, "loci", name, "res.json.gz"), "rt").read()
            assert text == want_json[l], (k, name)
            res = json.loads(text)
            assert res["genotype"] == ",".join(f"a{a}" for a in TRUTH[l]) and stats["calls"][l] == res["genotype"]
            _, bam_recs = PB.read_bam(os.path.join(out, "loci", name, "alns", "00.bam"))
            assert {rec["name"] for rec in bam_recs} == set(want_written[l]) <= set(want_names[l]), (k, name)
