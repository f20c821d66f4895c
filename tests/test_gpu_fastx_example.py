"""examples/recruit_reads.cpp: two FASTQ files (or one interleaved file) and two locus directories in, per-locus read files out: the
device route (--parse device) and the host route (--parse host) write the same files, and they hold what the binding recruits."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from locityper_amd import api, io as lio
from tests.test_gpu_example import build_example
from tests.test_gpu_sample_bam import _two_loci
from tests.test_gpu_sample_bam_example import _locus_dir
from tests.test_oracle_recruit import revcomp

pytestmark = pytest.mark.gpu


def test_recruit_reads_example_both_routes_write_the_same_files(tmp_path):
    exe = str(tmp_path / "recruit_reads")
    build_example(exe, "recruit_reads.cpp")
    loci = _two_loci()
    rng = np.random.default_rng(4)
    dirs = [str(tmp_path / "DB" / "loci" / name) for name in ("LA", "LB")]
    _locus_dir(dirs[0], loci[0], "c0\t10000\t13000\tLA\n")
    _locus_dir(dirs[1], loci[1], "c1\t20000\t23000\tLB\n")
    r1, r2, il = str(tmp_path / "r1.fq.gz"), str(tmp_path / "r2.fq"), str(tmp_path / "il.fq")
    qual = lambda n: "".join(chr(33 + int(q)) for q in rng.integers(2, 40, n))
    with gzip.open(r1, "wt") as a, open(r2, "w") as b, open(il, "w") as c:
        for i in range(400):
            if i % 4 == 3:                                                   # a foreign pair
                s1, s2 = (bytes(rng.choice(list(b"ACGT"), 150).astype(np.uint8).tolist()) for _ in range(2))
            else:
                al = loci[i % 2][int(rng.integers(0, 3))]
                p = int(rng.integers(0, len(al) - 500))
                s1, s2 = al[p:p + 150], revcomp(al[p + 300:p + 450])
            t1 = f"@pair{i}/1 first mate\n{s1.decode()}\n+\n{qual(150)}\n"
            t2 = f"@pair{i}/2\n{s2.decode()}\n+\n{qual(150)}\n"
            a.write(t1); b.write(t2); c.write(t1 + t2)
    outs = {}
    for inputs, extra in (([r1, r2], []), ([il], ["--interleaved"])):
        for parse in ("device", "host"):
            out = str(tmp_path / f"out_{parse}_{len(inputs)}")
            r = subprocess.run([exe, "-i"] + inputs + extra + ["-d", dirs[0], "-d", dirs[1] + "/", "--parse", parse, "--chunk", "96", "--window", "20000",
                                                               "-o", out], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout + r.stderr
            stats = json.loads(r.stdout.strip().splitlines()[-1])
            assert stats["parse"] == parse and stats["paired"] == 1 and stats["reads"] == 400 and stats["recruited"] >= 250
            if parse == "device":
                assert stats["records"] == 800 and stats["windows"] > 4 and stats["bytes_read"] == sum(os.path.getsize(p) for p in inputs)
            outs[parse, len(inputs)] = [open(os.path.join(out, name, "reads.fq"), "rb").read() for name in ("LA", "LB")]
    assert outs["device", 2] == outs["host", 2] == outs["device", 1] == outs["host", 1]
    assert all(len(t) > 10_000 for t in outs["device", 2])
    # the same through the binding
    ctx = api.Context(0)
    gt = api.Targets(ctx, api.recruit_params(paired=True))
    for alleles in loci:
        counts = [np.zeros(len(a) - 24, dtype=np.uint16) for a in alleles]
        gt.add_locus(np.frombuffer(b"".join(alleles), dtype=np.uint8), np.cumsum([0] + [len(a) for a in alleles]).astype(np.uint64),
                     np.concatenate(counts), np.cumsum([0] + [len(c) for c in counts]).astype(np.uint64), 25)
    gt.finalize()
    paths = [str(tmp_path / f"api{k}.fq") for k in range(2)]
    w = lio.FastxWriters(paths)
    dev = lio.FastxDevice(ctx, r1, r2)
    while dev.next(1000):
        cnt, lc = dev.recruit(gt)
        dev.write_recruited(w, cnt, lc)
    w.close()
    assert [open(p, "rb").read() for p in paths] == outs["device", 2]
