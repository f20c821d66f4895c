"""examples/count_kmers.cpp from compiled code: a genome FASTA and the sequences of a locus in, counts.bin (one KmerCounts block, the
reference record last) and the reference window out. The block must equal tests/pyref_kmer_count.py's tables, and
examples/build_locus_db.cpp must make of it the kmers.bin.br tests/pyref_db.py makes of those tables."""
import gzip
import json
import subprocess

import numpy as np
import pytest

from locityper_amd import api, io
from tests import pyref_db as RD
from tests import pyref_kmer_count as R
from tests.test_gpu_example import build_example

K = 25


def test_count_kmers_example_compiles_against_the_header(tmp_path):
    build_example(str(tmp_path / "count_kmers"), "count_kmers.cpp")


def _rand(rng, n):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)])


def _haplotype(rng, window, n_var):
    """the window with point changes, short deletions and insertions"""
    s = bytearray(window)
    for p in sorted(rng.integers(0, len(window) - 10, n_var), reverse=True):
        kind = rng.integers(0, 3)
        if kind == 0:
            s[p] = b"ACGT"[(b"ACGT".index(s[p]) + 1 + int(rng.integers(0, 3))) % 4]
        elif kind == 1:
            del s[p:p + int(rng.integers(1, 6))]
        else:
            s[p:p] = _rand(rng, int(rng.integers(1, 6)))
    return bytes(s)


@pytest.mark.gpu
def test_count_kmers_example_feeds_build_locus_db(tmp_path):
    rng = np.random.default_rng(41)
    win_start, win_end = 120_000, 128_000
    chr1 = bytearray(_rand(rng, 200_000))
    chr1[50_000:58_000] = chr1[win_start:win_end]                          # a second copy of the locus: counts of 2 and more
    chr1[30_000:31_000] = bytes(chr1[30_000:31_000]).lower()
    chr1[90_000:90_100] = b"N" * 100
    clean = bytes(chr1[win_start:win_end])
    chr1[win_start + 3_000:win_start + 3_030] = b"N" * 30                 # the N run of the reference record
    contigs = [("chr1", bytes(chr1)), ("chr2", _rand(rng, 100_000) + clean[1_000:2_000].lower())]
    names = [f"HG{i:03d}.1" for i in range(6)]
    haps = [_haplotype(rng, clean, 12) for _ in names]
    ref = R.standardize(bytes(chr1[win_start:win_end]))
    assert ref.count(b"N") == 30

    with gzip.open(tmp_path / "genome.fa.gz", "wb") as f:
        f.write(RD.multiline_fasta([n for n, _ in contigs], [s for _, s in contigs]))
    (tmp_path / "haps.fa").write_bytes(RD.multiline_fasta(names, haps))
    (tmp_path / "ref.fa").write_bytes(RD.multiline_fasta(["ref"], [ref]))
    exe = str(tmp_path / "count_kmers")
    build_example(exe, "count_kmers.cpp")
    r = subprocess.run([exe, "-g", str(tmp_path / "genome.fa.gz"), "-k", str(K), "-s", str(tmp_path / "haps.fa"), "-r", str(tmp_path / "ref.fa"),
                        "-R", f"chr1:{win_start}-{win_end}", str(tmp_path / "window.fa"), "-o", str(tmp_path / "counts.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    stats = json.loads(r.stdout.strip().splitlines()[-1])
    assert stats["genome_contigs"] == 2 and stats["genome_bases"] == sum(len(s) for _, s in contigs) and stats["n_seqs"] == 7

    tables = R.kmer_counts(contigs, haps + [R.fill_n(ref)], K, 2)
    assert max(int(t.max()) for t in tables) >= 2
    k, off, counts, used = api.parse_kmer_counts((tmp_path / "counts.bin").read_bytes())
    assert k == K and len(off) == 8 and used == len((tmp_path / "counts.bin").read_bytes())
    for i, t in enumerate(tables):
        assert np.array_equal(counts[int(off[i]):int(off[i + 1])], t), i
    assert (tmp_path / "counts.bin").read_bytes() == RD.kmer_counts_save(K, 2, tables)

    text = (tmp_path / "window.fa").read_bytes().split(b"\n")
    assert text[0] == f">chr1:{win_start}-{win_end}".encode() and b"".join(text[1:]) == ref

    dbexe = str(tmp_path / "build_locus_db")
    build_example(dbexe, "build_locus_db.cpp")
    r = subprocess.run([dbexe, str(tmp_path / "haps.fa"), str(tmp_path / "ref.fa"), str(tmp_path / "counts.bin"), str(tmp_path / "DB"), "L1"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = RD.build_locus(names, haps, ref, tables, K, 2, 15, 15, False)
    built = tmp_path / "DB" / "loci" / "L1"
    assert io.read_file(built / "kmers.bin.br") == want["kmers"]
    assert io.read_file(built / "haplotypes.fa.gz") == want["fasta"]
