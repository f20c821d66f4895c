"""examples/estimate_bg.cpp --fetch: the sample's whole indexed BAM file in place of the region's slice, the same distr.gz out."""
import gzip
import subprocess

import pytest

from tests import bg_fetch_cases as K, bg_synth
from tests.test_gpu_example import build_example


@pytest.mark.gpu
def test_fetch_route_writes_the_same_distr(tmp_path):
    s = bg_synth.Sample(region_len=100_000)
    refs = K.wide_refs(s)
    whole = K.write_indexed(tmp_path / "whole.bam", refs, K.with_foreign(s))
    plain = K.write_plain(tmp_path / "slice.bam", refs, s.records)
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
    payloads = []
    for bam, out, extra in ((plain, tmp_path / "load", []), (whole, tmp_path / "fetch", ["--fetch"]), (whole, tmp_path / "fetch_ix", ["--fetch", str(whole) + ".bai"])):
        r = subprocess.run([exe, str(bam), str(fa), str(cnt), f"{s.contig}:{s.start + 1}-{s.end}", "illumina", str(out)] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("fetched " in r.stdout) == bool(extra)
        payloads.append(gzip.open(out / "distr.gz", "rb").read())
    assert payloads[0] == payloads[1] == payloads[2] and len(payloads[0]) > 100
