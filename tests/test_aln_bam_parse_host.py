"""The host passes of the device reader of aln.bam (locityper_amd/csrc/lcty_aln_bam_parse.hpp: the header parse and the walk of record
lengths) run stand-alone on the CPU over a corpus of byte strings — the designs, every prefix of a small file, byte mutations —, built
with the address and undefined-behaviour sanitizers (scripts/aln_bam_probe_host.cpp): the verdicts are those of a Python restatement,
and no byte outside a case's buffer is read."""
import os
import subprocess

from tests import aln_bam_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_parse_and_walk_over_the_corpus(tmp_path):
    exe, corpus = str(tmp_path / "aln_bam_probe_host"), str(tmp_path / "corpus.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "locityper_amd", "csrc"), os.path.join(ROOT, "scripts", "aln_bam_probe_host.cpp"), "-o", exe], check=True)
    n = AC.write_corpus(corpus)
    assert n > 1900
    r = subprocess.run([exe, corpus], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith(f"{n} cases, ") and r.stdout.rstrip().endswith(" 0 wrong"), r.stdout
