"""The parsers of untrusted bytes in front of every BGZF reader (locityper_amd/csrc/lcty_bgzf_index.hpp: parse_bai; lcty_bgzf.hpp:
bgzf_head): their verdicts against a Python restatement, run by the stand-alone host probe under the address and undefined-behaviour
sanitizers (scripts/vcf_index_probe_host.cpp), and every prefix of a valid BAI index through lcty_sample_bam_open. No device is needed."""
import os
import struct
import subprocess

import pytest

from locityper_amd import cdefs, io as lio
from locityper_amd._lib import LocityperError
from tests import pyref_sample_bam as P
from tests import vcf_index_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFS = [("chrA", 100_000), ("chrB", 50_000)]
OK, NOT_A_BLOCK, TOO_LARGE = 0, 1, 2                                  # BgzfVerdict


def six_records():
    """Two references with records in several bins and 16 kb windows, and one record without coordinate."""
    M = [("M", 8)]
    return [P.rec(0, 100, "a", 0, M, "ACGTACGT"), P.rec(0, 120, "b", 0x10, M, "ACGTACGT"), P.rec(0, 40_000, "c", 0, M, "ACGTACGT"),
            P.rec(1, 5, "d", 0, M, "ACGTACGT"), P.rec(1, 33_000, "e", 0, M, "ACGTACGT"), P.rec(-1, -1, "f", 4, [], "ACGTACGT")]


def written(tmp_path):
    """-> (path of the BAM file, the bytes of its valid index)"""
    path = str(tmp_path / "six.bam")
    P.write_bam(path, REFS, six_records(), block_size=120)
    bai = open(path + ".bai", "rb").read()
    os.remove(path + ".bai")
    return path, bai


def bai_status(x, n_refs_of_header):
    """parse_bai restated: the status it gives the bytes x."""
    if x[:4] == b"CSI\1" or x[:2] == b"\x1f\x8b":
        return cdefs.ERR_UNSUPPORTED
    if len(x) < 8 or x[:4] != b"BAI\1":
        return cdefs.ERR_INVALID_DATA
    at = 4

    def take(fmt):
        nonlocal at
        n = struct.calcsize(fmt)
        if at + n > len(x):
            raise EOFError
        v = struct.unpack_from(fmt, x, at)[0]
        at += n
        return v
    try:
        n_ref = take("<I")
        if n_ref != n_refs_of_header:
            return cdefs.ERR_INVALID_DATA
        for _ in range(n_ref):
            for _ in range(take("<I")):
                take("<I")
                for _ in range(2 * take("<I")):
                    take("<Q")
            for _ in range(take("<I")):
                take("<Q")
    except EOFError:
        return cdefs.ERR_INVALID_DATA
    return 0                                                          # n_no_coor is optional, bytes behind it are ignored


def bgzf_head(p):
    """bgzf_head restated: (verdict, csize, isize, head) of the bytes p."""
    n = len(p)
    if n < 18 or p[0] != 0x1f or p[1] != 0x8b or p[2] != 8 or not p[3] & 4:
        return NOT_A_BLOCK, 0, 0, 0
    xlen = p[10] | p[11] << 8
    if 12 + xlen > n:
        return NOT_A_BLOCK, 0, 0, 0
    bsize, x = 0, 12
    while x + 4 <= 12 + xlen:
        slen = p[x + 2] | p[x + 3] << 8
        if p[x:x + 2] == b"BC" and slen == 2 and x + 6 <= 12 + xlen:
            bsize = (p[x + 4] | p[x + 5] << 8) + 1
        x += 4 + slen
    if bsize < 12 + xlen + 8 or bsize > n:
        return NOT_A_BLOCK, 0, 0, 0
    isize = struct.unpack_from("<I", p, bsize - 4)[0]
    return (TOO_LARGE if isize > 0x10000 else OK), bsize, isize, (12 + xlen if p[3] == 4 else 0)


def head_cases():
    """40 bytes: a valid block (18 bytes of header, 14 of a deflate stream nobody reads, CRC, ISIZE) and what is wrong with its like."""
    good = struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, 39) + bytes(range(14)) + struct.pack("<II", 0xDEADBEEF, 5)
    assert len(good) == 40

    def put(at, fmt, v):
        b = bytearray(good)
        struct.pack_into(fmt, b, at, v)
        return bytes(b)
    return [(good, OK), (put(10, "<H", 100), NOT_A_BLOCK), (put(14, "<H", 3), NOT_A_BLOCK), (put(16, "<H", 20), NOT_A_BLOCK),
            (put(36, "<I", 0x10001), TOO_LARGE), (good[:39], NOT_A_BLOCK)]


def test_the_restatements_on_hand_derived_answers(tmp_path):
    _, bai = written(tmp_path)
    assert bai_status(bai, 2) == 0 and bai_status(bai, 3) == cdefs.ERR_INVALID_DATA
    assert struct.unpack_from("<Q", bai, len(bai) - 8)[0] == 1 and struct.pack("<I", 37450) in bai          # n_no_coor, the pseudo-bin
    cases = head_cases()
    assert [bgzf_head(b)[0] for b, _ in cases] == [v for _, v in cases]
    assert bgzf_head(cases[0][0]) == (OK, 40, 5, 18) and bgzf_head(cases[4][0]) == (TOO_LARGE, 40, 0x10001, 18)


def test_parse_bai_and_bgzf_head_are_clean_under_the_sanitizers(tmp_path):
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main() { return 0; }\n",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("g++ has no sanitizer runtime")
    exe, corpus = str(tmp_path / "vcf_index_probe_host"), str(tmp_path / "corpus.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "locityper_amd", "csrc"), os.path.join(ROOT, "scripts", "vcf_index_probe_host.cpp"), "-o", exe], check=True)
    _, bai = written(tmp_path)
    n_ref_plus = bai[:4] + struct.pack("<I", 3) + bai[8:]
    designed = [(bai, 2, 0), (b"CSI\1" + bai[4:], 2, cdefs.ERR_UNSUPPORTED), (b"\x1f\x8b" + bai[2:], 2, cdefs.ERR_UNSUPPORTED),
                (n_ref_plus, 2, cdefs.ERR_INVALID_DATA)]
    bai_cases = designed + [(bai[:n], 2, bai_status(bai[:n], 2)) for n in range(len(bai))]
    assert [bai_status(b, r) for b, r, _ in designed] == [st for _, _, st in designed]
    heads = head_cases()
    n = VC.write_corpus(corpus)
    with open(corpus, "ab") as f:
        f.write(struct.pack("<I", len(bai_cases)))
        for b, n_refs, st in bai_cases:
            f.write(struct.pack("<III", len(b), st, n_refs) + b)
        f.write(struct.pack("<I", len(heads)))
        for b, v in heads:
            assert bgzf_head(b)[0] == v
            f.write(struct.pack("<IIIII", len(b), *bgzf_head(b)) + b)
    n += len(bai_cases) + len(heads)
    r = subprocess.run([exe, corpus], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith(f"{n} cases, ") and r.stdout.rstrip().endswith(" 0 wrong"), r.stdout


def test_every_prefix_of_a_valid_bai_through_open(tmp_path):
    path, bai = written(tmp_path)
    index = str(tmp_path / "prefix.bai")
    for n in range(len(bai) + 1):
        open(index, "wb").write(bai[:n])
        if n >= len(bai) - 8:                                        # the trailing n_no_coor is optional
            bam = lio.SampleBam(path, index)
            assert bam.contigs == ["chrA", "chrB"]
            bam.close()
            continue
        with pytest.raises(LocityperError) as e:
            lio.SampleBam(path, index)
        assert e.value.code == cdefs.ERR_INVALID_DATA, n
        assert ("is not a BAI index" if n < 8 else "truncated BAI index") in str(e.value), n
