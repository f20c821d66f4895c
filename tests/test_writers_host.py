"""The host code behind every write_recruited (locityper_amd/csrc/lcty_writers.hpp: the one loop write_recruited_units, and the text of a
BAM record, bam_record_text), no device: a stand-alone program under the address and undefined-behaviour sanitizers
(scripts/writers_probe_host.cpp) on designed pairs and answers, its per-locus files held to tests/pyref_fastx.py."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from locityper_amd import cdefs
from tests import pyref_fastx as PF
from tests import pyref_sample_bam as SB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = (1, 31, 32, 33, 63, 64, 65, 151, 256)
N_WRITERS, MAX_OUT = 4, 3


def _records():
    """45 pairs with the mate lengths of tests/test_gpu_read_chunk.py: N and other codes at the first and the last base, every fifth mate 2
    a reverse record, every seventh pair without qualities, every ninth a single read; a name that fills its field"""
    rng = np.random.default_rng(31)
    units = []
    for i in range(45):
        mates = []
        for e, n in enumerate((LENS[i % 9], LENS[(i + i // 9) % 9])):
            if e == 1 and i % 9 == 8:
                mates.append(None)
                continue
            s = list("".join(rng.choice(list("ACGT"), n)))
            if i % 5 == 0:
                s[0] = "N"
            if i % 5 == 1:
                s[-1] = "NRY="[i % 4]
            qual = None if i % 7 == 0 else bytes(int(q) for q in rng.integers(0, 60, n))
            flag = (0x41, 0x81)[e] | (0x10 if e == 1 and i % 5 == 0 else 0)
            name = "x" * 254 if i == 3 else f"pair{i}"
            mates.append(SB.rec(0, 100 + i, name, flag, [("M", n)] if i % 2 else [], "".join(s), qual))
        units.append(mates)
    return units


def _text_of(r):
    """BamRecord::write_to: a reverse record back to front and complemented (codes other than ACGT become N), qualities + 33"""
    seq, qual = r["seq"], r["qual"]
    if r["flag"] & 0x10:
        seq = "".join({"A": "T", "C": "G", "G": "C", "T": "A"}.get(c, "N") for c in reversed(seq))
        qual = None if qual is None else qual[::-1]
    return PF.record_text((r["name"].encode(), seq.encode(), None if qual is None else bytes(q + 33 for q in qual)))


def _answers(n):
    """0, 1, 2 and MAX_OUT loci in turn, as tests/test_gpu_recruited.py designs them; one count above MAX_OUT"""
    cnt = np.array([(0, 1, 2, MAX_OUT)[i % 4] for i in range(n)], dtype=np.uint32)
    loci = np.full((n, MAX_OUT), 0xFFFFFFFF, dtype=np.uint32)                 # beyond cnt: never read
    for i in range(n):
        a = (i // 4) % 4
        loci[i, :min(cnt[i], MAX_OUT)] = sorted(((a + j) % N_WRITERS for j in range(int(cnt[i]))))[:MAX_OUT]
    cnt[7] = MAX_OUT + 2                                                     # the first MAX_OUT are written, no more is read
    return cnt, loci


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("writers_probe")
    ok = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(d / "has_san")], input="int main() { return 0; }\n",
                        capture_output=True, text=True)
    if ok.returncode != 0:
        pytest.skip("g++ has no sanitizer runtime")
    exe = str(d / "writers_probe_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "locityper_amd", "csrc"), os.path.join(ROOT, "scripts", "writers_probe_host.cpp"), "-lz", "-o", exe], check=True)
    return exe


def _run(exe, tmp, units, cnt, loci):
    blobs, offs, at = [], [], 0
    for mates in units:
        row = []
        for r in mates:
            if r is None:
                row.append(-1)
                continue
            b = SB.record_bytes(r)
            row.append(at); blobs.append(b); at += len(b)
        offs.append(row)
    (tmp / "slice.bin").write_bytes(b"".join(blobs))
    paths = [str(tmp / (f"locus{l}.fq.gz" if l == 1 else f"locus{l}.fq")) for l in range(N_WRITERS)]
    with open(tmp / "answers.txt", "w") as f:
        f.write(f"{N_WRITERS} {MAX_OUT} {len(units)}\n" + "\n".join(paths) + "\n")
        for c, row, o in zip(cnt, loci, offs):
            f.write(f"{c} {' '.join(map(str, row))} {o[0]} {o[1]}\n")
    r = subprocess.run([exe, str(tmp / "answers.txt"), str(tmp / "slice.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = [(gzip.open(p, "rb") if p.endswith(".gz") else open(p, "rb")).read() for p in paths]
    return r.stdout.splitlines(), got


def _expected(units, cnt, loci):
    """-> (the bytes of every writer, units written, the first unit recruited beyond the writers or None)"""
    files, written = [b""] * N_WRITERS, 0
    for i, mates in enumerate(units):
        if not cnt[i]:
            continue
        text = b"".join(_text_of(r) for r in mates if r is not None)
        for j in range(min(int(cnt[i]), MAX_OUT)):
            if loci[i, j] >= N_WRITERS:
                return files, written, i
            files[loci[i, j]] += text
        written += 1
    return files, written, None


def test_the_loop_and_the_record_text_under_the_sanitizers(probe, tmp_path):
    units = _records()
    cnt, loci = _answers(len(units))
    assert set(cnt.tolist()) == {0, 1, 2, MAX_OUT, MAX_OUT + 2} and any(m[1] is None for m in units) and any(m[0]["qual"] is None for m in units)
    assert any(m[1] is not None and m[1]["flag"] & 0x10 and set(m[1]["seq"]) - set("ACGT") for m in units)
    want, written, beyond = _expected(units, cnt, loci)
    assert beyond is None and written == int((cnt > 0).sum()) and all(want)
    out, got = _run(probe, tmp_path, units, cnt, loci)
    assert out == [f"status 0 written {written}"]
    assert got == want


def test_a_locus_beyond_the_writers_is_refused_where_it_stands(probe, tmp_path):
    units = _records()
    cnt, loci = _answers(len(units))
    assert cnt[22] == 2
    loci[22, 1] = N_WRITERS                                                  # the unit's first locus is written, its second refused
    want, _, beyond = _expected(units, cnt, loci)
    assert beyond == 22
    out, got = _run(probe, tmp_path, units, cnt, loci)
    assert out[0] == f"status {cdefs.ERR_INVALID_INPUT} written 0"
    assert out[1] == f"record 22 is recruited to locus {N_WRITERS} of {N_WRITERS} writers"
    assert got == want
