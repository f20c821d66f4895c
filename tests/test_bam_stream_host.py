"""The reader of whole BAM files in windows (lcty_bam_stream_*), no device: the restatement tests/pyref_bam_stream.py against
answers written out by hand, the new entries and knobs against the header, and the host half (locityper_amd/csrc/
lcty_bam_stream_window.hpp: containers, windows, carry, enlargement, the change of file, the order of errors) as a stand-alone program
under the address and undefined-behaviour sanitizers (scripts/bam_stream_probe_host.cpp) held to the same restatement."""
import os
import re
import subprocess

import pytest

from locityper_amd import _lib, cdefs
from tests import bam_stream_cases as BC
from tests import pyref_bam_stream as PB
from tests import pyref_sample_bam as SB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["lcty_bam_stream_open", "lcty_bam_stream_close", "lcty_bam_stream_next"]


def _twelve():
    u = lambda name, flag, seq: SB.rec(-1, -1, name, flag | 4, [], seq, None)
    f0 = [u("a/1", 0x41, "ACGT"), u("a/1", 0x800, "GG"), u("a/2", 0x91, "AACN"), u("b/1", 0x51, "TTGCA")]
    f1 = [u("b/1", 0x100, "C"), u("x", 0x900, "")]
    f2 = [u("b/2", 0x81, "GAT"), u("c/2", 0x81, "AC"), u("c/1", 0x41, "R="), u("d/1", 0x41, "T"), u("d/1", 0x800, ""), u("d/2", 0x81, "A")]
    return [f0, f1, f2]


def test_pyref_on_twelve_records_in_three_files():
    files = _twelve()
    assert sum(len(f) for f in files) == 12
    s = PB.Stream(files, interleaved=True, paths=["x.bam", "y.bam", "z.bam"])
    assert s.refused is None
    assert [r["name"] for r in s.kept] == ["a/1", "a/2", "b/1", "b/2", "c/2", "c/1", "d/1", "d/2"]
    assert s.units == [(0, 1), (2, 3), (4, 5), (6, 7)]                          # b's mates lie in files 0 and 2; c's are taken as they come
    # a/2 and b/1 are reverse records: back to front and complemented, N stays N; IUPAC codes and '=' read N only when complemented
    assert s.mates() == [["ACGT", "NGTT"], ["TGCAA", "GAT"], ["AC", "R="], ["T", "A"]]
    assert s.totals() == (12, 8, 8, 4 + 4 + 5 + 3 + 2 + 2 + 1 + 1, 4)
    mate_len, mate_off, bases2, nmask = s.packed()
    assert mate_len.tolist() == [4, 4, 5, 3, 2, 2, 1, 1] and mate_off.tolist() == [32 * i for i in range(9)]
    assert bases2[0] == 0xE4 and bases2[2] == 0b11_11_10_00 and nmask.tolist() == [0, 1, 0, 0, 0, 3, 0, 0]
    assert s.text(which={1}) == b">b/1\nTGCAA\n>b/2\nGAT\n"
    # single-end: every kept record is a read
    s = PB.Stream(files, interleaved=False)
    assert s.units == [(k, None) for k in range(8)] and s.totals() == (12, 8, 8, 22, 8)
    # the first offending record in input order decides; what lies in front of it is handed out
    files[2][3]["name"] = "dd/1"
    s = PB.Stream(files, interleaved=True, paths=["x.bam", "y.bam", "z.bam"])
    assert s.units == [(0, 1), (2, 3), (4, 5)] and s.refused.status == SB.ERR_INVALID_DATA
    assert s.refused.what == "Interleaved input file(s) x.bam, y.bam, z.bam contains non matching first and second mate (dd/1 and d/2)"
    assert s.totals()[:3] == (11, 7, 7)
    s = PB.Stream([files[0], files[1]], interleaved=True, paths=["x.bam", "y.bam"])
    assert s.units == [(0, 1)] and s.refused.what == "Odd number of records in an interleaved input file(s) x.bam, y.bam"
    files[0][2]["seq"] = ""
    s = PB.Stream(files, interleaved=True)
    assert s.units == [] and s.refused.what == "Primary alignment for read a/2 has no sequence" and s.walked == 2
    assert PB.equal_names_fast(b"abc", b"xyz") and PB.equal_names_fast(b"abcd", b"xbzz") and not PB.equal_names_fast(b"abcd", b"aXcd")
    assert not PB.equal_names_fast(b"abcd", b"abcde") and PB.equal_names_fast(b"r/1", b"r/2")


def test_entries_are_declared_bound_and_refuse_null_arguments():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "locityper_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in ENTRIES:
        m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
        assert m, f"{name} is not declared in the header"
        assert hasattr(L, name) and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == len([a for a in m.group(1).split(",") if a.strip()]), name
    fields = re.search(r"typedef struct lcty_bam_stream_stats \{(.*?)\} lcty_bam_stream_stats;", header, flags=re.S).group(1)
    declared = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert declared == [n for n, _ in cdefs.BamStreamStats._fields_]
    bad = cdefs.ERR_INVALID_INPUT
    out = _lib.VP()
    assert L.lcty_bam_stream_open(None, None, 0, 0, out) == bad and not out.value
    assert L.lcty_bam_stream_open(None, None, 1, 0, None) == bad
    assert L.lcty_bam_stream_next(None, None, None, None) == bad
    L.lcty_bam_stream_close(None)                                             # like free(NULL)


def test_knobs_are_in_the_list_and_in_the_header():
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    api_src, header = read("locityper_amd", "csrc", "lcty_api.hip"), read("include", "locityper_hip.h")
    src, host = read("locityper_amd", "csrc", "lcty_bam_stream.hip"), read("locityper_amd", "csrc", "lcty_bam_stream_window.hpp")
    known = api_src[api_src.index("known[] = {"):api_src.index("nullptr};")]
    paragraph = header[:header.index("int32_t lcty_ctx_set_knob(")]
    asked = set(re.findall(r'knob\("(bam_stream_[a-z_]+)"', src))
    assert asked == {"bam_stream_window_bytes", "bam_stream_window_limit"}
    for name in asked:
        assert f'"{name}"' in known and f'"{name}"   ' in paragraph, name
    assert "WINDOW_DEFAULT = 1ull << 28, LIMIT_DEFAULT = 1ull << 33" in host and "default 2^28" in paragraph and "default 2^33" in paragraph


# ---------------------------------------------------------------- the host half under the sanitizers
def test_host_half_is_clean_under_the_sanitizers_and_equals_the_restatement(tmp_path):
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main() { return 0; }\n",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("g++ has no sanitizer runtime")
    exe = str(tmp_path / "bam_stream_probe_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "locityper_amd", "csrc"), os.path.join(ROOT, "scripts", "bam_stream_probe_host.cpp"), "-lz", "-o", exe], check=True)
    cases = BC.write_corpus(tmp_path)
    want = []
    for name, files, interleaved, paths in cases:
        s = PB.Stream(files, interleaved, paths)
        for u, mates in zip(s.units, s.mates()):
            want.append(f"{name} unit" + "".join(" -" if k is None else f" {k} [{s.kept[k]['name']}] {m}" for k, m in zip(u, mates)))
        want.append(f"{name} status {s.refused.status if s.refused else 0} {s.refused.what if s.refused else ''}")
        want.append(f"{name} totals " + " ".join(map(str, s.totals())))
    r = subprocess.run([exe, str(tmp_path / "corpus.tsv")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = r.stdout.splitlines()
    m = re.fullmatch(r"bam_stream_probe_host: (\d+) cases, (\d+) windowed runs, (\d+) enlarged windows, (\d+) bytes carried, 0 differences", got[-1])
    assert m and int(m.group(1)) == len(cases) and int(m.group(2)) == 4 * len(cases) and int(m.group(3)) > 0 and int(m.group(4)) > 0
    assert got[:-1] == want
    assert sum(" status 2 " in g for g in got) >= 3 * 11 and any("leaves the end of its file" in g for g in got)
