"""The corpus of FASTA / FASTQ inputs the device route is checked on (tests/test_fastx_parse_host.py on the CPU with the serial
executor of scripts/fastx_probe_host.cpp, tests/test_gpu_fastx_device.py on the device). A case is a dict: name, files (the bytes of
one or two files), interleaved, kind ("valid": every reader gives the same records; "error": the same records in front of the same
error; "mixed": FASTA and FASTQ records in one file, which the host reader accepts and the device route refuses)."""
import os

import numpy as np


def _fq(name, seq, qual=None, plus=b"+", eol=b"\n"):
    qual = b"I" * len(seq) if qual is None else qual
    return b"@" + name + eol + seq + eol + plus + eol + qual + eol


def _case(name, files, kind="valid", interleaved=False):
    return dict(name=name, files=[bytes(f) for f in files], kind=kind, interleaved=interleaved)


LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257]


def _seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(list(alphabet), n).astype(np.uint8).tolist()) if n else b""


def valid_cases():
    rng = np.random.default_rng(77)
    c = []
    c.append(_case("empty-file", [b""]))
    c.append(_case("empty-first-line", [b"\n@r\nAC\n+\nII\n"]))
    c.append(_case("one-record", [_fq(b"r1", b"ACGT")]))
    c.append(_case("crlf", [_fq(b"r1", b"ACGT", eol=b"\r\n") + _fq(b"r2 d", b"TTGA", eol=b"\r\n")]))
    c.append(_case("last-line-without-newline", [_fq(b"r1", b"ACGT") + b"@r2\nAC\n+\nII"]))
    c.append(_case("last-line-without-newline-ends-in-cr", [_fq(b"r1", b"ACG") + b"@r2\nACG\n+\nII\r"]))          # the \r stays: 3 == 3
    c.append(_case("description-after-space", [_fq(b"r1 some words here", b"ACGT") + _fq(b"r2  two", b"AC")]))
    c.append(_case("description-after-tab", [_fq(b"r1\tnot a description", b"ACGT") + _fq(b"r2\tx y", b"AC")]))
    c.append(_case("header-begins-with-space", [_fq(b" odd name", b"ACGT")]))
    c.append(_case("empty-sequence-and-qualities", [_fq(b"r1", b"") + _fq(b"r2", b"ACGT") + _fq(b"r3", b"")]))
    c.append(_case("qualities-begin-with-at-and-plus", [_fq(b"r1", b"ACGT", qual=b"@III") + _fq(b"r2", b"ACGT", qual=b"+III") + _fq(b"r3", b"AC", qual=b"@+")]))
    c.append(_case("plus-name-third-line", [_fq(b"r1", b"ACGT", plus=b"+r1") + _fq(b"r2", b"ACGT", plus=b"+r2 again")]))
    c.append(_case("empty-header-mid-file", [_fq(b"r1", b"ACGT") + _fq(b"r2", b"AC") + b"\n" + _fq(b"r3", b"ACGT") + _fq(b"r4", b"AC")]))
    c.append(_case("header-without-at", [b"r1\nACGT\n+\nIIII\n#r2 x\nAC\n+\nII\n"]))
    c.append(_case("other-bases", [_fq(b"low", b"acgtACGTnN") + _fq(b"iupac", b"RYKMSWBDHVN-*.ACGT") + _fq(b"n", b"N" * 70) + _fq(b"u", b"ACGU")]))
    c.append(_case("every-length", [b"".join(_fq(b"len%d" % n, _seq(rng, n)) for n in LENGTHS)]))
    c.append(_case("every-length-other-bases", [b"".join(_fq(b"len%d" % n, _seq(rng, n, b"ACGTNacgtRY")) for n in LENGTHS)]))
    c.append(_case("read-of-10000", [_fq(b"a", b"ACGT") + _fq(b"long", _seq(rng, 10_000, b"ACGTN")) + _fq(b"b", b"AC")]))
    # FASTA
    c.append(_case("fasta-one-line", [b">s1\nACGT\n>s2 d\nAC\n"]))
    c.append(_case("fasta-crlf-no-last-newline", [b">s1\r\nACGT\r\nAC\r\n>s2\r\nGG"]))
    c.append(_case("fasta-empty-lines-inside", [b">s1\nACGT\n\nAC\n\n\n>s2\n\nGG\n"]))
    c.append(_case("fasta-1-base-lines", [b">s1\n" + b"".join(bytes([b]) + b"\n" for b in _seq(rng, 70)) + b">s2\nA\nC\n"]))
    c.append(_case("fasta-7-base-lines", [b">s1\n" + b"".join(_seq(rng, 7, b"ACGTN") + b"\n" for _ in range(21)) + b">s2 x\n" + _seq(rng, 7) + b"\n" + _seq(rng, 3) + b"\n"]))
    c.append(_case("fasta-two-headers-in-a-row", [b">s1\n>s2\nACGT\n>s3\n>s4\nAC\n"]))
    c.append(_case("fasta-every-length", [b"".join(b">len%d\n" % n + b"".join(_seq(rng, min(60, n - k)) + b"\n" for k in range(0, n, 60)) for n in LENGTHS) + b">end\nA\n"]))
    c.append(_case("fasta-long", [b">long\n" + b"".join(_seq(rng, 80, b"ACGTN") + b"\n" for _ in range(125)) + b">b\nAC\n"]))
    # pairs
    il = b"".join(_fq(b"p%d/1" % i, _seq(rng, 20 + i)) + _fq(b"p%d/2" % i, _seq(rng, 33 - i)) for i in range(9))
    c.append(_case("interleaved", [il], interleaved=True))
    c.append(_case("interleaved-fasta", [b"".join(b">p%d/1\n" % i + _seq(rng, 9) + b"\n" + _seq(rng, 4) + b"\n>p%d/2\n" % i + _seq(rng, 5) + b"\n" for i in range(5))], interleaved=True))
    a = b"".join(_fq(b"pair%d/1 a long description that file two does not have, so that the windows of the two fall out of step" % i, _seq(rng, 40)) for i in range(12))
    b = b"".join(_fq(b"pair%d/2" % i, _seq(rng, 37)) for i in range(12))
    c.append(_case("two-files-out-of-step", [a, b]))
    c.append(_case("two-files-short-names", [_fq(b"a", b"AC") + _fq(b"bcd", b"ACG"), _fq(b"x", b"TT") + _fq(b"xyz", b"TTT")]))      # up to three bytes: the lengths alone
    c.append(_case("two-files-fastq-and-fasta", [_fq(b"p1/1", b"ACGT") + _fq(b"p2/1", b"AC"), b">p1/2\nTT\nGG\n>p2/2\nA\n"]))
    c.append(_case("two-files-empty", [b"", b""]))
    return c


def error_cases():
    ok = _fq(b"ok1", b"ACGT") + _fq(b"ok2", b"AC")
    incomplete, fmt, nonmatch = b"@bad\nACGT\n", b"@bad\nACGT\nIIII\n@x\n", b"@bad\nACGT\n+\nIII\n"
    c = []
    c.append(_case("incomplete-last", [ok + incomplete], "error"))
    c.append(_case("incomplete-header-only", [ok + b"@bad\n"], "error"))
    c.append(_case("incomplete-header-only-no-newline", [ok + b"@bad"], "error"))
    c.append(_case("format-last", [ok + b"@bad\nACGT\nIIII\n"], "error"))
    c.append(_case("format-empty-third-line", [ok + b"@bad\nACGT\n\nIIII\n"], "error"))
    c.append(_case("nonmatch-last", [ok + nonmatch], "error"))
    c.append(_case("nonmatch-missing-fourth-line", [ok + b"@bad\nACGT\n+\n"], "error"))
    c.append(_case("nonmatch-cr-kept-on-last-line", [ok + b"@bad\nACGT\n+\nIIII\r"], "error"))
    # an earlier record with one error, a different error later: the first one wins
    c.append(_case("format-then-nonmatch", [ok + b"@bad\nACGT\n-\nIIII\n" + ok + b"@worse\nAC\n+\nI\n"], "error"))
    c.append(_case("nonmatch-then-format", [ok + nonmatch + ok + b"@worse\nAC\n-\nII\n"], "error"))
    c.append(_case("nonmatch-then-incomplete", [ok + nonmatch + ok + b"@worse\nAC\n"], "error"))
    c.append(_case("format-far-before-nonmatch", [ok + fmt[:15] + ok * 40 + nonmatch], "error"))
    c.append(_case("error-behind-empty-header-is-not-read", [ok + b"\n" + nonmatch]))
    c.append(_case("fasta-empty-last", [b">s1\nACGT\n>s2\n"], "error"))
    c.append(_case("fasta-empty-last-no-newline", [b">s1\nACGT\n>s2"], "error"))
    c.append(_case("fasta-empty-only-empty-lines", [b">s1\nACGT\n>s2\n\n\n"], "error"))
    c.append(_case("fasta-empty-only-record", [b">s1\n"], "error"))
    # pairs
    c.append(_case("interleaved-odd", [_fq(b"a/1", b"AC") + _fq(b"a/2", b"AC") + _fq(b"b/1", b"AC")], "error", True))
    c.append(_case("interleaved-odd-at-empty-header", [_fq(b"a/1", b"AC") + b"\n" + _fq(b"a/2", b"AC")], "error", True))
    c.append(_case("interleaved-mismatch", [_fq(b"abcd", b"AC") + _fq(b"abcd", b"AC") + _fq(b"abcd", b"AC") + _fq(b"aXcd", b"AC")], "error", True))
    c.append(_case("interleaved-mismatch-of-lengths", [_fq(b"abc", b"AC") + _fq(b"abcd", b"AC")], "error", True))
    c.append(_case("interleaved-second-mate-bad-before-mismatch", [_fq(b"abcd", b"AC") + b"@aXcd\nAC\n+\nI\n"], "error", True))
    c.append(_case("interleaved-mismatch-before-later-error", [_fq(b"abcd", b"AC") + _fq(b"aXcd", b"AC") + nonmatch], "error", True))
    c.append(_case("two-files-different-length", [_fq(b"p1", b"AC") + _fq(b"p2", b"AC"), _fq(b"p1", b"AC")], "error"))
    c.append(_case("two-files-different-length-second-longer", [_fq(b"p1", b"AC"), _fq(b"p1", b"AC") + _fq(b"p2", b"AC")], "error"))
    c.append(_case("two-files-mismatch", [_fq(b"p1/1", b"AC") + _fq(b"pA/1", b"AC"), _fq(b"p1/2", b"AC") + _fq(b"pB/2", b"AC")], "error"))
    c.append(_case("two-files-first-bad-wins", [_fq(b"p1", b"AC") + nonmatch, _fq(b"p1", b"AC") + b"@worse\nAC\n-\nII\n"], "error"))
    c.append(_case("two-files-second-bad-though-first-ended", [_fq(b"p1", b"AC"), _fq(b"p1", b"AC") + nonmatch], "error"))
    c.append(_case("two-files-bad-record-before-mismatch", [_fq(b"p1/1", b"AC") + _fq(b"pA/1", b"AC"), _fq(b"p1/2", b"AC") + b"@pB/2\nAC\n+\nI\n"], "error"))
    return c


def mixed_cases():
    return [_case("mixed-fasta-in-fastq", [_fq(b"r1", b"ACGT") + b">s1\nAC\nGT\n" + _fq(b"r2", b"AC")], "mixed"),
            _case("mixed-fastq-in-fasta", [b">s1\nAC\nGT\n" + _fq(b"r1", b"ACGT") + b">s2\nAC\n"], "mixed")]


def property_case(seed=5, n=2000, fasta=False):
    """n seeded records: lengths 0 to 600, random line ends, (FASTA) random line widths"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ln = int(rng.integers(0, 601)) if i % 5 else int(rng.integers(0, 40))
        if fasta and ln == 0 and i == n - 1:
            ln = 1
        seq = _seq(rng, ln, b"ACGTACGTACGTNacgtRY")
        eol = b"\r\n" if rng.random() < 0.3 else b"\n"
        name = b"rec%d" % i + (b" desc %d" % i if i % 3 == 0 else b"")
        if fasta:
            out.append(b">" + name + eol)
            k = 0
            while k < ln:
                w = int(rng.integers(1, 90))
                out.append(seq[k:k + w] + (b"\r\n" if rng.random() < 0.3 else b"\n"))
                k += w
                if rng.random() < 0.05:
                    out.append(b"\n")
        else:
            out.append(_fq(name, seq, qual=_seq(rng, ln, b"!#+5?@IJ"), eol=eol))
    return _case("property-fasta" if fasta else "property-fastq", [b"".join(out)])


def all_cases():
    return valid_cases() + error_cases() + mixed_cases()


def write_case(case, directory):
    """the files of a case -> their paths"""
    os.makedirs(directory, exist_ok=True)
    paths = []
    for k, data in enumerate(case["files"]):
        p = os.path.join(directory, "%s.%d.txt" % (case["name"], k + 1))
        with open(p, "wb") as f:
            f.write(data)
        paths.append(p)
    return paths


def write_corpus(directory):
    """Every case, and corpus.tsv for scripts/fastx_probe_host.cpp: name, kind, interleaved (0 / 1), path 1, path 2 or "-" per line."""
    cases = all_cases() + [property_case(), property_case(fasta=True)]
    with open(os.path.join(directory, "corpus.tsv"), "w") as m:
        for c in cases:
            paths = write_case(c, directory)
            m.write("\t".join([c["name"], c["kind"], str(int(c["interleaved"])), paths[0], paths[1] if len(paths) > 1 else "-"]) + "\n")
    return cases
